"""Host checks of the batched fits' in-workgroup cosine solve (mvtv_small_cos.hip). No GPU.

The rules transcribed in tests/small_cos_model.py against the source, the LDS bound at every admitted (p, N, nb), the
GPU cases' coverage of the instantiations the launchers dispatch, and the float64 model of the kernel's index logic
against the long-double cosine-transform solve (oracle/spectral_ld.py) under the forward-error rule of §2.1:
max|x - x_ld| <= min(1e-12, 32 e64) max|x_ld|, e64 the float64 pocketfft evaluation's own distance from the long-double
one. The same model with r as one rounded double misses that bound on the long 1-D lines at sigma = 2e5, which is what
the h + l multipliers are for (§2.3).
"""
import os
import re

import numpy as np
import pytest

import small_batch_cases as S
import small_cos_model as M
from oracle import spectral_ld as SLD

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multivartv_amd", "csrc")
SIGMAS = [0.0, 1e-3, 3.7, 2e5]


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_rules_match_the_source():
    h = _src("mvtv_internal.h")
    assert int(re.search(r"constexpr uint32_t kSmallCosZLds = (\d+);", h).group(1)) == M.COS_Z_LDS_WORDS
    assert int(re.search(r"constexpr uint32_t kSmallCosMaxT = (\d+);", h).group(1)) == M.COS_MAX_T
    assert "return uint64_t(nb) * N <= kSmallCosZLds;" in h
    assert "size_t(g.N) + 9u * size_t(small_nt(g.N) / 64) + cp.tab_words" in h
    c = _src("mvtv_small_cos.hip")
    assert "if (g.m[j] >= g.m[ld]) ld = j;" in c                  # the longest, ties: the last
    assert "while (tpl * 2 * nlines <= nt) tpl *= 2;" in c
    assert "c.sl = int32_t((g.m[ld] + tpl - 1) / tpl);" in c
    assert "c.pitch[j] = g.m[j] | 1u;" in c and "off += g.m[j] * c.pitch[j];" in c
    assert M.COS_Z_LDS_WORDS < S.Z_LDS_WORDS
    assert M.line_dim([7]) == 0 and M.line_dim([64, 64]) == 1 and M.line_dim([2048, 2]) == 0
    assert M.line_dim([4, 4, 4, 16]) == 3 and M.line_dim([6, 6, 6, 6]) == 3 and M.line_dim([5, 9, 9]) == 2
    pl = M.plan([31, 33])
    assert (pl["ld"], pl["nt"], pl["nlines"], pl["tpl"], pl["sl"], pl["tab_words"]) == (1, 256, 31, 8, 5, 31 * 31)
    pl = M.plan([4096])
    assert (pl["tpl"], pl["sl"], pl["tab_words"]) == (1024, 4, 0)
    pl = M.plan([100])
    assert (pl["nt"], pl["tpl"], pl["sl"]) == (64, 64, 2)
    pl = M.plan([2048, 2])
    assert (pl["ld"], pl["nlines"], pl["tpl"], pl["sl"], pl["pitch"][1]) == (0, 2, 512, 4, 3)
    pl = M.plan([6, 6, 6, 6])
    assert (pl["nlines"], pl["tpl"], pl["sl"]) == (216, 4, 2)
    pl = M.plan([64, 64])
    assert (pl["tpl"], pl["sl"], pl["tab_words"]) == (16, 4, 64 * 65)


def _meshes_of(p, N):
    """Every admitted mesh shape of p dimensions with N nodes under the mixed-partial rule (m_0 = ... = m_{p-2} for
    p >= 3), each m_j >= 2."""
    if p == 1:
        return [[N]]
    if p == 2:
        return [[a, N // a] for a in range(2, N // 2 + 1) if N % a == 0]
    out = []
    a = 2
    while a ** (p - 1) * 2 <= N:
        if N % (a ** (p - 1)) == 0:
            out.append([a] * (p - 1) + [N // a ** (p - 1)])
        a += 1
    return out


def test_every_admitted_mesh_fits_the_plan_and_lds():
    """Every transformed dimension <= 64 points, nlines <= NT, a line's segments cover it, LDS <= 160 KiB for the loop
    with the most blocks and for the solve alone."""
    worst = 0
    for p in (1, 2, 3, 4):
        nb = max(S.n_blocks(p, o, w) for o in ("cpp", "py") for w in (True, False))
        cap = S.MAX_N4 if p == 4 else S.MAX_N
        for N in range(2 ** p, cap + 1):
            for m in _meshes_of(p, N):
                pl = M.plan(m)
                assert all(m[j] <= M.COS_MAX_T for j in range(p) if j != pl["ld"]), m
                assert pl["nlines"] * pl["tpl"] <= pl["nt"] and pl["tpl"] * pl["sl"] >= m[pl["ld"]], m
                assert pl["tpl"] & (pl["tpl"] - 1) == 0
                for nbk in range(1, nb + 1):
                    worst = max(worst, M.lds_bytes(m, nbk, True))
                    assert M.lds_bytes(m, nbk, True) <= M.LDS_LIMIT, (m, nbk)
                assert M.lds_bytes(m, 0, False) <= M.LDS_LIMIT
    print("largest loop LDS", worst)
    # the arithmetic bound behind it: sv + reductions + scan + the largest table + the z limit
    assert 8 * (4096 + 9 * 16 + 64 * 65 + M.COS_Z_LDS_WORDS) <= M.LDS_LIMIT


def gpu_loop_cases():
    """(m, order, weighted, pc) of the k_admm_cos runs of tests/test_gpu_small_cos.py."""
    out = []
    for m in S.SHAPES + M.EXTRA_SHAPES:
        out.append((m, "cpp", True, False))   # "I" cases under mode 1
        out.append((m, "cpp", True, True))    # "S" cases under mode 2
    for m in S.PATH_SHAPES:
        out.append((m, "cpp", True, True))
    return out


def test_gpu_cases_reach_every_dispatched_instantiation():
    c = _src("mvtv_small_cos.hip")
    disp = {(int(p), int(nt), z == "true") for p, nt, z in re.findall(r"MVTV_COS_GO\((\d), (\d+), (true|false)\);", c)}
    assert disp == M.reachable_loops()
    want = {f"k_admm_cos<{p}, {nt}, {'true' if z else 'false'}, {pc}>" for p, nt, z in disp for pc in ("true", "false")}
    got = {M.loop_name(m, pc, o, w) for m, o, w, pc in gpu_loop_cases()}
    assert got == want, sorted(want - got)
    solves = set(re.findall(r"go\((k_solve_cos<\d, \d+>)\)", c))
    assert solves == {f"k_solve_cos<{p}, {nt}>" for p in (1, 2, 3, 4) for nt in (64, 256, 1024)}
    assert {M.solve_name(m) for m in S.SHAPES} == solves
    # the existing kernel keeps its dispatch, and the new names stay out of the prefixes the CV test filters by
    assert not any(n.startswith(pre) for n in ("k_admm_cos", "k_solve_cos")
                   for pre in ("k_admm_small", "k_pcg", "k_gather", "k_edge", "k_cg3d"))


@pytest.mark.parametrize("wk", ["I", "S"])
def test_extra_shape_decisions_have_margin(wk):
    """The mesh this file adds to S.SHAPES for the GPU fits: its converged run's decisions sit >= 1e-6 from their
    thresholds, as tests/test_small_batch_host.py shows for the others, so the iteration count can be exact."""
    for m in M.EXTRA_SHAPES:
        res = S.slu_single((m, "cpp", True, wk))
        assert 2 <= res.iters < 3000
        assert S.margins(res.history) >= 1e-6, (res.iters, S.margins(res.history))


def _errors(m, order="cpp", weighted=True, plain_r=False, shift=1.0):
    rng = np.random.default_rng(sum(m) + len(m))
    b = rng.standard_normal(int(np.prod(m))) + 2.0
    deltas = S.deltas_of(m)
    o = 0 if order == "cpp" else 1
    fwd_ld, fwd_64 = SLD.forward_ld(m, b), SLD.forward_ld(m, b, np.float64)
    sym_ld = SLD.dtd_symbol_ld(m, deltas, o, weighted)
    sym_64 = SLD.dtd_symbol_ld(m, deltas, o, weighted, np.float64)
    out = []
    for sigma in SIGMAS:
        # (shift I + sigma A) x = b is (I + (sigma / shift) A) x = b / shift
        x_ld = SLD.solve_from_forward(fwd_ld, sym_ld, sigma / shift) / SLD.LD(shift)
        x_64 = SLD.solve_from_forward(fwd_64, sym_64, sigma / shift) / shift
        x = M.model_solve(m, deltas, sigma, b, shift=shift, order=order, weighted=weighted, plain_r=plain_r)
        scale = float(np.max(np.abs(x_ld)))
        e64 = float(np.max(np.abs(x_64 - x_ld))) / scale
        err = float(np.max(np.abs(x - x_ld))) / scale
        print(f"m={m} {order} w={weighted} sigma={sigma:g} plain={plain_r}: err {err:.2e}, e64 {e64:.2e}, "
              f"ratio {err / e64:.2f}")
        out.append((sigma, err, e64))
    return out


@pytest.mark.parametrize("m", S.SHAPES + M.EXTRA_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_model_matches_long_double(m):
    for sigma, err, e64 in _errors(m):
        assert e64 > 0.0
        assert err <= min(1e-12, 32.0 * e64), (m, sigma, err, e64)


@pytest.mark.parametrize("m", S.LAYOUT_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_model_matches_long_double_other_layouts(m):
    for order, weighted in S.LAYOUTS:
        if len(m) == 1 and order == "py" and weighted:
            continue
        for sigma, err, e64 in _errors(m, order, weighted):
            assert err <= min(1e-12, 32.0 * e64), (m, order, weighted, sigma, err, e64)


def test_model_with_a_shift():
    for m in ([100], [31, 33], [4, 4, 4]):
        for sigma, err, e64 in _errors(m, shift=0.37):
            assert err <= min(1e-12, 32.0 * e64), (m, sigma, err, e64)


@pytest.mark.parametrize("m", [[100], [1000], [4096]], ids=lambda m: str(m[0]))
def test_plain_double_r_misses_the_bound(m):
    """The teeth: r rounded to one double loses a relative 1e-16 / (1 - r) of the whole solve."""
    sigma, err, e64 = _errors(m, plain_r=True)[-1]
    assert sigma == 2e5 and err > min(1e-12, 32.0 * e64), (m, err, e64)
