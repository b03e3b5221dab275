"""The spectral solve on leading mesh dimensions longer than 4096: the two-pass cosine transform (k_dsc then k_dsr,
inverse k_dsr<true> then k_dsc<true>; mvtv_spectral.hip) through every layer that reaches it.

solve_spectral on meshes whose dimension 0 is longer than 4096 (the library's factorisation) and, with
``Problem.dct_split(dim, a)``, at lengths the one-workgroup kernels also take (every stride and factor shape at small
sizes; the same case after ``dct_split(dim, 0)`` runs the old kernels against the same reference and must launch none
of the new ones). Each case asserts from the launch log the exact new launches, names with template arguments, grids
and blocks, that tests/test_long_dct_host.py's ``plan`` (the transcription of launch_dct_split) predicts.

Forward error: test_gpu_dispatch.py's rule, unchanged. b = randn + 2, delta_j = (1 + 2e-4) / m_j (and one unit-weight
case), sigma in {0, 1e-3, 3.7, 2e5}: max|x_gpu - x_ld| <= min(1e-12, 32 e64) max|x_ld| with e64 the error of the
float64 pocketfft evaluation of the same formula against the long-double one (oracle/spectral_ld.py).

The ADMM loop: variant B under AUTO (6 fixed iterations and one converged run at tol = 1e-2) against
c_oracle.admm_rcpp_spectral; variants A and C on 8192 x 6 against oracle/variants_spectral.py, after the reference alone
has shown every decision >= 1e-6 from its threshold (lambda = 30 / 2, the values of test_gpu_long_lines.py: A 5
iterations, stopping margins 1.0 and adaptation margins >= 0.56; C 27 iterations at tol = 1e-2, stopping margins
>= 3.8e-3); W != I (AUTO picks the spectrally preconditioned PCG, whose M^-1 runs the split passes) against the C
oracle's Jacobi-PCG loop. Tolerances: the project's (iterations and rho exact, theta 1e-9 of max|theta_ref|, u 1e-9 of
max(1, max|u_ref|), r / s norms 1e-9 relative).

Still refused: a factor with a prime >= 11 or above 4096, dim = p - 1, a slab group with a long leading dimension.
"""
import functools
import os

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S
from test_long_dct_host import launches, plan, solve_launches

mv = pytest.importorskip("multivartv_amd")
c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd._lib import MVTV_BAD_ARG, MvtvError, launch_log  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402

pytestmark = pytest.mark.gpu

K_BOUND = 32.0
RTOL_DIRECT = 1e-12
SIGMAS = (0.0, 1e-3, 3.7, 2e5)
WORKERS = min(16, os.cpu_count() or 1)
NEW = ("k_dsc", "k_dsr")

# (name, mesh, {dim: a}, line_blocks, weighted); a = 0: the library's factorisation
AUTO = [("one_line_pair_pow2_factors", [8192, 2], {0: 0}, 0, True),
        ("unpaired_last_line", [8192, 3], {0: 0}, 0, True),
        ("grid_fills_the_chip", [8192, 600], {0: 0}, 0, True),
        ("radix_3_and_8", [4608, 16], {0: 0}, 0, True),
        ("radix_5_2_4", [5000, 8], {0: 0}, 0, True),
        ("radix_7_3_4", [8400, 4], {0: 0}, 0, True),
        ("odd_length", [6561, 2], {0: 0}, 0, True),
        ("both_factors_long", [1 << 20, 2], {0: 0}, 0, True),
        ("unit_weights", [8192, 3], {0: 0}, 0, False),
        # a factor of 4096: more than 64 KB of dynamic LDS (one row pair of 2 x 4097 slots; one column of 4097)
        ("one_row_pair_131_KB_of_lds", [8192, 2], {0: 2}, 0, True),
        ("one_column_of_4096", [8192, 3], {0: 4096}, 0, True)]
FORCED = [("smallest_pow2_split", [64, 2], {0: 8}, 0, True),
          ("smallest_pow2_split_odd_lines", [64, 3], {0: 8}, 0, True),
          ("factor_2_first", [48, 40], {0: 2}, 0, True),
          ("factor_2_second", [48, 40], {0: 24}, 0, True),
          ("non_pow2_factors_6x10", [60, 7], {0: 6}, 0, True),
          ("non_pow2_factors_7x15", [105, 4], {0: 7}, 0, True),
          ("factors_8x125", [1000, 9], {0: 8}, 0, True),
          ("factors_125x8", [1000, 9], {0: 125}, 0, True),
          ("long_line_few_lines", [4096, 5], {0: 64}, 0, True),
          ("split_and_blocked_line_solve", [64, 300], {0: 8}, 4, True),
          ("pow2_stride", [64, 64, 3], {1: 8}, 0, True),
          ("stride_48", [48, 48, 5], {0: 6, 1: 8}, 0, True),
          ("odd_lengths_and_stride", [45, 45, 4], {0: 5, 1: 9}, 0, True),
          ("long_stride_144", [12, 12, 12, 3], {2: 3}, 0, True),
          ("every_leading_dim_split", [12, 12, 12, 3], {0: 2, 1: 3, 2: 4}, 0, True)]
# every forced case also after dct_split(dim, 0): the one-workgroup kernels against the same reference
CASES = [c + (True,) for c in AUTO + FORCED] + [c + (False,) for c in FORCED]


def test_expected_shapes_of_the_named_cases():
    """What the named cases reach, from the plan alone (no GPU work)."""
    assert launches([8192, 2], 0) == [("k_dsc<false, true, false>", 3, 512), ("k_dsr<false, true>", 3, 512)]
    assert launches([8192, 3], 0, inverse=True) == [("k_dsr<true, true>", 5, 512), ("k_dsc<true, true, false>", 6, 512)]
    assert launches([8192, 600], 0, formb=True)[0] == ("k_dsc<false, true, true>", 900, 512)
    assert plan([1 << 20, 2], 0)["a"] == plan([1 << 20, 2], 0)["b"] == 1024
    assert launches([64, 64, 3], 1, 8)[0] == ("k_dsc<false, false, false>", 12 * 1, 512)
    assert [n for n, _, _ in solve_launches([12, 12, 12, 3], {0: 2, 1: 3, 2: 4})] == [
        "k_dsc<false, true, false>", "k_dsr<false, true>", "k_dsc<false, false, false>", "k_dsr<false, false>",
        "k_dsc<false, false, false>", "k_dsr<false, false>", "k_dsr<true, false>", "k_dsc<true, false, false>",
        "k_dsr<true, false>", "k_dsc<true, false, false>", "k_dsr<true, true>", "k_dsc<true, true, false>"]


@functools.lru_cache(maxsize=1)
def _case(name, split_on):
    """Everything one case's sigmas share, built once: the problem on the GPU, b, and the forward transforms and
    symbols of the long-double reference and of its float64 evaluation."""
    _, m, splits, blocks, weighted = next(c for c in AUTO + FORCED if c[0] == name)
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP, weighted=weighted)
    assert P.spectral_ok()
    for d, a in splits.items():
        P.dct_split(d, a)
        if not split_on:   # forced on, then back to automatic: the one-workgroup kernels again
            P.dct_split(d, 0)
    if blocks:
        P.line_blocks(blocks)
    ref = {}
    for key, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[key] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, "cpp", weighted, dtype))
    return P, b, ref


@pytest.mark.parametrize("name,split_on,sigma",
                         [(c[0], c[5], s) for c in CASES for s in SIGMAS],
                         ids=lambda v: str(v) if not isinstance(v, bool) else ("split" if v else "resident"))
def test_split_transform_forward_error(name, split_on, sigma):
    _, m, splits, blocks, weighted = next(c for c in AUTO + FORCED if c[0] == name)
    P, b, ref = _case(name, split_on)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    assert all(g[1:] == (1, 1) and bl[1:] == (1, 1) for _, g, bl in log)
    if split_on:
        assert new == solve_launches(m, splits), new
        if blocks:
            assert any(n.startswith("k_trib<1") for n, _, _ in log)
    else:
        assert not new and log, new
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    tag = f"{name} {'x'.join(map(str, m))} {'split' if split_on else 'resident'} sigma={sigma:g}"
    print(f"long dct {tag}: e64 {e64:.2e} gpu {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
    log_parity("long dct " + tag, e64=e64, err=err, ratio=err / max(e64, 1e-300),
               kernels=" | ".join(n for n, _, _ in log))
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


def test_every_dimension_long_has_only_the_split_tables():
    """4608 x 4100: no dimension has a resident transform (dim 0 split, dim 1 the blocked line solve), so the plan holds
    no length-m twiddle table at all. A constant is a fixed point of the solve whatever sigma (D 1 = 0), which needs no
    reference at 19 M nodes; the forward error of these kernels is the cases' above."""
    m = [4608, 4100]
    b = np.full(int(np.prod(m)), 2.5)
    with mv.Problem(m, b, deltas=[(1.0 + 2e-4) / v for v in m], order=mv.ORDER_CPP) as P:
        assert P.spectral_ok()
        with launch_log() as log:
            x = P.solve_spectral(3.7, b)
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    assert new == solve_launches(m, {0: 0}), new
    assert any(n.startswith("k_trib<1") for n, _, _ in log)
    assert float(np.max(np.abs(x - 2.5))) <= 1e-13 * 2.5


# ---- the ADMM loop -------------------------------------------------------------------------------------------------
LAM = 0.8


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize("fixed", [6, 0], ids=["fixed6", "converged"])
@pytest.mark.parametrize("m,splits", [([8192, 6], {}), ([48, 48, 5], {0: 6, 1: 8})], ids=["8192x6", "48x48x5"])
def test_variant_b_auto_takes_the_split_passes(m, splits, fixed):
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(y.size, y.mean())
    kw = dict(fixed_iters=fixed) if fixed else dict(tol=1e-2)
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert P.spectral_ok()
        for d, a in splits.items():
            P.dct_split(d, a)
        with launch_log() as log:
            tg, ug, rg, st = P.admm(LAM, th0, u=np.zeros(P.E), rho=LAM / 5, **kw)
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp_spectral(m, y, LAM, th, u, LAM / 5, deltas, workers=WORKERS, **kw)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    per_solve = solve_launches(m, splits or {0: 0}, formb=True)   # b formed on load by the first pass
    assert per_solve[0][0] == "k_dsc<false, true, true>"
    k = min(ref["iters"], 6)
    assert new[:k * len(per_solve)] == per_solve * k, new[:2 * len(per_solve)]
    assert st["iters"] == ref["iters"] and (fixed or ref["iters"] >= 10)
    assert rg == ref["rho"] and st["rho"] == ref["rho"]
    et, eu = _rel(tg, th), float(np.max(np.abs(ug - u)) / max(1.0, np.max(np.abs(u))))
    er = abs(st["r_norm"] - ref["r_norm"]) / ref["r_norm"]
    es = abs(st["s_norm"] - ref["s_norm"]) / ref["s_norm"]
    tag = "x".join(map(str, m))
    print(f"loop B {tag} fixed={fixed}: iters {ref['iters']} theta {et:.2e} u {eu:.2e} r {er:.2e} s {es:.2e}")
    log_parity(f"long dct loop B {tag} fixed={fixed}", theta=et, u=eu, r=er, s=es, iters=ref["iters"])
    assert et <= 1e-9 and eu <= 1e-9
    assert er <= 1e-9 and es <= 1e-9


@pytest.mark.parametrize("variant,lam,tol", [("A", 30.0, None), ("C", 2.0, 1e-2)], ids=["A", "C"])
def test_variants_a_and_c_on_a_long_leading_dimension(variant, lam, tol):
    from oracle import variants_spectral as V
    m = [8192, 6]
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    ymean = float(y.mean())
    th0 = np.full(y.size, ymean)
    kw = {} if tol is None else dict(tol=tol)
    fn = V.admm_cpp_spectral if variant == "A" else V.admm_py_spectral
    res = fn(m, y, lam, th0, ymean, deltas, order="cpp", weighted=True, **kw)
    # conditions on the reference alone: no decision of this run is a matter of rounding
    assert len(res.stop_margins) == res.iters + 1 and res.iters >= 2
    assert min(res.stop_margins) >= 1e-6, res.stop_margins
    if variant == "A":
        assert min(min(h["adapt_hi"], h["adapt_lo"]) for h in res.history) >= 1e-6, res.history
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        with launch_log() as log:
            th, u, rho, st = P.admm(lam, th0, u=None, rho=None, ymean=ymean,
                                    variant=mv.VARIANT_CPP if variant == "A" else mv.VARIANT_PY, **kw)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL
    assert [n for n, _, _ in log].count("k_dsc<false, true, true>") >= res.iters
    assert st["iters"] == res.iters and rho == res.rho
    et = _rel(th, res.theta)
    eu = float(np.max(np.abs(u - res.u)) / max(1.0, np.max(np.abs(res.u))))
    last = res.history[-1]
    log_parity(f"long dct loop {variant} 8192x6", theta=et, u=eu, iters=res.iters)
    assert et <= 1e-9 and eu <= 1e-9
    assert abs(st["dtheta_max"] - last["dtheta_max"]) <= max(1e-9 * abs(last["dtheta_max"]), 1e-12)


def test_w_mask_auto_takes_the_spectral_preconditioner():
    """W != I (3 in 5 nodes observed) on 8192 x 12: AUTO reports PCG_SPECTRAL, its M^-1 runs the split passes."""
    m = [8192, 12]
    y = towers(m)
    W = (np.random.default_rng(len(m)).permutation(y.size) % 5 < 3).astype(float)
    oty = W * y
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(W.size, oty.sum() / W.sum())
    lam, rho0, iters = 0.5, 0.1, 3
    with mv.Problem(m, oty, wdiag=W, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert not P.spectral_ok()
        with launch_log() as log:
            tg, ug, rg, st = P.admm(lam, th0, u=np.zeros(P.E), rho=rho0, fixed_iters=iters, pcg_rtol=1e-13)
    assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["pcg_unconverged"] == 0
    names = [n for n, _, _ in log]
    assert names.count("k_dsc<false, true, false>") >= iters, sorted(set(names))
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp(m, oty, lam, th, u, rho0, deltas, W=W, fixed_iters=iters, pcg_rtol=1e-13)
    assert rg == ref["rho"]
    et = _rel(tg, th)
    log_parity("long dct W mask 8192x12", theta=et, pcg_iters=int(st["pcg_iters"]))
    assert et <= 1e-9


# ---- argument checks and what stays refused ------------------------------------------------------------------------
@pytest.mark.parametrize("m,dim,a", [([88, 4], 0, 11), ([88, 4], 0, 8), ([8192, 4], 0, 3), ([8192, 4], 0, 1),
                                     ([8192, 4], 0, -2), ([8192, 4], 0, 8192), ([64, 4], 1, 2), ([64, 4], -1, 2),
                                     ([16, 16, 40], 2, 2), ([6 * 4099, 2], 0, 6)],
                         ids=["prime_11_factor", "prime_11_cofactor", "not_a_divisor", "a_is_1", "negative",
                              "a_is_m", "last_dimension", "negative_dim", "last_dimension_3d", "not_a_spectral_mesh"])
def test_dct_split_argument_checks(m, dim, a):
    y = np.ones(int(np.prod(m)))
    with mv.Problem(m, y, deltas=[1.0 / v for v in m]) as P:
        with pytest.raises(MvtvError) as e:
            P.dct_split(dim, a)
        assert e.value.status == MVTV_BAD_ARG
        if P.spectral_ok():
            P.dct_split(0, 0)


def test_a_cofactor_above_4096_is_refused():
    y = np.ones(1 << 15)
    with mv.Problem([1 << 14, 2], y, deltas=[1.0, 1.0]) as P:
        assert P.spectral_ok()
        with pytest.raises(MvtvError) as e:
            P.dct_split(0, 2)   # 2 x 8192
        assert e.value.status == MVTV_BAD_ARG
        P.dct_split(0, 4)
        P.dct_split(0, 0)


def test_slab_group_with_a_long_leading_dimension_is_still_refused():
    from multivartv_amd import slab
    m = [8192, 8]
    y = towers(m)
    with pytest.raises(MvtvError) as e:
        slab.run_local_group(m, y, [(1.0 + 2e-4) / v for v in m], 1.0, 2, fixed_iters=1)
    assert e.value.status == MVTV_BAD_ARG
