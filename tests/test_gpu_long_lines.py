"""The spectral solve on a last mesh dimension of any length: the blocked line solve (k_trib with k_trib_iface or
k_blk_iface<1> for p >= 2, k_tri1 with k_blk_iface<16> for p = 1; mvtv_spectral.hip) through every
layer that reaches it.

solve_spectral on meshes whose last dimension is longer than 4096 (automatic block count) and, with
``Problem.line_blocks(k)``, at lengths the one-workgroup kernels also solve (every tile and the uneven / ragged block
and segment shapes at small sizes; the same case with ``line_blocks(0)`` runs the old kernels against the same
reference). Each case asserts from the launch log that the three new launches ran at the expected grids and blocks
(the shapes of tests/test_long_lines_host.py's ``plan``, the transcription of line_blocks_plan).

Forward error: test_gpu_dispatch.py's rule, unchanged. b = randn + 2, delta_j = (1 + 2e-4) / m_j (and one unit-weight
case), sigma in {0, 1e-3, 3.7, 2e5}: max|x_gpu - x_ld| <= min(1e-12, 32 e64) max|x_ld| with e64 the error of the
float64 pocketfft evaluation of the same formula against the long-double one (oracle/spectral_ld.py).

The ADMM loop: variant B under AUTO (6 fixed iterations and one converged run at tol = 1e-2, 30 - 43 iterations)
against c_oracle.admm_rcpp_spectral; variants A and C on the 1-D mesh against oracle/variants_spectral.py, after the
reference alone has shown every decision >= 1e-6 from its threshold; W != I (AUTO picks the spectrally preconditioned
PCG, whose M^-1 runs the blocked solve) against the C oracle's Jacobi-PCG loop. Tolerances: the project's (iterations
and rho exact, theta 1e-9 of max|theta_ref|, u 1e-9 of max(1, max|u_ref|), r / s norms 1e-9 relative).

Still refused: a leading dimension above 4096, a one-rank slab with a last dimension above 4096, more blocks than rows.
"""
import functools
import os

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S
from test_long_lines_host import WAVE_IFACE_BELOW, cdiv, plan

mv = pytest.importorskip("multivartv_amd")
c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd._lib import MVTV_BAD_ARG, MvtvError, launch_log  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402

pytestmark = pytest.mark.gpu

K_BOUND = 32.0
RTOL_DIRECT = 1e-12
SIGMAS = (0.0, 1e-3, 3.7, 2e5)
WORKERS = min(16, os.cpu_count() or 1)
NEW = ("k_trib", "k_tri1", "k_blk_iface")

# (mesh, blocks, weighted): blocks 0 = automatic
AUTO = [([4097], 0, True), ([4099], 0, True), ([8192], 0, True), ([65537], 0, True), ([1 << 20], 0, True),
        ([64, 4100], 0, True), ([1024, 4099], 0, True), ([2, 5000], 0, True), ([3, 4100], 0, True),
        ([16, 16, 4100], 0, True), ([8, 8, 8, 4100], 0, True), ([4099], 0, False), ([48, 4100], 0, False)]
FORCED = [([1000], 3, True), ([37], 2, True), ([64, 64, 300], 4, True), ([128, 128, 135], 2, True),
          ([8, 8, 8, 100], 3, True), ([4096, 67], 2, True)]
# every forced case also with line_blocks(0): the one-workgroup kernels against the same reference
CASES = AUTO + FORCED + [(m, -1, w) for m, _, w in FORCED]


def _id(v):
    if isinstance(v, (tuple, list)):
        return "x".join(str(x) for x in v)
    return str(v)


def expected_launches(m, blocks):
    """[(kernel, grid, block)] of the blocked solve's three launches on mesh m (line_blocks_plan's shapes)."""
    nblk, tq, sl, nseg = plan(list(m), blocks)
    if len(m) == 1:
        return [("k_tri1<1, false>", nblk, 256), ("k_blk_iface<16>", 1, 1024), ("k_tri1<3, false>", nblk, 256)]
    nlines = int(np.prod(m[:-1]))
    ns = {64: 8, 16: 32, 4: 64}[tq]
    grid = cdiv(nlines, tq) * nblk
    iface = ("k_blk_iface<1>", nlines, 64) if nlines < WAVE_IFACE_BELOW else ("k_trib_iface", cdiv(nlines, 256), 256)
    return [(f"k_trib<1, 32, {tq}, {ns}>", grid, tq * nseg), iface, (f"k_trib<3, 32, {tq}, {ns}>", grid, tq * nseg)]


def test_expected_shapes_of_the_named_cases():
    """The block and segment shapes the issue names, from the plan alone (no GPU work)."""
    # 75-row blocks: 32 + 32 + 11; 67- / 68-row blocks
    assert expected_launches([64, 64, 300], 4)[0] == ("k_trib<1, 32, 64, 8>", 64 * 4, 64 * 3)
    assert expected_launches([128, 128, 135], 2)[0] == ("k_trib<1, 32, 64, 8>", 256 * 2, 64 * 3)
    assert expected_launches([8, 8, 8, 100], 3)[0] == ("k_trib<1, 32, 16, 32>", 32 * 3, 16 * 2)
    assert expected_launches([4096, 67], 2)[0] == ("k_trib<1, 32, 16, 32>", 256 * 2, 16 * 2)
    assert expected_launches([2, 5000], 0)[0][0] == "k_trib<1, 32, 4, 64>"
    assert expected_launches([1000], 3)[0] == ("k_tri1<1, false>", 3, 256)
    assert expected_launches([1 << 20], 0)[0] == ("k_tri1<1, false>", 256, 256)


@functools.lru_cache(maxsize=1)
def _case(m, blocks, weighted):
    """Everything one case's sigmas share, built once: the problem on the GPU, b, and the forward transforms and
    symbols of the long-double reference and of its float64 evaluation."""
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP, weighted=weighted)
    assert P.spectral_ok()
    if blocks > 0:
        P.line_blocks(blocks)
    elif blocks < 0:   # forced on, then back to automatic: the one-workgroup kernels again
        P.line_blocks(2)
        P.line_blocks(0)
    ref = {}
    for name, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[name] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, "cpp", weighted, dtype))
    return P, b, ref


@pytest.mark.parametrize("m,blocks,weighted,sigma", [(tuple(m), k, w, s) for m, k, w in CASES for s in SIGMAS], ids=_id)
def test_blocked_solve_forward_error(m, blocks, weighted, sigma):
    P, b, ref = _case(m, blocks, weighted)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    assert all(g[1:] == (1, 1) and bl[1:] == (1, 1) for _, g, bl in log)
    if blocks >= 0:
        assert new == expected_launches(m, blocks), new
    else:
        assert not new and log, new
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    tag = f"{_id(m)} blocks={blocks}{'' if weighted else ' unit weights'} sigma={sigma:g}"
    print(f"long lines {tag}: e64 {e64:.2e} gpu {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
    log_parity("long lines " + tag, e64=e64, err=err, ratio=err / max(e64, 1e-300),
               kernels=" | ".join(n for n, _, _ in log))
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


# ---- the ADMM loop -------------------------------------------------------------------------------------------------
LOOP_MESHES = [[5000], [48, 4100], [12, 12, 4100]]
LAM = 0.8


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize("fixed", [6, 0], ids=["fixed6", "converged"])
@pytest.mark.parametrize("m", LOOP_MESHES, ids=_id)
def test_variant_b_auto_takes_the_spectral_solve(m, fixed):
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(y.size, y.mean())
    kw = dict(fixed_iters=fixed) if fixed else dict(tol=1e-2)
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert P.spectral_ok()
        with launch_log() as log:
            tg, ug, rg, st = P.admm(LAM, th0, u=np.zeros(P.E), rho=LAM / 5, **kw)
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp_spectral(m, y, LAM, th, u, LAM / 5, deltas, workers=WORKERS, **kw)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL
    names = [n for n, _, _ in log]
    first = "k_tri1<1, true>" if len(m) == 1 else expected_launches(m, 0)[0][0]   # p = 1: b formed on load
    assert names.count(first) >= min(ref["iters"], 6), sorted(set(names))
    assert st["iters"] == ref["iters"] and (fixed or ref["iters"] >= 20)
    assert rg == ref["rho"] and st["rho"] == ref["rho"]
    et, eu = _rel(tg, th), float(np.max(np.abs(ug - u)) / max(1.0, np.max(np.abs(u))))
    er = abs(st["r_norm"] - ref["r_norm"]) / ref["r_norm"]
    es = abs(st["s_norm"] - ref["s_norm"]) / ref["s_norm"]
    print(f"loop B {_id(m)} fixed={fixed}: iters {ref['iters']} theta {et:.2e} u {eu:.2e} r {er:.2e} s {es:.2e}")
    log_parity(f"long lines loop B {_id(m)} fixed={fixed}", theta=et, u=eu, r=er, s=es, iters=ref["iters"])
    assert et <= 1e-9 and eu <= 1e-9
    assert er <= 1e-9 and es <= 1e-9


@pytest.mark.parametrize("variant,lam,tol", [("A", 30.0, None), ("C", 2.0, 1e-2)], ids=["A", "C"])
def test_variants_a_and_c_on_a_long_line(variant, lam, tol):
    from oracle import variants_spectral as V
    m = [5000]
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
    assert [n for n, _, _ in log].count("k_tri1<1, true>") >= res.iters
    assert st["iters"] == res.iters and rho == res.rho
    et = _rel(th, res.theta)
    eu = float(np.max(np.abs(u - res.u)) / max(1.0, np.max(np.abs(res.u))))
    last = res.history[-1]
    log_parity(f"long lines loop {variant} 5000", theta=et, u=eu, iters=res.iters)
    assert et <= 1e-9 and eu <= 1e-9
    assert abs(st["dtheta_max"] - last["dtheta_max"]) <= max(1e-9 * abs(last["dtheta_max"]), 1e-12)


def test_w_mask_auto_takes_the_spectral_preconditioner():
    """W != I (3 in 5 nodes observed) on 48 x 4100: AUTO reports PCG_SPECTRAL, its M^-1 runs the blocked solve."""
    m = [48, 4100]
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
    assert names.count(expected_launches(m, 0)[0][0]) >= iters, sorted(set(names))
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp(m, oty, lam, th, u, rho0, deltas, W=W, fixed_iters=iters, pcg_rtol=1e-13)
    assert rg == ref["rho"]
    et = _rel(tg, th)
    log_parity("long lines W mask 48x4100", theta=et, pcg_iters=int(st["pcg_iters"]))
    assert et <= 1e-9


# ---- still refused -------------------------------------------------------------------------------------------------
def test_leading_dimension_above_4096_is_still_refused():
    m = [4100, 4100]
    y = np.ones(int(np.prod(m)))
    with mv.Problem(m, y, deltas=[1.0 / v for v in m]) as P:
        assert not P.spectral_ok()
        with pytest.raises(MvtvError) as e:
            P.admm(1.0, y, u=np.zeros(P.E), rho=0.2, fixed_iters=1, theta_solver=mv.SOLVER_SPECTRAL)
        assert e.value.status == MVTV_BAD_ARG
        with pytest.raises(MvtvError) as e:
            P.line_blocks(4)
        assert e.value.status == MVTV_BAD_ARG


def test_one_rank_slab_with_a_long_last_dimension_is_still_refused():
    from multivartv_amd import slab
    m = [8, 4100]
    y = towers(m)
    with pytest.raises(MvtvError) as e:
        slab.run_local_group(m, y, [(1.0 + 2e-4) / v for v in m], 1.0, 1, fixed_iters=1)
    assert e.value.status == MVTV_BAD_ARG


def test_line_blocks_argument_checks():
    for m, bad in (([37], (38, 1, -1)), ([16, 16, 40], (41, 1)), ([10000], (2,)), ([16, 5000], (2,))):
        y = np.ones(int(np.prod(m)))
        with mv.Problem(m, y, deltas=[1.0 / v for v in m]) as P:
            for k in bad:   # more blocks than rows; 1; negative; a block longer than a workgroup's segments
                with pytest.raises(MvtvError) as e:
                    P.line_blocks(k)
                assert e.value.status == MVTV_BAD_ARG, (m, k)
            P.line_blocks(m[-1])   # one row per block is a valid shape
            P.line_blocks(0)
