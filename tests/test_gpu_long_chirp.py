"""The spectral solve on leading mesh dimensions of any length, opt-in: the chirp-z cosine transform (k_chc, k_chr,
k_cho, both directions; mvtv_spectral.hip) through every layer that reaches it.

A freshly created problem behaves as before: 4099 x 2 is refused. ``Problem.dct_chirp(dim)`` (or MVTV_DCT_CHIRP=1 at
creation) switches the transform on along a dimension and re-evaluates the mesh gate; ``dct_chirp(dim, a, b)`` forces
the convolution length M = a b at any m, which is how every stride, factor shape and radix is reached at small sizes
(the same case after ``dct_chirp(dim, 0, 0)`` runs the resident kernels against the same reference and must launch none
of the new ones). Each case asserts from the launch log the exact new launches, names with template arguments, grids
and blocks, that tests/test_long_chirp_host.py's ``plan`` (the transcription of launch_dct_chirp) predicts.

Forward error: test_gpu_dispatch.py's rule, unchanged. b = randn + 2, delta_j = (1 + 2e-4) / m_j (and one unit-weight
case), sigma in {0, 1e-3, 3.7, 2e5}: max|x_gpu - x_ld| <= min(1e-12, 32 e64) max|x_ld| with e64 the error of the
float64 pocketfft evaluation of the same formula against the long-double one (oracle/spectral_ld.py).

The ADMM loop: variant B under AUTO on 4099 x 6 (6 fixed iterations and one converged run at tol = 1e-2) against
c_oracle.admm_rcpp_spectral; variants A and C on 4099 x 6 against oracle/variants_spectral.py at lambda = 30 / 2, after
the reference alone has shown every decision >= 1e-6 from its threshold; W != I on 4099 x 12 (AUTO picks the spectrally
preconditioned PCG, whose M^-1 runs the chirp passes) against the C oracle's Jacobi-PCG loop. Tolerances: the project's
(iterations and rho exact, theta 1e-9 of max|theta_ref|, u 1e-9 of max(1, max|u_ref|), r / s norms 1e-9 relative).
"""
import functools
import os

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S
from test_long_chirp_host import chirp_auto, solve_launches

mv = pytest.importorskip("multivartv_amd")
c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd._lib import MVTV_BAD_ARG, MvtvError, launch_log  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402

pytestmark = pytest.mark.gpu

K_BOUND = 32.0
RTOL_DIRECT = 1e-12
SIGMAS = (0.0, 1e-3, 3.7, 2e5)
WORKERS = min(16, os.cpu_count() or 1)
NEW = ("k_chc", "k_chr", "k_cho")

# (name, mesh, {dim: (a, b) or None for the library's}, {dim: a} of dct_split, line_blocks, weighted)
AUTO = [("prime_length_one_line_pair", [4099, 2], {0: None}, {}, 0, True),
        ("unpaired_last_line", [4099, 3], {0: None}, {}, 0, True),
        ("unit_weights", [4099, 3], {0: None}, {}, 0, False),
        ("grid_fills_the_chip", [4100, 600], {0: None}, {}, 0, True),
        ("camera_frame_length", [8256, 4], {0: None}, {}, 0, True),
        ("twice_a_prime", [8198, 2], {0: None}, {}, 0, True),
        ("convolution_of_131220", [65537, 2], {0: None}, {}, 0, True),
        ("no_resident_dimension", [4100, 4100], {0: None}, {}, 0, True),
        # a factor of 4096: more than 64 KB of dynamic LDS (one row of 4097 slots; one orbit of 2 x 4097)
        ("one_row_of_4096", [4099, 2], {0: (3, 4096)}, {}, 0, True),
        ("one_orbit_131_KB_of_lds", [4099, 2], {0: (4096, 3)}, {}, 0, True)]
FORCED = [("exactly_2m_minus_1", [23, 2], {0: (5, 9)}, {}, 0, True),
          ("factors_6x8", [22, 2], {0: (6, 8)}, {}, 0, True),
          ("factors_6x8_odd_lines", [22, 3], {0: (6, 8)}, {}, 0, True),
          ("factors_5x15", [37, 4], {0: (5, 15)}, {}, 0, True),
          ("factors_8x10", [37, 4], {0: (8, 10)}, {}, 0, True),
          ("factor_2_first", [13, 40], {0: (2, 16)}, {}, 0, True),
          ("factor_2_second", [13, 40], {0: (16, 2)}, {}, 0, True),
          ("smooth_m", [100, 7], {0: (10, 20)}, {}, 0, True),
          ("powers_of_two", [64, 2], {0: (8, 16)}, {}, 0, True),
          ("chirp_and_blocked_line_solve", [22, 300], {0: (6, 8)}, {}, 4, True),
          ("stride_22_dim_1_alone", [22, 22, 3], {1: (6, 8)}, {}, 0, True),
          ("stride_22_dims_0_and_1", [22, 22, 3], {0: (6, 8), 1: (5, 9)}, {}, 0, True),
          ("odd_stride", [45, 45, 4], {0: (9, 10), 1: (7, 14)}, {}, 0, True),
          ("stride_121_dim_2_alone", [11, 11, 11, 3], {2: (3, 7)}, {}, 0, True),
          ("every_leading_dim", [11, 11, 11, 3], {0: (3, 7), 1: (4, 6), 2: (5, 5)}, {}, 0, True),
          ("split_and_chirp_together", [24, 24, 3], {1: (6, 8)}, {0: 4}, 0, True)]
# every forced case also after dct_chirp(dim, 0, 0): the resident kernels against the same reference
CASES = [c + (True,) for c in AUTO + FORCED] + [c + (False,) for c in FORCED]


@functools.lru_cache(maxsize=1)
def _case(name, chirp_on):
    """Everything one case's sigmas share, built once: the problem on the GPU, b, and the forward transforms and
    symbols of the long-double reference and of its float64 evaluation."""
    _, m, chirps, splits, blocks, weighted = next(c for c in AUTO + FORCED if c[0] == name)
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP, weighted=weighted)
    assert P.spectral_ok() == all(v <= 4096 for v in m[:-1])
    for d, ab in chirps.items():
        P.dct_chirp(d, *(ab or (-1, 0)))
        assert P.dct_chirp_factors(d) == (ab or chirp_auto(m[d]))
        if not chirp_on:   # forced on, then off: the one-workgroup kernels again
            P.dct_chirp(d, 0, 0)
            assert P.dct_chirp_factors(d) == (0, 0)
    assert P.spectral_ok()
    for d, a in splits.items():
        P.dct_split(d, a)
    if blocks:
        P.line_blocks(blocks)
    ref = {}
    for key, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[key] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, "cpp", weighted, dtype))
    return P, b, ref


@pytest.mark.parametrize("name,chirp_on,sigma",
                         [(c[0], c[6], s) for c in CASES for s in SIGMAS],
                         ids=lambda v: str(v) if not isinstance(v, bool) else ("chirp" if v else "resident"))
def test_chirp_transform_forward_error(name, chirp_on, sigma):
    _, m, chirps, splits, blocks, weighted = next(c for c in AUTO + FORCED if c[0] == name)
    P, b, ref = _case(name, chirp_on)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    assert all(g[1:] == (1, 1) and bl[1:] == (1, 1) for _, g, bl in log)
    if chirp_on:
        assert new == solve_launches(m, chirps), new
        if blocks or m[-1] > 4096:
            assert any(n.startswith("k_trib<1") for n, _, _ in log)
        if splits:
            assert any(n.startswith("k_dsc<") for n, _, _ in log)
    else:
        assert not new and log, new
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    tag = f"{name} {'x'.join(map(str, m))} {'chirp' if chirp_on else 'resident'} sigma={sigma:g}"
    print(f"long chirp {tag}: e64 {e64:.2e} gpu {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
    log_parity("long chirp " + tag, e64=e64, err=err, ratio=err / max(e64, 1e-300),
               kernels=" | ".join(n for n, _, _ in log))
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


# ---- the default is unchanged, and the switch -------------------------------------------------------------------------
def _oracle_check(P, m, y, deltas, lam=0.8, iters=3):
    """An AUTO run on the Jacobi-PCG loop against the C oracle's."""
    th0 = np.full(y.size, y.mean())
    tg, ug, rg, st = P.admm(lam, th0, u=np.zeros(P.E), rho=lam / 5, fixed_iters=iters, pcg_rtol=1e-13)
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp(m, y, lam, th, u, lam / 5, deltas, fixed_iters=iters, pcg_rtol=1e-13)
    assert rg == ref["rho"]
    assert float(np.max(np.abs(tg - th))) <= 1e-9 * float(np.max(np.abs(th)))
    return st


def test_default_is_unchanged_and_the_switch_goes_both_ways():
    m = [4099, 2]
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert not P.spectral_ok() and P.dct_chirp_factors(0) == (0, 0)
        assert _oracle_check(P, m, y, deltas)["theta_solver"] == mv.SOLVER_PCG
        P.dct_chirp(0, -1)
        assert P.spectral_ok() and P.dct_chirp_factors(0) == (84, 98)
        th0 = np.full(y.size, y.mean())
        with launch_log() as log:
            _, _, _, st = P.admm(0.8, th0, u=np.zeros(P.E), rho=0.16, fixed_iters=2)
        assert st["theta_solver"] == mv.SOLVER_SPECTRAL
        assert [n for n, _, _ in log].count("k_chc<false, true, true>") == 2
        P.line_blocks(2)          # the calls that need a spectral mesh work now
        P.line_blocks(0)
        P.dct_chirp(0, 0, 0)
        assert not P.spectral_ok()
        with pytest.raises(MvtvError) as e:
            P.solve_spectral(1.0, y)
        assert e.value.status == MVTV_BAD_ARG
        with pytest.raises(MvtvError) as e:
            P.line_blocks(2)
        assert e.value.status == MVTV_BAD_ARG
        with launch_log() as log:
            st = _oracle_check(P, m, y, deltas)
        assert st["theta_solver"] == mv.SOLVER_PCG
        assert not [n for n, _, _ in log if n.startswith(NEW)]


def test_off_gives_everything_back_and_on_again_rebuilds_it():
    """4099 x 4100: no dimension has a resident transform, so the spectral period owns the chirp scratch and the blocked
    line solve's buffers. Off releases them (the mesh is refused, line_blocks cannot reach them); on again must rebuild
    both. A constant is a fixed point of the solve whatever sigma (D 1 = 0), which needs no reference at 16.8 M nodes;
    the forward error of these kernels is the cases' above."""
    m = [4099, 4100]
    b = np.full(int(np.prod(m)), 2.5)
    with mv.Problem(m, b, deltas=[(1.0 + 2e-4) / v for v in m], order=mv.ORDER_CPP) as P:
        for _ in range(2):
            assert not P.spectral_ok()
            P.dct_chirp(0)
            assert P.spectral_ok() and P.dct_chirp_factors(0) == (84, 98)
            with launch_log() as log:
                x = P.solve_spectral(3.7, b)
            new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
            assert new == solve_launches(m, {0: None}), new
            assert any(n.startswith("k_trib<1") for n, _, _ in log)
            assert float(np.max(np.abs(x - 2.5))) <= 1e-13 * 2.5
            P.dct_chirp(0, 0, 0)
            with pytest.raises(MvtvError) as e:
                P.solve_spectral(3.7, b)
            assert e.value.status == MVTV_BAD_ARG


def test_environment_variable_switches_a_new_problem_on(monkeypatch):
    m = [4099, 2]
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    monkeypatch.setenv("MVTV_DCT_CHIRP", "1")
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert P.spectral_ok() and P.dct_chirp_factors(0) == (84, 98)
    with mv.Problem([8192, 2], np.ones(16384), deltas=[1.0, 1.0]) as P:   # a two-pass factorisation exists: split
        assert P.spectral_ok() and P.dct_chirp_factors(0) == (0, 0)
    monkeypatch.setenv("MVTV_DCT_CHIRP", "0")
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert not P.spectral_ok()
    monkeypatch.delenv("MVTV_DCT_CHIRP")
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert not P.spectral_ok()


# ---- the ADMM loop -------------------------------------------------------------------------------------------------
LAM = 0.8


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


@pytest.mark.parametrize("fixed", [6, 0], ids=["fixed6", "converged"])
def test_variant_b_auto_takes_the_chirp_passes(fixed):
    m = [4099, 6]
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(y.size, y.mean())
    kw = dict(fixed_iters=fixed) if fixed else dict(tol=1e-2)
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        P.dct_chirp(0)
        assert P.spectral_ok()
        with launch_log() as log:
            tg, ug, rg, st = P.admm(LAM, th0, u=np.zeros(P.E), rho=LAM / 5, **kw)
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp_spectral(m, y, LAM, th, u, LAM / 5, deltas, workers=WORKERS, **kw)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL
    new = [(n, g[0], bl[0]) for n, g, bl in log if n.startswith(NEW)]
    per_solve = solve_launches(m, {0: None}, formb=True)   # b formed on load by the first pass
    assert per_solve[0][0] == "k_chc<false, true, true>"
    k = min(ref["iters"], 6)
    assert new[:k * len(per_solve)] == per_solve * k, new[:2 * len(per_solve)]
    # every solve of the run, not only the first ones: one b-forming column launch each, the whole log solve by solve
    # (iterations enqueued ahead of a converged run's stop return at once but are launched: whole solves too)
    assert [n for n, _, _ in new].count("k_chc<false, true, true>") >= ref["iters"]
    assert len(new) % len(per_solve) == 0 and new == per_solve * (len(new) // len(per_solve))
    if fixed:
        assert len(new) == fixed * len(per_solve)
    assert st["iters"] == ref["iters"] and (fixed or ref["iters"] >= 10)
    assert rg == ref["rho"] and st["rho"] == ref["rho"]
    et, eu = _rel(tg, th), float(np.max(np.abs(ug - u)) / max(1.0, np.max(np.abs(u))))
    er = abs(st["r_norm"] - ref["r_norm"]) / ref["r_norm"]
    es = abs(st["s_norm"] - ref["s_norm"]) / ref["s_norm"]
    print(f"loop B 4099x6 fixed={fixed}: iters {ref['iters']} theta {et:.2e} u {eu:.2e} r {er:.2e} s {es:.2e}")
    log_parity(f"long chirp loop B 4099x6 fixed={fixed}", theta=et, u=eu, r=er, s=es, iters=ref["iters"])
    assert et <= 1e-9 and eu <= 1e-9
    assert er <= 1e-9 and es <= 1e-9


@pytest.mark.parametrize("variant,lam,tol", [("A", 30.0, None), ("C", 2.0, 1e-2)], ids=["A", "C"])
def test_variants_a_and_c_on_a_prime_leading_dimension(variant, lam, tol):
    """4099 x 6 at the lambda of test_gpu_long_dct.py (30 and 2). The reference alone, before any GPU work: A 5
    iterations, stopping margins 1.0, adaptation margins >= 0.56; C 23 iterations at tol = 1e-2, stopping margins
    >= 3.4e-2 (asserted below, >= 1e-6 each)."""
    from oracle import variants_spectral as V
    m = [4099, 6]
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
        P.dct_chirp(0)
        with launch_log() as log:
            th, u, rho, st = P.admm(lam, th0, u=None, rho=None, ymean=ymean,
                                    variant=mv.VARIANT_CPP if variant == "A" else mv.VARIANT_PY, **kw)
    assert st["theta_solver"] == mv.SOLVER_SPECTRAL
    assert [n for n, _, _ in log].count("k_chc<false, true, true>") >= res.iters
    assert st["iters"] == res.iters and rho == res.rho
    et = _rel(th, res.theta)
    eu = float(np.max(np.abs(u - res.u)) / max(1.0, np.max(np.abs(res.u))))
    last = res.history[-1]
    log_parity(f"long chirp loop {variant} 4099x6", theta=et, u=eu, iters=res.iters)
    assert et <= 1e-9 and eu <= 1e-9
    assert abs(st["dtheta_max"] - last["dtheta_max"]) <= max(1e-9 * abs(last["dtheta_max"]), 1e-12)


def test_w_mask_auto_takes_the_spectral_preconditioner():
    """W != I (3 in 5 nodes observed) on 4099 x 12: AUTO reports PCG_SPECTRAL, its M^-1 runs the chirp passes."""
    m = [4099, 12]
    y = towers(m)
    W = (np.random.default_rng(len(m)).permutation(y.size) % 5 < 3).astype(float)
    oty = W * y
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(W.size, oty.sum() / W.sum())
    lam, rho0, iters = 0.5, 0.1, 3
    with mv.Problem(m, oty, wdiag=W, deltas=deltas, order=mv.ORDER_CPP) as P:
        P.dct_chirp(0)
        assert not P.spectral_ok()
        with launch_log() as log:
            tg, ug, rg, st = P.admm(lam, th0, u=np.zeros(P.E), rho=rho0, fixed_iters=iters, pcg_rtol=1e-13)
    assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["pcg_unconverged"] == 0
    names = [n for n, _, _ in log]
    assert names.count("k_chc<false, true, false>") >= iters, sorted(set(names))
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp(m, oty, lam, th, u, rho0, deltas, W=W, fixed_iters=iters, pcg_rtol=1e-13)
    assert rg == ref["rho"]
    et = _rel(tg, th)
    log_parity("long chirp W mask 4099x12", theta=et, pcg_iters=int(st["pcg_iters"]))
    assert et <= 1e-9


# ---- argument checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,dim,a,b", [([22, 4], 0, 4, 10), ([22, 4], 0, 11, 8), ([22, 4], 0, 8, 11),
                                       ([22, 4], 0, 8192, 2), ([22, 4], 0, 2, 8192), ([22, 4], 0, 1, 64),
                                       ([22, 4], 0, 64, 1), ([22, 4], 0, 0, 8), ([22, 4], 0, -2, 8),
                                       ([22, 4], 1, 6, 8), ([22, 4], -1, 6, 8), ([16, 16, 40], 2, 6, 8),
                                       ([22, 4], 1, -1, 0)],
                         ids=["m_40_below_43", "prime_11_factor", "prime_11_cofactor", "factor_above_4096",
                              "cofactor_above_4096", "a_is_1", "b_is_1", "a_0_b_not", "negative", "last_dimension",
                              "negative_dim", "last_dimension_3d", "last_dimension_auto"])
def test_dct_chirp_argument_checks(m, dim, a, b):
    y = np.ones(int(np.prod(m)))
    with mv.Problem(m, y, deltas=[1.0 / v for v in m]) as P:
        with pytest.raises(MvtvError) as e:
            P.dct_chirp(dim, a, b)
        assert e.value.status == MVTV_BAD_ARG
        assert P.spectral_ok() and P.dct_chirp_factors(0) == (0, 0)
        P.dct_chirp(0, 6, 8)      # 48 >= 43: the problem is still usable
        P.dct_chirp(0, 0, 0)


def test_forced_split_and_chirp_exclude_each_other_in_both_orders():
    y = np.ones(24 * 4)
    with mv.Problem([24, 4], y, deltas=[1.0, 1.0]) as P:
        P.dct_split(0, 4)
        with pytest.raises(MvtvError) as e:
            P.dct_chirp(0, 6, 8)
        assert e.value.status == MVTV_BAD_ARG
        with pytest.raises(MvtvError) as e:
            P.dct_chirp(0, -1)
        assert e.value.status == MVTV_BAD_ARG
        P.dct_chirp(0, 0, 0)      # off is always accepted
        P.dct_split(0, 0)
        P.dct_chirp(0, 6, 8)
        with pytest.raises(MvtvError) as e:
            P.dct_split(0, 4)
        assert e.value.status == MVTV_BAD_ARG
        P.dct_split(0, 0)         # automatic is always accepted
        assert P.dct_chirp_factors(0) == (6, 8)
        P.dct_chirp(0, 0, 0)
        P.dct_split(0, 4)
        P.dct_split(0, 0)


def test_no_convolution_length_past_the_largest_m(monkeypatch):
    """a = -1 on m > (4096^2 + 1) / 2: no M = a b >= 2m - 1 with both factors <= 4096 exists. 8388610 x 2 (16.8 M
    nodes) is created on the Jacobi-PCG path like any refused mesh; the call is MVTV_BAD_ARG and changes nothing, and
    MVTV_DCT_CHIRP=1 leaves such a dimension off. One line shorter than the limit would be accepted (the rule:
    tests/test_long_chirp_host.py)."""
    m = [8388610, 2]
    assert chirp_auto(m[0]) is None and chirp_auto((4096 * 4096 + 1) // 2) == (4096, 4096)
    y = np.ones(int(np.prod(m)))
    with mv.Problem(m, y, deltas=[1.0, 1.0]) as P:
        assert not P.spectral_ok()
        with pytest.raises(MvtvError) as e:
            P.dct_chirp(0, -1)
        assert e.value.status == MVTV_BAD_ARG
        assert not P.spectral_ok() and P.dct_chirp_factors(0) == (0, 0)
        with pytest.raises(MvtvError) as e:   # forced factors cannot reach 2m - 1 either
            P.dct_chirp(0, 4096, 4096)
        assert e.value.status == MVTV_BAD_ARG
        assert not P.spectral_ok()
    monkeypatch.setenv("MVTV_DCT_CHIRP", "1")
    with mv.Problem(m, y, deltas=[1.0, 1.0]) as P:
        assert not P.spectral_ok() and P.dct_chirp_factors(0) == (0, 0)


def test_slab_ranks_refuse_the_chirp_transform(monkeypatch):
    from multivartv_amd import slab
    m = [64, 8]
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    comms = slab.Comm.local_group(2)
    ranks = [slab.SlabADMM(m, y[r * 256:(r + 1) * 256], deltas, float(y.mean()), comms[r], device=0) for r in range(2)]
    try:
        for rk in ranks:
            for args in ((0, -1, 0), (0, 9, 14), (0, 0, 0)):
                with pytest.raises(MvtvError) as e:
                    rk.P.dct_chirp(*args)
                assert e.value.status == MVTV_BAD_ARG
    finally:
        for rk in ranks:
            rk.close()
        for c in comms:
            c.close()
    # a two-rank local slab group with a prime leading dimension stays refused, with the variable set too
    monkeypatch.setenv("MVTV_DCT_CHIRP", "1")
    m = [4099, 8]
    with pytest.raises(MvtvError) as e:
        slab.run_local_group(m, towers(m), [(1.0 + 2e-4) / v for v in m], 1.0, 2, fixed_iters=1)
    assert e.value.status == MVTV_BAD_ARG
