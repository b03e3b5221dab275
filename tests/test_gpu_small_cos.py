"""GPU checks of the batched fits' in-workgroup cosine theta-solve (mvtv_problem_batch_cosine, mvtv_solve_batch;
k_solve_cos, k_admm_cos in mvtv_small_cos.hip).

The solve alone against the long-double cosine-transform solve (oracle/spectral_ld.py) under the forward-error rule of
DESIGN.md §2.1, max|x - x_ld| <= min(1e-12, 32 e64) max|x_ld|; the loop kernels against the CPU oracles of
tests/test_gpu_small_batch.py with that file's bounds (iterations and rho exact; theta within 1e-9 max|theta_ref|; u
within 1e-9 max(1, max|u_ref|); norms and eps within 1e-9 relative; pcg_rtol 1e-13). Every case asserts its launches.
"""
import math

import numpy as np
import pytest

import small_batch_cases as S
import small_cos_model as M
from oracle import c_oracle as CO
from oracle import spectral_ld as SLD

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import _lib, slab  # noqa: E402

pytestmark = pytest.mark.gpu

ORD = {"cpp": mv.ORDER_CPP, "py": mv.ORDER_PY}
ORDN = {"cpp": 0, "py": 1}
RTOL = 1e-13
MVTV_OK, MVTV_BAD_ARG = 0, 2
SIGMAS = [0.0, 1e-3, 3.7, 2e5]
SHIFT, SHIFT_SIGMA = 0.37, 3.7


def _problem(m, order="cpp", weighted=True):
    return mv.Problem(m, np.zeros(int(np.prod(m))), deltas=S.deltas_of(m), order=ORD[order], weighted=weighted)


def _close(got, ref, what, floor=0.0):
    """1e-9 relative. A residual norm whose exact value is zero (a fit that ends flat on [2]: r = -D theta with
    theta_0 = theta_1) is rounding noise in the reference too, a few ulp of the terms it is a difference of, and no two
    solvers round alike: where the reference itself is within `floor`, the rounding floor of those terms in float64,
    the GPU value only has to be within it too."""
    if abs(ref) <= floor:
        assert abs(got) <= floor, (what, got, ref, floor)
    else:
        assert abs(got - ref) <= 1e-9 * abs(ref), (what, got, ref)


def _floors(P, E, N, theta, u, rho):
    """The float64 rounding floors of r = alpha - D theta and s = rho D^T (u - u_old): four roundings of eps a term
    (theta's or u's own last bit twice, the product with the block weight, the difference), terms of size
    w_max max|theta| over E rows, and rho w_max max|u| over 2^p edges a node and N nodes."""
    eps = np.finfo(np.float64).eps
    wmax = max(abs(w) for _, _, w in P.block_info())
    return {"r_norm": 4 * eps * math.sqrt(E) * wmax * float(np.max(np.abs(theta))),
            "s_norm": 4 * eps * math.sqrt(N) * abs(rho) * wmax * 2 ** P.p * float(np.max(np.abs(u)))}


def _check_launches(log, name, nbatch, iters_per_lambda):
    nt = int(name.split(",")[1])
    assert log and all(e == (name, (nbatch, 1, 1), (nt, 1, 1)) for e in log), log[:4]
    assert len(log) <= sum(math.ceil(max(it, 1) / S.CHUNK) + 1 for it in iters_per_lambda)


# ---------------------------------------------------------------- the solve alone
SOLVE_CASES = [(m, "cpp", True) for m in S.SHAPES + M.EXTRA_SHAPES]
SOLVE_CASES += [(m, o, w) for m in S.LAYOUT_SHAPES for (o, w) in S.LAYOUTS if not (len(m) == 1 and o == "py" and w)]


@pytest.mark.parametrize("case", SOLVE_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1]}{'w' if c[2] else 'u'}")
def test_solve_batch_matches_long_double(case):
    """The four sigma as one batch plus a member with shift 0.37 (sigma 3.7)."""
    m, order, weighted = case
    rng = np.random.default_rng(sum(m) + len(m))
    N = int(np.prod(m))
    b = rng.standard_normal(N) + 2.0
    deltas = S.deltas_of(m)
    fwd_ld, fwd_64 = SLD.forward_ld(m, b), SLD.forward_ld(m, b, np.float64)
    sym_ld = SLD.dtd_symbol_ld(m, deltas, ORDN[order], weighted)
    sym_64 = SLD.dtd_symbol_ld(m, deltas, ORDN[order], weighted, np.float64)
    sig = SIGMAS + [SHIFT_SIGMA]
    shift = [1.0] * len(SIGMAS) + [SHIFT]
    with _problem(m, order, weighted) as P:
        with _lib.launch_log() as log:
            x = P.solve_batch(np.tile(b, (len(sig), 1)), sig, shift)
        with _lib.launch_log() as log1:
            x1 = P.solve_batch(np.tile(b, (len(SIGMAS), 1)), SIGMAS)   # shift = None
    nt = S.nt_rule(N)
    assert log == [(M.solve_name(m), (len(sig), 1, 1), (nt, 1, 1))]
    assert log1 == [(M.solve_name(m), (len(SIGMAS), 1, 1), (nt, 1, 1))]
    np.testing.assert_array_equal(x1, x[:len(SIGMAS)])
    for k, (s, sh) in enumerate(zip(sig, shift)):
        x_ld = SLD.solve_from_forward(fwd_ld, sym_ld, s / sh) / SLD.LD(sh)
        x_64 = SLD.solve_from_forward(fwd_64, sym_64, s / sh) / sh
        scale = float(np.max(np.abs(x_ld)))
        e64 = float(np.max(np.abs(x_64 - x_ld))) / scale
        err = float(np.max(np.abs(x[k] - x_ld))) / scale
        print(f"m={m} {order} w={weighted} sigma={s:g} shift={sh:g}: err {err:.2e}, e64 {e64:.2e}, ratio {err / e64:.2f}")
        assert err <= min(1e-12, 32.0 * e64), (m, s, sh, err, e64)


# ---------------------------------------------------------------- single fits
FIT_CASES = [(m, "cpp", True, wk) for m in S.SHAPES + M.EXTRA_SHAPES for wk in ("I", "S")]


@pytest.mark.parametrize("c", FIT_CASES, ids=S.case_id)
def test_single_fit_matches_oracle(c):
    """W = I under mode 1 (the exact solve), scattered W under mode 2 (the preconditioned PCG): fixed_iters = 6 and a
    converged run."""
    m, order, weighted, wk = c
    pc = wk == "S"
    oty, W, ym = S.problem(m, wk)
    N = int(np.prod(m))
    E = CO.num_edges(m, order=ORDN[order], weighted=int(weighted))
    lam, tol = S.LAM_SINGLE, S.conv_tol(m)
    name = M.loop_name(m, pc, order, weighted)
    with _problem(m, order, weighted) as P:
        P.batch_cosine(2 if pc else 1)
        assert P.batch_cosine_mode() == (2 if pc else 1)
        for fixed in (6, 0):
            th, u = np.full(N, ym), np.zeros(E)
            ref = CO.admm_rcpp(m, oty, lam, th, u, lam / 5.0, S.deltas_of(m), W=W, order=ORDN[order],
                               weighted=int(weighted), fixed_iters=fixed, tol=tol, pcg_rtol=RTOL)
            with _lib.launch_log() as log:
                thetas, us, rhos, stats, status = P.path_batch(
                    oty, [lam], np.full(N, ym), [lam / 5.0], wdiag=W, want_u=True, fixed_iters=fixed, tol=tol,
                    pcg_rtol=RTOL)
            st = stats[0][0]
            print(S.case_id(c), "fixed" if fixed else "converged", "iters", st["iters"], ref["iters"], "rho", st["rho"],
                  ref["rho"], "dtheta", np.max(np.abs(thetas[0, 0] - th)) / np.max(np.abs(th)), "du",
                  np.max(np.abs(us[0] - u)), "pcg", st["pcg_iters"], st["pcg_iters_max"], "jacobi", ref["pcg_iters"])
            assert status == MVTV_OK and st["status"] == MVTV_OK
            assert st["iters"] == ref["iters"] and (fixed == 0 or st["iters"] == 6)
            if fixed == 0:
                assert st["iters"] == S.slu_single(c).iters
            assert st["rho"] == ref["rho"] and rhos[0, 0] == ref["rho"]
            assert np.max(np.abs(thetas[0, 0] - th)) <= 1e-9 * np.max(np.abs(th))
            assert np.max(np.abs(us[0] - u)) <= 1e-9 * max(1.0, np.max(np.abs(u)))
            floors = _floors(P, E, N, th, u, ref["rho"])
            for k in ("r_norm", "s_norm", "eps_pri", "eps_dual"):
                _close(st[k], ref[k], k, floors.get(k, 0.0))
            if pc:
                assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["pcg_unconverged"] == 0
                assert st["pcg_iters"] >= st["pcg_iters_max"] >= 1
            else:
                assert st["theta_solver"] == mv.SOLVER_SPECTRAL
                assert st["pcg_iters"] == 0 and st["pcg_iters_max"] == 0 and st["pcg_unconverged"] == 0
            _check_launches(log, name, 1, [st["iters"]])


@pytest.mark.parametrize("m", S.PATH_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_path_matches_mbs_path_rcpp(m):
    oty, W, ym = S.problem(m, "S")
    N = int(np.prod(m))
    ref = S.slu_path(m)
    with _problem(m) as P:
        P.batch_cosine(2)
        with _lib.launch_log() as log:
            thetas, us, rhos, stats, status = P.path_batch(oty, S.LAMS, np.full(N, ym), [S.LAMS[0] / 5.0], wdiag=W,
                                                           want_u=True, pcg_rtol=RTOL)
    print(m, "iters", [s["iters"] for s in stats[0]], [r.iters for r in ref], "pcg a solve",
          [round(s["pcg_iters"] / max(s["iters"], 1), 1) for s in stats[0]])
    assert status == MVTV_OK
    assert [s["iters"] for s in stats[0]] == [r.iters for r in ref]
    assert [s["rho"] for s in stats[0]] == [r.rho for r in ref] and list(rhos[0]) == [r.rho for r in ref]
    assert all(s["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and s["pcg_unconverged"] == 0 for s in stats[0])
    for l, r in enumerate(ref):
        assert np.max(np.abs(thetas[0, l] - r.theta)) <= 1e-9 * np.max(np.abs(r.theta)), l
    assert np.max(np.abs(us[0] - ref[-1].u)) <= 1e-9 * max(1.0, np.max(np.abs(ref[-1].u)))
    _check_launches(log, M.loop_name(m, True), 1, [r.iters for r in ref])


# ---------------------------------------------------------------- mixed kinds
def _stat_tuple(s):
    return tuple(s[k] for k in ("iters", "status", "r_norm", "s_norm", "eps_pri", "eps_dual", "rho", "pcg_iters",
                                "pcg_iters_max", "pcg_unconverged", "theta_solver"))


def test_mixed_kinds_in_one_batch():
    """300 members on 10 x 10 under AUTO with wdiag given: rows of all ones (W = I) and scattered rows, shuffled. Each
    member reports its own solver; equal inputs give identical bits, and the bits of the nbatch = 1 run."""
    m, N = [10, 10], 100
    probs = []
    for seed, lam in enumerate(S.LAMS):
        wk = "I" if seed % 2 == 0 else "S"
        oty, W, ym = S.problem(m, wk, seed)
        probs.append((oty, np.ones(N) if W is None else W, ym, lam, wk))
    which = np.random.default_rng(5).permutation(np.arange(300) % 5)
    oty = np.stack([probs[k][0] for k in which])
    W = np.stack([probs[k][1] for k in which])
    th0 = np.stack([np.full(N, probs[k][2]) for k in which])
    lam = np.array([[probs[k][3]] for k in which])
    small, cos_x, cos_p = S.instantiation(m), M.loop_name(m, False), M.loop_name(m, True)
    with _problem(m) as P:
        for mode in (1, 2):
            P.batch_cosine(mode)
            with _lib.launch_log() as log:
                thetas, _, rhos, stats, status = P.path_batch(oty, lam, th0, lam[:, 0] / 5.0, wdiag=W, pcg_rtol=RTOL)
            assert status == MVTV_OK
            assert {e[0] for e in log} == {cos_x, small if mode == 1 else cos_p}
            assert all(e[1] == (300, 1, 1) and e[2] == (64, 1, 1) for e in log)
            other = mv.SOLVER_PCG if mode == 1 else mv.SOLVER_PCG_SPECTRAL
            for k in range(5):
                o, w, ym, lk, wk = probs[k]
                t1, _, r1, s1, _ = P.path_batch(o, [lk], np.full(N, ym), [lk / 5.0], wdiag=w, pcg_rtol=RTOL)
                assert s1[0][0]["theta_solver"] == (mv.SOLVER_SPECTRAL if wk == "I" else other)
                assert (s1[0][0]["pcg_iters"] == 0) == (wk == "I")
                for b in np.flatnonzero(which == k):
                    np.testing.assert_array_equal(thetas[b], t1[0])
                    assert rhos[b, 0] == r1[0, 0] and _stat_tuple(stats[b][0]) == _stat_tuple(s1[0][0])


def test_pcg_spectral_on_identity_member_takes_one_iteration():
    """M = A when W = I: the preconditioned PCG converges in one iteration a solve (two allowed)."""
    m, N = [10, 10], 100
    oty, _, ym = S.problem(m, "I")
    E = CO.num_edges(m)
    th, u = np.full(N, ym), np.zeros(E)
    ref = CO.admm_rcpp(m, oty, 0.5, th, u, 0.1, S.deltas_of(m), fixed_iters=6, pcg_rtol=RTOL)
    with _problem(m) as P:
        P.batch_cosine(2)
        with _lib.launch_log() as log:
            thetas, _, _, stats, status = P.path_batch(oty, [0.5], np.full(N, ym), [0.1], fixed_iters=6, pcg_rtol=RTOL,
                                                       theta_solver=mv.SOLVER_PCG_SPECTRAL)
    st = stats[0][0]
    print("PCG_SPECTRAL on W = I: pcg iterations", st["pcg_iters"], "over", st["iters"], "solves, max", st["pcg_iters_max"])
    assert status == MVTV_OK and st["iters"] == 6 and st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL
    assert 1 <= st["pcg_iters_max"] <= 2 and st["pcg_iters"] <= 2 * st["iters"] and st["pcg_unconverged"] == 0
    assert st["rho"] == ref["rho"]
    assert np.max(np.abs(thetas[0, 0] - th)) <= 1e-9 * np.max(np.abs(th))
    _check_launches(log, M.loop_name(m, True), 1, [6])


def test_pcg_cap_counts_and_strict_status():
    m, N = [10, 10], 100
    oty, W, ym = S.problem(m, "S")
    with _problem(m) as P:
        P.batch_cosine(2)
        _, _, _, stats, status = P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, fixed_iters=4, pcg_rtol=RTOL,
                                              pcg_max_iter=1)
        st = stats[0][0]
        assert status == MVTV_OK and st["status"] == MVTV_OK and st["iters"] == 4
        assert st["pcg_unconverged"] == 4 and st["pcg_iters"] == 4 and st["pcg_iters_max"] == 1
        assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL
        with pytest.raises(mv.MvtvError) as e:
            P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, fixed_iters=4, pcg_rtol=RTOL, pcg_max_iter=1,
                         pcg_strict=1)
        assert e.value.status == 7   # MVTV_PCG_NOT_CONVERGED
        _, _, _, stats, status = P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, fixed_iters=4, pcg_rtol=RTOL,
                                              pcg_strict=1)
        assert status == MVTV_OK and stats[0][0]["pcg_unconverged"] == 0 and stats[0][0]["pcg_iters_max"] > 1


# ---------------------------------------------------------------- the switch
def _refused(P, **kw):
    N = P.N
    args = dict(oty=np.ones((2, N)), lambdas=[0.5], theta_init=np.zeros((2, N)), rho_init=[0.1, 0.1], wdiag=None)
    args.update(kw)
    with _lib.launch_log() as log:
        with pytest.raises(mv.MvtvError) as e:
            P.path_batch(args.pop("oty"), args.pop("lambdas"), args.pop("theta_init"), args.pop("rho_init"), **args)
    assert e.value.status == MVTV_BAD_ARG, e.value.args
    assert log == []


def test_mode_zero_after_mode_two_is_the_default_again():
    m, N = [10, 10], 100
    oty, W, ym = S.problem(m, "S")
    args = (np.stack([oty, oty]), [0.5], np.full((2, N), ym), [0.1, 0.1])
    kw = dict(wdiag=np.stack([W, np.ones(N)]), want_u=True, pcg_rtol=RTOL)
    with _problem(m) as P:
        assert P.batch_cosine_mode() == 0
        before = P.path_batch(*args, **kw)
        P.batch_cosine(2)
        mid = P.path_batch(*args, **kw)
        assert [s[0]["theta_solver"] for s in mid[3]] == [mv.SOLVER_PCG_SPECTRAL, mv.SOLVER_SPECTRAL]
        P.batch_cosine(0)
        assert P.batch_cosine_mode() == 0
        _refused(P, theta_solver=mv.SOLVER_SPECTRAL)
        _refused(P, theta_solver=mv.SOLVER_PCG_SPECTRAL)
        with _lib.launch_log() as log:
            after = P.path_batch(*args, **kw)
        assert {e[0] for e in log} == {S.instantiation(m)}
        for k in (0, 1, 2):
            np.testing.assert_array_equal(before[k], after[k])
        assert [[_stat_tuple(s) for s in mb] for mb in before[3]] == [[_stat_tuple(s) for s in mb] for mb in after[3]]
        assert all(s[0]["theta_solver"] == mv.SOLVER_PCG for s in after[3])


def test_solver_options_under_the_switch():
    """PCG forces Jacobi for all; SPECTRAL needs W = I everywhere; PCG_SPECTRAL needs mode 2."""
    m, N = [10, 10], 100
    oty, W, ym = S.problem(m, "S")
    mixed = np.stack([W, np.ones(N)])
    with _problem(m) as P:
        for mode in (1, 2):
            P.batch_cosine(mode)
            _refused(P, theta_solver=mv.SOLVER_SPECTRAL, wdiag=mixed)
            with _lib.launch_log() as log:
                _, _, _, stats, _ = P.path_batch(np.stack([oty, oty]), [0.5], np.full((2, N), ym), [0.1, 0.1],
                                                 wdiag=mixed, fixed_iters=3, theta_solver=mv.SOLVER_PCG)
            assert {e[0] for e in log} == {S.instantiation(m)}
            assert all(s[0]["theta_solver"] == mv.SOLVER_PCG for s in stats)
            with _lib.launch_log() as log:
                _, _, _, stats, _ = P.path_batch(np.stack([oty, oty]), [0.5], np.full((2, N), ym), [0.1, 0.1],
                                                 wdiag=np.ones((2, N)), fixed_iters=3, theta_solver=mv.SOLVER_SPECTRAL)
            assert {e[0] for e in log} == {M.loop_name(m, False)}
            assert all(s[0]["theta_solver"] == mv.SOLVER_SPECTRAL for s in stats)
        P.batch_cosine(1)
        _refused(P, theta_solver=mv.SOLVER_PCG_SPECTRAL)
        with pytest.raises(mv.MvtvError) as e:
            P.batch_cosine(3)
        assert e.value.status == MVTV_BAD_ARG and P.batch_cosine_mode() == 1


def test_switch_and_solve_refused_where_the_batch_is():
    for mm in S.REFUSED_SHAPES:
        with _problem(mm) as P:
            for mode in (0, 1, 2):
                with pytest.raises(mv.MvtvError) as e:
                    P.batch_cosine(mode)
                assert e.value.status == MVTV_BAD_ARG
            with _lib.launch_log() as log:
                with pytest.raises(mv.MvtvError) as e:
                    P.solve_batch(np.ones((1, P.N)), [1.0])
            assert e.value.status == MVTV_BAD_ARG and log == []
    ml = [8, 8, 6]
    Ps = slab._Slab(ml, np.zeros(8 * 8 * 6), S.deltas_of([8, 8, 10]), mv.ORDER_CPP, 0, 10, 0, 5, 0, 1)
    try:
        with pytest.raises(mv.MvtvError) as e:
            Ps.batch_cosine(1)
        assert e.value.status == MVTV_BAD_ARG
    finally:
        Ps.close()
    with _problem([10, 10]) as P:
        for bad in (dict(sigma=[-1.0]), dict(sigma=[float("nan")]), dict(sigma=[1.0], shift=[0.0])):
            with _lib.launch_log() as log:
                with pytest.raises(mv.MvtvError) as e:
                    P.solve_batch(np.ones((1, 100)), **bad)
            assert e.value.status == MVTV_BAD_ARG and log == []
