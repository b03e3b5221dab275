"""GPU parity of the batched small-mesh fits (mvtv_path_batch / Problem.path_batch; k_admm_small, one workgroup per
batch member) against the CPU oracles: oracle/c_oracle.admm_rcpp (pcg_rtol 1e-13) for the single fits,
mvtv_oracle.mbs_path_rcpp / admm_rcpp (SuperLU) for the paths and the mixed-endings batch.

Tolerances, the project's: iterations and rho exact; theta within 1e-9 max|theta_ref|; u within
1e-9 max(1, max|u_ref|); r / s norms and eps within 1e-9 relative; GPU pcg_rtol = 1e-13. That the iteration counts can
be exact is shown on the reference alone in tests/test_small_batch_host.py (every decision >= 1e-6 from its threshold),
which also shows that these cases reach every instantiation of the kernel.

The 5^4 path's reference is 966 SuperLU factorisations of an 81-point matrix, about 12 s of CPU; it is computed once a
process (tests/small_batch_cases.py caches it for the host test and this one).
"""
import math

import numpy as np
import pytest

import small_batch_cases as S
from oracle import c_oracle as CO
from oracle import mvtv_oracle as O

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import _lib, slab  # noqa: E402

pytestmark = pytest.mark.gpu

ORD = {"cpp": mv.ORDER_CPP, "py": mv.ORDER_PY}
ORDN = {"cpp": 0, "py": 1}
RTOL = 1e-13
MVTV_OK, MVTV_MAXITER, MVTV_BAD_ARG = 0, 1, 2


def _problem(m, order="cpp", weighted=True):
    """The geometry handle: its own data is irrelevant to path_batch."""
    return mv.Problem(m, np.zeros(int(np.prod(m))), deltas=S.deltas_of(m), order=ORD[order], weighted=weighted)


def _close(got, ref, what):
    assert abs(got - ref) <= 1e-9 * abs(ref), (what, got, ref)


def _check_launches(log, name, nbatch, iters_per_lambda):
    """Only k_admm_small of the expected instantiation, grid = nbatch, block = NT, and per lambda at most
    ceil(max iterations / chunk) + 1 launches."""
    nt = int(name.split(",")[1])
    assert log and all(e == (name, (nbatch, 1, 1), (nt, 1, 1)) for e in log), log[:4]
    assert len(log) <= sum(math.ceil(max(it, 1) / S.CHUNK) + 1 for it in iters_per_lambda)


@pytest.mark.parametrize("c", S.single_cases(), ids=S.case_id)
def test_single_fit_matches_oracle(c):
    """nbatch = 1, n_lambda = 1: fixed_iters = 6 and a converged run, W = I through wdiag = NULL."""
    m, order, weighted, wk = c
    oty, W, ym = S.problem(m, wk)
    N = int(np.prod(m))
    E = CO.num_edges(m, order=ORDN[order], weighted=int(weighted))
    lam, tol = S.LAM_SINGLE, S.conv_tol(m)
    name = S.instantiation(m, order, weighted)
    with _problem(m, order, weighted) as P:
        assert P.batch_ok() and P.E == E
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
                  np.max(np.abs(us[0] - u)), "pcg", st["pcg_iters"], st["pcg_iters_max"])
            assert status == MVTV_OK and st["status"] == MVTV_OK
            assert st["iters"] == ref["iters"] and (fixed == 0 or st["iters"] == 6)
            if fixed == 0:
                assert st["iters"] == S.slu_single(c).iters   # the count whose margins the host test checked
            assert st["rho"] == ref["rho"] and rhos[0, 0] == ref["rho"]
            assert np.max(np.abs(thetas[0, 0] - th)) <= 1e-9 * np.max(np.abs(th))
            assert np.max(np.abs(us[0] - u)) <= 1e-9 * max(1.0, np.max(np.abs(u)))
            for k, rk in (("r_norm", "r_norm"), ("s_norm", "s_norm"), ("eps_pri", "eps_pri"), ("eps_dual", "eps_dual")):
                _close(st[k], ref[rk], k)
            assert st["theta_solver"] == mv.SOLVER_PCG and st["pcg_unconverged"] == 0
            assert st["pcg_iters"] >= st["pcg_iters_max"] >= 1
            _check_launches(log, name, 1, [st["iters"]])


@pytest.mark.parametrize("m", S.PATH_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_path_matches_mbs_path_rcpp(m):
    """The 5-lambda warm-started grid: every lambda's iteration count and rho exact, u after the last lambda."""
    oty, W, ym = S.problem(m, "S")
    N = int(np.prod(m))
    ref = S.slu_path(m)   # O.mbs_path_rcpp, computed once a process
    with _problem(m) as P:
        with _lib.launch_log() as log:
            thetas, us, rhos, stats, status = P.path_batch(oty, S.LAMS, np.full(N, ym), [S.LAMS[0] / 5.0], wdiag=W,
                                                           want_u=True, pcg_rtol=RTOL)
    print(m, "iters", [s["iters"] for s in stats[0]], [r.iters for r in ref])
    assert status == MVTV_OK
    assert [s["iters"] for s in stats[0]] == [r.iters for r in ref]
    assert [s["rho"] for s in stats[0]] == [r.rho for r in ref] and list(rhos[0]) == [r.rho for r in ref]
    for l, r in enumerate(ref):
        assert np.max(np.abs(thetas[0, l] - r.theta)) <= 1e-9 * np.max(np.abs(r.theta)), l
    assert np.max(np.abs(us[0] - ref[-1].u)) <= 1e-9 * max(1.0, np.max(np.abs(ref[-1].u)))
    _check_launches(log, S.instantiation(m), 1, [r.iters for r in ref])


def _stat_tuple(s):
    return tuple(s[k] for k in ("iters", "status", "r_norm", "s_norm", "eps_pri", "eps_dual", "rho", "pcg_iters",
                                "pcg_iters_max", "pcg_unconverged"))


def test_members_are_independent_of_position_and_batch_size():
    """300 members (more than one round of 256 CUs) built from 5 distinct (data, lambda) problems on 10 x 10 in
    shuffled order: equal inputs give identical bits in theta, rho and every stat, and the bits of the nbatch = 1 run."""
    m = [10, 10]
    N = 100
    probs = [S.problem(m, "S", seed) + (lam,) for seed, lam in enumerate(S.LAMS)]
    which = np.random.default_rng(5).permutation(np.arange(300) % 5)
    oty = np.stack([probs[k][0] for k in which])
    W = np.stack([probs[k][1] for k in which])
    th0 = np.stack([np.full(N, probs[k][2]) for k in which])
    lam = np.array([[probs[k][3]] for k in which])
    with _problem(m) as P:
        thetas, _, rhos, stats, status = P.path_batch(oty, lam, th0, lam[:, 0] / 5.0, wdiag=W, pcg_rtol=RTOL)
        assert status == MVTV_OK
        assert max(s[0]["iters"] for s in stats) > S.CHUNK   # more than one launch
        assert len({s[0]["iters"] for s in stats}) == 5
        for k in range(5):
            o, w, ym, lk = probs[k]
            t1, _, r1, s1, _ = P.path_batch(o, [lk], np.full(N, ym), [lk / 5.0], wdiag=w, pcg_rtol=RTOL)
            for b in np.flatnonzero(which == k):
                np.testing.assert_array_equal(thetas[b], t1[0])
                assert rhos[b, 0] == r1[0, 0] and _stat_tuple(stats[b][0]) == _stat_tuple(s1[0][0])


def test_mixed_endings_and_max_counter():
    """Members that end after very different iteration counts in one batch, then the same batch under
    max_counter = 5: the call returns MVTV_MAXITER, the member that stops within 5 iterations reports MVTV_OK, and
    every member matches its own reference."""
    members = S.mixed_members()
    m, N = S.MIXED_M, 100
    oty = np.stack([mb[0] for mb in members])
    W = np.stack([mb[1] for mb in members])
    th0 = np.stack([np.full(N, mb[2]) for mb in members])
    lam = np.array([[mb[3]] for mb in members])
    with _problem(m) as P:
        for cap in (3000, 5):
            with _lib.launch_log() as log:
                thetas, us, rhos, stats, status = P.path_batch(oty, lam, th0, lam[:, 0] / 5.0, wdiag=W, want_u=True,
                                                               pcg_rtol=RTOL, max_counter=cap)
            refs = [S.slu_member(j, cap) for j in range(len(members))]
            print("cap", cap, "iters", [s[0]["iters"] for s in stats], [r.iters for r in refs])
            hit = [r.iters >= cap for r in refs]
            assert status == (MVTV_MAXITER if any(hit) else MVTV_OK) and (cap != 5 or (any(hit) and not all(hit)))
            for j, r in enumerate(refs):
                st = stats[j][0]
                assert st["status"] == (MVTV_MAXITER if hit[j] else MVTV_OK)
                assert st["iters"] == r.iters and st["rho"] == r.rho
                assert np.max(np.abs(thetas[j, 0] - r.theta)) <= 1e-9 * np.max(np.abs(r.theta))
                assert np.max(np.abs(us[j] - r.u)) <= 1e-9 * max(1.0, np.max(np.abs(r.u)))
                h = r.history[-1]
                print("member", j, {k: abs(st[k] - h[k]) / abs(h[k]) for k in ("r_norm", "s_norm", "eps_pri", "eps_dual")})
                for k in ("r_norm", "s_norm", "eps_pri", "eps_dual"):
                    _close(st[k], h[k], k)
            _check_launches(log, S.instantiation(m), len(members), [max(r.iters for r in refs)])


def test_pcg_cap_counts_and_strict_status():
    """pcg_max_iter = 3 on 10 x 10: every theta-solve stops at the cap, is counted in pcg_unconverged, and the run goes
    on (the C oracle's loop under the same cap gives the same theta); with pcg_strict the member stops at its first
    capped solve and the call returns MVTV_PCG_NOT_CONVERGED."""
    m, N = [10, 10], 100
    oty, W, ym = S.problem(m, "S")
    E = CO.num_edges(m)
    th, u = np.full(N, ym), np.zeros(E)
    ref = CO.admm_rcpp(m, oty, 0.5, th, u, 0.1, S.deltas_of(m), W=W, fixed_iters=4, pcg_rtol=RTOL, pcg_maxit=3)
    with _problem(m) as P:
        thetas, us, rhos, stats, status = P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, want_u=True,
                                                       fixed_iters=4, pcg_rtol=RTOL, pcg_max_iter=3)
        st = stats[0][0]
        print("capped", st, ref, np.max(np.abs(thetas[0, 0] - th)) / np.max(np.abs(th)))
        assert status == MVTV_OK and st["status"] == MVTV_OK and st["iters"] == 4
        assert st["pcg_unconverged"] == 4 and st["pcg_iters"] == 12 and st["pcg_iters_max"] == 3
        assert ref["iters"] == 4 and ref["pcg_iters"] == 12 and st["rho"] == ref["rho"]
        assert np.max(np.abs(thetas[0, 0] - th)) <= 1e-9 * np.max(np.abs(th))
        assert np.max(np.abs(us[0] - u)) <= 1e-9 * max(1.0, np.max(np.abs(u)))
        with pytest.raises(mv.MvtvError) as e:
            P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, fixed_iters=4, pcg_rtol=RTOL, pcg_max_iter=3,
                         pcg_strict=1)
        assert e.value.status == 7   # MVTV_PCG_NOT_CONVERGED
        # an uncapped call afterwards converges every solve
        _, _, _, stats, status = P.path_batch(oty, [0.5], np.full(N, ym), [0.1], wdiag=W, fixed_iters=4, pcg_rtol=RTOL,
                                              pcg_strict=1)
        assert status == MVTV_OK and stats[0][0]["pcg_unconverged"] == 0 and stats[0][0]["pcg_iters_max"] > 3


def _refused(P, **kw):
    N = P.N
    args = dict(oty=np.ones((2, N)), lambdas=[0.5], theta_init=np.zeros((2, N)), rho_init=[0.1, 0.1], wdiag=None)
    args.update(kw)
    with _lib.launch_log() as log:
        with pytest.raises(mv.MvtvError) as e:
            P.path_batch(args.pop("oty"), args.pop("lambdas"), args.pop("theta_init"), args.pop("rho_init"), **args)
    assert e.value.status == MVTV_BAD_ARG, e.value.args
    assert log == []


def test_refusals_make_no_launch_and_leave_the_problem_intact():
    m = [10, 10]
    oty, W, ym = S.problem(m, "S")
    with mv.Problem(m, oty, wdiag=W, deltas=S.deltas_of(m)) as P:
        P.state_set(np.full(100, ym), None, 0.1)
        before = P.run(0.5, fixed_iters=4)
        th_b, u_b, rho_b = P.state_get()
        _refused(P, variant=mv.VARIANT_CPP)
        _refused(P, variant=mv.VARIANT_PY)
        _refused(P, theta_solver=mv.SOLVER_SPECTRAL)
        _refused(P, theta_solver=mv.SOLVER_PCG_SPECTRAL)
        _refused(P, sigma=1.0)
        _refused(P, oty=np.ones((0, 100)), theta_init=np.zeros((0, 100)), rho_init=[])   # nbatch < 1
        _refused(P, lambdas=np.zeros((2, 0)))                                              # n_lambda < 1
        _refused(P, lambdas=[0.5, -0.1])
        _refused(P, rho_init=[0.1, 0.0])
        _refused(P, rho_init=[float("nan"), 0.1])
        _refused(P, rho_init=[0.1, float("inf")])
        bad = np.ones((2, 100))
        bad[1, 7] = -1.0
        _refused(P, wdiag=bad)
        bad = np.ones((2, 100))
        bad[1] = 0.0
        _refused(P, wdiag=bad)
        # a good call in between, then the problem's own state and data are what they were
        P.path_batch(np.stack([oty, oty]), [0.5], np.zeros((2, 100)), [0.1, 0.1], wdiag=np.stack([W, W]), fixed_iters=3)
        P.state_set(np.full(100, ym), None, 0.1)
        after = P.run(0.5, fixed_iters=4)
        th_a, u_a, rho_a = P.state_get()
        assert _stat_tuple(before) == _stat_tuple(after) and rho_a == rho_b
        np.testing.assert_array_equal(th_a, th_b)
        np.testing.assert_array_equal(u_a, u_b)
    for mm in S.REFUSED_SHAPES:
        with _problem(mm) as P:
            assert not P.batch_ok()
            _refused(P)
    # a slab rank: planes 0..4 of 10 plus the ghost plane above
    ml = [8, 8, 6]
    Ps = slab._Slab(ml, np.zeros(8 * 8 * 6), S.deltas_of([8, 8, 10]), mv.ORDER_CPP, 0, 10, 0, 5, 0, 1)
    try:
        assert not Ps.batch_ok()
        _refused(Ps)
    finally:
        Ps.close()
