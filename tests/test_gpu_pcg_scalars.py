"""The PCG scalars: iterates after k iterations and the stop, for all three PCGs, against textbook PCG
(tests/pcg_ref.py).

x += alpha p and r -= alpha q stay consistent for any alpha, and any beta still gives a descent direction, so a p.q,
r.z or |r|^2 that loses one workgroup's partial (in block_reduce_store, in k_finalize, in a padded workgroup, in the
DOT kernels' inactive lanes) only costs iterations: no comparison of a converged theta sees it. Here the solve is cut
after k = 1 ... 6 iterations (rtol unreachable, max_iter = k) and its iterate must equal the reference's x_k to
1e-11 of max|x_k| (the bound of test_gpu_parity.test_fused_pcg_stops_after_odd_and_even_iterations; float64 against
long double sits at 2e-14 and one dropped 256-cell share of p.q at 2e-4 or more: tests/test_pcg_ref_host.py). Then a
solve with a finite rtol, chosen from the reference's residuals alone where they drop by a factor >= 4 across it,
must stop at the reference's iteration.

Paths, each proved by the launch log of every call: generic k_apply_A<.., DOT> with k_pcg_update / k_pcg_pupdate
(p = 1, 2, 4 and MVTV_PCG=classic for p = 3), the fused k_cg3d with several tiles and dim-2 chunks, and pcgs_solve
(through the ADMM loop: theta_1 of one iteration is the k-th PCG iterate) with the DOT instantiations of k_apply2d /
k_apply3d / k_apply3d2 / k_apply4d at chunks of two planes on padded grids (W_DIAG, and W_NONE with W = I), both
sides of the std(W) >= 0.1 dbar switch of the diagonal scaling (k_pcgs_sinv), and the seven-launch form whose r.z
and |r|^2 are reduced inside k_dct8.
Achieved errors and stop counts go to $MVTV_PARITY_LOG."""
import functools
import os

import numpy as np
import pytest

import pcg_ref as PR
import stencil_ref as R
import test_stencil_tiling_host as T
from conftest import log_parity

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL_ITERATE = 1e-11
RTOL_RELRES = 1e-6   # the recursive residual carries about 1e-15 |b| of rounding; a lost tile of |r|^2 is percent-sized
SIGMA = 2.7
KMAX = 6


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _names(log, prefix):
    return [(n, g[0]) for n, g, _ in log if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------ Jacobi PCG (Problem.solve)
# name -> (mesh, path, sigma of the stop test: small enough for the reference's residuals to drop by >= 4 a step)
JACOBI = {
    "p1": ([5000], "generic", 0.1),
    "p2": ([300, 41], "generic", 0.02),
    "p4": ([6, 6, 6, 40], "generic", 0.002),
    "p3-fused-tiles": ([70, 70, 20], "fused", 0.01),
    "p3-fused-chunks": ([20, 20, 34], "fused", 0.01),
    "p3-classic": ([40, 40, 12], "classic", 0.01),
}


@functools.lru_cache(maxsize=None)
def _jacobi_ref(name, weighted, sigma, k):
    m = JACOBI[name][0]
    W, b, x0, A, Minv = PR.jacobi_case(m, weighted, sigma)
    xs, rel = PR.pcg_iterates(A, Minv, b, x0, k)
    return W, b, x0, xs, rel


def _jacobi_problem(name, W, weighted):
    m, path, _ = JACOBI[name]
    if path == "classic":   # read while the Problem is created (test_gpu_cg3d.test_fused_matches_classic_iterates)
        os.environ["MVTV_PCG"] = "classic"
    try:
        return mv.Problem(m, np.zeros(W.size), wdiag=W if weighted else None, deltas=R.DELTAS[:len(m)],
                          order=mv.ORDER_CPP)
    finally:
        os.environ.pop("MVTV_PCG", None)


def _check_jacobi_log(log, name, weighted, k):
    """the launches of one solve cut at k iterations; names as the launch log prints them (WMode 1 = W_IDENTITY,
    2 = W_DIAG; k_cg3d<WMode, MODE, waves>: MODE 0 prologue, 1 first iteration, 3 / 2 odd / even later ones)"""
    m, path, _ = JACOBI[name]
    p, w = len(m), 2 if weighted else 1
    if path == "fused":
        modes = [0] + [1 if j == 0 else (3 if j & 1 else 2) for j in range(k)]
        cg = _names(log, "k_cg3d<")
        assert [n for n, _ in cg] == [f"k_cg3d<{w}, {mode}, 16>" for mode in modes]
        tiles = T.cdiv(m[0], 60) * T.cdiv(m[1], 44)   # cg3d::TX, Shape<16>::TY (mvtv_cg3d.hip:54-62)
        assert len({g for _, g in cg}) == 1 and cg[0][1] > tiles and cg[0][1] % 8 == 0
        assert len(_names(log, "k_finalize")) == k + 1 and len(_names(log, "k_cg_xflush")) == 1
        assert not _names(log, "k_apply_A<")
        return
    assert not _names(log, "k_cg3d<")
    for kern, count in ((f"k_pcg_init<{p}, {w}>", 1), (f"k_apply_A<{p}, {w}, true, true>", k),
                        (f"k_pcg_update<{p}, {w}>", k), (f"k_pcg_pupdate<{p}, {w}>", k)):
        got = _names(log, kern.split("<")[0] + "<")
        assert [n for n, _ in got] == [kern] * count
        assert all(g >= 2 for _, g in got)   # several workgroups' partials enter every scalar
    assert len(_names(log, "k_finalize")) == 1 + 2 * k


@pytest.mark.parametrize("weighted", [False, True], ids=["W=I", "W=diag"])
@pytest.mark.parametrize("name", list(JACOBI))
def test_jacobi_iterates(name, weighted):
    W, b, x0, xs, rel = _jacobi_ref(name, weighted, SIGMA, KMAX)
    errs = {}
    with _jacobi_problem(name, W, weighted) as P:
        for k in range(1, KMAX + 1):
            with launch_log() as log:
                x, it, rr = P.solve(SIGMA, b, x0=x0, rtol=1e-300, max_iter=k)
            _check_jacobi_log(log, name, weighted, k)
            errs[f"k{k}"] = _rel(x, xs[k - 1])
            print(f"{name} weighted={weighted} k={k}: it {it}, iterate error {errs[f'k{k}']:.2e}, "
                  f"relres {rr:.6e} (reference {rel[k - 1]:.6e})")
            assert it == k
            assert errs[f"k{k}"] <= RTOL_ITERATE, k
            assert abs(rr - rel[k - 1]) <= RTOL_RELRES * rel[k - 1], k
    log_parity(f"pcg_iterates/jacobi/{name}/{'W=diag' if weighted else 'W=I'}", **errs)


@pytest.mark.parametrize("name", list(JACOBI))
def test_jacobi_stop(name):
    sigma = JACOBI[name][2]
    W, b, x0, xs, rel = _jacobi_ref(name, True, sigma, 40)
    fb = PR.first_below(rel)
    assert fb is not None, rel   # the case must give the property: another seed or sigma, never a smaller ratio
    k, rtol = fb
    with _jacobi_problem(name, W, True) as P:
        x, it, rr = P.solve(sigma, b, x0=x0, rtol=rtol, max_iter=2000)
    print(f"{name}: reference stops at {k} (relres {rel[k - 2]:.3e} -> {rel[k - 1]:.3e}, rtol {rtol:.3e}); "
          f"GPU at {it} with relres {rr:.6e}")
    log_parity(f"pcg_stop/jacobi/{name}", k_ref=k, k_gpu=it, relres_err=abs(rr - rel[k - 1]) / rel[k - 1])
    assert it == k
    assert abs(rr - rel[k - 1]) <= RTOL_RELRES * rel[k - 1]


# ---------------------------------------------------------------- spectrally preconditioned PCG (through the ADMM loop)
# name -> (mesh, weights, rho_0, seven-launch form, rho_0 of the stop test or None: one stop test per mesh)
SPECTRAL = {
    "2d-fold": ([270, 41], "fold", 6.0, False, 25.6),
    "2d-counts": ([270, 41], "counts", 0.04, False, None),
    "2d-fused7-fold": ([256, 24], "fold", 6.0, True, 25.6),
    "2d-fused7-counts": ([256, 24], "counts", 0.04, True, None),
    "3d-fused7-fold": ([64, 64, 24], "fold", 6.0, True, 25.6),
    "3d-fused7-counts": ([64, 64, 24], "counts", 0.1, True, None),
    "3d2": ([140, 140, 70], "fold", 6.0, False, 100.0),
    "3d1": ([135, 135, 100], "fold", 6.0, False, 25.6),
    "4d": ([12, 12, 12, 301], "fold", 6.0, False, 400.0),
    # W = I under PCG_SPECTRAL: the W_NONE DOT instantiations (the centre weight + 1). M = A there, so x_1 is the
    # solution (alpha_1 = r.z / p.q = 1) and later iterations divide rounding noise: k = 1 only
    "2d-identity": ([270, 41], "identity", 6.0, False, None),
    "3d2-identity": ([140, 140, 70], "identity", 6.0, False, None),
    "3d1-identity": ([135, 135, 100], "identity", 6.0, False, None),
    "4d-identity": ([12, 12, 12, 301], "identity", 6.0, False, None),
}
KS = (1, 2, 3, 4, 6)


@functools.lru_cache(maxsize=2)
def _spectral_ref(name, rho, k):
    m, kind = SPECTRAL[name][:2]
    c = PR.spectral_case(m, kind, rho)
    c["xs"], c["rel"] = PR.pcg_iterates(c["A"], c["Minv"], c["b"], c["th0"], k)
    return c


@pytest.fixture(scope="module")
def problems():
    """one Problem per (mesh, weights), shared by the iterate and the stop test (W and O^T y do not depend on rho)"""
    pool = {}

    def get(name, c):
        m, kind = SPECTRAL[name][:2]
        key = (tuple(m), kind)
        if key not in pool:
            pool[key] = mv.Problem(m, c["oty"], wdiag=None if kind == "identity" else c["W"],
                                   deltas=R.DELTAS[:len(m)], order=mv.ORDER_CPP)
        return pool[key]

    yield get
    for P in pool.values():
        P.close()


def _theta1(P, c, rho, rtol, maxit):
    """theta after one ADMM iteration from (theta_0, u = 0, rho): the PCG iterate the theta-solve stopped at"""
    with launch_log() as log:
        th, _, _, st = P.admm(1.0, c["th0"], u=np.zeros(P.E), rho=rho, fixed_iters=1, pcg_rtol=rtol, pcg_max_iter=maxit,
                              pcg_strict=0, theta_solver=mv.SOLVER_PCG_SPECTRAL)
    assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["iters"] == 1
    return th, st, log


def _check_spectral_log(log, name, scaled, k):
    """k iterations of pcgs_solve: k DOT launches of the mesh's marching kernel (W_DIAG) on the transcribed grid; the
    diagonal scaling's k_pcgs_sinv exactly when std(W) >= 0.1 dbar; in the seven-launch form (dct_pcg_fusable,
    mvtv_spectral.hip:5008) k_dct8's last template argument is 1 on the pass that carries the x / r update and 2 on
    the one that reduces r.z and |r|^2, and k_pcgs_vec runs 2 + k times instead of 2 + 3 k"""
    m, kind, _, fused7, _ = SPECTRAL[name]
    kern, grid = T.kernel_of(m), T.tiling(m)[5]
    dot = [(n, g) for n, g in _names(log, kern + "<") if n.endswith("true>")]
    assert dot == [(f"{kern}<{0 if kind == 'identity' else 2}, true>", grid)] * k
    assert bool(_names(log, "k_pcgs_sinv<")) == scaled
    carry = [n for n, _ in _names(log, "k_dct8<") if n.endswith(", 1>")]
    reduce_ = [(n, g) for n, g in _names(log, "k_dct8<") if n.endswith(", 2>")]
    assert len(carry) == len(reduce_) == (k if fused7 else 0)
    assert all(g >= 2 for _, g in reduce_)
    assert len(_names(log, "k_pcgs_vec")) == (2 + k if fused7 else 2 + 3 * k)


@pytest.mark.parametrize("name", list(SPECTRAL))
def test_spectral_iterates(name, problems):
    m, kind, rho, _, _ = SPECTRAL[name]
    ks = KS if kind != "identity" else KS[:1]
    c = _spectral_ref(name, rho, max(ks))
    assert c["scaled"] == (kind == "counts")
    assert np.all(c["W"] == 1.0) == (kind == "identity") and np.ptp(c["th0"]) > 1.0
    P = problems(name, c)
    errs = {}
    for k in ks:
        th, st, log = _theta1(P, c, rho, 1e-300, k)
        _check_spectral_log(log, name, c["scaled"], k)
        errs[f"k{k}"] = _rel(th, c["xs"][k - 1])
        print(f"{name} rho={rho} scaled={c['scaled']} k={k}: pcg_iters {st['pcg_iters']}, "
              f"iterate error {errs[f'k{k}']:.2e}")
        assert st["pcg_iters"] == k
        assert errs[f"k{k}"] <= RTOL_ITERATE, k
    log_parity(f"pcg_iterates/spectral/{name}", **errs)


@pytest.mark.parametrize("name", [n for n in SPECTRAL if SPECTRAL[n][4] is not None])
def test_spectral_stop(name, problems):
    rho = SPECTRAL[name][4]
    c = _spectral_ref(name, rho, 10)
    fb = PR.first_below(c["rel"])
    assert fb is not None, c["rel"]   # the case must give the property: another seed or rho, never a smaller ratio
    k, rtol = fb
    th, st, log = _theta1(problems(name, c), c, rho, rtol, 200)
    print(f"{name} rho={rho}: reference stops at {k} (relres {c['rel'][k - 2]:.3e} -> {c['rel'][k - 1]:.3e}, "
          f"rtol {rtol:.3e}); GPU at {st['pcg_iters']}, unconverged {st['pcg_unconverged']}")
    log_parity(f"pcg_stop/spectral/{name}", k_ref=k, k_gpu=st["pcg_iters"], unconverged=st["pcg_unconverged"])
    assert st["pcg_iters"] == k
    assert st["pcg_unconverged"] == 0
