"""The nominal block orders (MVTV_ORDER_CPP_NOMINAL = 2, MVTV_ORDER_PY_NOMINAL = 3: block b differences along exactly
the dims of its code) on the GPU, on meshes the reference orders refuse: unequal m_0, m_1 (and m_2 at p = 4). The
references are the oracle's own functions on nominal blocks (tests/nominal_ref.py; on the CPU alone:
tests/test_nominal_host.py).

Bounds are those of the tests that check the same code under the reference orders:

* D, D^T: componentwise (|S| + 2) u a and (2^p + nb) u a (tests/test_gpu_operators_wide.py); W + sigma D^T D:
  2 (3^p + 2^p + p + 4) u (|W| |x| + sigma a) (tests/test_gpu_stencil_march.py).
* the spectral solve: min(1e-12, 32 e64) max|x_ld| against long double at the four sigma of tests/test_gpu_dispatch.py.
* ADMM against SuperLU: iterations and rho exact, theta within 1e-9 max|theta|, u within 1e-9 max(1, max|u|)
  (DESIGN.md §2); the cases' decisions stay 1e-6 from their thresholds (asserted on the references).
* lambda_max: 1e-9 relative (tests/test_gpu_lambda_max.py), on a right-hand side for which the reference's CG is
  well conditioned.
* batched fits: the tolerances of tests/test_gpu_small_batch.py; the CV driver: the selected lambda exact, the
  device-scored MSEs within 2 (n + 4) u of the host-scored ones and the unbatched run's within 1e-7 relative
  (tests/test_gpu_cv_batch.py's two bounds: the same fits scored twice, and fits by different theta-solvers).
"""
import functools

import numpy as np
import pytest

import nominal_ref as R
import small_batch_cases as S
import stencil_ref as SR
import test_oracle_diff_ld as T
from conftest import log_parity
from oracle import diff_ld as DL
from oracle import mvtv_oracle as O
from oracle import spectral_ld as SP
from oracle import stencil_ld as SL

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import _lib, cv, slab  # noqa: E402
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

ORD = {"cpp": mv.ORDER_CPP_NOMINAL, "py": mv.ORDER_PY_NOMINAL}
U = 2.0 ** -53


def _mid(m):
    return "x".join(map(str, m))


def _lid(v):
    return f"{v[0]}{'w' if v[1] else 'u'}"


def _problem(m, oty=None, wdiag=None, order="cpp", weighted=True, deltas=None):
    N = int(np.prod(m))
    return mv.Problem(list(m), np.zeros(N) if oty is None else oty, wdiag=wdiag,
                      deltas=R.deltas_of(m) if deltas is None else deltas, order=ORD[order], weighted=weighted)


# ------------------------------------------------------------------------------------------ creation
@pytest.mark.parametrize("m", [(6, 5, 4), (5, 4, 3, 2)], ids=_mid)
def test_creation(m):
    N = int(np.prod(m))
    for order in (mv.ORDER_CPP, mv.ORDER_PY):   # the reference rule still refuses the mesh
        with pytest.raises(mv.DimMismatchError):
            mv.Problem(list(m), np.zeros(N), deltas=R.deltas_of(m), order=order)
    for order, weighted in R.LAYOUTS:
        blks = R.blocks_of(m, order, weighted)
        E, rows = R.info(m, blks)
        with _problem(m, order=order, weighted=weighted) as P:
            assert (P.N, P.E, P.nb) == (N, E, len(blks))
            assert P.block_info() == rows


def test_slab_creation_is_refused():
    m, deltas = [6, 6, 4], R.deltas_of([6, 6, 6])
    with pytest.raises(mv.MvtvError) as e:   # planes 0 .. 2 of 6 and the ghost above them
        slab._Slab(m, np.zeros(6 * 6 * 4), deltas, mv.ORDER_CPP_NOMINAL, 0, 6, 0, 3, 0, 1)
    assert e.value.status == _lib.MVTV_BAD_ARG and "slab" in str(e.value)
    with slab._Slab(m, np.zeros(6 * 6 * 4), deltas, mv.ORDER_CPP, 0, 6, 0, 3, 0, 1) as P:
        assert P.nb == 7


# ------------------------------------------------------------------------------------------ operators
# 70 x 9 x 5: x crosses a 64-node chunk and a 64-column tile, m_1 below a fused tile's 14 rows
OP_MESHES = [(6, 5, 4), (70, 9, 5), (5, 4, 3, 2), (9, 4, 6, 3)]


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=_lid)
@pytest.mark.parametrize("m", OP_MESHES, ids=_mid)
def test_operators(m, layout):
    order, weighted = layout
    p, N = len(m), int(np.prod(m))
    blks = R.blocks(p, T.DELTAS[:p], order, weighted)
    lens = DL.block_lengths(m, blks)
    rng = np.random.default_rng(4000 + sum(m))
    th, v = rng.standard_normal(N), rng.standard_normal(sum(lens))
    W = SR.make_w(m)
    with _problem(m, wdiag=W, order=order, weighted=weighted, deltas=T.DELTAS[:p]) as P:
        assert P.E == sum(lens)
        with launch_log() as log:
            d = P.apply_D(th)
        assert log[0][0] == f"k_apply_D<{p}, {ORD[order]}>"
        with launch_log() as log:
            g = P.apply_Dt(v)
        assert log[-1][0] == f"k_gather<{p}, {ORD[order]}, 0, false>"
        q = {s: P.apply_A(s, th) for s in (0.0, 0.37, 25.6)}
    rD = T.ratio_D(m, blks, d, DL.apply_D(m, blks, th), DL.apply_D(m, blks, th, absval=True))
    rDt = T.ratio_Dt(m, blks, g, DL.apply_Dt(m, blks, v), DL.apply_Dt(m, blks, v, absval=True))
    dtd, a = SL.apply_dtd(m, blks, th), SL.apply_dtd(m, blks, th, absval=True)
    rA = {s: SR.ratio(q[s], W, s, th, dtd, a)[0] for s in q}
    print(f"{_mid(m)} {_lid(layout)}: D {rD:.3f}, D^T {rDt:.3f} of their bounds; A {rA} of u (bound {SR.c_bound(p)})")
    log_parity(f"nominal operators/{_mid(m)}/{_lid(layout)}", D=rD, Dt=rDt, A=max(rA.values()), c_A=SR.c_bound(p))
    assert rD <= 1.0 and rDt <= 1.0
    assert all(r <= SR.c_bound(p) for r in rA.values()), rA


# ------------------------------------------------------------------------------------------ spectral solve
SIGMAS = (0.0, 1e-3, 3.7, 2e5)   # tests/test_gpu_dispatch.py
SPEC_MESHES = [(16, 8, 5), (12, 10, 7), (11, 13, 5), (128, 64, 3), (8, 4, 16, 3), (6, 5, 4, 3)]


@functools.lru_cache(maxsize=1)
def _spec_case(m):
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    blks = R.blocks_of(m)
    ref = {name: (SP.forward_ld(m, b, dt), R.dtd_symbol(m, blks, dt)) for name, dt in (("ld", np.longdouble),
                                                                                        ("f64", np.float64))}
    return _problem(m, oty=b), b, ref


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("m", SPEC_MESHES, ids=_mid)
def test_spectral_solve(m, sigma):
    P, b, ref = _spec_case(m)
    assert P.spectral_ok()
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    x_ld = SP.solve_from_forward(*ref["ld"], sigma)
    x64 = SP.solve_from_forward(*ref["f64"], sigma)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    kernels = " | ".join(f"{n} {g[0]}x{bk[0]}" for n, g, bk in log)
    print(f"nominal spectral {_mid(m)} sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e}; {kernels}")
    log_parity(f"nominal spectral {_mid(m)} sigma={sigma:g}", e64=e64, err=err, kernels=kernels)
    assert len(log) >= 2 * len(m) - 1   # a pass per dimension each way, the last dimension's in one
    assert err <= min(1e-12, 32.0 * e64), (err, e64)


# ------------------------------------------------------------------------------------------ ADMM against SuperLU
FUSED = {(70, 9, 5): "k_admm3a", (5, 4, 3, 2): "k_admm4a"}
SOLVERS = {"I": ("SPECTRAL", "PCG"), "S": ("PCG_SPECTRAL", "PCG")}


@pytest.mark.parametrize("c", R.admm_cases(), ids=R.case_id)
def test_admm_matches_superlu(c):
    m, order, weighted, wk = c
    oty, W, ym = R.data(m, wk)
    ref, margin = R.slu(c)
    assert margin >= R.MARGIN and ref.iters >= 2
    N, nb = oty.size, len(R.blocks_of(m, order, weighted))
    with _problem(m, oty=oty, wdiag=W, order=order, weighted=weighted) as P:
        E = P.E
        assert E == ref.u.size
        for solver in SOLVERS[wk]:
            with launch_log() as log:
                th, u, rho, st = P.admm(R.LAM, np.full(N, ym), u=np.zeros(E), rho=R.LAM / 5.0, tol=R.tol_of(m),
                                        pcg_rtol=1e-13, theta_solver=getattr(mv, "SOLVER_" + solver))
            e_th = float(np.max(np.abs(th - ref.theta)) / np.max(np.abs(ref.theta)))
            e_u = float(np.max(np.abs(u - ref.u)) / max(1.0, np.max(np.abs(ref.u))))
            print(f"{R.case_id(c)} {solver}: iters {st['iters']} ({ref.iters}) rho {rho} ({ref.rho}) theta {e_th:.2e} "
                  f"u {e_u:.2e}")
            log_parity(f"nominal admm {R.case_id(c)} {solver}", theta=e_th, u=e_u, iters=int(ref.iters))
            assert st["theta_solver"] == getattr(mv, "SOLVER_" + solver) and st["pcg_unconverged"] == 0
            assert st["iters"] == ref.iters
            assert rho == ref.rho and st["rho"] == ref.rho
            assert e_th <= 1e-9 and e_u <= 1e-9
            if tuple(m) in FUSED:   # the fused pass ran, in the nominal order's instantiation
                k = FUSED[tuple(m)]
                fused = {n for n, _, _ in log if n.startswith(("k_admm3a", "k_admm4a", "k_admm2d"))}
                expect = {f"{k}<{ORD[order]}, {um}, false, {nb}, false>" for um in (0, 1)}
                # the log keeps a run's last 8192 launches: a PCG run's first iteration (u explicit in the edge
                # buffer, UM = 0) may have left it, the later ones (u read from z, UM = 1) cannot
                if log[0][0].startswith("#"):
                    assert solver != "SPECTRAL" and expect - {f"{k}<{ORD[order]}, 0, false, {nb}, false>"} <= fused
                    assert fused <= expect, fused
                else:
                    assert fused == expect, fused


@pytest.mark.parametrize("v", R.VARIANT_CASES, ids=lambda v: f"{v[0]}-{_mid(v[1])}")
def test_variants_A_and_C(v):
    var, m, order, weighted, lam, tol = v
    ref, margin = R.variant_run(v)
    assert margin >= R.MARGIN and ref.iters >= 2
    oty, _, ym = R.data(m, "I")
    with _problem(m, oty=oty, order=order, weighted=weighted) as P:
        th, u, rho, st = P.admm(lam, np.full(oty.size, ym), u=None, rho=None, ymean=ym, tol=tol, pcg_rtol=1e-13,
                                variant=mv.VARIANT_CPP if var == "A" else mv.VARIANT_PY)
    e_th = float(np.max(np.abs(th - ref.theta)) / np.max(np.abs(ref.theta)))
    e_u = float(np.max(np.abs(u - ref.u)) / max(1.0, np.max(np.abs(ref.u))))
    print(f"variant {var} {_mid(m)}: iters {st['iters']} ({ref.iters}) rho {rho} ({ref.rho}) theta {e_th:.2e} u {e_u:.2e}")
    assert st["iters"] == ref.iters and rho == ref.rho
    assert e_th <= 1e-9 and e_u <= 1e-9


def test_nominal_fit_differs_from_the_reference_fit():
    m = (8, 8, 8)
    oty, _, ym = R.data(m, "I")
    fits = []
    for order in (mv.ORDER_CPP, mv.ORDER_CPP_NOMINAL):
        with mv.Problem(list(m), oty, deltas=R.deltas_of(m), order=order) as P:
            info = P.block_info()
            th, _, _, st = P.admm(R.LAM, np.full(oty.size, ym), u=np.zeros(P.E), rho=R.LAM / 5.0)
        fits.append((th, info, st["iters"]))
    (a, ia, _), (b, ib, _) = fits
    assert [r[1] for r in ia].count(0b101) == 2 and 0b110 not in [r[1] for r in ia]   # {1,2} acts as {0,2}
    assert sorted(r[1] for r in ib) == [1, 2, 3, 4, 5, 6, 7]
    ref, _ = R.slu((m, "cpp", True, "I"))
    assert np.max(np.abs(b - ref.theta)) <= 1e-9 * np.max(np.abs(ref.theta))
    assert np.max(np.abs(a - b)) >= 1e-4 * np.max(np.abs(b))


@pytest.mark.parametrize("m", [(33, 31), (20,)], ids=_mid)
def test_same_results_up_to_two_dims(m):
    oty, W, ym = S.problem(list(m), "S")
    N = oty.size
    out = []
    for order in (mv.ORDER_CPP, mv.ORDER_CPP_NOMINAL):
        with mv.Problem(list(m), oty, wdiag=W, deltas=R.deltas_of(m), order=order) as P:
            x = np.random.default_rng(9).standard_normal(N)
            with launch_log() as log:
                res = [P.apply_D(x), P.apply_A(0.37, x), np.array(P.lambda_max())]
                th, u, rho, st = P.admm(0.5, np.full(N, ym), u=np.zeros(P.E), rho=0.1, fixed_iters=12)
            out.append((res + [th, u, np.array([rho, st["r_norm"], st["s_norm"]])], [n for n, _, _ in log]))
    (a, la), (b, lb) = out
    assert la == lb   # the instantiations of order 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------ path, lambda_max
def test_path():
    m = (6, 5, 4)
    oty, W, ym = R.data(m, "S")
    ref, margin = R.path_ref(m)
    assert margin >= R.MARGIN
    with _problem(m, oty=oty, wdiag=W) as P:
        thetas, rhos, stats = P.path(R.PATH_LAMS, np.full(oty.size, ym), R.PATH_LAMS[0] / 5.0, pcg_rtol=1e-13)
    assert [s["iters"] for s in stats] == [r.iters for r in ref]
    assert list(rhos) == [r.rho for r in ref]
    for th, r in zip(thetas, ref):
        assert np.max(np.abs(th - r.theta)) <= 1e-9 * np.max(np.abs(r.theta))


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=_lid)
def test_lambda_max(layout):
    c = R.LamMaxCase((6, 5, 4), *layout)
    ref, it_ref = O.lam_max_pinv_rcpp(R.build_D(c.m, c.blocks), c.b)
    with _problem(c.m, oty=c.b, order=layout[0], weighted=layout[1], deltas=c.deltas) as P:
        v, it = P.lambda_max()
    print(f"lambda_max 6x5x4 {_lid(layout)}: {v} ({ref}), {it} ({it_ref}) iterations, closed form {c.closed_form[0]}")
    assert it == it_ref
    assert abs(v - ref) <= 1e-9 * ref
    assert abs(v - c.closed_form[0]) <= 1e-9 * c.closed_form[0]


# ------------------------------------------------------------------------------------------ batched fits
@pytest.mark.parametrize("wk", ["I", "S"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("layout", [("cpp", True), ("py", False)], ids=_lid)
@pytest.mark.parametrize("m", [(6, 5, 4), (5, 4, 3, 2)], ids=_mid)
def test_path_batch(m, layout, mode, wk):
    order, weighted = layout
    oty, W, ym = R.data(m, wk)
    N = oty.size
    ref, margin = R.slu((m, order, weighted, wk))
    assert margin >= R.MARGIN
    with _problem(m, oty=oty, wdiag=W, order=order, weighted=weighted) as P:
        assert P.batch_ok()
        P.batch_cosine(mode)
        # two members with the same data: a grid of more than one workgroup
        thetas, us, rhos, stats, status = P.path_batch(np.stack([oty, oty]), [R.LAM], np.full((2, N), ym),
                                                       [R.LAM / 5.0] * 2, wdiag=None if W is None else
                                                       np.stack([W, W]), want_u=True, pcg_rtol=1e-13)
        th1, u1, rho1, st1 = P.admm(R.LAM, np.full(N, ym), u=np.zeros(P.E), rho=R.LAM / 5.0, pcg_rtol=1e-13)
    assert status == 0
    want = mv.SOLVER_SPECTRAL if (mode == 1 and wk == "I") else mv.SOLVER_PCG
    for b in range(2):
        st = stats[b][0]
        assert st["theta_solver"] == want and st["pcg_unconverged"] == 0
        assert st["iters"] == ref.iters == st1["iters"]
        assert st["rho"] == ref.rho == rho1 and rhos[b, 0] == ref.rho
        for th, u in ((ref.theta, ref.u), (th1, u1)):
            assert np.max(np.abs(thetas[b, 0] - th)) <= 1e-9 * np.max(np.abs(th))
            assert np.max(np.abs(us[b] - u)) <= 1e-9 * max(1.0, np.max(np.abs(u)))


# ------------------------------------------------------------------------------------------ the CV driver
def test_cv_driver_on_4x5x6():
    n, m = 300, [4, 5, 6]
    rng = np.random.default_rng(17)
    x = rng.uniform(0, 1, size=(n, 3))
    y = np.where(np.all(x > 0.45, axis=1), 1.0, 0.0) + 0.5 * x[:, 0] + 0.3 * rng.standard_normal(n)
    with pytest.raises(mv.DimMismatchError):
        cv.mbs_impl(x, y, m, n_lambda=8, folds=5, seed=3, group=False)
    kw = dict(n_lambda=8, folds=5, seed=3, group=False, nominal=True)
    plain = cv.mbs_impl(x, y, m, **kw)
    batched = cv.mbs_impl(x, y, m, batched=True, **kw)
    device = cv.mbs_impl(x, y, m, batched=True, device_cv=True, **kw)
    lam = [md["lambda"] for md in plain["models"]]
    for out in (batched, device):
        assert [md["lambda"] for md in out["models"]] == lam
        assert out["lambda_minmse_ind"] == plain["lambda_minmse_ind"]
    assert len(lam) == 8 and np.all(np.diff(lam) < 0)
    # the device scores the fits of batched=True: both within (k + 4) u of the exact MSE, k <= n points an entry
    assert np.all(np.abs(device["cv.mses"] - batched["cv.mses"]) <= 2 * (n + 4) * U * batched["cv.mses"])
    for a, b in zip(device["models"], batched["models"]):
        assert np.array_equal(a["theta_hat"], b["theta_hat"])
        assert abs(a["mse"] - b["mse"]) <= 2 * (n + 4) * U * b["mse"]
    # the unbatched legs solve theta by PCG under the spectral preconditioner at pcg_rtol 1e-10, the batched ones by
    # Jacobi-PCG in the workgroup: different fits of the same problems
    assert np.allclose(plain["cv.mses"], batched["cv.mses"], rtol=1e-7, atol=0)
    for a, b in zip(plain["models"], batched["models"]):
        assert np.max(np.abs(a["theta_hat"] - b["theta_hat"])) <= 1e-7 * max(1.0, np.max(np.abs(b["theta_hat"])))
    assert np.max(np.abs(plain["theta_hat"] - batched["theta_hat"])) <= 1e-7 * np.max(np.abs(batched["theta_hat"]))
