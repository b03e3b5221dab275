"""The whole k-fold CV of a batch-admitted mesh as one call on the device (mvtv_cv_batch, Problem.cv_batch,
cv.mbs_impl(batched=True, device_cv=True); kernels k_fold_sums and k_cv_mse of multivartv_amd/csrc/mvtv_cv.hip;
DESIGN.md §2.10). Every case is a 5-lambda path (small_batch_cases.LAMS) on at most 1000 points.

1. Device setup = host setup: the members cv_batch builds on the device give the fits Problem.path_batch gives on the
   members cv.mbs_impl(batched=True) builds on the host (nearest + interp_weights): thetas, rhos and every stats field
   but `seconds` equal, bit for bit.
2. The same on adversarial runs (a node of 300 points, a node inside one fold, empty nodes, +-1e16 / 1 interleaved).
3. The scoring kernel against exact arithmetic: |gpu - exact| <= (k + 4) 2^-53 exact for an entry of k points (one
   rounding for the difference and one for the square give (1 + u)^3 per non-negative term, at most k - 1 roundings
   for any summation order, one for the division).
4. - 6. cv.mbs_impl(batched=True, device_cv=True) against the oracle (as test_batched_mbs_impl_matches_oracle), against
   the host-setup driver, and its launch log.
7. Refusals, after each of which the same problem still runs a valid call.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import cv_batch_cases as K
import small_batch_cases as S

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import _lib, cv  # noqa: E402
from multivartv_amd.utils import create_deltas, interp_weights  # noqa: E402

pytestmark = pytest.mark.gpu

LAMS = K.LAMS
U = 2.0 ** -53


def _problem(m, x):
    """The problem cv.mbs_impl makes for (x, m), and the axes of its mesh."""
    axes = cv.tensor_axes(cv.create_mesh(x, m), m)
    P = _lib.Problem(m, np.zeros(int(np.prod(m))), deltas=create_deltas(x, m), order=_lib.ORDER_CPP, weighted=True)
    return P, axes


def _host_members(P, axes, x, y, fold, folds):
    """(O^T y, W, theta_0 scalar) per member, as cv.mbs_impl(batched=True) builds them."""
    out = []
    for item in range(1 + (folds if folds > 1 else 0)):
        tr = slice(None) if item == 0 else fold != item - 1
        idx = P.nearest(axes, x[tr])
        W, oty = interp_weights(idx, P.N, y[tr])
        out.append((oty, W, y[tr].mean()))
    return out


def _assert_same_fits(P, axes, x, y, fold, folds, **opts):
    """Assertion 1; returns cv_batch's result."""
    mem = _host_members(P, axes, x, y, fold, folds)
    B = len(mem)
    res = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=folds, theta0=[mb[2] for mb in mem], want_fold_thetas=True,
                     **opts)
    thetas, _, rhos, stats, status = P.path_batch(
        np.stack([mb[0] for mb in mem]), LAMS, np.stack([np.full(P.N, mb[2]) for mb in mem]),
        np.full(B, LAMS[0] / 5.0), wdiag=np.stack([mb[1] for mb in mem]), **opts)
    assert np.all(np.isfinite(thetas))
    assert np.array_equal(res["thetas"][0], thetas[0, 0])          # the members' first-lambda theta ...
    for b in range(1, B):
        assert np.array_equal(res["fold_thetas"][b - 1, 0], thetas[b, 0]), b
    assert np.array_equal(res["thetas"], thetas[0])                # ... and every lambda's
    assert np.array_equal(res["fold_thetas"], thetas[1:])
    assert np.array_equal(res["rhos"], rhos)
    assert res["status"] == status
    for b in range(B):
        for l in range(len(LAMS)):
            a, r = dict(res["stats"][b][l]), dict(stats[b][l])
            a.pop("seconds"), r.pop("seconds")
            assert a == r, (b, l)
    assert np.array_equal(res["mesh_index"], P.nearest(axes, x))
    return res


def _exact_mean_sq(theta_at, target):
    """mean((theta_at - target)^2) from long double terms summed without error (math.fsum over each term's two double
    halves, and once more for the remainder of the rounded sum), as a long double."""
    d = theta_at.astype(np.longdouble) - target.astype(np.longdouble)
    t = d * d
    hi = t.astype(np.float64)
    lo = (t - hi.astype(np.longdouble)).astype(np.float64)
    parts = list(hi) + list(lo)
    s = math.fsum(parts)
    r = math.fsum(parts + [-s])
    return (np.longdouble(s) + np.longdouble(r)) / np.longdouble(theta_at.size)


def _assert_scores_exact(res, y, ref, fold, folds):
    """Assertion 3 on one cv_batch result (with fold thetas)."""
    idx = res["mesh_index"]
    worst = 0.0
    for l in range(len(LAMS)):
        entries = [(res["model_mses"][l], res["thetas"][l][idx], ref)]
        if folds <= 1:
            entries.append((res["mse_mat"][l, 0], res["thetas"][l][idx], y))
        else:
            for f in range(folds):
                te = fold == f
                entries.append((res["mse_mat"][l, f], res["fold_thetas"][f, l][idx[te]], y[te]))
        for got, th, target in entries:
            k = target.size
            exact = _exact_mean_sq(th, target)
            err = abs(np.longdouble(got) - exact)
            worst = max(worst, float(err / (exact * U)) / (k + 4))
            assert err <= (k + 4) * np.longdouble(U) * exact, (l, k, float(got), float(exact))
    print(f"scoring: worst |gpu - exact| / ((k + 4) u exact) = {worst:.3f}")


# ---- 1, 3: per case ---------------------------------------------------------------------------------------
SETUP_CASES = [(c, 0) for c in K.CASES] + [(c, 2) for c in K.CASES if c[0] == [10, 10]]


@pytest.mark.parametrize("case,cosine", SETUP_CASES, ids=[f"{K.case_id(c)}-cos{k}" for c, k in SETUP_CASES])
def test_device_setup_equals_host_setup_and_scores_are_exact(case, cosine):
    m, n, folds = case
    x, y, fold = K.data(case)
    P, axes = _problem(m, x)
    with P:
        if cosine:
            P.batch_cosine(cosine)
        res = _assert_same_fits(P, axes, x, y, fold, folds)
        if cosine:
            assert {st["theta_solver"] for sts in res["stats"] for st in sts} == {_lib.SOLVER_PCG_SPECTRAL}
    _assert_scores_exact(res, y, y, fold, folds)


# ---- 2: adversarial sums --------------------------------------------------------------------------------------
def test_adversarial_sums():
    axes, x, y, fold, node = K.adversarial()
    members, N = 4, 20
    W, oty = K.fold_sums_model(node, y, fold, N, members)
    with _lib.Problem([20], np.zeros(N), deltas=[1.0], order=_lib.ORDER_CPP, weighted=True) as P:
        assert np.array_equal(P.nearest(axes, x), node)
        mem = _host_members(P, axes, x, y, fold, 3)
        # the host members are the left-to-right sums of the model, which are not the exact sums
        assert np.array_equal(np.stack([mb[0] for mb in mem]), oty) and np.array_equal(np.stack([mb[1] for mb in mem]), W)
        assert W[0, 3] == 300 and W[2, 7] == 0 and W[1, 7] == 40 and oty[0, 3] != math.fsum(y[node == 3])
        _assert_same_fits(P, axes, x, y, fold, 3)


# ---- 3: many points a thread ----------------------------------------------------------------------------------
def test_scores_exact_with_several_points_a_thread():
    """n = 1000 on 31 x 33 with three folds: every thread of k_cv_mse's 256 holds several points of the final member,
    and the folds' 333 or 334 test points are spread over the strided order."""
    m, n, folds = [31, 33], 1000, 3
    x, y = K.scattered(n, 2, seed=23)
    fold = cv.kfoldinds(n, folds, K.FOLD_SEED)
    ref = np.where(np.all(x > 0.6, axis=1), 1.0, 0.0)
    P, axes = _problem(m, x)
    with P:
        res = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=folds, ref=ref, want_fold_thetas=True)
        again = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=folds, ref=ref, want_fold_thetas=True)
    _assert_scores_exact(res, y, ref, fold, folds)
    assert np.array_equal(res["mse_mat"], again["mse_mat"]) and np.array_equal(res["model_mses"], again["model_mses"])


def test_default_start_is_the_sequential_mean():
    """theta0 = None: each member starts from the mean of its y summed in data order (the C++ host's mean())."""
    case = ([10, 10], 100, 5)
    x, y, fold = K.data(case)
    th0 = []
    for b in range(6):
        s, k = 0.0, 0
        for i in range(y.size):
            if b == 0 or fold[i] != b - 1:
                s, k = s + y[i], k + 1
        th0.append(s / k)
    P, axes = _problem(case[0], x)
    with P:
        a = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=5, want_fold_thetas=True)
        b = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=5, theta0=th0, want_fold_thetas=True)
    assert np.array_equal(a["thetas"], b["thetas"]) and np.array_equal(a["fold_thetas"], b["fold_thetas"])
    assert np.array_equal(a["mse_mat"], b["mse_mat"])


# ---- 4, 5, 6: the driver ----------------------------------------------------------------------------------------
def _log_now():
    """The launch log so far, parsed as _lib.launch_log does, without ending the recording."""
    L = _lib.lib()
    n = int(L.mvtv_launch_log_read(None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    L.mvtv_launch_log_read(buf, n + 1)
    out = []
    for line in buf.value.decode().splitlines():
        assert not line.startswith("#"), line   # the ring has not overflowed
        name, grid, block = line.split("\t")
        out.append((name, tuple(int(v) for v in grid.split()), tuple(int(v) for v in block.split())))
    return out


@functools.lru_cache(maxsize=None)
def _host_driver(case):
    m, n, folds = case
    x, y, _ = K.data((list(m), n, folds))
    return cv.mbs_impl(x, y, list(m), lambdas=LAMS, folds=folds, seed=K.FOLD_SEED, group=False, batched=True)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_device_cv_driver(case, monkeypatch):
    m, n, folds = case
    x, y, fold = K.data(case)
    host = _host_driver((tuple(m), n, folds))   # before Problem.admm is wrapped: its folds = 1 refit calls it too
    # the log is read when the C call begins and ends, and when the folds = 1 refit begins (the refit's five launches
    # a PCG iteration can overrun the ring, as in tests/test_gpu_small_batch_cv.py)
    marks = []
    plain_admm, plain_cvb = mv.Problem.admm, mv.Problem.cv_batch

    def admm(self, *a, **kw):
        marks.append(("refit", _log_now()))
        return plain_admm(self, *a, **kw)

    def cv_batch(self, *a, **kw):
        marks.append(("begin", _log_now()))
        out = plain_cvb(self, *a, **kw)
        marks.append(("end", _log_now()))
        return out
    monkeypatch.setattr(mv.Problem, "admm", admm)
    monkeypatch.setattr(mv.Problem, "cv_batch", cv_batch)
    with _lib.launch_log() as log:
        out = cv.mbs_impl(x, y, m, lambdas=LAMS, folds=folds, seed=K.FOLD_SEED, group=False, batched=True,
                          device_cv=True)
    assert fold is None or np.array_equal(fold, cv.kfoldinds(n, folds, K.FOLD_SEED))

    # 4. against the oracle
    ref = K.oracle(case)
    assert K.cv_gap(ref["cv_mses"]) >= 1e-5
    assert out["lambda_minmse_ind"] == ref["best"] + 1
    assert np.allclose(out["cv.mses"], ref["cv_mses"], rtol=1e-7, atol=0)
    scale = np.max(np.abs(ref["best_theta"]))
    assert np.max(np.abs(out["theta_hat"] - ref["best_theta"])) <= 1e-7 * scale
    for i, r in enumerate(ref["final"]):
        assert np.max(np.abs(out["models"][i]["theta_hat"] - r.theta)) <= 1e-7 * max(1.0, np.max(np.abs(r.theta)))

    # 5. against the host-setup driver: the same fits, the same selection, and MSEs within 2 (k + 4) u, both sides
    # being within (k + 4) u of the exact value, k the entry's point count. An entry of cv.mses is made from all n
    # points: with F folds of k_f points it takes 3 roundings a term, k_f - 1 for a fold's sum, its division, F - 1
    # for the row sum and its division, k_f + F + 3 <= n + 4 in all since every other fold holds a point: k = n.
    for a, b in zip(out["models"], host["models"]):
        assert np.array_equal(a["theta_hat"], b["theta_hat"])
    assert np.all(np.abs(out["cv.mses"] - host["cv.mses"]) <= 2 * (n + 4) * U * host["cv.mses"])
    for a, b in zip(out["models"], host["models"]):
        assert abs(a["mse"] - b["mse"]) <= 2 * (n + 4) * U * b["mse"]
    assert out["lambda_minmse_ind"] == host["lambda_minmse_ind"]

    # 6. the launch log of the C call, and of the driver up to the refit
    assert [t for t, _ in marks] == ["begin", "end"] + (["refit"] if folds == 1 else [])
    call = marks[1][1][len(marks[0][1]):]
    members = 1 + (folds if folds > 1 else 0)
    names = [e[0] for e in call]
    assert names.count(f"k_nearest<{len(m)}>") == 1 and sum(nm.startswith("k_nearest") for nm in names) == 1
    assert names.count("k_fold_sums") == 1 and names.count("k_cv_mse") == 1
    assert call[names.index("k_cv_mse")][1] == (len(LAMS) * members, 1, 1)
    name = S.instantiation(m)
    nt = S.nt_rule(int(np.prod(m)))
    small = [e for e in call if e[0].startswith("k_admm_small")]
    assert small and all(e == (name, (members, 1, 1), (nt, 1, 1)) for e in small)
    first, last = call.index(small[0]), len(call) - 1 - call[::-1].index(small[-1])
    assert call[first:last + 1] == small
    assert names.index("k_fold_sums") < first and last < names.index("k_cv_mse")
    upto = marks[2][1] if folds == 1 else log
    loop = ("k_edge_update", "k_edge3d", "k_gather", "k_pcg", "k_admm_control", "k_admm3d", "k_cg3d")
    assert not [e for e in upto if e[0].startswith(loop)]


# ---- 7: refusals ------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(_lib.MvtvError) as e:
        fn()
    assert e.value.status == _lib.MVTV_BAD_ARG


def test_refusals_leave_the_problem_usable():
    case = ([10, 10], 100, 2)
    m = case[0]
    x, y, fold = K.data(case)
    P, axes = _problem(m, x)
    with P:
        good = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=2)

        def valid():
            again = P.cv_batch(axes, x, y, LAMS, fold=fold, folds=2)
            assert np.array_equal(again["mse_mat"], good["mse_mat"]) and np.array_equal(again["thetas"], good["thetas"])
        bad = fold.copy()
        bad[17] = 2                                   # a label = folds
        _refused(lambda: P.cv_batch(axes, x, y, LAMS, fold=bad, folds=2))
        valid()
        bad[17] = -1
        _refused(lambda: P.cv_batch(axes, x, y, LAMS, fold=bad, folds=2))
        valid()
        _refused(lambda: P.cv_batch(axes, x, y, LAMS, fold=fold, folds=3))             # fold 2 has no point
        valid()
        _refused(lambda: P.cv_batch(axes, x, y, LAMS, fold=np.zeros(100, dtype=int), folds=2))   # all points in fold 0
        valid()
        xn = x.copy()
        xn[5, 1] = np.nan
        _refused(lambda: P.cv_batch(axes, xn, y, LAMS, fold=fold, folds=2))
        valid()
        _refused(lambda: P.cv_batch(axes, x, y, [1.0, -0.5], fold=fold, folds=2))       # what path_batch refuses
        valid()
        _refused(lambda: P.cv_batch(axes, x, y, LAMS, fold=fold, folds=2, theta_solver=_lib.SOLVER_SPECTRAL))
        valid()
    xb, yb = K.scattered(400, 2, seed=1)
    Pb, axb = _problem([100, 100], xb)
    with Pb:
        _refused(lambda: Pb.cv_batch(axb, xb, yb, LAMS))                               # a 100 x 100 mesh
        assert Pb.nearest(axb, xb).shape == (400,)


def test_driver_refusals():
    x, y = K.scattered(400, 2, seed=1)
    with pytest.raises(ValueError):
        cv.mbs_impl(x, y, [10, 10], lambdas=LAMS, folds=1, group=False, device_cv=True)
    with pytest.raises(ValueError):
        cv.mbs_impl(x, y, [10, 10], lambdas=LAMS, folds=1, group=False, batched=True, device_cv=True,
                    _runner=lambda kind, f: (np.zeros(len(LAMS)), None))
    with pytest.raises(ValueError):
        cv.mbs_impl(x, y, [100, 100], lambdas=LAMS, folds=1, group=False, batched=True, device_cv=True)
    mesh = cv.create_mesh(x, [10, 10])[::-1].copy()                                     # not a tensor product
    with pytest.raises(ValueError):
        cv.mbs_impl(x, y, [10, 10], mesh=mesh, lambdas=LAMS, folds=1, group=False, batched=True, device_cv=True)
    out = cv.mbs_impl(x, y, [10, 10], lambdas=LAMS, folds=2, group=False, batched=True, device_cv=True)
    assert 1 <= out["lambda_minmse_ind"] <= len(LAMS)
