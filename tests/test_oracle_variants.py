"""Pin the matrix-free variant A / C loops (oracle/variants_spectral.py: C-oracle D / D^T, exact DCT solve) against
the SuperLU loops of oracle/mvtv_oracle.py and against the reference's own variant-A outputs (tests/golden/cpp_*)."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import mvtv_oracle as O

c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd.synth import towers  # noqa: E402
from oracle import variants_spectral as V  # noqa: E402

MESHES = [[12, 12, 8], [5, 5, 5, 3], [14, 9]]
LAYOUTS = [("cpp", True), ("cpp", False), ("py", True), ("py", False)]


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, list) else str(v)


def _problem(m, order, weighted):
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    blocks = O.block_table(len(m), deltas if (weighted or order == "cpp") else None, order, unit_weights=not weighted)
    return y, deltas, O.build_D(m, blocks)


@pytest.mark.parametrize("m", [[6, 6, 5], [4, 4, 4, 3]], ids=_id)
def test_apply_Dt_matches_matrix(m):
    rng = np.random.default_rng(3)
    for order, weighted in LAYOUTS:
        _, deltas, D = _problem(m, order, weighted)
        o, w = (0 if order == "cpp" else 1), int(weighted)
        assert c_oracle.num_edges(m, o, w) == D.shape[0]
        v = rng.standard_normal(D.shape[0])
        ref = D.T @ v
        got = c_oracle.apply_Dt(m, v, deltas, o, w)
        assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref))), (order, weighted)
        th = rng.standard_normal(D.shape[1])
        assert np.max(np.abs(c_oracle.apply_D(m, th, deltas, o, w) - D @ th)) <= 1e-13, (order, weighted)
    with pytest.raises(ValueError):
        c_oracle.apply_Dt(m, np.zeros(3), deltas)


def _same_run(ref, got):
    assert got.iters == ref.iters
    assert got.rho == ref.rho
    assert np.max(np.abs(got.theta - ref.theta)) <= 1e-10
    assert np.max(np.abs(got.u - ref.u)) <= 1e-10
    assert len(got.history) == len(ref.history) == ref.iters
    np.testing.assert_allclose([h["dtheta_max"] for h in got.history], [h["dtheta_max"] for h in ref.history],
                               rtol=1e-10, atol=0.0)


@pytest.mark.parametrize("order,weighted", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("lam", [2.0, 30.0])
@pytest.mark.parametrize("m", MESHES, ids=_id)
def test_variant_a_matches_superlu_loop(m, lam, order, weighted):
    y, deltas, D = _problem(m, order, weighted)
    th0 = np.full(y.size, y.mean())
    ref = O.admm_cpp(D, y, np.ones(y.size), lam, th0, y.mean(), record=True)
    got = V.admm_cpp_spectral(m, y, lam, th0, y.mean(), deltas, order=order, weighted=weighted)
    _same_run(ref, got)
    for hr, hg in zip(ref.history, got.history):
        assert hg["rho"] == hr["rho"]
        assert hg["r_norm"] == pytest.approx(hr["r_norm"], rel=1e-10, abs=1e-14)
        assert hg["s_norm"] == pytest.approx(hr["s_norm"], rel=1e-10, abs=1e-14)
    assert len(got.stop_margins) == got.iters + 1
    # the trajectory mode and an explicit u0 take the same statements
    rng = np.random.default_rng(5)
    u0 = 1.0 / lam + 0.01 * rng.standard_normal(D.shape[0])
    ref = O.admm_cpp(D, y, np.ones(y.size), lam, th0, y.mean(), fixed_iters=3, record=True, u0=u0)
    got = V.admm_cpp_spectral(m, y, lam, th0, y.mean(), deltas, order=order, weighted=weighted, fixed_iters=3, u0=u0)
    _same_run(ref, got)
    assert got.stop_margins == []


@pytest.mark.parametrize("order,weighted", LAYOUTS, ids=lambda v: str(v))
@pytest.mark.parametrize("m", MESHES, ids=_id)
def test_variant_c_matches_superlu_loop(m, order, weighted):
    y, deltas, D = _problem(m, order, weighted)
    th0 = np.full(y.size, y.mean())
    ref = O.admm_py(D, y, np.ones(y.size), 2.0, th0, y.mean(), record=True)
    got = V.admm_py_spectral(m, y, 2.0, th0, y.mean(), deltas, order=order, weighted=weighted)
    _same_run(ref, got)
    assert len(got.stop_margins) == got.iters + 1
    ref = O.admm_py(D, y, np.ones(y.size), 2.0, th0, y.mean(), tol=1e-2, record=True)
    got = V.admm_py_spectral(m, y, 2.0, th0, y.mean(), deltas, order=order, weighted=weighted, tol=1e-2)
    _same_run(ref, got)
    assert got.iters < len(got.stop_margins) and got.history[-1]["dtheta_max"] <= 1e-2


def test_solve_callable_with_a_superlu_factor():
    """W != I: the loop takes the caller's solve(sigma, b); with the factor admm_cpp builds it is the same loop."""
    from scipy.sparse import diags
    from scipy.sparse.linalg import splu
    m = [9, 9, 4]
    y, deltas, D = _problem(m, "cpp", True)
    W = (np.random.default_rng(9).permutation(y.size) % 5 < 3).astype(float)
    oty = W * y
    ym = float(oty.sum() / W.sum())
    th0 = np.full(y.size, ym)
    crossD = (D.T @ D).tocsc()

    def solve(sigma, b):
        return splu((diags(W) + sigma * crossD).tocsc()).solve(b)

    ref = O.admm_cpp(D, oty, W, 30.0, th0, ym, record=True)
    got = V.admm_cpp_spectral(m, oty, 30.0, th0, ym, deltas, solve=solve)
    _same_run(ref, got)


@pytest.mark.parametrize("name", ["cpp_2d_16", "cpp_3d_8_unit", "cpp_2d_12_frac"])
def test_variant_a_matches_reference_outputs(name):
    """The assertions of test_oracle_golden.test_cpp_variant, on the matrix-free loop."""
    meta, g = load_golden(name)
    m = meta["m"]
    res = V.admm_cpp_spectral(m, g["y"], meta["lam"], g["theta0"], meta["ymean"], meta["deltas"], order="cpp",
                              weighted=not meta["unit"])
    assert res.iters == meta["iters"]
    assert res.rho == meta["rho"]
    assert np.max(np.abs(res.theta - g["theta"])) <= 1e-11 * np.max(np.abs(g["theta"]))
    hist = np.array([[h["r_norm"], h["s_norm"], h["rho"]] for h in res.history])
    np.testing.assert_allclose(hist, g["hist"], rtol=1e-8, atol=1e-14)
