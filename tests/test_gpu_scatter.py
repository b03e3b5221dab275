"""GPU parity of the scattered-data setup through the C ABI:
nearest1 / nearest_interp_matrix (rcpp-code/MultivarTV/src/utils.cpp:267-304), create_cache_objects'
diag(O^T O) and O^T y (rcpp…/solvers.cpp:36-44) and mbs_predict (:161-165).

The checker is the oracle's brute-force scan over every mesh row (oracle/mvtv_oracle.py
nearest_index, first minimum as arma's index_min) and numpy's bincount (sequential per-node sums in
data order). Bar: mesh indices identical; W and O^T y bit-identical, shown by ADMM runs from the GPU
setup and from the host setup agreeing bit for bit."""
import numpy as np
import pytest

import nearest_ref as NR
from oracle import mvtv_oracle as O

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import cv  # noqa: E402
from multivartv_amd._lib import MVTV_BAD_ARG  # noqa: E402

pytestmark = pytest.mark.gpu


def _points(n, p, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, size=(n, p)), rng.standard_normal(n)


def _axes(x, m):
    mesh = cv.create_mesh(x, m)
    axes = cv.tensor_axes(mesh, m)
    assert axes is not None
    return mesh, axes


@pytest.mark.parametrize("m,n", [([50], 400), ([12, 9], 500), ([8, 8, 8], 700), ([5, 5, 5, 5], 600)])
def test_nearest_matches_bruteforce(m, n):
    x, _ = _points(n, len(m), seed=sum(m))
    mesh, axes = _axes(x, m)
    # edge cases: points on nodes, on cell midpoints (near-ties), outside the mesh box
    extra = [mesh[3], mesh[-1], 0.5 * (mesh[0] + mesh[1]), mesh[0] - 1.0, mesh[-1] + 1.0]
    x = np.vstack([x, np.array(extra)])
    with mv.Problem(m, np.zeros(int(np.prod(m)))) as P:
        got = P.nearest(axes, x)
    np.testing.assert_array_equal(got, O.nearest_index(x, mesh))


def test_nearest_exact_ties_take_lower_node():
    m = [5, 4]
    axes = [np.arange(5.0), np.arange(4.0)]
    mesh = np.stack([g.reshape(-1, order="F") for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    x = np.array([[0.5, 0.5], [1.5, 2.0], [3.0, 2.5], [3.5, 2.5], [4.0, 3.0]])
    with mv.Problem(m, np.zeros(20)) as P:
        got = P.nearest(axes, x)
    np.testing.assert_array_equal(got, O.nearest_index(x, mesh))
    np.testing.assert_array_equal(got, [0, 11, 13, 13, 19])


@pytest.mark.parametrize("m,n", [([16, 16], 3000), ([8, 8, 8], 300), ([32, 32], 1024)])
def test_set_scattered_bit_identical_to_host_setup(m, n):
    x, y = _points(n, len(m), seed=7 + n)
    mesh, axes = _axes(x, m)
    N = int(np.prod(m))
    idx = O.nearest_index(x, mesh)
    W = np.bincount(idx, minlength=N).astype(float)
    oty = np.bincount(idx, weights=y, minlength=N)
    deltas = O.create_deltas_rcpp(x, m)
    th0 = np.full(N, y.mean())
    with mv.Problem(m, oty, wdiag=W, deltas=deltas, order=mv.ORDER_CPP) as Ph, \
            mv.Problem(m, np.zeros(N), deltas=deltas, order=mv.ORDER_CPP) as Pg:
        got_idx = Pg.set_scattered(axes, x, y)
        np.testing.assert_array_equal(got_idx, idx)
        # W itself: A x with sigma = 0 and x = 1 is W exactly
        np.testing.assert_array_equal(Pg.apply_A(0.0, np.ones(N)), W)
        rh = Ph.admm(0.05, th0, rho=0.01, fixed_iters=6, return_u=False)
        rg = Pg.admm(0.05, th0, rho=0.01, fixed_iters=6, return_u=False)
        np.testing.assert_array_equal(rg[0], rh[0])
        assert rg[2] == rh[2]


def test_one_point_per_node_gives_identity_weights():
    m = [16, 16]
    axes = [np.linspace(0, 1, 16), np.linspace(0, 2, 16)]
    grid = np.stack([g.reshape(-1, order="F") for g in np.meshgrid(*axes, indexing="ij")], axis=1)
    perm = np.random.default_rng(3).permutation(256)
    y = np.random.default_rng(4).standard_normal(256)
    with mv.Problem(m, np.zeros(256)) as P:
        idx = P.set_scattered(axes, grid[perm] + 1e-3, y)
        np.testing.assert_array_equal(idx, perm)
        assert P.spectral_ok()
        th = np.arange(256.0)
        P.state_set(th, None, 1.0)
        np.testing.assert_array_equal(P.apply_A(0.0, th), th)


def test_predict_is_theta_at_nearest_node():
    m = [10, 12]
    x, y = _points(400, 2, seed=11)
    mesh, axes = _axes(x, m)
    xt, _ = _points(77, 2, seed=12)
    with mv.Problem(m, np.zeros(120)) as P:
        P.set_scattered(axes, x, y)
        th = np.random.default_rng(5).standard_normal(120)
        P.state_set(th, None, 1.0)
        np.testing.assert_array_equal(P.predict(axes, xt), th[O.nearest_index(xt, mesh)])
        assert P.predict(axes, np.empty((0, 2))).size == 0


# ------------------------------------------------------------------------------------------------------------------
# The setup at the shapes where it can go wrong: non-uniform axes (k_nearest's first guess of the
# bracket is wrong and the binary search runs), edge points, the radix sort's end_bit boundaries, long and aligned runs
# of equal keys, a summation order only left-to-right reproduces, W = I detection, and the second trip of the
# grid-stride loops. Inputs and the fast reference: tests/nearest_ref.py (pinned in tests/test_nearest_ref_host.py);
# every point lies inside the domain stated there. The reference is the brute-force scan wherever n N <= 1e8.
def _ref_index(axes, x):
    assert NR.in_domain(axes, x).all()
    N = int(np.prod([len(a) for a in axes]))
    if len(x) * N <= 10 ** 8:
        return O.nearest_index(x, NR.mesh_of(axes))
    return NR.nearest_fast(axes, x)


def _check_setup(m, axes, x, y, Pg=None):
    """indices identical, W exact, O^T y bit-identical (ADMM from the GPU setup and from the host setup agree bit for
    bit); returns the indices"""
    N = int(np.prod(m))
    idx = _ref_index(axes, x)
    W = np.bincount(idx, minlength=N).astype(float)
    oty = np.bincount(idx, weights=y, minlength=N)
    deltas = [1.0 / v for v in m]
    th0 = np.full(N, 0.25)
    own = Pg is None
    identity = bool(np.all(W == 1.0))
    Pg = mv.Problem(m, np.zeros(N), deltas=deltas, order=mv.ORDER_CPP) if own else Pg
    try:
        with mv.Problem(m, oty, wdiag=None if identity else W, deltas=deltas, order=mv.ORDER_CPP) as Ph:
            got = Pg.set_scattered(axes, x, y)
            np.testing.assert_array_equal(got, idx)
            np.testing.assert_array_equal(Pg.nearest(axes, x[:1000]), idx[:1000])
            np.testing.assert_array_equal(Pg.apply_A(0.0, np.ones(N)), W)
            assert Pg.spectral_ok() == identity == Ph.spectral_ok()
            rh = Ph.admm(0.05, th0, rho=0.01, fixed_iters=4, return_u=False, theta_solver=mv.SOLVER_PCG)
            rg = Pg.admm(0.05, th0, rho=0.01, fixed_iters=4, return_u=False, theta_solver=mv.SOLVER_PCG)
            np.testing.assert_array_equal(rg[0], rh[0])
            assert rg[2] == rh[2]
    finally:
        if own:
            Pg.close()
    return idx


NONUNIFORM = [([97], "random"), ([2], "random"), ([4096], "geometric"), ([64, 64], "random"), ([2, 300], "geometric"),
              ([40, 2], "random"), ([16, 16, 16], "geometric"), ([12, 12, 2], "random"), ([8, 8, 8, 8], "random"),
              ([6, 6, 6, 2], "geometric"), ([9, 9, 9, 5], "integer")]


@pytest.mark.parametrize("m,kind", NONUNIFORM, ids=[f"{'x'.join(map(str, m))}-{k}" for m, k in NONUNIFORM])
def test_setup_on_nonuniform_axes_and_edge_points(m, kind):
    """n >= 20 000 over the widened box plus the edge points: on nodes, midpoints in 1 .. p dims at once (exact on the
    integer axes: the lower node), one ulp either side of both, outside every face, edge and corner by 1e-3, 1 and
    1e3 box widths"""
    rng = np.random.default_rng(41 + sum(m))
    # spacings within 1e3 of one another; within 4 on the long axes, so that 1e3 box widths outside stays inside the
    # domain of identical indices (nearest_ref.in_domain)
    spread = 1e3 if max(m) <= 64 else 4.0
    axes = NR.geometric_axes(m, rng, spread) if kind == "geometric" else NR.AXES[kind](m, rng)
    mids, low = NR.midpoint_points(axes, 3, rng)
    x = np.vstack([NR.box_points(axes, 20000, rng), NR.edge_points(axes, rng), mids])
    x = x[rng.permutation(len(x))]
    y = rng.standard_normal(len(x))
    _check_setup(m, axes, x, y)
    if kind == "integer":
        with mv.Problem(m, np.zeros(int(np.prod(m)))) as P:
            np.testing.assert_array_equal(P.nearest(axes, mids), low)


@pytest.mark.parametrize("N", [255, 256, 257, 4096, 4097])
def test_radix_end_bit_boundaries(N):
    """the sort covers ceil(log2 N) key bits: N one below, at and one above a power of two, points on node 0 and on
    node N - 1 (the key with every sorted bit set, or the only key with the top bit)"""
    rng = np.random.default_rng(N)
    axes = NR.random_axes([N], rng)
    x = np.concatenate([rng.uniform(axes[0][0], axes[0][-1], 3000), np.repeat(axes[0][[0, -1]], 5)])[:, None]
    x = x[rng.permutation(len(x))]
    idx = _check_setup([N], axes, x, rng.standard_normal(len(x)))
    assert idx.min() == 0 and idx.max() == N - 1


def _on_nodes(axes, nodes, rng):
    """points a little off the given nodes (well inside their cells)"""
    m = [len(a) for a in axes]
    sub = np.stack(np.unravel_index(nodes, m, order="F"), axis=1)
    x = np.stack([np.asarray(axes[j])[sub[:, j]] for j in range(len(m))], axis=1)
    return x + rng.uniform(-0.2, 0.2, x.shape) * np.array([np.min(np.diff(a)) for a in axes])


def test_every_node_hit_256_times():
    """run starts of the sorted order on workgroup boundaries (k_run_sums: 256 threads, a run per starting thread)"""
    rng = np.random.default_rng(51)
    m = [8, 8]
    axes = NR.random_axes(m, rng)
    nodes = rng.permutation(np.repeat(np.arange(64), 256))
    idx = _check_setup(m, axes, _on_nodes(axes, nodes, rng), rng.standard_normal(nodes.size))
    np.testing.assert_array_equal(np.bincount(idx), np.full(64, 256))


def test_one_long_run_among_sparse_others_and_a_second_setup():
    """300 000 points on one node (one thread sums a run that crosses 1172 workgroups) among 40 others, most nodes
    empty; then a second set_scattered on the same problem whose data leaves those nodes empty: no stale W or O^T y"""
    rng = np.random.default_rng(52)
    m = [16, 16]
    axes = NR.geometric_axes(m, rng)
    nodes = np.concatenate([np.full(300000, 137), rng.choice(128, 40, replace=False)])
    nodes = nodes[rng.permutation(nodes.size)]
    x, y = _on_nodes(axes, nodes, rng), rng.standard_normal(nodes.size)
    deltas = [1.0 / v for v in m]
    with mv.Problem(m, np.zeros(256), deltas=deltas, order=mv.ORDER_CPP) as Pg:
        idx = _check_setup(m, axes, x, y, Pg=Pg)
        np.testing.assert_array_equal(idx, nodes)
        assert np.count_nonzero(np.bincount(idx, minlength=256)) <= 41
        nodes2 = 128 + rng.choice(128, 30, replace=False)
        nodes2 = nodes2[nodes2 != 137]
        idx2 = _check_setup(m, axes, _on_nodes(axes, nodes2, rng), rng.standard_normal(nodes2.size), Pg=Pg)
        np.testing.assert_array_equal(idx2, nodes2)
        assert not np.intersect1d(idx, idx2).size


def test_summation_order_is_the_references():
    """runs of 1e16, 1, -1e16 in every order: left to right the sums are 0, 1 or 2 ulp-sized leftovers that no other
    order (pairwise, sorted, exact) reproduces; numpy's bincount adds in data order as the reference's sparse product
    does"""
    import math
    rng = np.random.default_rng(53)
    m = [4, 4]
    axes = NR.random_axes(m, rng)
    pat = np.array([1e16, 1.0, -1e16, 1.0, 3.0, -1e16, 1e16, 1.0])
    nodes, y = [], []
    for k in range(16):
        reps = 1 + k % 3
        v = np.concatenate([np.roll(pat, k)] * reps)
        nodes.append(np.full(v.size, k))
        y.append(v)
    nodes, y = np.concatenate(nodes), np.concatenate(y)
    perm = rng.permutation(nodes.size)   # the data order: nodes interleaved, magnitudes mixed within every run
    nodes, y = nodes[perm], y[perm]
    oty = np.bincount(nodes, weights=y, minlength=16)
    exact = np.array([math.fsum(y[nodes == k]) for k in range(16)])
    assert np.count_nonzero(oty != exact) >= 8   # the order matters on most nodes
    idx = _check_setup(m, axes, _on_nodes(axes, nodes, rng), y)
    np.testing.assert_array_equal(idx, nodes)


def test_identity_weights_are_detected_only_when_exact():
    """n = N with every node once: W = I, the spectral solve applies; n = N with one node twice and one empty: not"""
    rng = np.random.default_rng(54)
    m = [16, 16]
    axes = NR.random_axes(m, rng)
    nodes = rng.permutation(256)
    y = rng.standard_normal(256)
    with mv.Problem(m, np.zeros(256), deltas=[1 / 16, 1 / 16]) as P:
        np.testing.assert_array_equal(P.set_scattered(axes, _on_nodes(axes, nodes, rng), y), nodes)
        assert P.spectral_ok()
        np.testing.assert_array_equal(P.apply_A(0.0, np.ones(256)), np.ones(256))
        twice = nodes.copy()
        twice[17] = twice[200]
        idx = _check_setup(m, axes, _on_nodes(axes, twice, rng), y, Pg=P)
        np.testing.assert_array_equal(idx, twice)
        assert not P.spectral_ok()
        W = P.apply_A(0.0, np.ones(256))
        assert W[twice[200]] == 2.0 and W[nodes[17]] == 0.0 and W.sum() == 256.0
        # and back
        P.set_scattered(axes, _on_nodes(axes, nodes, rng), y)
        assert P.spectral_ok()


def test_large_n_second_trip_of_nearest_and_run_sums():
    """n = 2^24 + 4097 on m = [257]: k_nearest and k_run_sums (65 536 workgroups of 256) take a second trip. One of the
    suite's two large cases (DESIGN.md §2.5 has its wall time)."""
    rng = np.random.default_rng(55)
    m = [257]
    n = (1 << 24) + 4097
    axes = NR.random_axes(m, rng)
    x = NR.box_points(axes, n, rng, pad=0.01)
    x[-4097:, 0] = np.resize(axes[0], 4097)   # the second trip's share: on the nodes
    y = rng.standard_normal(n)
    idx = _check_setup(m, axes, x, y)
    assert idx[-1] == 4096 % 257 and np.bincount(idx, minlength=257).min() > 0


def test_large_n_predict_and_fitted():
    """n = 1 048 576 + 300 on a 2-D mesh: k_gather_index (4096 workgroups of 256) takes a second trip in both
    mvtv_predict and mvtv_fitted. The other large case."""
    rng = np.random.default_rng(56)
    m = [30, 20]
    n = (1 << 20) + 300
    axes = NR.geometric_axes(m, rng)
    x = NR.box_points(axes, n, rng)
    idx = NR.nearest_fast(axes, x)
    assert NR.in_domain(axes, x).all()
    some = rng.choice(n, 2000, replace=False)
    some[:300] = np.arange(n - 300, n)
    np.testing.assert_array_equal(idx[some], O.nearest_index(x[some], NR.mesh_of(axes)))
    th = rng.standard_normal(600)
    with mv.Problem(m, np.zeros(600)) as P:
        P.state_set(th, None, 1.0)
        np.testing.assert_array_equal(P.predict(axes, x), th[idx])
        np.testing.assert_array_equal(P.fitted(idx), th[idx])


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_scattered_rejects_non_finite_points(bad):
    """an infinite coordinate has no nearest node (every distance is inf: the reference returns node 0, the bracket
    corners a node of the clamped face): refused like NaN, by nearest, set_scattered and predict alike"""
    axes = [np.arange(5.0), np.arange(4.0)]
    x = np.array([[1.0, 2.0], [2.2, 1.0], [3.0, 0.5]])
    with mv.Problem([5, 4], np.zeros(20)) as P:
        P.set_scattered(axes, x, np.ones(3))
        for j in (0, 1):
            xb = x.copy()
            xb[2 - j, j] = bad
            for call in (lambda: P.nearest(axes, xb), lambda: P.set_scattered(axes, xb, np.ones(3)),
                         lambda: P.predict(axes, xb)):
                with pytest.raises(mv.MvtvError) as e:
                    call()
                assert e.value.status == MVTV_BAD_ARG
        # a refused call leaves the earlier setup in place
        np.testing.assert_array_equal(P.apply_A(0.0, np.ones(20)), np.bincount([11, 7, 3], minlength=20).astype(float))


def test_scattered_rejects_bad_axes():
    with mv.Problem([4, 4], np.zeros(16)) as P:
        with pytest.raises(mv.MvtvError):
            P.nearest([np.array([0.0, 2.0, 1.0, 3.0]), np.arange(4.0)], np.zeros((3, 2)))
        with pytest.raises(ValueError):
            P.nearest([np.arange(3.0), np.arange(4.0)], np.zeros((3, 2)))
