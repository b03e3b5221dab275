"""tests/nearest_ref.py pinned against the oracle's brute-force scan (oracle.mvtv_oracle.nearest_index) on every
kind of axis and edge point tests/test_gpu_scatter.py uses, at small N, and the two points where the scan's index is
not the bracket corners': far outside the box (float64 absorbs the other axes) and infinite coordinates. No GPU."""
import numpy as np
import pytest

import nearest_ref as NR
from oracle import mvtv_oracle as O

# p = 1 .. 4 within the reference's dimension rule (m_0 = m_1 (= m_2) where a mixed block lacks dim 0), an axis of
# two nodes in each p
MESHES = [(2,), (9,), (2, 7), (6, 5), (5, 5, 2), (4, 4, 6), (3, 3, 3, 2), (4, 4, 4, 3)]


@pytest.mark.parametrize("kind", sorted(NR.AXES))
@pytest.mark.parametrize("m", MESHES, ids=lambda m: "x".join(str(v) for v in m))
def test_fast_reference_is_the_scan(m, kind):
    rng = np.random.default_rng(31 + sum(m))
    axes = NR.AXES[kind](m, rng)
    assert all(np.all(np.diff(a) > 0) for a in axes)
    x = np.vstack([NR.box_points(axes, 400, rng), NR.edge_points(axes, rng)])
    assert NR.in_domain(axes, x).all()
    mesh = NR.mesh_of(axes)
    ref = O.nearest_index(x, mesh)
    np.testing.assert_array_equal(NR.nearest_fast(axes, x), ref)
    # what the edge points are: nodes map to themselves, and so do their one-ulp neighbours
    nodes, at = NR.node_points(axes, 12, rng)
    np.testing.assert_array_equal(O.nearest_index(nodes, mesh), at)
    near = NR.neighbours(nodes)
    np.testing.assert_array_equal(O.nearest_index(near, mesh), np.tile(at, len(near) // 12))


@pytest.mark.parametrize("m", MESHES, ids=lambda m: "x".join(str(v) for v in m))
def test_exact_midpoints_take_the_lower_node(m):
    rng = np.random.default_rng(32 + sum(m))
    axes = NR.integer_axes(m, rng)
    mids, low = NR.midpoint_points(axes, 4, rng)
    assert np.all(mids == np.round(mids))   # exact: ties in 1 .. p dims at once
    np.testing.assert_array_equal(O.nearest_index(mids, NR.mesh_of(axes)), low)
    np.testing.assert_array_equal(NR.nearest_fast(axes, mids), low)


def test_far_outside_the_box_the_scan_is_not_the_corners():
    """x = (3.7, 1e9) on arange(5) x arange(4): (1e9 - 3)^2 absorbs every (3.7 - i)^2, the five nodes of the last row
    tie and the scan takes the first, 15; the bracket corners are nodes 18 and 19. ``in_domain`` says so, and the
    same point 1e3 box widths out is inside."""
    axes = [np.arange(5.0), np.arange(4.0)]
    mesh = NR.mesh_of(axes)
    x = np.array([[3.7, 1e9]])
    assert O.nearest_index(x, mesh)[0] == 15
    assert NR.nearest_fast(axes, x)[0] == 18
    assert not NR.in_domain(axes, x)[0]
    near = np.array([[3.7, 3e3]])
    assert NR.in_domain(axes, near)[0]
    assert O.nearest_index(near, mesh)[0] == NR.nearest_fast(axes, near)[0] == 19
    # the bound is a sufficient condition, not the edge itself: the first failure lies beyond it
    d = 3.0 + 2.0 ** np.arange(10, 40)
    far = np.stack([np.full(d.size, 3.7), d], axis=1)
    same = O.nearest_index(far, mesh) == NR.nearest_fast(axes, far)
    assert same[NR.in_domain(axes, far)].all() and not same.all()


def test_infinite_coordinates_have_no_nearest_node():
    """every distance to a point with an infinite coordinate is inf, the scan's first minimum is node 0; the bracket
    corners lie on the clamped face. The library refuses such points (MVTV_BAD_ARG) as it refuses NaN."""
    axes = [np.arange(5.0), np.arange(4.0)]
    x = np.array([[2.2, np.inf], [-np.inf, 1.0]])
    np.testing.assert_array_equal(O.nearest_index(x, NR.mesh_of(axes)), [0, 0])
    assert list(NR.nearest_fast(axes, x)) != [0, 0]
    assert not NR.in_domain(axes, x).any()
