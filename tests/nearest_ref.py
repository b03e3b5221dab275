"""Reference and inputs for the scattered-data setup tests (tests/test_nearest_ref_host.py on the CPU,
tests/test_gpu_scatter.py on the GPU).

``nearest_fast`` is a second statement of what the reference's brute-force scan (nearest1, rcpp…/utils.cpp:280-287;
oracle.mvtv_oracle.nearest_index) returns on a tensor mesh: per axis the bracket of the point by ``searchsorted``,
then the squared distances of the 2^p bracket corners summed over dims 0 .. p-1 in float64 (numpy multiplies and adds
in separate passes: no fused multiply-add), the lowest node among the minima. It costs O(n p log m) where the scan
costs O(n N), so it serves the cases with n N > 1e8; everything smaller is checked against the scan itself.

Domain. The corner with the nearest node on every axis has the smallest distance in exact arithmetic, and float64
addition and multiplication are monotone, so some corner always attains the scan's minimum *value*. The scan's
*index* can still differ: when the point is so far from the box on one axis that float64 absorbs the other axes'
squared distances, nodes outside the bracket tie with the corners, and the scan takes the lowest index over all N
nodes. Axes arange(5), arange(4) and x = (3.7, 1e9): every node of the last row ties at 1e18, the scan returns 15,
the corners give 18. A computed distance is a sum of p terms, each within (p + 2) u relative of its exact value
(one subtraction, one multiplication, p - 1 additions; u = 2^-53). Replacing an out-of-bracket coordinate on axis j by
the nearer bracket end lowers the exact distance by at least g_j (2 r_j + g_j), so no node outside the bracket can
tie with a corner when, on every axis j,

    g_j (2 r_j + g_j) >= 4 (p + 2) 2^-53 sum_i R_i^2                                  (``in_domain``)

g_j: the smallest spacing of axis j; r_j: the distance from x_j to its nearest node of axis j; R_i: the distance from
x_i to the farther end of its bracket on axis i (to the nearest node when x_i lies outside the axis). Inside that
domain the indices are the scan's, bit for bit. A point inside the box meets it whenever the axes' spacings stay
within a factor 2^25 / sqrt(p (p + 2)) of one another; a point at distance d outside the box meets it up to about
d <= 2^25.5 g_min / sqrt(p + 2) (1.9e7 spacings at p = 4) when the box is small beside d."""
import itertools

import numpy as np

U = 2.0 ** -53


def mesh_of(axes):
    """the column-major tensor mesh (dim 0 fastest) of create_mesh, one row per node"""
    grids = np.meshgrid(*axes, indexing="ij")
    return np.stack([g.reshape(-1, order="F") for g in grids], axis=1)


def _brackets(axes, x):
    """per axis: (lo index, has two ends, value at lo end, value at hi end): [ax[b-1], ax[b]] with b the lower bound
    of x, one end beyond the axis' first or last node"""
    out = []
    for j, ax in enumerate(axes):
        ax = np.asarray(ax, dtype=np.float64)
        b = np.searchsorted(ax, x[:, j], side="left")
        two = (b > 0) & (b < ax.size)
        lo = np.where(b == 0, 0, b - 1)
        hi = np.where(two, lo + 1, lo)
        out.append((lo, two, ax[lo], ax[hi]))
    return out


def nearest_fast(axes, x):
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    p = len(axes)
    br = _brackets(axes, x)
    strides = np.cumprod([1] + [len(a) for a in axes[:-1]]).astype(np.int64)
    t = []
    for j in range(p):
        lo, two, vl, vh = br[j]
        d0, d1 = x[:, j] - vl, x[:, j] - vh
        t.append((d0 * d0, d1 * d1))
    best = np.full(len(x), np.inf)
    best_node = np.full(len(x), np.iinfo(np.int64).max, dtype=np.int64)
    for s in range(1 << p):
        ok = np.ones(len(x), dtype=bool)
        node = np.zeros(len(x), dtype=np.int64)
        d = np.zeros(len(x))
        for j in range(p):
            bit = (s >> j) & 1
            lo, two, _, _ = br[j]
            if bit:
                ok &= two
            node += (lo + bit) * strides[j]
            d = d + t[j][bit]
        take = ok & ((d < best) | ((d == best) & (node < best_node)))
        best = np.where(take, d, best)
        best_node = np.where(take, node, best_node)
    return best_node


def in_domain(axes, x):
    """per point: whether the condition of the module docstring holds (the indices are then the brute-force scan's)"""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    p = len(axes)
    finite = np.all(np.isfinite(x), axis=1)
    x = np.where(finite[:, None], x, 0.0)
    S = np.zeros(len(x))
    gain = np.full(len(x), np.inf)
    for j, (lo, two, vl, vh) in enumerate(_brackets(axes, x)):
        dl, dh = np.abs(x[:, j] - vl), np.abs(x[:, j] - vh)
        r, R = np.minimum(dl, dh), np.maximum(dl, dh)
        S += R * R
        g = float(np.min(np.diff(np.asarray(axes[j], dtype=np.float64))))
        gain = np.minimum(gain, g * (2.0 * r + g))
    return finite & (gain >= 4.0 * (p + 2) * U * S)


# ------------------------------------------------------------------------------------------ axes
def random_axes(m, rng):
    """node i at (i + U(0, 0.8)) h: no two spacings alike, every spacing between 0.2 and 1.8 of the mean"""
    return [(np.arange(int(mj)) + rng.uniform(0.0, 0.8, int(mj))) * (3.0 / int(mj)) - 1.0 for mj in m]


def geometric_axes(m, rng, spread=1e3):
    """spacings growing geometrically from one end (from the other on odd dims), the last ``spread`` times the first:
    nodes clustered there, so the uniform first guess of the bracket is wrong for most points"""
    axes = []
    for j, mj in enumerate(m):
        ratio = spread ** (1.0 / max(1, int(mj) - 2))
        a = np.concatenate([[0.0], np.cumsum(ratio ** np.arange(int(mj) - 1))])
        a = a / a[-1]
        axes.append(np.sort(1.0 - a) if j % 2 else a)
    return axes


def integer_axes(m, rng):
    """even integer spacings 2, 4, 6 in random order: every midpoint is an integer and every distance exact, so
    midpoints tie exactly"""
    return [np.concatenate([[0.0], np.cumsum(2.0 * rng.integers(1, 4, int(mj) - 1))]) - 7.0 for mj in m]


AXES = {"random": random_axes, "geometric": geometric_axes, "integer": integer_axes}


# ------------------------------------------------------------------------------------------ points
def box_points(axes, n, rng, pad=0.05):
    """uniform over the box widened by ``pad`` widths on every side"""
    lo = np.array([a[0] for a in axes])
    hi = np.array([a[-1] for a in axes])
    w = hi - lo
    return rng.uniform(lo - pad * w, hi + pad * w, size=(n, len(axes)))


def node_points(axes, n, rng):
    """points exactly on nodes, nodes 0 and N - 1 among them; returns (points, node of each)"""
    m = [len(a) for a in axes]
    sub = np.stack([rng.integers(0, mj, n) for mj in m], axis=1)
    sub[0] = 0
    sub[1] = np.array(m) - 1
    strides = np.cumprod([1] + m[:-1])
    return np.stack([np.asarray(axes[j])[sub[:, j]] for j in range(len(m))], axis=1), sub @ strides


def midpoint_points(axes, per, rng):
    """midpoints of a cell in k = 1 .. p dims at once (every subset of dims, ``per`` cells each), the other
    coordinates on the cell's lower node; returns (points, lower node of each). Exact ties on integer_axes."""
    m = [len(a) for a in axes]
    p = len(m)
    strides = np.cumprod([1] + m[:-1])
    pts, low = [], []
    for k in range(1, p + 1):
        for dims in itertools.combinations(range(p), k):
            for _ in range(per):
                c = [int(rng.integers(0, max(1, mj - 1))) for mj in m]
                x = [float(axes[j][c[j]]) for j in range(p)]
                for j in dims:
                    x[j] = 0.5 * (float(axes[j][c[j]]) + float(axes[j][c[j] + 1]))
                pts.append(x)
                low.append(int(np.dot(c, strides)))
    return np.array(pts), np.array(low, dtype=np.int64)


def neighbours(pts):
    """np.nextafter either side of every coordinate: all 3^p - 1 one-ulp moves of each point for p <= 2, the 2 p
    single-coordinate moves and the two all-coordinate moves beyond"""
    pts = np.asarray(pts, dtype=np.float64)
    p = pts.shape[1]
    if p <= 2:
        moves = [s for s in itertools.product((-1, 0, 1), repeat=p) if any(s)]
    else:
        moves = [tuple(sg if i == j else 0 for i in range(p)) for j in range(p) for sg in (-1, 1)]
        moves += [(-1,) * p, (1,) * p]
    out = []
    for s in moves:
        q = pts.copy()
        for j, sg in enumerate(s):
            if sg:
                q[:, j] = np.nextafter(q[:, j], sg * np.inf)
        out.append(q)
    return np.vstack(out)


def outside_points(axes, rng, factors=(1e-3, 1.0, 1e3)):
    """beyond every face, edge and corner of the box (each of the 3^p - 1 sign patterns), by each factor of the box
    width; the coordinates of the other dims anywhere inside"""
    lo = np.array([a[0] for a in axes])
    hi = np.array([a[-1] for a in axes])
    w = hi - lo
    pts = []
    for s in itertools.product((-1, 0, 1), repeat=len(axes)):
        if not any(s):
            continue
        for f in factors:
            x = rng.uniform(lo, hi)
            for j, sg in enumerate(s):
                if sg:
                    x[j] = (lo[j] - f * w[j]) if sg < 0 else (hi[j] + f * w[j])
            pts.append(x)
    return np.array(pts)


def edge_points(axes, rng, per=3):
    """all of the above but the bulk: nodes, midpoints, their one-ulp neighbours, outside points"""
    nodes, _ = node_points(axes, 8 * per, rng)
    mids, _ = midpoint_points(axes, per, rng)
    return np.vstack([nodes, mids, neighbours(nodes), neighbours(mids), outside_points(axes, rng)])
