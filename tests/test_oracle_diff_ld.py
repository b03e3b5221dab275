"""oracle/diff_ld.py (matrix-free long-double D and D^T) pinned against the sparse oracle and the C oracle, the
componentwise bounds of tests/test_gpu_operators_wide.py with their teeth shown on the CPU, and the launch geometry
of the public D / D^T (mvtv_apply_D / mvtv_apply_Dt, mvtv_capi.cpp) transcribed, with the named meshes of the GPU
test checked for what each is for. No GPU.

Bounds (u = 2^-53, a = the absval result of oracle/diff_ld.py, derived from the kernels' operation counts):

  D    k_apply_D forms a[S'] by a butterfly of subtractions, one level per dim; only the |S'| levels along the dims of
       S' touch the entry a block stores, so that entry is a sum of 2^|S'| values of theta that went through |S'|
       roundings each at most, then one multiplication by w_b:
           |got - ld| <= c_D(b) u a,   c_D(b) = |S'(b)| + 2 <= p + 2
       (|S'| + 1 roundings; + 1 covers the second-order terms (1 + u)^(p+1) - 1 - (p + 1) u and the long-double
       reference's own rounding, 2^-11 u per operation). Import and export move values without arithmetic.
  D^T  k_gather<P, ORD, U_EXPLICIT, false> adds the 2^|S'| terms of a block to 0.0 (the first addition is exact:
       2^|S'| - 1 roundings), then gu = fma(w_b, sum, gu) once per block: a block's share goes through one rounding in
       its own fma and one in each later block's, at most nb in all:
           |got - ld| <= c_Dt u a,   c_Dt = (2^p - 1) + nb + 1 = 2^p + nb
       (+ 1 as above): 3, 7, 15, 31 for p = 1 .. 4 with nb = 2^p - 1 blocks.

Neither is tuned: the float64 evaluations of the same formulas below sit at 0.04 to 0.61 of them, the GPU at 0.06 to
0.67."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import c_oracle
from oracle import diff_ld as DL
from oracle import mvtv_oracle as O

LD = np.longdouble
U = 2.0 ** -53
DELTAS = [0.9, 1.1, 0.8, 1.25]   # no power of two: the weight multiplications round
# (block order, weighted): cpp weighted, cpp unit, py weighted (no all-ones block), py unweighted
ORDERS = [("cpp", True), ("cpp", False), ("py", True), ("py", False)]


def blocks_of(p, order, weighted):
    return O.block_table(p, DELTAS[:p] if weighted else None, order, unit_weights=not weighted)


def runs(meshes):
    """every mesh in the four orders; Python's create_D with deltas has no block at p = 1 (the library refuses it)"""
    return [(tuple(m), o, w) for m in meshes for o, w in ORDERS if not (len(m) == 1 and o == "py" and w)]


def run_id(r):
    m, o, w = r
    return "x".join(str(v) for v in m) + f"-{o}-{'w' if w else 'unit'}"


# ------------------------------------------------------------------------------------------ bounds
def c_D(blocks):
    """per row of D: |S'(b)| + 2 for the rows of block b"""
    return [len(blk.Sp) + 2 for blk in blocks]


def c_Dt(p, nb):
    return 2 ** p + nb


def _ratio(got, ref, a, c):
    """max_i |got_i - ref_i| / (c_i u a_i); where a_i = 0 the output must be exactly 0 (inf otherwise)"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    den = LD(U) * np.asarray(c, dtype=LD) * a
    pos = den > 0
    r = float(np.max(err[pos] / den[pos])) if pos.any() else 0.0
    if (err[~pos] != 0).any():
        r = float("inf")
    return r


def ratio_D(m, blocks, got, ref, a):
    """worst |got - ref| / (c_D(b) u a) over the rows of D: at most 1 within the bound"""
    c = np.repeat(c_D(blocks), DL.block_lengths(m, blocks))
    return _ratio(got, ref, a, c)


def ratio_Dt(m, blocks, got, ref, a):
    return _ratio(got, ref, a, float(c_Dt(len(m), len(blocks))))


# ------------------------------------------------------------------------------------------ launch geometry
K_THREADS, K_MAX_GRID = 256, 2048   # mvtv_internal.h: kThreads, kMaxGrid
ELEM_CAP = 4096                     # elem_grid, mvtv_kernels.hip
K_MAX_CG_BLOCKS, K_MAX_RED = 8192, 8


def cdiv(a, b):
    return (a + b - 1) // b


def stream_grid(N):
    """P->grid (mvtv_problem_create): the grid of k_apply_D and k_gather, 256 nodes a workgroup and trip"""
    return min(cdiv(N, K_THREADS), K_MAX_GRID)


def elem_grid(n):
    """elem_grid (mvtv_kernels.hip): the grid of k_edges_import / k_edges_export over one block's n edges"""
    return min(max(cdiv(n, 256), 1), ELEM_CAP)


def eaos(m):
    """Geom.eaos (mvtv_problem_create): the 64-node-chunk edge layout, on for p = 3 where the fused edge pass applies
    and p = 4 where the marching edge kernel does, when N is a multiple of 64. Both launchers shrink their chunk
    count until the grid fits the partials buffer, so each applies unless its in-plane tiles alone overflow it."""
    m = [int(v) for v in m]
    N = int(np.prod(m))
    if len(m) == 3:
        tiles = cdiv(m[0], 64) * cdiv(m[1], 14)                      # f3d_args: 64 x (f3a::IH - 1) tiles
        ok = cdiv(tiles, 8) * 8 * 7 <= K_MAX_CG_BLOCKS * K_MAX_RED   # fused3d_ok
    elif len(m) == 4:
        tiles = cdiv(m[0], 64) * cdiv(m[1], 4) * m[2]                # e4d_args
        ok = cdiv(tiles, 8) * 8 <= K_MAX_CG_BLOCKS                   # edge4d_ok
    else:
        return False
    return ok and N % 64 == 0


def trips(n, grid, threads=256):
    """the most trips a thread of the grid-stride loop takes over n items"""
    return cdiv(n, grid * threads)


# the meshes of tests/test_gpu_operators_wide.py
WIDE = [(300,), (1048876,), (300, 7), (1030, 1030), (64, 64, 130), (65, 65, 130), (28, 28, 28, 25), (27, 27, 27, 28)]


def test_wide_meshes_are_what_they_are_for():
    geo = {}
    for m in WIDE:
        N = int(np.prod(m))
        lens = DL.block_lengths(m, blocks_of(len(m), "py", False))   # all 2^p - 1 blocks
        geo[m] = (N, stream_grid(N), trips(N, stream_grid(N)), max(trips(n, elem_grid(n)) for n in lens), eaos(m))
        for o, w in ORDERS:   # the reference's dimension-mismatch rule
            O.check_dims(m, blocks_of(len(m), o, w))
    # two workgroups, the second ragged
    assert geo[(300,)][1:4] == (2, 1, 1) and 300 % 256 != 0
    # the kernel grid wraps and so does import / export of the only block
    assert geo[(1048876,)][1:4] == (2048, 3, 2)
    assert DL.block_lengths((1048876,), blocks_of(1, "cpp", True)) == [1048875]
    # dim-0 rows cross workgroup boundaries (256 is no multiple of 300); block-major
    assert geo[(300, 7)][1] == 9 and 256 % 300 != 0 and not geo[(300, 7)][4]
    # both wraps, the mixed block's included
    assert geo[(1030, 1030)][1:4] == (2048, 3, 2)
    mixed = [n for blk, n in zip(blocks_of(2, "cpp", True), DL.block_lengths((1030, 1030), blocks_of(2, "cpp", True)))
             if len(blk.Sp) == 2]
    assert mixed == [1029 * 1029] and trips(mixed[0], elem_grid(mixed[0])) == 2
    # N > 524 288 (second trip of the streaming kernels), chunked against block-major
    for chunked, plain in (((64, 64, 130), (65, 65, 130)), ((28, 28, 28, 25), (27, 27, 27, 28))):
        assert geo[chunked][0] > K_MAX_GRID * K_THREADS and geo[plain][0] > K_MAX_GRID * K_THREADS
        assert geo[chunked][2] == 2 and geo[plain][2] == 2
        assert geo[chunked][4] and not geo[plain][4]
    assert len(blocks_of(4, "cpp", True)) == 15 and len(blocks_of(4, "py", True)) == 14


# ------------------------------------------------------------------------------------------ pins
# p = 1 .. 4; (5, 5, 7), (4, 4, 4, 5) and (6, 6, 6, 3): m_0 = m_1 (= m_2) with another length after it, where a mixed
# block without dim 0 differences dim 0 in place of its lowest dim (the S' rule) over a reduced grid of its own
SMALL = [(9,), (2,), (7, 5), (2, 3), (6, 6, 6), (5, 5, 7), (4, 4, 4, 5), (6, 6, 6, 3), (3, 3, 3, 3)]


@pytest.mark.parametrize("dtype", [LD, np.float64], ids=["ld", "f64"])
@pytest.mark.parametrize("run", runs(SMALL), ids=run_id)
def test_matches_build_D(run, dtype):
    m, order, weighted = run
    blocks = blocks_of(len(m), order, weighted)
    D = O.build_D(m, blocks)
    assert sum(DL.block_lengths(m, blocks)) == D.shape[0]
    rng = np.random.default_rng(21)
    th = rng.standard_normal(D.shape[1])
    v = rng.standard_normal(D.shape[0])
    for got, ref in ((DL.apply_D(m, blocks, th, dtype), D @ th),
                     (DL.apply_Dt(m, blocks, v, dtype), D.T @ v),
                     (DL.apply_D(m, blocks, th, dtype, absval=True), abs(D) @ np.abs(th)),
                     (DL.apply_Dt(m, blocks, v, dtype, absval=True), abs(D).T @ np.abs(v))):
        assert got.dtype == dtype and got.shape == ref.shape
        assert float(np.max(np.abs(got - ref))) <= 1e-14 * float(np.max(np.abs(ref)))
    # the support is the sparse matrix's, exactly: one non-zero per block
    one = np.zeros(D.shape[0])
    off = 0
    for n in DL.block_lengths(m, blocks):
        one[off + int(rng.integers(0, n))] = rng.uniform(1.0, 2.0)
        off += n
    assert np.array_equal(DL.apply_Dt(m, blocks, one, dtype) != 0, (abs(D).T @ one) != 0)


@pytest.mark.parametrize("m,order,weighted", [((100003,), "cpp", True), ((317, 316), "cpp", True),
                                              ((47, 47, 47), "py", True), ((18, 18, 18, 18), "cpp", True),
                                              ((47, 47, 46), "cpp", False)])
def test_matches_c_oracle(m, order, weighted):
    """more than 1e5 nodes per p, against the C oracle's matrix-free D and D^T"""
    p = len(m)
    blocks = blocks_of(p, order, weighted)
    O.check_dims(m, blocks)
    assert int(np.prod(m)) > 10 ** 5
    rng = np.random.default_rng(22)
    th = rng.standard_normal(int(np.prod(m)))
    o, w = (0 if order == "cpp" else 1), int(weighted)
    d_ref = c_oracle.apply_D(m, th, DELTAS[:p], o, w)
    d = DL.apply_D(m, blocks, th)
    assert d.shape == d_ref.shape
    assert float(np.max(np.abs(d - d_ref))) <= 1e-14 * float(np.max(np.abs(d_ref)))
    v = rng.standard_normal(d_ref.size)
    g_ref = c_oracle.apply_Dt(m, v, DELTAS[:p], o, w)
    g = DL.apply_Dt(m, blocks, v)
    assert float(np.max(np.abs(g - g_ref))) <= 1e-14 * float(np.max(np.abs(g_ref)))


# ------------------------------------------------------------------------------------------ teeth
def _block(m, blk, drop_corner=None, clamp_dim=None, scale=1.0):
    """build_block with a defect: corner ``drop_corner`` (a subset of S' as a bit mask over its dims) missing;
    ``clamp_dim`` j: the anchors one short of the upper face of dim j (i_j = m_j - 2) take themselves for their
    + e_j neighbour, the clamp of a face anchor applied one node early; ``scale``: the weight times that."""
    m = [int(v) for v in m]
    rd = O.reduced_dims(m, blk.Sp)
    R = int(np.prod(rd))
    grids = np.meshgrid(*[np.arange(v, dtype=np.int64) for v in rd], indexing="ij")
    idx = [g.ravel(order="F") for g in grids]
    rows, cols, vals = [], [], []
    k = len(blk.Sp)
    for t in range(1 << k):
        if t == drop_corner:
            continue
        shifted = [a.copy() for a in idx]
        sign = 1.0
        for q in range(k):
            if (t >> q) & 1:
                j = blk.Sp[q]
                step = np.ones(R, dtype=np.int64)
                if j == clamp_dim:
                    step[idx[j] == m[j] - 2] = 0
                shifted[j] = shifted[j] + step
                sign = -sign
        rows.append(np.arange(R, dtype=np.int64))
        cols.append(O._lin(shifted, m))
        vals.append(np.full(R, sign * blk.w * scale))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(R, int(np.prod(m))))


def _stack(m, blocks, k=None, **defect):
    return sp.vstack([_block(m, blk, **(defect if i == k else {})) for i, blk in enumerate(blocks)]).tocsr()


TEETH = [(37,), (37, 9), (9, 9, 7), (5, 5, 5, 6)]


@pytest.mark.parametrize("m", TEETH, ids=lambda m: "x".join(str(v) for v in m))
def test_bounds_have_teeth(m):
    """float64 evaluations of the correct operators stay within the bounds; a block weight off by 1e-13 relative
    (900 u), one corner dropped from one block and a clamp applied one node before an upper face do not. The defect
    is added to the float64 result as (D_defect - D) theta, so the clean part rounds as the clean run does.

    Every block's weight is caught by both: by D at 120 to 300 times the bound, by D^T, where one block's share of a
    node competes with 2^p + nb roundings of all of them, at 4.4 times or more at p = 4 (printed)."""
    p = len(m)
    blocks = blocks_of(p, "cpp", True)
    D0 = _stack(m, blocks)
    assert abs(D0 - O.build_D(m, blocks)).max() == 0.0
    rng = np.random.default_rng(23)
    th = rng.standard_normal(D0.shape[1])
    v = rng.standard_normal(D0.shape[0])
    d_ld, d_a = DL.apply_D(m, blocks, th), DL.apply_D(m, blocks, th, absval=True)
    g_ld, g_a = DL.apply_Dt(m, blocks, v), DL.apply_Dt(m, blocks, v, absval=True)
    d64, g64 = DL.apply_D(m, blocks, th, np.float64), DL.apply_Dt(m, blocks, v, np.float64)
    rd = lambda got: ratio_D(m, blocks, got, d_ld, d_a)     # noqa: E731
    rg = lambda got: ratio_Dt(m, blocks, got, g_ld, g_a)    # noqa: E731
    print(f"{m}: float64 D {rd(d64):.2f}, D^T {rg(g64):.2f} (bound 1)")
    assert rd(d64) <= 1.0 and rg(g64) <= 1.0
    # the sparse products (another summation order) as well
    assert rd(D0 @ th) <= 1.0 and rg(D0.T @ v) <= 1.0
    for k, blk in enumerate(blocks):
        Dw = _stack(m, blocks, k, scale=1.0 + 1e-13) - D0
        rw, rwt = rd(d64 + Dw @ th), rg(g64 + Dw.T @ v)
        print(f"  block {k} S'={blk.Sp}: weight + 1e-13: D {rw:.1f}, D^T {rwt:.1f}")
        assert rw > 1.0 and rwt > 1.0
        Dc = _stack(m, blocks, k, drop_corner=(1 << len(blk.Sp)) - 1) - D0
        assert rd(d64 + Dc @ th) > 1e10 and rg(g64 + Dc.T @ v) > 1e10
        Df = _stack(m, blocks, k, clamp_dim=blk.Sp[-1]) - D0
        assert rd(d64 + Df @ th) > 1e10 and rg(g64 + Df.T @ v) > 1e10
