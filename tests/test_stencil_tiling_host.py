"""Launch geometry of the marching stencil operators (k_apply2d / k_apply3d / k_apply3d2 / k_apply4d,
multivartv_amd/csrc/mvtv_cg3d.hip), transcribed, and the named shapes of tests/test_gpu_stencil_march.py and
tests/test_gpu_pcg_scalars.py checked for the tiling property each is named for. No GPU.

Each transcription returns (tiles_x, tiles_y, chunk, nchunks, nblocks, grid): in-plane tiles, the planes (rows) of the
marched dimension a workgroup owns, the chunk count, the workgroups that own cells and the launched grid, which is
nblocks padded to a multiple of 8 for the kernels' XCD remap bid = (blockIdx & 7) (grid >> 3) + (blockIdx >> 3);
workgroups with bid >= nblocks own nothing.

A GPU test asserts the logged grid against these, so a change of a launcher's rule fails there first and the shapes
below have to move with it: a case whose property no longer holds gets a new shape, never a weaker property."""
import pytest


def cdiv(a, b):
    return (a + b - 1) // b


def pad8(n):
    return cdiv(n, 8) * 8


def tiling2d(m):
    """launch_apply2d (mvtv_cg3d.hip:881-886): 256-column tiles, chunks of >= 8 rows, at most 8192 / tiles_x chunks."""
    m0, m1 = (int(v) for v in m)
    tiles_x = cdiv(m0, 256)
    ny = max(1, min(max(1, m1 // 8), 8192 // tiles_x))
    ychunk = cdiv(m1, ny)
    ny = cdiv(m1, ychunk)
    nblocks = tiles_x * ny
    return tiles_x, 1, ychunk, ny, nblocks, pad8(nblocks)


def two_cells(m):
    """launch_apply3d (mvtv_cg3d.hip:649-651): two cells a lane where m0 is even (the library's device buffers are
    16-B aligned, the other half of the rule)."""
    return int(m[0]) % 2 == 0


def tiling3d(m):
    """launch_apply3d (mvtv_cg3d.hip:652-659): 128 x 4 tiles and at most 4096 / tiles chunks with two cells a lane,
    64 x 4 tiles and 8192 / tiles with one."""
    m0, m1, m2 = (int(v) for v in m)
    two = two_cells(m)
    tiles_x = cdiv(m0, 128) if two else cdiv(m0, 64)
    tiles_y = cdiv(m1, 4)
    tiles = tiles_x * tiles_y
    nz = max(1, min(m2, (4096 if two else 8192) // max(1, tiles)))
    zchunk = cdiv(m2, nz)
    nz = cdiv(m2, zchunk)
    nblocks = tiles * nz
    return tiles_x, tiles_y, zchunk, nz, nblocks, pad8(nblocks)


K_MAX_CG_BLOCKS, K_MAX_RED = 8192, 8   # mvtv_internal.h:184-185


def tiling4d(m):
    """launch_apply4d (mvtv_cg3d.hip:782-790): 64 x 4 tiles per (dim 2) plane, at most 8192 / (tiles m2) chunks of
    dim 3; None where it refuses (the caller falls back to the generic kernel)."""
    m0, m1, m2, m3 = (int(v) for v in m)
    tiles_x, tiles_y = cdiv(m0, 64), cdiv(m1, 4)
    items = tiles_x * tiles_y * m2
    nw = max(1, min(m3, 8192 // max(1, items)))
    wchunk = cdiv(m3, nw)
    nw = cdiv(m3, wchunk)
    if items * nw > K_MAX_CG_BLOCKS * K_MAX_RED:
        return None
    nblocks = items * nw
    return tiles_x, tiles_y, wchunk, nw, nblocks, pad8(nblocks)


def tiling(m):
    return {2: tiling2d, 3: tiling3d, 4: tiling4d}[len(m)](m)


def kernel_of(m):
    """the marching kernel apply_A runs on mesh m"""
    return {2: "k_apply2d", 3: "k_apply3d2" if len(m) == 3 and two_cells(m) else "k_apply3d", 4: "k_apply4d"}[len(m)]


# name -> mesh: the operator cases of tests/test_gpu_stencil_march.py
CASES = {
    "2d-a": [257, 41], "2d-b": [513, 17], "2d-c": [256, 16], "2d-d": [5, 300], "2d-e": [300, 5], "2d-f": [4, 70000],
    "3d2-a": [130, 130, 71], "3d2-b": [34, 34, 500], "3d2-c": [258, 258, 48],
    "3d1-a": [65, 65, 251], "3d1-b": [129, 129, 100],
    "4d-a": [12, 12, 12, 301], "4d-b": [65, 65, 65, 8], "4d-c": [6, 6, 6, 40],
}
# the meshes on which tests/test_gpu_pcg_scalars.py reaches the DOT instantiations
PCG_CASES = {"pcg-2d": [270, 41], "pcg-3d2": [140, 140, 70], "pcg-3d1": [135, 135, 100], "pcg-4d": [12, 12, 12, 301]}


def last(m, chunk, nchunks):
    """planes (rows) of the last chunk"""
    return int(m[-1]) - chunk * (nchunks - 1)


def test_2d_cases():
    tx, _, ch, n, nb, grid = tiling2d(CASES["2d-a"])
    assert (tx, ch, n, nb, grid) == (2, 9, 5, 10, 16)
    assert CASES["2d-a"][0] - 256 == 1 and last(CASES["2d-a"], ch, n) == 5
    tx, _, ch, n, nb, grid = tiling2d(CASES["2d-b"])
    assert (tx, n) == (3, 2)
    tx, _, ch, n, nb, grid = tiling2d(CASES["2d-c"])
    assert (tx, ch, n) == (1, 8, 2) and CASES["2d-c"][0] == 256 and last(CASES["2d-c"], ch, n) == 8
    tx, _, ch, n, nb, grid = tiling2d(CASES["2d-d"])
    assert (n, grid) == (34, 40) and last(CASES["2d-d"], ch, n) == 3
    tx, _, ch, n, nb, grid = tiling2d(CASES["2d-e"])
    assert CASES["2d-e"][1] < 8 and n == 1 and ch == CASES["2d-e"][1]
    m = CASES["2d-f"]
    tx, _, ch, n, nb, grid = tiling2d(m)
    assert m[1] // 8 > 8192 // tx and n <= 8192 // tx and ch > 8   # the cap, not the 8-row rule, sets the chunks


def test_3d_two_cell_cases():
    for name in ("3d2-a", "3d2-b", "3d2-c"):
        assert two_cells(CASES[name]) and kernel_of(CASES[name]) == "k_apply3d2"
    tx, ty, ch, n, nb, grid = tiling3d(CASES["3d2-a"])
    assert (tx * ty, ch, n) == (66, 2, 36) and last(CASES["3d2-a"], ch, n) == 1
    tx, ty, ch, n, nb, grid = tiling3d(CASES["3d2-b"])
    assert tx == 1 and CASES["3d2-b"][0] // 2 == 17 and ch == 2 and nb == 2250 and grid > nb
    m = CASES["3d2-c"]
    tx, ty, ch, n, nb, grid = tiling3d(m)
    assert tx == 3 and (m[0] - 256) // 2 == 1 and m[1] % 4 != 0 and ch == 3


def test_3d_one_cell_cases():
    for name in ("3d1-a", "3d1-b"):
        assert not two_cells(CASES[name]) and kernel_of(CASES[name]) == "k_apply3d"
    m = CASES["3d1-a"]
    tx, ty, ch, n, nb, grid = tiling3d(m)
    assert tx == 2 and m[0] - 64 == 1 and ch == 2 and last(m, ch, n) == 1 and grid > nb
    tx, ty, ch, n, nb, grid = tiling3d(CASES["3d1-b"])
    assert tx == 3 and ch == 2 and grid > nb


def test_4d_cases():
    for name in ("4d-a", "4d-b", "4d-c"):
        m = CASES[name]
        assert m[0] == m[1] == m[2]   # the reference's D needs it (oracle.mvtv_oracle.check_dims)
    m = CASES["4d-a"]
    tx, ty, ch, n, nb, grid = tiling4d(m)
    assert (ch, n) == (2, 151) and last(m, ch, n) == 1 and grid > nb
    m = CASES["4d-b"]
    tx, ty, ch, n, nb, grid = tiling4d(m)
    assert tx == 2 and (ch, n) == (3, 3) and last(m, ch, n) == 2 and grid > nb
    m = CASES["4d-c"]
    tx, ty, ch, n, nb, grid = tiling4d(m)
    assert tx * ty == 2 and tx == 1 and m[1] % 4 != 0 and ch == 1


def test_pcg_cases():
    tx, _, ch, n, nb, grid = tiling2d(PCG_CASES["pcg-2d"])
    assert tx == 2 and n > 1 and grid > nb
    m = PCG_CASES["pcg-3d2"]
    assert kernel_of(m) == "k_apply3d2"
    tx, ty, ch, n, nb, grid = tiling3d(m)
    assert (ch, nb, grid) == (2, 2450, 2456)
    m = PCG_CASES["pcg-3d1"]
    assert kernel_of(m) == "k_apply3d"
    tx, ty, ch, n, nb, grid = tiling3d(m)
    assert ch == 2 and grid > nb
    tx, ty, ch, n, nb, grid = tiling4d(PCG_CASES["pcg-4d"])
    assert ch == 2 and grid > nb


@pytest.mark.parametrize("name", sorted(CASES) + sorted(PCG_CASES))
def test_every_case_is_within_the_launchers_limits(name):
    """the DOT launches write a row of `partials` per workgroup: grids stay within its rows (launch_apply2d :906,
    launch_apply4d :788); every mesh stays a few million nodes"""
    m = {**CASES, **PCG_CASES}[name]
    t = tiling(m)
    assert t is not None and t[5] % 8 == 0 and t[4] <= t[5] < t[4] + 8
    assert t[5] <= K_MAX_CG_BLOCKS * K_MAX_RED
    n = 1
    for v in m:
        n *= v
    assert n <= 3_300_000
