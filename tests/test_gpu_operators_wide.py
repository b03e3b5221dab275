"""The public D and D^T (Problem.apply_D / apply_Dt: k_apply_D<P, ORD>, k_gather<P, ORD, U_EXPLICIT, false>,
k_edges_export, k_edges_import; mvtv_kernels.hip) past one grid, against long double (oracle/diff_ld.py). The same
import, export and gather set up every warm start with a non-zero u.

Meshes (what each is for is asserted in tests/test_oracle_diff_ld.py from a transcription of the launch geometry):
two ragged workgroups; a 1-D mesh whose streaming grid wraps (N > 2048 x 256) and whose only block wraps the import /
export grid (> 4096 x 256 edges); dim-0 rows across workgroup boundaries; a 2-D mesh with both wraps, the mixed block
included; 3-D and 4-D meshes past one grid in the chunked (N % 64 = 0) and the block-major edge layout. Each in the
four block orders (cpp weighted / unit, py weighted / unweighted), theta and v = randn.

Asserted per case, componentwise with u = 2^-53 and a the sum of the absolute values of every term of an output:

    |D theta - ld| <= (|S'(b)| + 2) u a on the rows of block b,     |D^T v - ld| <= (2^p + nb) u a

(derivation and teeth: tests/test_oracle_diff_ld.py). Both outputs are compared position by position over all E
(N) values, so an exported padding anchor would shift every later edge of its block. D^T of a v that is non-zero on
exactly one edge per block must be non-zero on exactly the reference's nodes: the import index arithmetic, exactly.
From the launch log each call is one k_apply_D / k_gather launch of the expected instantiation on the transcribed
grid, plus one export / import launch per block. The worst ratios go to $MVTV_PARITY_LOG."""
import functools

import numpy as np
import pytest

import test_oracle_diff_ld as T
from conftest import log_parity
from oracle import diff_ld as DL

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = T.runs(T.WIDE)


@functools.lru_cache(maxsize=2)
def _inputs(m, E):
    rng = np.random.default_rng(3000 + sum(m))
    th, v = rng.standard_normal(int(np.prod(m))), rng.standard_normal(E)
    th.setflags(write=False)
    v.setflags(write=False)
    return th, v


def _one_per_block(lens, rng):
    """non-zero on one edge per block: the first, the last, or one anywhere (past the first trip of a wrapped grid
    with probability one half there)"""
    one = np.zeros(sum(lens))
    off = 0
    for k, n in enumerate(lens):
        e = (0, n - 1, int(rng.integers(0, n)))[k % 3] if k else int(rng.integers(n // 2, n))
        one[off + e] = rng.uniform(1.0, 2.0)
        off += n
    return one


@pytest.mark.parametrize("run", RUNS, ids=T.run_id)
def test_D_and_Dt(run):
    m, order, weighted = run
    p, N = len(m), int(np.prod(m))
    blocks = T.blocks_of(p, order, weighted)
    lens = DL.block_lengths(m, blocks)
    nb, E = len(blocks), sum(lens)
    th, v = _inputs(m, E)
    ordn = 0 if order == "cpp" else 1
    grid = T.stream_grid(N)
    moves = [T.elem_grid(n) for n in lens]
    with mv.Problem(list(m), np.zeros(N), deltas=T.DELTAS[:p], order=mv.ORDER_CPP if order == "cpp" else mv.ORDER_PY,
                    weighted=weighted) as P:
        assert (P.E, P.nb) == (E, nb)
        with launch_log() as log:
            d = P.apply_D(th)
        assert [(n, g[0], b[0]) for n, g, b in log] == \
            [(f"k_apply_D<{p}, {ordn}>", grid, 256)] + [("k_edges_export", g, 256) for g in moves]
        with launch_log() as log:
            gq = P.apply_Dt(v)
        assert [(n, g[0], b[0]) for n, g, b in log] == \
            [("k_edges_import", g, 256) for g in moves] + [(f"k_gather<{p}, {ordn}, 0, false>", grid, 256)]
        one = _one_per_block(lens, np.random.default_rng(5))
        g1 = P.apply_Dt(one)
    rD = T.ratio_D(m, blocks, d, DL.apply_D(m, blocks, th), DL.apply_D(m, blocks, th, absval=True))
    rDt = T.ratio_Dt(m, blocks, gq, DL.apply_Dt(m, blocks, v), DL.apply_Dt(m, blocks, v, absval=True))
    ref1, a1 = DL.apply_Dt(m, blocks, one), DL.apply_Dt(m, blocks, one, absval=True)
    r1 = T.ratio_Dt(m, blocks, g1, ref1, a1)
    print(f"{T.run_id(run)}: D {rD:.3f} of its bound (c <= {p + 2}), D^T {rDt:.3f} (c = {T.c_Dt(p, nb)}), "
          f"one edge per block {r1:.3f}")
    log_parity(f"operators_wide/{T.run_id(run)}", D=rD, Dt=rDt, Dt_one=r1, c_D=p + 2, c_Dt=T.c_Dt(p, nb))
    assert rD <= 1.0
    assert rDt <= 1.0
    assert np.array_equal(g1 != 0, a1 != 0)
    assert r1 <= 1.0
