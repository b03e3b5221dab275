"""Pins oracle/stencil_ld.py (the matrix-free long-double W + sigma D^T D) against the sparse oracle's
D^T D on the shapes of test_gpu_parity.SHAPES (every block order / weight mode a caller builds) and against the C
oracle's matrix-free D^T (D x) on one mesh of about 1e5 nodes per p. No GPU."""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import mvtv_oracle as O
from oracle import stencil_ld as SL

# test_gpu_parity.SHAPES (that module needs the package to import; the list is restated so this file does not)
SHAPES = [([9], None, "cpp", False), ([7, 5], [0.3, 0.7], "cpp", False), ([6, 6, 6], [0.5, 0.25, 0.125], "cpp", False),
          ([5, 5, 7], [0.2, 0.3, 0.4], "cpp", True), ([4, 4, 4, 5], [0.5, 0.25, 0.125, 0.3], "cpp", False),
          ([6, 5], None, "py", False), ([5, 5, 5], [0.5, 0.25, 0.125], "py", False), ([4, 4, 4, 4], None, "py", False)]


def _blocks(m, deltas, order, unit):
    weighted = (deltas is not None) and not unit
    return O.block_table(len(m), deltas if weighted else None, order, unit_weights=unit)


def test_shapes_are_the_parity_suites():
    """the restated list is test_gpu_parity's (compared as source text: importing that module needs the library)"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py")).read()
    node = next(n for n in ast.parse(src).body
                if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "SHAPES")
    theirs = ast.literal_eval(node.value)
    assert [(list(m), d, o, u) for m, d, o, u in theirs] == [(list(m), d, o, u) for m, d, o, u in SHAPES]


@pytest.mark.parametrize("m,deltas,order,unit", SHAPES)
@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_apply_dtd_matches_build_D(m, deltas, order, unit, dtype):
    blocks = _blocks(m, deltas, order, unit)
    D = O.build_D(m, blocks)
    rng = np.random.default_rng(11)
    N = int(np.prod(m))
    x = rng.standard_normal(N)
    ref = D.T @ (D @ x)
    got = SL.apply_dtd(m, blocks, x, dtype=dtype)
    assert got.dtype == dtype
    assert float(np.max(np.abs(got - ref))) <= 1e-14 * float(np.max(np.abs(ref)))
    # |D|^T |D| |x| bounds the abs-value sum from above (|L| = |d|^T |d| per dim) and equals it: no cancellation
    aref = abs(D).T @ (abs(D) @ np.abs(x))
    agot = SL.apply_dtd(m, blocks, x, dtype=dtype, absval=True)
    assert float(np.max(np.abs(agot - aref))) <= 1e-14 * float(np.max(aref))
    w = rng.integers(0, 4, N).astype(np.float64)
    for sigma in (0.0, 0.37, 25.6):
        a = SL.apply_A(m, blocks, w, sigma, x, dtype=dtype)
        aref = O.apply_A(D, w, sigma, x)
        assert float(np.max(np.abs(a - aref))) <= 1e-14 * float(np.max(np.abs(aref)))
    a1 = SL.apply_A(m, blocks, None, 0.37, x, dtype=dtype)
    assert float(np.max(np.abs(a1 - O.apply_A(D, np.ones(N), 0.37, x)))) <= 1e-14 * float(np.max(np.abs(a1)))


@pytest.mark.parametrize("m,order,weighted", [([100003], "cpp", True), ([317, 316], "cpp", True),
                                              ([46, 46, 47], "py", True), ([18, 18, 18, 17], "cpp", True),
                                              ([46, 46, 47], "cpp", False)])
def test_apply_dtd_matches_c_oracle(m, order, weighted):
    """about 1e5 nodes per p, against the C oracle's matrix-free D^T (D x)"""
    p = len(m)
    deltas = [0.5, 0.25, 0.125, 0.3][:p]
    blocks = O.block_table(p, deltas if weighted else None, order, unit_weights=not weighted)
    O.check_dims(m, blocks)
    rng = np.random.default_rng(12)
    x = rng.standard_normal(int(np.prod(m)))
    o, w = (0 if order == "cpp" else 1), int(weighted)
    ref = c_oracle.apply_Dt(m, c_oracle.apply_D(m, x, deltas, o, w), deltas, o, w)
    got = SL.apply_dtd(m, blocks, x)
    assert float(np.max(np.abs(got - ref))) <= 1e-14 * float(np.max(np.abs(ref)))
