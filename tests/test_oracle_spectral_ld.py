"""Pin the long-double spectral reference (oracle/spectral_ld.py, the yardstick of tests/test_gpu_dispatch.py)
against SciPy's SuperLU factorisation of the assembled I + sigma D^T D."""
import numpy as np
import pytest

from oracle import mvtv_oracle as O
from oracle import spectral_ld as S

CASES = [([6, 6, 4], [0.5, 0.25, 0.125], "cpp", True), ([6, 6, 4], None, "py", False),
         ([5, 5, 5, 3], [0.1, 0.2, 0.3, 0.4], "cpp", True), ([7, 12], [0.3, 0.7], "py", True),
         ([7, 12], [0.3, 0.7], "cpp", True)]


def _cond(blocks, sigma):
    """cond(I + sigma D^T D) <= 1 + sigma sum_b w_b^2 4^|S'(b)| (tests/test_gpu_spectral.py _cond)"""
    return 1.0 + sigma * sum(b.w * b.w * 4.0 ** len(b.Sp) for b in blocks)


@pytest.mark.parametrize("m,deltas,order,weighted", CASES)
@pytest.mark.parametrize("sigma", [0.05, 400.0])
def test_spectral_ld_vs_superlu(m, deltas, order, weighted, sigma):
    blocks = O.block_table(len(m), deltas if weighted else None, order, unit_weights=not weighted)
    D = O.build_D(m, blocks)
    N = int(np.prod(m))
    b = np.random.default_rng(3).standard_normal(N) + 2.0
    ref = O._solver(np.ones(N), (D.T @ D).tocsc(), sigma).solve(b)
    x = S.spectral_solve_ld(m, deltas, sigma, b, order=order, weighted=weighted)
    assert x.dtype == np.longdouble and x.shape == (N,)
    err = float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
    print(f"{m} {order} sigma {sigma}: long-double spectral vs SuperLU {err:.2e}")
    # SuperLU is backward stable: forward error ~ eps cond(A)
    assert err <= max(1e-12, 2e-16 * _cond(blocks, sigma))
    # the float64 evaluation of the same formula sits at rounding level of the long-double one
    x64 = S.spectral_solve_ld(m, deltas, sigma, b, order=order, weighted=weighted, dtype=np.float64)
    assert x64.dtype == np.float64
    assert float(np.max(np.abs(x64 - x)) / np.max(np.abs(x))) <= 1e-14


def test_forward_is_shared_across_sigma():
    """forward_ld once, solve_from_forward per sigma: the same numbers as the one-call form; sigma = 0 is the
    identity to long-double rounding."""
    m, deltas = [6, 6, 4], [0.5, 0.25, 0.125]
    b = np.random.default_rng(4).standard_normal(144) + 2.0
    fwd, sym = S.forward_ld(m, b), S.dtd_symbol_ld(m, deltas)
    for sigma in (0.0, 3.7):
        x = S.solve_from_forward(fwd, sym, sigma)
        assert np.array_equal(x, S.spectral_solve_ld(m, deltas, sigma, b))
    assert float(np.max(np.abs(S.solve_from_forward(fwd, sym, 0.0) - b))) <= 1e-17


def test_dimension_rule():
    """3-D meshes need m_0 = m_1 (the reference's mixed-partial construction)."""
    with pytest.raises(O.DimMismatch):
        S.dtd_symbol_ld([6, 5, 4], [0.5, 0.25, 0.125])
