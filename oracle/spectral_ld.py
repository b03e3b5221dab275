"""Long-double reference of the spectral theta-solve — CPU ORACLE, TEST INFRASTRUCTURE ONLY.

x = IDCT(DCT(b) / (1 + sigma sym)) with scipy.fft's orthonormal DCT-II on ``np.longdouble`` (pocketfft's long-double
kernels; x87 80-bit on x86-64, eps 1.1e-19) and the symbol of D^T D built in long double from ``block_table`` with a
long-double pi. It shares no code with the GPU path and none of its float64 round-off, so a forward comparison
max|x_gpu - x_ld| sees errors of a few eps that a residual through the GPU's own stencil cannot (tests/test_gpu_dispatch.py).

The same functions with ``dtype=np.float64`` evaluate the same formula in float64 pocketfft: the distance of that
result from the long-double one (e64) is the round-off a float64 evaluation of this formula has on a given mesh and
sigma, the yardstick of the GPU bound.

Mixed-partial dimension rule (check_dims): a block whose nominal set starts after dim 0 needs m_0 = m_{min S}, so 3-D
meshes need m_0 = m_1 and 4-D meshes m_0 = m_1 = m_2.
"""
from __future__ import annotations

import numpy as np
import scipy.fft as sfft

from .mvtv_oracle import block_table, check_dims

LD = np.longdouble


def _order_name(order):
    return order if isinstance(order, str) else ("cpp" if order == 0 else "py")


def dtd_symbol_ld(m, deltas, order=0, weighted=True, dtype=LD):
    """sum_S cS[S] prod_{j in S} 4 sin^2(pi k_j / (2 m_j)) on the (k_0, ..., k_{p-1}) grid (Fortran order) in
    ``dtype``: the eigenvalues of D^T D in the cosine basis, cS[S] = sum of w_b^2 over blocks with S'(b) = S."""
    p = len(m)
    blocks = block_table(p, deltas if weighted else None, _order_name(order), unit_weights=not weighted)
    check_dims(m, blocks)
    cS = {}
    for blk in blocks:
        w = dtype(blk.w)   # the float64 weight defines the operator; squares and sums in dtype
        cS[blk.Sp] = cS.get(blk.Sp, dtype(0.0)) + w * w
    pi = dtype(4.0) * np.arctan(dtype(1.0))
    lam = [dtype(4.0) * np.sin(pi * np.arange(mj, dtype=dtype) / dtype(2 * int(mj))) ** 2 for mj in m]
    out = np.zeros([int(v) for v in m], dtype=dtype, order="F")
    for S, c in cS.items():
        term = np.full([1] * p, c, dtype=dtype)
        for j in S:
            shape = [1] * p
            shape[j] = int(m[j])
            term = term * lam[j].reshape(shape)
        out += term
    return out


def forward_ld(m, b, dtype=LD, workers=-1):
    """Orthonormal DCT-II of b (N values, dim 0 fastest) over every dimension, in ``dtype``."""
    shape = [int(v) for v in m]
    bb = np.asarray(b, dtype=np.float64).reshape(shape, order="F").astype(dtype, order="F")
    return sfft.dctn(bb, type=2, norm="ortho", workers=workers)


def solve_from_forward(fwd, sym, sigma, workers=-1):
    """x (N values, dim 0 fastest, in fwd's dtype) from forward_ld's transform and dtd_symbol_ld's symbol."""
    dtype = fwd.dtype.type
    t = fwd / (dtype(1.0) + dtype(float(sigma)) * sym)
    return sfft.idctn(t, type=2, norm="ortho", workers=workers).ravel(order="F")


def spectral_solve_ld(m, deltas, sigma, b, order=0, weighted=True, dtype=LD):
    """(I + sigma D^T D) x = b by cosine transforms in ``dtype`` (long double by default)."""
    return solve_from_forward(forward_ld(m, b, dtype), dtd_symbol_ld(m, deltas, order, weighted, dtype), sigma)
