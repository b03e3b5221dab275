"""Matrix-free high-precision W + sigma D^T D — CPU ORACLE, TEST INFRASTRUCTURE ONLY.

D^T D = sum_b w_b^2 (x)_{j in S'(b)} L_j with L_j the 1-D Neumann Laplacian along dim j (diagonal 1, 2, ..., 2, 1,
off-diagonals -1) and the identity along the other dims: block b of ``mvtv_oracle.build_D`` differences the reduced
grid along every dim of its effective set S'(b), and (d^T d) of a 1-D first difference d is L. The products below
apply one L per dim to an array reshaped column-major (dim 0 fastest), in ``np.longdouble`` by default (x87 80-bit
on x86-64, eps 1.1e-19), so a mesh of millions of nodes costs seconds and shares neither code nor float64 round-off
with the GPU's stencil kernels (k_apply2d / k_apply3d / k_apply3d2 / k_apply4d, mvtv_cg3d.hip).

``absval=True`` gives a = sum_b w_b^2 ((x)_j |L_j|) |x|, the sum of the absolute values of every term that enters
one output: the scale of a componentwise rounding bound (tests/test_gpu_stencil_march.py).

The same functions with ``dtype=np.float64`` evaluate the same formula in float64.

Pinned against ``build_D`` and the C oracle's ``apply_Dt(apply_D(x))`` in tests/test_oracle_stencil_ld.py.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def _lap(a, axis, absval):
    """L (or |L|) along ``axis``: out_i = (a_i - a_{i-1}) [i > 0] + (a_i - a_{i+1}) [i < m - 1], every minus a
    plus for |L|."""
    out = np.zeros_like(a)
    n = a.shape[axis]
    if n < 2:
        return out
    lo = [slice(None)] * a.ndim
    hi = [slice(None)] * a.ndim
    lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
    lo, hi = tuple(lo), tuple(hi)
    d = a[hi] + a[lo] if absval else a[hi] - a[lo]
    if absval:
        out[lo] += d
    else:
        out[lo] -= d
    out[hi] += d
    return out


def apply_dtd(m, blocks, x, dtype=LD, absval=False):
    """D^T D x (N values, dim 0 fastest) in ``dtype`` for the blocks of ``mvtv_oracle.block_table`` (each block's
    effective set ``Sp`` and weight ``w``); ``absval``: the same sum with |L_j| and |x|."""
    shape = [int(v) for v in m]
    X = np.asarray(x).reshape(shape, order="F").astype(dtype, order="F")   # float64 input converts exactly
    if absval:
        X = np.abs(X)
    cS = {}
    for blk in blocks:
        w = dtype(blk.w)   # the float64 weight defines the operator; squares and sums in dtype
        cS[tuple(blk.Sp)] = cS.get(tuple(blk.Sp), dtype(0.0)) + w * w
    memo = {(): X}

    def prod(S):   # (x)_{j in S} L_j X, one more L than the product over S without its last dim
        if S not in memo:
            memo[S] = _lap(prod(S[:-1]), S[-1], absval)
        return memo[S]

    out = np.zeros(shape, dtype=dtype, order="F")
    for S in sorted(cS):
        out += cS[S] * prod(S)
    return out.ravel(order="F")


def apply_A(m, blocks, W, sigma, x, dtype=LD):
    """(W + sigma D^T D) x in ``dtype``; W = None is the identity."""
    xx = np.asarray(x).astype(dtype)
    wx = xx if W is None else np.asarray(W, dtype=np.float64).astype(dtype) * xx
    return wx + dtype(float(sigma)) * apply_dtd(m, blocks, x, dtype)
