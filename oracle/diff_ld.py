"""Matrix-free high-precision D and D^T — CPU ORACLE, TEST INFRASTRUCTURE ONLY.

Block b of ``mvtv_oracle.build_D`` is w_b times the iterated first difference d_j : a_i -> a_i - a_{i+1} along every
dim j of its effective set S'(b), over the reduced grid (m_j - 1 along j in S'), rows in column-major order; D stacks
the blocks in ``block_table``'s order. The products below take those differences (or their adjoints) of an array
reshaped column-major (dim 0 fastest), in ``np.longdouble`` by default (x87 80-bit on x86-64, eps 1.1e-19), so a mesh
of millions of nodes costs seconds and shares neither code nor float64 round-off with the GPU's k_apply_D / k_gather
(mvtv_kernels.hip) and the edge import / export kernels.

``absval=True`` gives the sum of the absolute values of every term that enters one output: w_b sum of |theta| over
the 2^|S'| corners of an edge for D, and |D|^T |v| for D^T: the scale of a componentwise rounding bound
(tests/test_gpu_operators_wide.py).

The same functions with ``dtype=np.float64`` evaluate the same formula in float64.

Pinned against ``build_D`` and the C oracle's apply_D / apply_Dt in tests/test_oracle_diff_ld.py.
"""
from __future__ import annotations

import numpy as np

from .mvtv_oracle import reduced_dims

LD = np.longdouble


def _sl(ndim, axis, s):
    out = [slice(None)] * ndim
    out[axis] = s
    return tuple(out)


def _diff(a, axis, absval):
    """d (or |d|) along ``axis``: out_i = a_i - a_{i+1} (plus for |d|), one shorter along ``axis``."""
    n = a.shape[axis]
    lo, hi = a[_sl(a.ndim, axis, slice(0, n - 1))], a[_sl(a.ndim, axis, slice(1, n))]
    return lo + hi if absval else lo - hi


def _diff_t(a, axis, absval):
    """d^T (or |d|^T) along ``axis``: out_i = a_i [i < m - 1] - a_{i-1} [i > 0] (plus for |d|^T), one longer."""
    shape = list(a.shape)
    n = shape[axis]
    shape[axis] = n + 1
    out = np.zeros(shape, dtype=a.dtype, order="F")
    out[_sl(a.ndim, axis, slice(0, n))] += a
    if absval:
        out[_sl(a.ndim, axis, slice(1, n + 1))] += a
    else:
        out[_sl(a.ndim, axis, slice(1, n + 1))] -= a
    return out


def block_lengths(m, blocks):
    return [int(np.prod(reduced_dims(m, blk.Sp))) for blk in blocks]


def apply_D(m, blocks, theta, dtype=LD, absval=False):
    """D theta (E values, blocks in order, each raveled column-major over its reduced grid) in ``dtype``;
    ``absval``: |D| |theta|."""
    shape = [int(v) for v in m]
    X = np.asarray(theta).reshape(shape, order="F").astype(dtype, order="F")   # float64 input converts exactly
    if absval:
        X = np.abs(X)
    memo = {(): X}

    def prod(S):   # the differences along every dim of S, one more than along S without its last dim
        if S not in memo:
            memo[S] = _diff(prod(S[:-1]), S[-1], absval)
        return memo[S]

    out = []
    for blk in blocks:
        w = dtype(blk.w)
        out.append(((abs(w) if absval else w) * prod(tuple(blk.Sp))).ravel(order="F"))
    return np.concatenate(out) if out else np.zeros(0, dtype=dtype)


def apply_Dt(m, blocks, v, dtype=LD, absval=False):
    """D^T v (N values, dim 0 fastest) in ``dtype``; ``absval``: |D|^T |v|."""
    shape = [int(x) for x in m]
    V = np.asarray(v).astype(dtype)
    if absval:
        V = np.abs(V)
    out = np.zeros(shape, dtype=dtype, order="F")
    off = 0
    for blk in blocks:
        rd = reduced_dims(shape, blk.Sp)
        R = int(np.prod(rd))
        a = V[off:off + R].reshape(rd, order="F")
        off += R
        for j in blk.Sp:
            a = _diff_t(a, j, absval)
        w = dtype(blk.w)
        out += (abs(w) if absval else w) * a
    if off != V.size:
        raise ValueError(f"v holds {V.size} values, D has {off} rows")
    return out.ravel(order="F")
