"""The componentwise bound of the stencil-operator tests (tests/test_gpu_stencil_march.py on the GPU,
tests/test_pcg_ref_host.py for its teeth on the CPU) and a float64 numpy model of the marching kernels' arithmetic.

Bound. One output of q = (W + sigma D^T D) x is a sum of 3^p products K_t x_n over the stencil's neighbours, K_t =
sigma sum_S cS[S] prod_j f_j(t_j) by offset class t (launch_apply2d / 3d / 4d, mvtv_cg3d.hip:660-671, :791-802,
:887-898). Every term of K_t has the sign (-1)^|t| (a term is non-zero only for t inside S), so neither K_t nor
the scale a = sum_t |K_t| sum |x_n| / sigma = sum_b w_b^2 ((x)|L_j|) |x| (oracle.stencil_ld.apply_dtd, absval) hides
a cancellation. With u = 2^-53: K_t, a sum of at most 2^p - 1 terms of p factors each times sigma, carries at most
(2^p + p + 1) u relative; accumulating 3^p products adds at most 3^p u; the W term 2 u; a factor 2 for second-order
terms and fma against separate operations:

    |q - q_ld| <= c u (|W| |x| + sigma a),   c = 2 (3^p + 2^p + p + 4)

derived, not tuned: 38, 84, 210 for p = 2, 3, 4."""
import functools

import numpy as np

from oracle import mvtv_oracle as O
from oracle import stencil_ld as SL

U = 2.0 ** -53
DELTAS = [0.5, 0.25, 0.125, 0.3]


def c_bound(p):
    return 2 * (3 ** p + 2 ** p + p + 4)


def blocks_of(p, order="cpp", unit=False):
    """deltas [0.5, 0.25, 0.125, 0.3][:p]; unit: every block weight 1"""
    return O.block_table(p, None if unit else DELTAS[:p], order, unit_weights=unit)


def make_x(m, seed=0):
    return np.random.default_rng(1000 + seed + sum(int(v) for v in m)).standard_normal(int(np.prod(m)))


def make_w(m, seed=0):
    """W = integers 0 .. 3, zeros included"""
    rng = np.random.default_rng(2000 + seed + sum(int(v) for v in m))
    return rng.integers(0, 4, int(np.prod(m))).astype(np.float64)


@functools.lru_cache(maxsize=4)
def reference(m, order="cpp", unit=False, seed=0):
    """(x, D^T D x, a) of mesh m (a tuple) in long double, built once per mesh and shared by every sigma and W."""
    x = make_x(m, seed)
    blocks = blocks_of(len(m), order, unit)
    O.check_dims(m, blocks)
    dtd = SL.apply_dtd(m, blocks, x)
    a = SL.apply_dtd(m, blocks, x, absval=True)
    for v in (x, dtd, a):
        v.setflags(write=False)
    return x, dtd, a


def ratio(q, W, sigma, x, dtd, a):
    """max_i |q_i - q_ld,i| / (u (|W_i| |x_i| + sigma a_i)) with q_ld = W x + sigma dtd in long double, and max|q_ld|;
    where the scale is 0 (W_i = 0 and sigma = 0) the output must be exactly 0 (inf otherwise)."""
    LD = np.longdouble
    xl = x.astype(LD)
    wx = xl if W is None else W.astype(LD) * xl
    qld = wx + LD(sigma) * dtd
    den = LD(U) * (np.abs(wx) + LD(sigma) * a)
    err = np.abs(np.asarray(q, dtype=np.float64).astype(LD) - qld)
    pos = den > 0
    r = float(np.max(err[pos] / den[pos])) if pos.any() else 0.0
    if (err[~pos] != 0).any():
        r = float("inf")
    return r, float(np.max(np.abs(qld))), float(np.max(err))


def stencil_weights(p, blocks, sigma, w_identity):
    """K[t], t = sum_j |o_j| 2^j, as the launchers form it in float64: cS[S] = sum of w_b^2 by effective set (bit j
    of S: dim j), K_t = sigma sum_S cS[S] prod_j (j in S ? (o_j ? -1 : 2) : (o_j ? 0 : 1)), + 1 at t = 0 for W = I."""
    cS = np.zeros(1 << p)
    for blk in blocks:
        cS[sum(1 << j for j in blk.Sp)] += blk.w * blk.w
    K = np.zeros(1 << p)
    for t in range(1 << p):
        kk = 0.0
        for S in range(1, 1 << p):
            prod = cS[S]
            for j in range(p):
                off = (t >> j) & 1
                prod *= ((-1.0 if off else 2.0) if (S >> j) & 1 else (0.0 if off else 1.0))
            kk += prod
        K[t] = sigma * kk
    if w_identity:
        K[0] += 1.0
    return K


def class_sums(m, x, wrong_mirror_col=None):
    """v[t], t = sum_j |o_j| 2^j: per offset class the sum of x over the mirrored neighbours (a neighbour past the
    mesh is the cell itself), built a dimension at a time. wrong_mirror_col = c: column c of dim 0 takes itself for
    its right neighbour c + 1, the defect of a tile edge (lane 63 / 255) that mirrors instead of loading."""
    p = len(m)
    X = np.asarray(x, dtype=np.float64).reshape([int(v) for v in m], order="F")
    v = {0: X}
    for j in range(p):
        n = X.shape[j]
        lo = np.clip(np.arange(n) - 1, 0, n - 1)
        hi = np.clip(np.arange(n) + 1, 0, n - 1)
        if j == 0 and wrong_mirror_col is not None:
            hi[wrong_mirror_col] = wrong_mirror_col
        for t, A in list(v.items()):
            v[t | (1 << j)] = np.take(A, lo, axis=j) + np.take(A, hi, axis=j)
    return [v[t] for t in range(1 << p)]


def model_apply(K, v, x, W=None):
    """float64 model of the marching kernels: q = sum_t K_t v_t (+ W x) over class_sums' v."""
    out = np.zeros_like(v[0])
    for t in range(len(v)):
        out += K[t] * v[t]
    out = out.ravel(order="F")
    if W is not None:
        out = out + W * x
    return out
