"""lambda_max where the reference's CG is well conditioned: the two recurrences, the right-hand sides and the closed
form for tests/test_lammax_ref_host.py (CPU) and tests/test_gpu_lambda_max.py (GPU).

The reference finds lambda_max from x = pinv(D^T D) O^T y by a hand-written CG: the released package's cg / mypinv
(rcpp-code/MultivarTV/src/utils.cpp:306-355; CG on the normal equations of A = D^T D from x = 0, relative stop
||A (b - A x)|| < 1e-4 ||A b||, lambda_max = 5 max|D x|) and the research code's (cpp-code/utils.cpp:354-404; plain CG
from x = mean(b), absolute stop ||b - A x|| < 0.01, lambda_max = max|D x|). On scattered data both run to their
iteration cap and round-off decides the value, so tests/test_gpu_cv.py and tests/test_gpu_cxx_cpp.py can ask for 5e-3
and 1e-2 only. Here b is a sum of K = 4 eigenvectors of D^T D,

    b = s sum_k a_k v_k,   v_k = (x)_j cos(pi k_j (i_j + 1/2) / m_j),   (D^T D) v_k = lam_k v_k

with lam_k the symbol sum_S cS[S] prod_{j in S} 4 sin^2(pi k_j / (2 m_j)) (oracle/spectral_ld.py). In exact arithmetic
both CGs stop after exactly K iterations at x = s sum_k a_k v_k / lam_k (plus a constant for the second, which D
annihilates), so lambda_max is a closed form: max|D x| through oracle/diff_ld.py in long double. The frequencies are
high, k_j about (0.5, 0.65, 0.8, 0.97) m_j: the eigenvalues are among the operator's largest, CG's steps are short and
round-off in the other modes is not amplified (three low modes ran to 210 iterations); they differ along every
dimension, so the four eigenvalues stay apart whichever block's weight dominates.

The residual norms of the four-component problem are those of CG on diag(lam_k) with right-hand side a_k ||v_k||
(``model_residuals``: a 4 x 4 problem in long double), which fixes the scale s, a power of two, so that the research
code's absolute test sits between iterations K - 1 and K: ||r_{K-1}|| in [16, 32) against the threshold 0.01, and
picks the amplitudes a_k from a short list (``AMPS_MENU``).
"""
import functools
import math

import numpy as np

from oracle import diff_ld as DL
from oracle import mvtv_oracle as O
from oracle import stencil_ld as SL

LD = np.longdouble
K = 4
FRACTIONS = (0.5, 0.65, 0.8, 0.97)
# amplitude sets, the highest mode the strongest (it carries max|D x| into the block with the most differences); a
# case takes the first whose K-component model leaves the released package's residual at K - 1 above 1.15e-2 (100
# times the stop threshold and 15 % more)
AMPS_MENU = ((0.4, -0.6, 0.9, 1.6), (1.0, -0.8, 1.2, 0.9), (0.25, -0.5, 1.0, 2.0), (1.0, -1.0, 1.0, 1.0),
             (2.0, -1.0, 0.7, 1.0))
RTOL_RCPP, ATOL_CPP = 1e-4, 0.01


# ------------------------------------------------------------------------------------------ the two recurrences
def cg_rcpp(A, b, dtype=np.float64, beta_on_r=False):
    """cg of rcpp…/utils.cpp:306-341 over a callable A (oracle.mvtv_oracle.lam_max_pinv_rcpp line by line): returns
    (x, iterations, [sqrt(rsnew) / rsold0 after each iteration]). beta_on_r: the defect p = p + beta r."""
    b = np.asarray(b).astype(dtype)
    x = np.zeros(b.size, dtype=dtype)
    d = b - A(x)
    r = A(d)
    p = r.copy()
    rsold0 = np.sqrt(r @ r)
    rsold = rsold0 ** 2
    rsnew = rsold + dtype(1.0)
    t = A(p)
    it, hist = 0, []
    maxit = b.size if b.size < 2000 else 2000
    while np.sqrt(rsnew) >= dtype(RTOL_RCPP) * rsold0:
        alpha = rsold / np.sqrt(t @ t) ** 2
        x = x + alpha * p
        d = d - alpha * t
        r = A(d)
        rsnew = np.sqrt(r @ r) ** 2
        it += 1
        hist.append(float(np.sqrt(rsnew) / rsold0))
        if it == maxit:
            break
        p = (p + (rsnew / rsold) * r) if beta_on_r else (r + (rsnew / rsold) * p)
        t = A(p)
        rsold = rsnew
    return x, it, hist


def cg_cpp(A, b, dtype=np.float64, beta_on_r=False):
    """cg of cpp-code/utils.cpp:354-386 (oracle.mvtv_oracle.lam_max_pinv_cpp line by line): returns (x, iterations,
    [sqrt(rsnew) after each iteration])."""
    b = np.asarray(b).astype(dtype)
    x = np.full(b.size, b.mean(), dtype=dtype)
    r = b - A(x)
    p = r.copy()
    rsold = r @ r
    rsnew = rsold + dtype(1.0)
    maxit = 500 if b.size < 400 else 100
    it, hist = 0, []
    while np.sqrt(rsnew) >= dtype(ATOL_CPP):
        Ap = A(p)
        alpha = rsold / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        rsnew = r @ r
        it += 1
        hist.append(float(np.sqrt(rsnew)))
        if it == maxit:
            break
        p = (p + (rsnew / rsold) * r) if beta_on_r else (r + (rsnew / rsold) * p)
        rsold = rsnew
    return x, it, hist


def operator(m, blocks, dtype):
    """A = D^T D, matrix-free (oracle/stencil_ld.py)"""
    return lambda v: SL.apply_dtd(m, blocks, v, dtype)


# ------------------------------------------------------------------------------------------ modes and the closed form
def modes(m, dims=None):
    """K frequency vectors: k_j = round(f m_j) within 1 .. m_j - 1 for j in ``dims`` (all by default), 0 elsewhere.
    On a short dimension, where two fractions round to one frequency, the lower modes step down by one each (m_j = 6:
    2, 3, 4, 5), so the K eigenvalues stay apart along every dimension of at least five nodes."""
    dims = range(len(m)) if dims is None else dims
    per_dim = []
    for j, mj in enumerate(m):
        if j not in dims:
            per_dim.append([0] * K)
            continue
        k = [min(max(int(round(f * int(mj))), 1), int(mj) - 1) for f in FRACTIONS]
        for i in range(K - 2, -1, -1):
            k[i] = max(1, min(k[i], k[i + 1] - 1))
        per_dim.append(k)
    ks = [tuple(per_dim[j][i] for j in range(len(m))) for i in range(K)]
    assert len(set(ks)) == K, (m, ks)
    return ks


def _cos(mj, k, dtype=LD):
    pi = dtype(4.0) * np.arctan(dtype(1.0))
    # the argument reduced exactly: k (2 i + 1) mod 4 m
    n = (int(k) * (2 * np.arange(int(mj), dtype=np.int64) + 1)) % (4 * int(mj))
    return np.cos(pi * n.astype(dtype) / dtype(2 * int(mj)))


def combine(m, ks, coef, dtype=LD):
    """sum_k coef_k v_k (N values, dim 0 fastest) in ``dtype``"""
    out = np.zeros([int(v) for v in m], dtype=dtype, order="F")
    for k, c in zip(ks, coef):
        term = np.full([1] * len(m), dtype(c), dtype=dtype)
        for j, mj in enumerate(m):
            shape = [1] * len(m)
            shape[j] = int(mj)
            term = term * _cos(mj, k[j], dtype).reshape(shape)
        out += term
    return out.ravel(order="F")


def eigenvalues(m, blocks, ks, dtype=LD):
    """the symbol at ks, from the blocks' own weights (cS[S'] = sum w_b^2)"""
    pi = dtype(4.0) * np.arctan(dtype(1.0))
    out = []
    for k in ks:
        lam = dtype(0.0)
        for blk in blocks:
            t = dtype(blk.w) * dtype(blk.w)
            for j in blk.Sp:
                t = t * dtype(4.0) * np.sin(pi * dtype(k[j]) / dtype(2 * int(m[j]))) ** 2
            lam = lam + t
        out.append(lam)
    return out


def model_residuals(lam, c):
    """the residual histories of both CGs on diag(lam) with right-hand side c (the K-component problem that the
    full one is in exact arithmetic), in long double: (rcpp's relative, cpp's absolute per unit scale)"""
    lam = np.array(lam, dtype=LD)
    A = lambda v: lam * v   # noqa: E731
    _, it_r, hr = cg_rcpp(A, np.array(c, dtype=LD), LD)
    # plain CG without the mean start (the modes have zero mean)
    b = np.array(c, dtype=LD)
    x, r = np.zeros(K, dtype=LD), b.copy()
    p, rs, hc = r.copy(), r @ r, []
    for _ in range(K):
        Ap = A(p)
        al = rs / (p @ Ap)
        x, r = x + al * p, r - al * Ap
        rn = r @ r
        hc.append(float(np.sqrt(rn)))
        p, rs = r + (rn / rs) * p, rn
    return hr, hc


class Case:
    """one lambda_max problem: mesh, blocks, b (float64) and the closed form"""

    def __init__(self, m, order="cpp", weighted=True, deltas=None, dims=None):
        self.m = [int(v) for v in m]
        self.p = len(self.m)
        self.order, self.weighted = order, weighted
        self.deltas = [1.0] * self.p if deltas is None else [float(v) for v in deltas]
        self.blocks = O.block_table(self.p, self.deltas if weighted else None, order, unit_weights=not weighted)
        O.check_dims(self.m, self.blocks)
        self.ks = modes(self.m, dims)
        self.lam = eigenvalues(self.m, self.blocks, self.ks)
        norms = [math.sqrt(np.prod([mj / 2.0 if kj else float(mj) for mj, kj in zip(self.m, k)])) for k in self.ks]
        lam_top = float(self.lam[-1])
        # after the fixed sets: the lower modes raised by (lam_K / lam_k)^g, for the cases whose eigenvalues lie far
        # apart (a short dimension under a dominating mixed block), where the residual A (b - A x) hides them
        menu = AMPS_MENU + tuple(tuple(sg * (lam_top / float(l)) ** g for sg, l in zip((1.0, -1.0, 1.0, 1.0), self.lam))
                                 for g in (0.5, 1.0, 1.5, 2.0))
        for amps in menu:
            self.amps = amps
            self.model_rcpp, hc = model_residuals(self.lam, [a * n for a, n in zip(amps, norms)])
            if len(self.model_rcpp) == K and self.model_rcpp[K - 2] >= 1.15e-2:
                break
        else:
            raise AssertionError(f"no amplitude set keeps the residual at K - 1 up on {self.m} {order} {deltas}")
        # s = 2^e with s ||r_{K-1}|| in [16, 32)
        self.scale = 2.0 ** (4 - math.floor(math.log2(hc[K - 2])))
        self.model_cpp = [self.scale * v for v in hc]
        self.coef = [self.scale * a for a in self.amps]

    @property
    def name(self):
        return "x".join(str(v) for v in self.m) + f"-{self.order}-{'w' if self.weighted else 'unit'}"

    @functools.cached_property
    def b(self):
        b = combine(self.m, self.ks, self.coef).astype(np.float64)
        b.setflags(write=False)
        return b

    @functools.cached_property
    def x_exact(self):
        return combine(self.m, self.ks, [LD(c) / l for c, l in zip(self.coef, self.lam)])

    def max_abs_D(self, x, blocks=None):
        """(max|D x|, the block that holds the first row attaining it) in long double"""
        blocks = self.blocks if blocks is None else blocks
        d = np.abs(DL.apply_D(self.m, blocks, np.asarray(x), LD))
        row = int(np.argmax(d))
        ends = np.cumsum(DL.block_lengths(self.m, blocks))
        return d[row], int(np.searchsorted(ends, row, side="right"))

    @functools.cached_property
    def closed_form(self):
        """(lambda_max of the released package, of the research code, block of the argmax row of |D x|)"""
        v, blk = self.max_abs_D(self.x_exact)
        return float(LD(5.0) * v), float(v), blk


# ------------------------------------------------------------------------------------------ the cases
DELTAS = [0.9, 1.1, 0.8, 1.25]
SMALL = [(600,), (40, 33), (12, 12, 9), (6, 6, 6, 5)]
LARGE = [(1048876,), (1030, 520), (65, 65, 130), (28, 28, 28, 25)]
# (block order, weighted): cpp weighted, cpp unit, py weighted (no all-ones block; none at all at p = 1), py unweighted
ORDERS = [("cpp", True), ("cpp", False), ("py", True), ("py", False)]
STEER = 16.0
# the steered 4-D cases: every frequency of (6, 6, 6, 5)'s last dim below 3 shrinks under a difference (2 sin(pi k /
# 2 m) < 1.2), so a block gains nothing from differencing it; on 8 x 8 x 8 x 7 every difference gains 1.25 or more
STEERED = [(600,), (40, 33), (12, 12, 9), (8, 8, 8, 7)]


def specs():
    """(m, order, weighted, deltas, dims, target) of every GPU case. Plain: the eight meshes in the four orders with
    DELTAS, all dims excited. Steered, on the small meshes of ``STEERED``, so that the first row attaining max|D x|
    lies in a chosen block: with weights, w_b = prod_{j not in b} delta_j is the largest by a factor 16 when
    delta_j = 16 outside b and 1 / 16 inside (target: the block's index); without, the modes are constant along the
    dims outside S', every block that differences one of those gives 0 and the blocks with that S' give the most
    (target: S'; blocks of equal S' and weight have equal rows, no max can tell them apart)."""
    out = []
    for m in SMALL + LARGE:
        p = len(m)
        for order, weighted in ORDERS:
            if p == 1 and order == "py" and weighted:
                continue
            out.append((m, order, weighted, tuple(DELTAS[:p]), None, None))
    for m in STEERED:
        p = len(m)
        for order, weighted in ORDERS:
            if p == 1 and order == "py" and weighted:
                continue
            blocks = O.block_table(p, [1.0] * p if weighted else None, order, unit_weights=not weighted)
            if weighted:
                for t, blk in enumerate(blocks):
                    deltas = tuple(1.0 / STEER if j in blk.S else STEER for j in range(p))
                    out.append((m, order, weighted, deltas, None, t))
            else:
                for Sp in sorted({blk.Sp for blk in blocks}):
                    out.append((m, order, weighted, tuple(DELTAS[:p]), Sp, Sp))
    return out


def spec_id(s):
    m, order, weighted, deltas, dims, target = s
    name = "x".join(str(v) for v in m) + f"-{order}-{'w' if weighted else 'unit'}"
    if target is not None:
        name += "-argmax-" + ("".join(str(j) for j in target) if isinstance(target, tuple) else f"b{target}")
    return name


@functools.lru_cache(maxsize=2)
def case(s):
    m, order, weighted, deltas, dims, _ = s
    return Case(m, order, weighted, deltas, dims)
