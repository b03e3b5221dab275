"""Shared by tests/test_small_batch_host.py and tests/test_gpu_small_batch*.py: the transcription of the batched
small-mesh kernel's admission formula and launch rules (multivartv_amd/csrc/mvtv_internal.h small_ok, small_nt,
small_zlds) and the test problems, built once per process.

Problems. `problem(m, wkind, ...)`: a noisy step on the mesh. wkind "I": mesh == data (W = I). wkind "S": N scattered
points binned to their nearest node, so W holds counts and about a third of the nodes are empty (W = 0).
deltas_j = (1 + 2e-4) / m_j as create_deltas gives on the unit cube.
"""
import functools
import math

import numpy as np

from oracle import mvtv_oracle as O

CHUNK = 32          # kSmallChunk: ADMM iterations a launch runs at most
MAX_N = 4096        # kSmallMaxN (p <= 3)
MAX_N4 = 1296       # kSmallMaxN4 (p = 4)
Z_LDS_WORDS = 14336  # kSmallZLds: nb * N up to which the edge state stays in LDS

LAMS = [2.0, 1.0, 0.5, 0.2, 0.05]   # the warm-started grid of the issue's iteration table


def admitted(m):
    N = int(np.prod(m))
    return N <= (MAX_N4 if len(m) == 4 else MAX_N)


def nt_rule(N):
    return 64 if N <= 256 else (256 if N <= 1024 else 1024)


def n_blocks(p, order="cpp", weighted=True):
    return len(O.block_table(p, [1.0] * p if weighted else None, order, unit_weights=not weighted and order == "cpp"))


def instantiation(m, order="cpp", weighted=True):
    """The kernel name the launch log shows for mesh m."""
    N, p = int(np.prod(m)), len(m)
    zlds = n_blocks(p, order, weighted) * N <= Z_LDS_WORDS
    return f"k_admm_small<{p}, {nt_rule(N)}, {'true' if zlds else 'false'}>"


def reachable_instantiations():
    """Every (P, NT, ZLDS) some admitted mesh reaches, from the rules alone: N ranges over what the NT class and the
    admission allow, nb over the block counts of the four layouts."""
    out = set()
    for p in (1, 2, 3, 4):
        nbs = {n_blocks(p, o, w) for o in ("cpp", "py") for w in (True, False)}
        cap = MAX_N4 if p == 4 else MAX_N
        for N in range(2 ** p, cap + 1):
            for nb in nbs:
                out.add(f"k_admm_small<{p}, {nt_rule(N)}, {'true' if nb * N <= Z_LDS_WORDS else 'false'}>")
    return out


# The shapes of the single fits: the smallest at which each path can go wrong (two nodes a dimension, one wave, a
# ragged last wave, every NT class, four nodes a thread), plus 11^3 (p = 3 at NT = 1024 with z in LDS), 5^4 (p = 4 at
# NT = 256) and 4 x 4 x 4 x 16 (p = 4 at NT = 256 with z in HBM: fifteen blocks of 1024 words), which reach the
# instantiations the others leave out.
SHAPES = [
    [2], [20], [100], [1000], [4096],
    [2, 2], [10, 10], [31, 33], [64, 64], [2, 2048], [2048, 2],
    [2, 2, 2], [4, 4, 4], [7, 7, 7], [11, 11, 11], [16, 16, 16],
    [2, 2, 2, 2], [4, 4, 4, 4], [5, 5, 5, 5], [4, 4, 4, 16], [6, 6, 6, 6],
]
# one mesh per p for the other three block layouts (order, weighted)
LAYOUT_SHAPES = [[100], [10, 10], [4, 4, 4], [4, 4, 4, 4]]
LAYOUTS = [("cpp", False), ("py", True), ("py", False)]
PATH_SHAPES = [[20], [10, 10], [4, 4, 4], [5, 5, 5, 5]]
REFUSED_SHAPES = [[4097], [7, 7, 7, 7]]


def single_cases():
    """(m, order, weighted, wkind) of every single fit."""
    cases = [(m, "cpp", True, wk) for m in SHAPES for wk in ("I", "S")]
    # (p = 1 has no weighted py layout: its only block is the all-ones one, which that layout drops)
    cases += [(m, o, w, "S") for m in LAYOUT_SHAPES for (o, w) in LAYOUTS if not (len(m) == 1 and o == "py" and w)]
    return cases


def case_id(c):
    m, order, weighted, wk = c
    return "x".join(str(v) for v in m) + f"-{order}{'w' if weighted else 'u'}-{wk}"


def deltas_of(m):
    return [(1.0 + 2e-4) / v for v in m]


def conv_tol(m):
    """The converged run's tol: 1e-2 on the N >= 1000 shapes and on 5^4 (625 nodes, an 81-point factorisation per
    iteration: 4 s of SuperLU at 1e-4), which keeps the reference short; the default 1e-4 below."""
    return 1e-2 if int(np.prod(m)) >= 600 else 1e-4


LAM_SINGLE = 0.5


@functools.lru_cache(maxsize=None)
def _problem(m, wkind, seed):
    m = list(m)
    N, p = int(np.prod(m)), len(m)
    rng = np.random.default_rng(1000 * seed + 7 * N + p)
    axes = [(np.arange(v) + 0.5) / v for v in m]
    grids = np.meshgrid(*axes, indexing="ij")
    coords = np.stack([g.reshape(-1, order="F") for g in grids], axis=1)   # column-major nodes
    step = lambda x: np.where(np.all(x > 0.45, axis=1), 1.0, 0.0) + 0.5 * x[:, 0]
    if wkind == "I":
        y = step(coords) + 0.3 * rng.standard_normal(N)
        return y, None, float(y.mean())
    n = max(N, 4)
    x = rng.uniform(0, 1, size=(n, p))
    y = step(x) + 0.3 * rng.standard_normal(n)
    idx = np.zeros(n, dtype=np.int64)
    stride = 1
    for j in range(p):
        idx += np.minimum((x[:, j] * m[j]).astype(np.int64), m[j] - 1) * stride
        stride *= m[j]
    W = np.bincount(idx, minlength=N).astype(np.float64)
    oty = np.bincount(idx, weights=y, minlength=N)
    assert W.max() > 0
    return oty, W, float(y.mean())


def problem(m, wkind, seed=0):
    """(oty, W or None, mean y)."""
    return _problem(tuple(m), wkind, seed)


@functools.lru_cache(maxsize=None)
def _D(m, order, weighted):
    p = len(m)
    return O.build_D(list(m), O.block_table(p, deltas_of(m) if weighted else None, order,
                                            unit_weights=(order == "cpp" and not weighted)))


def D_of(m, order="cpp", weighted=True):
    return _D(tuple(m), order, weighted)


def margins(history, tol_unused=None):
    """Smallest relative distance of a decision from its threshold over a recorded run (the rule of DESIGN.md §2.2):
    r against 10 s and s against 10 r (adapt_step), r against eps_pri and s against eps_dual (the stopping test)."""
    best = math.inf
    for h in history:
        r, s = h["r_norm"], h["s_norm"]
        for a, b in ((r, 10 * s), (s, 10 * r), (r, h["eps_pri"]), (s, h["eps_dual"])):
            best = min(best, abs(a - b) / max(abs(a), abs(b), 1e-300))
    return best


@functools.lru_cache(maxsize=None)
def _slu_single(m, order, weighted, wkind, tol, max_counter):
    """The converged single fit on the SuperLU oracle, recorded."""
    oty, W, ym = problem(m, wkind)
    D = D_of(m, order, weighted)
    N, E = D.shape[1], D.shape[0]
    Wv = np.ones(N) if W is None else W
    return O.admm_rcpp(D, oty, Wv, LAM_SINGLE, np.full(N, ym), np.zeros(E), LAM_SINGLE / 5.0, tol=tol,
                       max_counter=max_counter, record=True)


def slu_single(c, max_counter=3000):
    m, order, weighted, wk = c
    return _slu_single(tuple(m), order, weighted, wk, conv_tol(m), max_counter)


@functools.lru_cache(maxsize=None)
def _slu_path(m, wkind, seed):
    oty, W, ym = problem(m, wkind, seed)
    D = D_of(m)
    Wv = np.ones(D.shape[1]) if W is None else W
    # mbs_path_rcpp itself, with its admm_rcpp calls recording their histories (for the margins)
    plain = O.admm_rcpp
    O.admm_rcpp = functools.partial(plain, record=True)
    try:
        return O.mbs_path_rcpp(D, oty, Wv, LAMS, ym)
    finally:
        O.admm_rcpp = plain


def slu_path(m, wkind="S", seed=0):
    return _slu_path(tuple(m), wkind, seed)


MIXED_M = [10, 10]


@functools.lru_cache(maxsize=None)
def mixed_members():
    """The mixed-endings batch on 10 x 10: the scattered problem cold-started at each lambda of the grid (tens to
    hundreds of iterations), and one member whose data is 1e-4 N(0, 1) noise about zero: its residuals (8e-4, of the
    size of its state) are below eps (1e-4 sqrt(E) and up) after the first iteration, so it also stops under
    max_counter = 5. Tuples (oty, W, mean y, lambda)."""
    oty, W, ym = problem(MIXED_M, "S")
    out = [(oty, W, ym, lam) for lam in LAMS]
    rng = np.random.default_rng(77)
    y = 1e-4 * rng.standard_normal(W.size)
    out.append((W * y, W, float((W * y).sum() / W.sum()), 0.5))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def slu_member(j, max_counter=3000):
    oty, W, ym, lam = mixed_members()[j]
    D = D_of(MIXED_M)
    N, E = D.shape[1], D.shape[0]
    return O.admm_rcpp(D, oty, W, lam, np.full(N, ym), np.zeros(E), lam / 5.0, max_counter=max_counter, record=True)
