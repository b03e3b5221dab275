"""References of the nominal block orders (MVTV_ORDER_CPP_NOMINAL / MVTV_ORDER_PY_NOMINAL: block b differences along
exactly the dims of its code) for tests/test_nominal_host.py (CPU) and tests/test_gpu_nominal.py (GPU).

The oracle serves unchanged: a ``Block`` of ``oracle.mvtv_oracle.block_table`` with its effective set replaced by its
nominal one (``Sp = S``) is a nominal block, and ``build_block``, ``oracle/diff_ld.py`` and ``oracle/stencil_ld.py``
read only ``Sp``. D is stacked without ``check_dims``, the reference's refusal of m_0 != m_{min S}, which the nominal
rule does not have. The symbol of D^T D,

    sum_S w_S^2 prod_{j in S} 4 sin^2(pi k_j / (2 m_j)),

is built here because ``oracle.spectral_ld.dtd_symbol_ld`` calls ``check_dims``; it goes with that module's
``forward_ld`` / ``solve_from_forward``.
"""
import dataclasses
import functools
import math

import numpy as np
import scipy.sparse as sp

import lammax_ref as L
import small_batch_cases as S
from oracle import mvtv_oracle as O

LD = np.longdouble

ORDER_CPP_NOMINAL, ORDER_PY_NOMINAL = 2, 3   # mvtv_block_order
ORDN = {"cpp": ORDER_CPP_NOMINAL, "py": ORDER_PY_NOMINAL}
# (row order, weighted): the four layouts of the reference's callers
LAYOUTS = [("cpp", True), ("cpp", False), ("py", True), ("py", False)]


def deltas_of(m):
    return [(1.0 + 2e-4) / v for v in m]


def blocks(p, deltas=None, order="cpp", weighted=True):
    """block_table's rows and weights with S(b) = nominal(b)"""
    tab = O.block_table(p, deltas if weighted else None, order, unit_weights=not weighted)
    return [dataclasses.replace(blk, Sp=blk.S) for blk in tab]


def blocks_of(m, order="cpp", weighted=True, deltas=None):
    return blocks(len(m), deltas_of(m) if deltas is None else deltas, order, weighted)


def build_D(m, blks):
    return sp.vstack([O.build_block(m, b) for b in blks]).tocsr()


@functools.lru_cache(maxsize=None)
def _D(m, order, weighted):
    return build_D(list(m), blocks_of(m, order, weighted))


def D_of(m, order="cpp", weighted=True):
    """the nominal D of mesh m with deltas_of(m), built once a process"""
    return _D(tuple(m), order, weighted)


def mask(S):
    return sum(1 << j for j in S)


def info(m, blks):
    """(E, [(code, set mask, weight)]) as mvtv_problem_edges / mvtv_problem_block_info report them"""
    return O.num_edges(m, blks), [(b.b, mask(b.Sp), b.w) for b in blks]


def kron_dtd(m, blks):
    """sum_S w_S^2 (x)_{j in S} L_j, L_j the 1-D Neumann Laplacian of m_j points (dim 0 fastest: the last factor)"""
    def lap(n):
        d = sp.diags([-np.ones(n - 1), np.ones(n - 1)], [0, 1], shape=(n - 1, n))
        return (d.T @ d).tocsr()
    out = sp.csr_matrix((int(np.prod(m)),) * 2)
    for b in blks:
        term = sp.identity(1, format="csr")
        for j, mj in enumerate(m):
            term = sp.kron(lap(int(mj)) if j in b.Sp else sp.identity(int(mj), format="csr"), term, format="csr")
        out = out + (b.w * b.w) * term
    return out


def dtd_symbol(m, blks, dtype=LD):
    """the eigenvalues of D^T D on the (k_0, ..., k_{p-1}) grid (Fortran order) in ``dtype``; the float64 weights
    define the operator, squares and sums are taken in dtype (as oracle.spectral_ld.dtd_symbol_ld does)"""
    p = len(m)
    pi = dtype(4.0) * np.arctan(dtype(1.0))
    lam = [dtype(4.0) * np.sin(pi * np.arange(mj, dtype=dtype) / dtype(2 * int(mj))) ** 2 for mj in m]
    out = np.zeros([int(v) for v in m], dtype=dtype, order="F")
    for b in blks:
        term = np.full([1] * p, dtype(b.w) * dtype(b.w), dtype=dtype)
        for j in b.Sp:
            shape = [1] * p
            shape[j] = int(m[j])
            term = term * lam[j].reshape(shape)
        out += term
    return out


# ------------------------------------------------------------------------------------------ ADMM parity cases
MARGIN = 1e-6
ADMM_MESHES = [(6, 5, 4), (70, 9, 5), (8, 8, 8), (5, 4, 3, 2)]
LAM = 0.5
# the data seed of small_batch_cases.problem: with it no adapt or stopping comparison of any case's SuperLU run comes
# within MARGIN of its threshold (the smallest margin is 1e-4; tests/test_nominal_host.py asserts it on the CPU)
SEED = 0


def tol_of(m):
    """small_batch_cases.conv_tol: 1e-2 from 600 nodes on (70 x 9 x 5: a second of SuperLU instead of six), else the
    default 1e-4"""
    return S.conv_tol(m)


def admm_cases():
    """(mesh, row order, weighted, W kind): W = I ("I") and W = the counts of scattered points ("S")"""
    return [(m, o, w, wk) for m in ADMM_MESHES for o, w in LAYOUTS for wk in ("I", "S")]


def case_id(c):
    m, o, w, wk = c
    return "x".join(map(str, m)) + f"-{o}{'w' if w else 'u'}-{wk}"


def data(m, wk):
    """(O^T y, W or None, mean y)"""
    return S.problem(list(m), wk, SEED)


@functools.lru_cache(maxsize=None)
def slu(c):
    """the case's converged variant-B run against SuperLU on the nominal D, with its smallest decision margin"""
    m, o, w, wk = c
    oty, W, ym = data(m, wk)
    D = D_of(m, o, w)
    N = D.shape[1]
    res = O.admm_rcpp(D, oty, np.ones(N) if W is None else W, LAM, np.full(N, ym), np.zeros(D.shape[0]), LAM / 5.0,
                      tol=tol_of(m), record=True)
    return res, S.margins(res.history)


def variant_margins(history, variant, tol=1e-3):
    """smallest relative distance of a decision of a recorded variant A / C run from its threshold: max|theta -
    theta_old| against tol, and for A r against 20 s and s against 20 r"""
    best = math.inf
    for h in history:
        pairs = [(h["dtheta_max"], tol)]
        if variant == "A":
            pairs += [(h["r_norm"], 20 * h["s_norm"]), (h["s_norm"], 20 * h["r_norm"])]
        for a, b in pairs:
            best = min(best, abs(a - b) / max(abs(a), abs(b), 1e-300))
    return best


PATH_LAMS = [2.0, 1.0, 0.5]


@functools.lru_cache(maxsize=None)
def path_ref(m, order="cpp", weighted=True, wk="S"):
    """mbs_path_rcpp (theta, u, rho carried along PATH_LAMS from mean y, 0, lambda_0 / 5) on the nominal D, each run
    recorded: ([AdmmResult], smallest decision margin)"""
    oty, W, ym = data(m, wk)
    D = D_of(m, order, weighted)
    N = D.shape[1]
    theta, u, rho = np.full(N, ym), np.zeros(D.shape[0]), PATH_LAMS[0] / 5.0
    out, margin = [], math.inf
    for lam in PATH_LAMS:
        res = O.admm_rcpp(D, oty, np.ones(N) if W is None else W, lam, theta, u, rho, record=True)
        out.append(res)
        margin = min(margin, S.margins(res.history))
        theta, u, rho = res.theta, res.u, res.rho
    return out, margin


# one case each of variants A and C: (variant, mesh, row order, weighted, lambda, tol), W = I
VARIANT_CASES = [("A", (6, 5, 4), "cpp", True, 2.0, 1e-3), ("C", (5, 4, 3, 2), "py", True, 2.0, 1e-2)]


@functools.lru_cache(maxsize=None)
def variant_run(v):
    """the case's converged run of admm_cpp / admm_py (SuperLU) on the nominal D, with its smallest decision margin"""
    var, m, o, w, lam, tol = v
    oty, _, ym = data(m, "I")
    D = D_of(m, o, w)
    N = D.shape[1]
    fn = O.admm_cpp if var == "A" else O.admm_py
    res = fn(D, oty, np.ones(N), lam, np.full(N, ym), ym, tol=tol, record=True)
    return res, variant_margins(res.history, var, tol)


# ------------------------------------------------------------------------------------------ lambda_max
class LamMaxCase(L.Case):
    """lammax_ref.Case (O^T y a sum of K eigenvectors of D^T D, lambda_max a closed form) on the nominal blocks: the
    cosine products are eigenvectors under either rule, the eigenvalues come from the blocks' own sets"""

    def __init__(self, m, order="cpp", weighted=True, deltas=None):
        self.m = [int(v) for v in m]
        self.p = len(self.m)
        self.order, self.weighted = order, weighted
        self.deltas = list(L.DELTAS[:self.p]) if deltas is None else [float(v) for v in deltas]
        self.blocks = blocks(self.p, self.deltas, order, weighted)
        self.ks = L.modes(self.m)
        self.lam = L.eigenvalues(self.m, self.blocks, self.ks)
        norms = [math.sqrt(np.prod([mj / 2.0 if kj else float(mj) for mj, kj in zip(self.m, k)])) for k in self.ks]
        for amps in L.AMPS_MENU:
            self.amps = amps
            self.model_rcpp, hc = L.model_residuals(self.lam, [a * n for a, n in zip(amps, norms)])
            if len(self.model_rcpp) == L.K and self.model_rcpp[L.K - 2] >= 1.15e-2:
                break
        else:
            raise AssertionError(f"no amplitude set keeps the residual at K - 1 up on {self.m} {order}")
        self.scale = 2.0 ** (4 - math.floor(math.log2(hc[L.K - 2])))
        self.model_cpp = [self.scale * v for v in hc]
        self.coef = [self.scale * a for a in self.amps]
