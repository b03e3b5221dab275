"""Matrix-free twins of the variant A / C reference loops — CPU ORACLE, TEST INFRASTRUCTURE ONLY.

``mvtv_oracle.admm_cpp`` / ``admm_py`` restate the reference's loops (cpp-code/solvers.cpp:90-130,
code/solvers.py:53-76) over a sparse D and a SuperLU factor, which limits them to meshes of a few thousand nodes.
The loops here keep the same statements in the same order and swap the operators: D and D^T come from the C oracle
(``c_oracle.apply_D`` / ``apply_Dt``, matrix-free), and (I + sigma D^T D) theta = b is solved exactly in the cosine
basis (``scipy.fft.dctn`` / ``idctn`` over ``c_oracle.dtd_symbol``) as ``c_oracle.admm_rcpp_spectral`` does for
variant B. A caller with W != I passes its own ``solve(sigma, b)`` (a SuperLU factor, say).

Every iteration is recorded with the margins of the decisions it took, so that a test can require its cases to sit
away from every threshold before it compares a GPU run's iteration count with the oracle's.

Pinned against the SuperLU loops and the reference's own outputs in tests/test_oracle_variants.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import c_oracle
from .mvtv_oracle import AdmmResult, MaxIterError, softthresh


@dataclass
class VariantResult(AdmmResult):
    # |dtheta / tol - 1| of every loop-condition test, the one that ended the run included (entry 0: the test on
    # theta_0 against the initial theta_old); empty under fixed_iters, where no such test is made
    stop_margins: list = field(default_factory=list)


def _code(order, weighted):
    if order not in ("cpp", "py"):
        raise ValueError(order)
    return (0 if order == "cpp" else 1), (1 if weighted else 0)


def operators(m, deltas, order="cpp", weighted=True):
    """(D, Dt) as callables on flat arrays, in the block order / weights of ``block_table(p, deltas, order,
    unit_weights=not weighted)``."""
    o, w = _code(order, weighted)
    dl = [1.0] * len(m) if deltas is None else [float(v) for v in deltas]
    return (lambda x: c_oracle.apply_D(m, x, dl, o, w)), (lambda v: c_oracle.apply_Dt(m, v, dl, o, w))


def dct_solver(m, deltas, order="cpp", weighted=True, workers=-1):
    """solve(sigma, b) of (I + sigma D^T D) x = b by the orthonormal DCT-II over the symbol of D^T D."""
    import scipy.fft as sfft
    o, w = _code(order, weighted)
    shape = [int(v) for v in m]
    sym = c_oracle.dtd_symbol(m, [1.0] * len(m) if deltas is None else deltas, o, w)

    def solve(sigma, b):
        t = sfft.dctn(np.asarray(b, dtype=np.float64).reshape(shape, order="F"), type=2, norm="ortho",
                      workers=workers)
        t /= 1.0 + sigma * sym
        return sfft.idctn(t, type=2, norm="ortho", workers=workers).ravel(order="F")

    return solve


def _margin(value, threshold):
    """Relative distance of a compared quantity from its threshold (inf when either side is not finite)."""
    if not (math.isfinite(value) and math.isfinite(threshold)) or threshold == 0.0:
        return math.inf if value != threshold else 0.0
    return abs(value / threshold - 1.0)


def admm_cpp_spectral(m, oty, lam, theta0, ymean, deltas, order="cpp", weighted=True, sigma=None, tol=1e-3,
                      max_counter=2000, fixed_iters=None, u0=None, solve=None, workers=-1) -> VariantResult:
    """Variant A (``mvtv_oracle.admm_cpp``): sigma = lambda fixed, rho an int truncated after every adaptation, an
    infinite threshold at rho = 0, s from the new alpha and the old u, stop when max|theta - theta_old| <= tol.

    history[k]: dtheta_max, r_norm, s_norm, rho (the one iteration k ran with), rho_next, and the adaptation margins
    adapt_hi = |(r/s) / 20 - 1|, adapt_lo = |(r/s) / (1/20) - 1| (inf where s = 0 < r)."""
    D, Dt = operators(m, deltas, order, weighted)
    if solve is None:
        solve = dct_solver(m, deltas, order, weighted, workers)
    sig = float(lam if sigma is None else sigma)
    oty = np.asarray(oty, dtype=np.float64).ravel()
    theta = np.array(theta0, dtype=np.float64).ravel()
    alpha = D(theta)
    E = alpha.size
    u = np.full(E, 1.0 / lam) if u0 is None else np.array(u0, dtype=np.float64).ravel()
    thetaold = np.full_like(theta, ymean - 0.1)
    counter = 1
    rho = int(lam)
    res = VariantResult(theta, u, float(rho), 0)
    it = 0
    while True:
        if fixed_iters is not None:
            if it >= fixed_iters:
                break
        else:
            dth = float(np.max(np.abs(theta - thetaold)))
            res.stop_margins.append(_margin(dth, tol))
            if not dth > tol:
                break
        thetaold = theta
        b = oty + rho * Dt(alpha + u)
        theta = solve(sig, b)
        Dtheta = D(theta)
        thr = lam / rho if rho != 0 else math.inf
        alpha = softthresh(Dtheta - u, thr)
        s = rho * Dt(alpha + u)
        r = alpha - Dtheta
        u = u + r
        counter += 1
        it += 1
        r_norm = float(np.sqrt(r @ r))
        s_norm = float(np.sqrt(s @ s))
        if fixed_iters is None and counter > max_counter:
            raise MaxIterError("Failed to converge!")
        ratio = r_norm / s_norm if s_norm > 0.0 else (math.inf if r_norm > 0.0 else math.nan)
        if r_norm > 20 * s_norm:
            rho_next, u = 20.0 * rho, 0.05 * u
        elif s_norm > 20 * r_norm:
            rho_next, u = 0.1 * rho, 10.0 * u
        else:
            rho_next = float(rho)
        res.history.append(dict(dtheta_max=float(np.max(np.abs(theta - thetaold))), r_norm=r_norm, s_norm=s_norm,
                                rho=float(rho), rho_next=float(int(rho_next)), adapt_hi=_margin(ratio, 20.0),
                                adapt_lo=_margin(ratio, 1.0 / 20.0)))
        rho = int(rho_next)
    res.theta, res.u, res.rho, res.iters = theta, u, float(rho), it
    return res


def admm_py_spectral(m, oty, tune, theta0, ymean, deltas, order="py", weighted=True, sigma=None, tol=1e-3,
                     fixed_iters=None, u0=None, solve=None, max_iters=100000, workers=-1) -> VariantResult:
    """Variant C (``mvtv_oracle.admm_py``): rho = lambda = tune, threshold lambda / rho, no adaptation, stop when
    max|theta - theta_old| <= tol (theta_old starts at mean(y) - 1).

    history[k]: dtheta_max, r_norm, rho."""
    D, Dt = operators(m, deltas, order, weighted)
    if solve is None:
        solve = dct_solver(m, deltas, order, weighted, workers)
    sig = float(tune if sigma is None else sigma)
    lam = rho = float(tune)
    oty = np.asarray(oty, dtype=np.float64).ravel()
    theta = np.array(theta0, dtype=np.float64).ravel()
    alpha = D(theta)
    E = alpha.size
    u = np.full(E, 1.0 / lam) if u0 is None else np.array(u0, dtype=np.float64).ravel()
    thetaold = np.full_like(theta, ymean - 1.0)
    res = VariantResult(theta, u, rho, 0)
    it = 0
    while True:
        if fixed_iters is not None:
            if it >= fixed_iters:
                break
        else:
            dth = float(np.max(np.abs(theta - thetaold)))
            res.stop_margins.append(_margin(dth, tol))
            if not dth > tol or it >= max_iters:
                break
        thetaold = theta
        b = oty + rho * Dt(alpha + u)
        theta = solve(sig, b)
        Dtheta = D(theta)
        alpha = softthresh(Dtheta - u, lam / rho)
        r = alpha - Dtheta
        u = u + r
        it += 1
        res.history.append(dict(dtheta_max=float(np.max(np.abs(theta - thetaold))), r_norm=float(np.sqrt(r @ r)),
                                rho=rho))
    res.theta, res.u, res.rho, res.iters = theta, u, rho, it
    return res
