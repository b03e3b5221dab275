"""Textbook preconditioned conjugate gradients, the reference of the PCG tests (tests/test_gpu_parity.py,
tests/test_gpu_pcg_scalars.py, tests/test_pcg_ref_host.py), and the two preconditioners the library's PCGs use.

The library's three PCGs (the three-kernel one and the fused Chronopoulos-Gear k_cg3d of pcg_solve, and pcgs_solve
with the cosine-transform preconditioner, both functions of mvtv_capi.cpp) are this method up to rounding, so their
k-th iterate must equal x_k here to rounding. That is the one check that sees a wrong alpha or beta: x += alpha p and
r -= alpha q stay consistent for any alpha, so a converged solve hides a lost partial sum."""
import numpy as np


def pcg_iterates(A, Minv, b, x0, k, pq=None):
    """k iterations of PCG on A x = b from x0: ([x_1 .. x_k], [relres_1 .. relres_k]) with relres_i =
    sqrt(|r_i|^2 / |b|^2) of the recursive residual r_i = r_{i-1} - alpha q, the quantity k_finalize tests
    (mvtv_kernels.hip: bnorm2 = sum b^2 at :500 / :518, rnorm2 = sum r^2 at :514 / :535, done when rnorm2 <=
    rtol^2 bnorm2 at :516 / :537; pcg_solve and pcgs_solve of mvtv_capi.cpp return sqrt(rnorm2 / bnorm2) as relres).

    A and Minv are callables; the arithmetic runs in b's dtype (float64 or long double). ``pq(p, q)`` replaces the
    inner product p.q (tests/test_pcg_ref_host.py drops one workgroup's share with it)."""
    b = np.asarray(b)
    x = np.array(x0, dtype=b.dtype)
    r = b - A(x)
    z = Minv(r)
    p = z.copy()
    rz = r @ z
    b2 = b @ b
    xs, rel = [], []
    for _ in range(k):
        q = A(p)
        al = rz / (p @ q if pq is None else pq(p, q))
        x = x + al * p
        r = r - al * q
        z = Minv(r)
        rz, rz0 = r @ z, rz
        p = z + (rz / rz0) * p
        xs.append(x.copy())
        rel.append(float(np.sqrt((r @ r) / b2)))
    return xs, rel


def dtd_diagonal(m, blocks, dtype=np.float64):
    """diag(D^T D) = sum_S cS[S] prod_{j in S} l_j with l_j = 1 at the two ends of dim j and 2 inside
    (jacobi_diag, mvtv_kernels.hip:36-53), flat with dim 0 fastest."""
    p = len(m)
    out = np.zeros([int(v) for v in m], dtype=dtype, order="F")
    for blk in blocks:
        term = np.full([1] * p, dtype(blk.w) * dtype(blk.w), dtype=dtype)
        for j in blk.Sp:
            lj = np.full(int(m[j]), 2.0, dtype=dtype)
            lj[0] -= 1.0
            lj[-1] -= 1.0
            shape = [1] * p
            shape[j] = int(m[j])
            term = term * lj.reshape(shape)
        out = out + term
    return out.ravel(order="F")


def dtd_diagonal_mean(m, blocks):
    """mean over the mesh of diag(D^T D): sum_S cS[S] prod_{j in S} 2 (m_j - 1) / m_j (cmean in pcgs_solve,
    mvtv_capi.cpp)."""
    acc = 0.0
    for blk in blocks:
        prod = blk.w * blk.w
        for j in blk.Sp:
            prod *= 2.0 * (int(m[j]) - 1) / int(m[j])
        acc += prod
    return acc


def spectral_preconditioner(m, blocks, W, sigma, solve, dtype=np.float64):
    """M^-1 = S A0^-1 S of pcgs_solve (mvtv_capi.cpp): A0 = w0 I + sigma D^T D with w0 = mean(W) (its w0),
    inverted exactly by ``solve(s, b)`` = (I + s D^T D)^-1 b as solve(sigma / w0, r) / w0; S = I while
    std(W) < 0.1 dbar, dbar = w0 + sigma mean diag(D^T D) (its dbar and scaled), else S = diag(sqrt(dbar / d)) with d =
    W + sigma diag(D^T D) (k_pcgs_sinv, mvtv_kernels.hip:668-674; applied to r before the solve and to z after it,
    k_pcgs_vec ops 0-2, :632-649). Returns (Minv, scaled)."""
    W = np.asarray(W, dtype=np.float64)
    w0 = float(W.mean())
    dbar = w0 + sigma * dtd_diagonal_mean(m, blocks)
    scaled = bool(W.std() >= 0.1 * dbar)
    s0, iw0 = dtype(sigma / w0), dtype(1.0 / w0)
    if not scaled:
        return (lambda r: solve(s0, r) * iw0), False
    d = W.astype(dtype) + dtype(sigma) * dtd_diagonal(m, blocks, dtype)
    S = np.sqrt(dtype(dbar) / d)
    return (lambda r: S * (solve(s0, S * r) * iw0)), True


def fold_weights(n, seed):
    """one CV fold of five held out: W = 1, zero on a fifth of the nodes"""
    return (np.random.default_rng(seed).permutation(n) % 5 != 0).astype(np.float64)


def count_weights(n, seed):
    """counts of 3 n / 5 scattered observations per node: zeros on about half the nodes"""
    return np.bincount(np.random.default_rng(seed).integers(0, n, 3 * n // 5), minlength=n).astype(np.float64)


def theta0(m, seed):
    """a smooth field plus noise (not constant: D theta0 != 0)"""
    grids = np.meshgrid(*[np.linspace(0.0, 1.0, int(v)) for v in m], indexing="ij")
    s = sum(np.sin(2.0 * (j + 1) * g) for j, g in enumerate(grids)).ravel(order="F")
    return s + 0.3 * np.random.default_rng(seed).standard_normal(s.size)


def jacobi_case(m, weighted, sigma, seed=5):
    """(W, b, x0, A, Minv) of a Jacobi-PCG case through Problem.solve: float64 numpy over the sparse oracle's D
    (deltas [0.5, 0.25, 0.125, 0.3][:p], cpp order), W = uniform(0.5, 2) or the identity, random b and x0."""
    from oracle import mvtv_oracle as O
    p, n = len(m), int(np.prod(m))
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 2.0, n) if weighted else np.ones(n)
    D = O.build_D(m, O.block_table(p, [0.5, 0.25, 0.125, 0.3][:p], "cpp"))
    DtD = (D.T @ D).tocsr()
    dinv = 1.0 / (W + sigma * np.asarray(DtD.diagonal()).ravel())
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    return W, b, x0, (lambda v: W * v + sigma * (DtD @ v)), (lambda r: dinv * r)


def spectral_case(m, kind, rho, seed=0):
    """One theta-solve of the variant-B ADMM start (rcpp-code/MultivarTV/src/solvers.cpp:101-113, as
    oracle.mvtv_oracle.admm_rcpp / c_oracle.admm_rcpp restate it): alpha_0 = D theta_0, u_0 = 0, so
    (W + rho D^T D) theta = O^T y + rho D^T (alpha_0 + u_0), warm-started at theta_0. Weights: ``fold`` (one CV fold
    of five held out), ``counts`` (scattered observations) or ``identity``; D and D^T from the matrix-free C oracle,
    A0's inverse from variants_spectral.dct_solver. Returns dict(W, oty, th0, b, A, Minv, scaled)."""
    from oracle import mvtv_oracle as O
    from oracle import variants_spectral as VS
    p, n = len(m), int(np.prod(m))
    deltas = [0.5, 0.25, 0.125, 0.3][:p]
    blocks = O.block_table(p, deltas, "cpp")
    O.check_dims(m, blocks)
    W = {"fold": lambda: fold_weights(n, 70 + seed), "counts": lambda: count_weights(n, 80 + seed),
         "identity": lambda: np.ones(n)}[kind]()
    oty = W * np.random.default_rng(90 + seed).standard_normal(n)
    th0 = theta0(m, 100 + seed)
    Dop, Dt = VS.operators(m, deltas, "cpp", True)
    b = oty + rho * Dt(Dop(th0))
    Minv, scaled = spectral_preconditioner(m, blocks, W, rho, VS.dct_solver(m, deltas, "cpp", True))
    return dict(W=W, oty=oty, th0=th0, b=b, A=lambda v: W * v + rho * Dt(Dop(v)), Minv=Minv, scaled=scaled)


def first_below(relres, thr=1e-6, ratio=4.0):
    """(k, rtol) for a stop test that rounding cannot move: k is the first iteration with relres_k < thr, and it must
    sit a factor `ratio` below relres_{k-1}; rtol is their geometric mean. None where the sequence gives no such k."""
    for i, v in enumerate(relres):
        if v < thr:
            if i == 0 or relres[i - 1] / v < ratio:
                return None
            rtol = float(np.sqrt(relres[i - 1] * v))
            if min(relres[:i]) < rtol * np.sqrt(ratio):   # PCG residuals are not monotone: no earlier stop either
                return None
            return i + 1, rtol
    return None
