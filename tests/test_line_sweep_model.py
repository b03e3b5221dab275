"""Numpy transcription of the marching line sweeps of the 3-D spectral solve (mvtv_spectral.hip k_sweep).

The sweeps replace the dim-1 forward transform, the dim-2 line solve and the dim-1 inverse transform by a down sweep,
the chunk interface (k_trisr_iface) and an up sweep. This file transcribes, in float64 and in the kernels' order of
operations: the chunk bounds, the line constants, the down sweep's recursions (B, Fs and the running power p), the
interface's carries with its (r^k, 1 - r^k) pairs and mirror closure, and the up sweep's recovery f_i = B_i - r B_{i+1},
the binary powering of r^(hi-i) and the F recursion. The transforms along dims 0 and 1 are scipy's (the kernels' own
transforms are k_dct8's, covered by tests/test_gpu_dispatch.py). Checked against the long-double reference
oracle/spectral_ld.py with the bound of tests/test_gpu_dispatch.py: min(1e-12, 32 e64), e64 the error of the float64
evaluation of the reference's own formula.

A second test walks the thread -> coefficient ownership of a k_sweep tile: every (k0, k1) of the 16 x 512 tile belongs
to exactly one register of one thread, and the Makhoul load / store positions of the first and last FFT stages cover
every point of dim 1 once.
"""
import numpy as np
import pytest
import scipy.fft as sfft

from oracle import spectral_ld as S
from oracle.mvtv_oracle import block_table

SIGMAS = (0.0, 1e-3, 3.7, 2e5)
# (mesh, chunks): degenerate lines, uneven chunks, every plane a chunk, two and three tiles' worth of lines
CASES = [([16, 16, 2], 1), ([16, 16, 2], 2), ([16, 16, 7], 3), ([16, 16, 40], 40), ([32, 32, 33], 1), ([32, 32, 33], 4),
         ([32, 32, 33], 16), ([48, 48, 5], 2), ([16, 16, 512], 8)]


def chunk_bounds(m2, C):
    return [(m2 * k // C, m2 * (k + 1) // C) for k in range(C)]


def line_constants(m, deltas, sigma, w0=1.0):
    """c0, c1 per (k0, k1) as the kernels build them: c0 = w0 + sigma sum_{S without dim 2}, c1 = sigma sum_{S with dim 2}."""
    cS = np.zeros(8)
    for blk in block_table(3, deltas, "cpp"):
        mask = sum(1 << j for j in blk.Sp)
        cS[mask] += blk.w * blk.w
    lam = [4.0 * np.sin(np.pi * np.arange(mj) / (2.0 * mj)) ** 2 for mj in m]
    l0, l1 = lam[0][:, None], lam[1][None, :]
    c0 = np.full((m[0], m[1]), w0)
    c1 = np.zeros((m[0], m[1]))
    for Sm in range(1, 8):
        if cS[Sm] == 0.0:
            continue
        prod = sigma * cS[Sm] * np.ones((m[0], m[1]))
        if Sm & 1:
            prod = prod * l0
        if Sm & 2:
            prod = prod * l1
        if Sm & 4:
            c1 = c1 + prod
        else:
            c0 = c0 + prod
    return c0, c1


def powt_mul(a, b):
    return a[0] * b[0], a[0] * b[1] + a[1]


def powt_pow(x, n):
    y = (np.ones_like(x[0]), np.zeros_like(x[0]))
    while n:
        if n & 1:
            y = powt_mul(y, x)
        x = powt_mul(x, x)
        n >>= 1
    return y


def pow_times(r, n, y):
    """y r^n by the up sweep's binary powering (no division by r)."""
    rp = r.copy()
    y = y.copy()
    while n:
        if n & 1:
            y = y * rp
        rp = rp * rp
        n >>= 1
    return y


def sweeps(f, c0, c1, C, scale=1.0):
    """f[k0, k1, i] (dims 0 and 1 transformed) -> x, by down sweep, interface, up sweep over C chunks of dim 2."""
    m2 = f.shape[2]
    D = np.sqrt(c0 * (c0 + 4.0 * c1))
    den = 1.0 / (c0 + 2.0 * c1 + D)
    r = 2.0 * c1 * den
    r1 = (r, (c0 + D) * den)
    sd = scale / D
    bounds = chunk_bounds(m2, C)
    Bst = np.empty_like(f)
    coef = np.empty((C, 2) + f.shape[:2])
    for k, (lo, hi) in enumerate(bounds):                      # down
        B = np.zeros_like(r)
        Fs = np.zeros_like(r)
        p = np.ones_like(r)
        for i in range(hi - 1, lo - 1, -1):
            B = f[:, :, i] + r * B
            Fs = Fs + p * f[:, :, i]
            p = p * r
            Bst[:, :, i] = B
        coef[k, 0], coef[k, 1] = Fs, B
    lr = np.empty_like(coef)                                   # interface (k_trisr_iface, G = C, rank 0)
    nlo = m2 // C
    plo = powt_pow(r1, nlo)
    rlo, rhi = plo[0], plo[0] * r1[0]
    rblk = [rlo if hi - lo == nlo else rhi for lo, hi in bounds]
    acc = np.zeros_like(r)
    for k in range(C):
        lr[k, 0] = acc
        acc = acc * rblk[k] + coef[k, 0]
    bcc = np.zeros_like(r)
    for k in range(C - 1, -1, -1):
        lr[k, 1] = bcc
        bcc = bcc * rblk[k] + coef[k, 1]
    pm = powt_pow(r1, m2)
    idet = 1.0 / powt_mul(pm, pm)[1]
    fm1, bm = (bcc + pm[0] * acc) * idet, (acc + pm[0] * bcc) * idet
    pf = np.ones_like(r)
    pb = np.ones_like(r)
    for k in range(C):
        kb = C - 1 - k
        lr[k, 0] = pf * fm1 + lr[k, 0]
        lr[kb, 1] = pb * bm + lr[kb, 1]
        pf = pf * rblk[k]
        pb = pb * rblk[kb]
    x = np.empty_like(f)
    for k, (lo, hi) in enumerate(bounds):                      # up
        F, Bin = lr[k, 0].copy(), lr[k, 1]
        for i in range(lo, hi):
            cur = Bst[:, :, i]
            nxt = Bst[:, :, i + 1] if i + 1 < hi else np.zeros_like(r)
            fi = cur - r * nxt
            x[:, :, i] = sd * (cur + pow_times(r, hi - i, Bin) + r * F)
            F = r * F + fi
    return x


@pytest.mark.parametrize("m,C", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_sweeps_against_long_double(m, C):
    N = int(np.prod(m))
    b = np.random.default_rng(3000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    ref = {name: (S.forward_ld(m, b, dt), S.dtd_symbol_ld(m, deltas, 0, True, dt))
           for name, dt in (("ld", np.longdouble), ("f64", np.float64))}
    bb = b.reshape(m, order="F")
    f = sfft.dctn(bb, type=2, norm="ortho", axes=(0, 1))
    for sigma in SIGMAS:
        c0, c1 = line_constants(m, deltas, sigma)
        x = sfft.idctn(sweeps(f, c0, c1, C), type=2, norm="ortho", axes=(0, 1)).ravel(order="F")
        x_ld = S.solve_from_forward(*ref["ld"], sigma)
        x64 = S.solve_from_forward(*ref["f64"], sigma)
        scale = float(np.max(np.abs(x_ld)))
        e64 = float(np.max(np.abs(x64 - x_ld))) / scale
        err = float(np.max(np.abs(x - x_ld))) / scale
        print(f"sweep model {m} C={C} sigma {sigma:g}: e64 {e64:.2e} model {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
        assert err <= min(1e-12, 32.0 * e64), (sigma, err, e64)


def test_chunk_bounds_cover_the_planes():
    for m2 in (2, 7, 33, 40, 512):
        for C in range(1, min(m2, 64) + 1):
            b = chunk_bounds(m2, C)
            assert b[0][0] == 0 and b[-1][1] == m2
            assert all(b[k][1] == b[k + 1][0] for k in range(C - 1))
            lens = {hi - lo for lo, hi in b}
            assert min(lens) >= 1 and lens <= {m2 // C, m2 // C + 1}


def test_tile_ownership():
    """k_sweep<9>: thread t = j * 8 + c (j < 64, c < 8) owns lines k0 = 2c, 2c + 1 of its tile and the dim-1
    coefficients ka = j + 64 s, kb = M - ka (M / 2 for ka = 0), s < 4; the radix-8 first stage reads Makhoul positions
    n = j + 64 q and the last stage leaves the same positions, sample k = 2n (n < M / 2) or 2 (M - 1 - n) + 1."""
    M, TPL, NCL = 512, 64, 8
    owned = np.zeros((16, M), dtype=int)
    loads = np.zeros((16, M), dtype=int)
    stores = np.zeros((16, M), dtype=int)
    for t in range(NCL * TPL):
        j, c = t // NCL, t % NCL
        for s in range(4):
            ka = j + s * TPL
            kb = M - ka if ka else M // 2
            for k1 in (ka, kb):
                owned[2 * c:2 * c + 2, k1] += 1
        for q in range(8):
            for n, cnt in ((j + TPL * q, loads), ((j // (M // 8)) * M + j % (M // 8) + q * (M // 8), stores)):
                k = 2 * n if n < M // 2 else 2 * (M - 1 - n) + 1
                cnt[2 * c:2 * c + 2, k] += 1
    assert (owned == 1).all() and (loads == 1).all() and (stores == 1).all()
