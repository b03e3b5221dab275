"""Numpy transcription of the up sweep's two-level exponent (mvtv_spectral.hip k_sweep<L, true>), in the
style of tests/test_line_sweep_model.py, whose chunk bounds, line constants, down sweep and interface this file reuses
through that model's own functions.

The up sweep needs r^(hi-i) Bin at plane i. With hi - i = 8 a + b, b < 8, the kernel keeps Q = r^(8 a) Bin in Bin's
registers and forms r^b Q per plane (at most two squarings and three products); Q is rebuilt from Bin, (r^8)^a by
binary powering, at the chunk's start and whenever a drops. No division by r: sigma = 0 gives r = 0, and sigma = 1e-40
makes r^8 underflow inside the ladder, where the factor belongs to a term below the result's rounding.

Checked against the long-double reference oracle/spectral_ld.py with its bound min(1e-12, 32 e64), e64 the error of
the float64 evaluation of the reference's own formula, on the CASES of tests/test_line_sweep_model.py and on chunks of
7 and 15 (a chunk that starts at b = 7), 8, 9, 16, 17 and 65 planes (the exponent's boundaries 8 | 9 and 16 | 17, and
a >= 8).
"""
import numpy as np
import pytest
import scipy.fft as sfft

from oracle import spectral_ld as S
from test_line_sweep_model import CASES, chunk_bounds, line_constants, pow_times, powt_mul, powt_pow

SIGMAS = (0.0, 1e-40, 1e-3, 3.7, 2e5)
# chunks that start at b = 7 (7 and 15 planes); chunk lengths 8, 9, 16, 17 and 65 as one chunk, and as the two lengths
# of a split (8 | 9, 16 | 17, 65 | 65)
CHUNK_CASES = [([16, 16, 7], 1), ([16, 16, 15], 1), ([16, 16, 8], 1), ([16, 16, 9], 1), ([16, 16, 16], 1),
               ([16, 16, 17], 1), ([16, 16, 65], 1), ([16, 16, 17], 2), ([16, 16, 33], 2), ([16, 16, 130], 2)]


def requant(r, a, Bin):
    """Q = (r^8)^a Bin: r^8 by three squarings, its power by the binary ladder."""
    r8 = r * r
    r8 = r8 * r8
    r8 = r8 * r8
    return pow_times(r8, a, Bin)


def low_power(r, b, Q):
    """r^b Q, b < 8, in the kernel's order: <= 2 squarings and <= 3 products."""
    y = Q.copy()
    rp = r.copy()
    if b & 1:
        y = y * rp
    if b > 1:
        rp = rp * rp
        if b & 2:
            y = y * rp
        if b > 3:
            rp = rp * rp
            y = y * rp
    return y


def sweeps_two_level(f, c0, c1, C, scale=1.0):
    """tests/test_line_sweep_model.py::sweeps with the up sweep's r^(hi-i) Bin by the two-level exponent."""
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
    lr = np.empty_like(coef)                                   # interface
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
        Q = requant(r, (hi - lo) >> 3, Bin)
        for i in range(lo, hi):
            n = hi - i
            b = n & 7
            if b == 7 and i > lo:                              # Bin reloaded a step ahead, at b = 0
                Q = requant(r, n >> 3, Bin)
            cur = Bst[:, :, i]
            nxt = Bst[:, :, i + 1] if i + 1 < hi else np.zeros_like(r)
            fi = cur - r * nxt
            x[:, :, i] = sd * (cur + low_power(r, b, Q) + r * F)
            F = r * F + fi
    return x


def test_two_level_exponent_is_the_power():
    """r^b (r^8)^a Bin against r^n Bin in long double for every n <= 70: a few roundings, and exact zeros at r = 0."""
    rng = np.random.default_rng(11)
    r = np.concatenate([[0.0, 1e-40, 1e-5, 0.5, 1.0 - 1e-9], rng.uniform(0.0, 1.0, 59)])
    Bin = rng.standard_normal(r.size)
    for n in range(1, 71):
        got = low_power(r, n & 7, requant(r, n >> 3, Bin))
        want = (r.astype(np.longdouble) ** n * Bin.astype(np.longdouble))
        # a product's rounding u = eps / 2 enters r^n Bin once per factor it feeds (a squaring doubles the count of
        # its operand and adds one): at most n + 1 of them, so (n + 1) u < n eps; below the normal range, absolutely
        assert np.all(np.abs(got - want) <= n * np.finfo(float).eps * np.abs(want) + np.finfo(float).tiny), n
        assert got[0] == 0.0


@pytest.mark.parametrize("m,C", CASES + CHUNK_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_two_level_sweeps_against_long_double(m, C):
    N = int(np.prod(m))
    b = np.random.default_rng(3000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    ref = {name: (S.forward_ld(m, b, dt), S.dtd_symbol_ld(m, deltas, 0, True, dt))
           for name, dt in (("ld", np.longdouble), ("f64", np.float64))}
    bb = b.reshape(m, order="F")
    f = sfft.dctn(bb, type=2, norm="ortho", axes=(0, 1))
    for sigma in SIGMAS:
        c0, c1 = line_constants(m, deltas, sigma)
        x = sfft.idctn(sweeps_two_level(f, c0, c1, C), type=2, norm="ortho", axes=(0, 1)).ravel(order="F")
        x_ld = S.solve_from_forward(*ref["ld"], sigma)
        x64 = S.solve_from_forward(*ref["f64"], sigma)
        scale = float(np.max(np.abs(x_ld)))
        e64 = float(np.max(np.abs(x64 - x_ld))) / scale
        err = float(np.max(np.abs(x - x_ld))) / scale
        print(f"two-level model {m} C={C} sigma {sigma:g}: e64 {e64:.2e} model {err:.2e} "
              f"ratio {err / max(e64, 1e-300):.1f}")
        assert err <= min(1e-12, 32.0 * e64), (sigma, err, e64)
