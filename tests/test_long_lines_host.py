"""Host model of the blocked line solve along a last dimension of any length (k_trib / k_tri1 and their interfaces
k_trib_iface / k_blk_iface, mvtv_spectral.hip).

A float64 numpy transcription of the kernels' index logic: the block rule [floor(m k / nblk), floor(m (k + 1) / nblk)),
segments of sl rows with a shorter last one and empty ones after it (a block of the shorter length in a workgroup
sized for the longer), the multipliers r^rows (1 for an empty segment), the workgroup's weighted scan (64-lane
shuffle steps, then the waves' pairs in order), phase 1's pairs from zero carries, the interface over the blocks
(a thread a line, or runs of blocks per thread and the same scan: one line on 16 waves for p = 1, a wave a line
for p >= 2 with few lines) with the mirror closure, and
phase 3's rerun from the carries. Checked against the long-double cosine-transform solve (oracle/spectral_ld.py) on
the 1-D and 2-D shapes of tests/test_gpu_long_lines.py, with that file's forward-error rule. No GPU."""
import numpy as np
import pytest
import scipy.fft as sfft

from oracle import spectral_ld as SLD
from oracle.mvtv_oracle import block_table

SMAX, R1, NT1 = 32, 16, 256   # trib::SMAX, tri1::R, tri1::NT
WAVE_IFACE_BELOW = 8192        # p >= 2: fewer lines than this take the interface a wave a line (k_blk_iface<1>)


def cdiv(a, b):
    return (a + b - 1) // b


def plan(m, blocks=0):
    """line_blocks_plan: (nblk, tq, sl, nseg) for the mesh m (tq = 0: the p = 1 kernel); None where it refuses."""
    p, ml = len(m), int(m[-1])
    nlines = int(np.prod(m[:-1])) if p > 1 else 1
    if blocks < 0 or blocks == 1 or blocks > ml:
        return None
    if p == 1:
        nb = blocks or cdiv(ml, NT1 * R1)
        return None if cdiv(ml, nb) > NT1 * R1 else (nb, 0, R1, NT1)
    narrow, nmax = (16, 32 * SMAX) if nlines >= 16 else (4, 64 * SMAX)
    if blocks:
        nb, nhi = blocks, cdiv(ml, blocks)
        tq = 64 if (nlines >= 64 and nhi <= 8 * SMAX and (nlines // 64) * nb >= 256) else narrow
        if tq != 64 and nhi > nmax:
            return None
    else:
        nb = cdiv(ml, 8 * SMAX)
        if nlines >= 64 and (nlines // 64) * nb >= 256:
            tq = 64
        else:
            tq = narrow
            nb = max(cdiv(ml, nmax), min(cdiv(ml, 128), cdiv(512, cdiv(nlines, tq))))
    nhi = cdiv(ml, nb)
    sl = min(SMAX, nhi)
    return nb, tq, sl, cdiv(nhi, sl)


def consts(c0, c1):
    D = np.sqrt(c0 * (c0 + 4.0 * c1))
    den = 1.0 / (c0 + 2.0 * c1 + D)
    return 2.0 * c1 * den, (c0 + D) * den, D   # r, 1 - r (cancellation-free), D


def tpow(t, n):
    """1 - r^n from t = 1 - r alone (tpow): t_{a+b} = t_a + t_b - t_a t_b, a few eps relative whatever n."""
    y, x = np.zeros_like(t), t.copy()
    while n:
        if n & 1:
            y = (y + x) - y * x
        x = (x + x) - x * x
        n >>= 1
    return y


def mul2(t):
    """The multiplier 1 - t as h + l (mul2_from_t): h rounded, l what the rounding lost where h >= 1/2."""
    h = 1.0 - t
    return h, np.where(h >= 0.5, (1.0 - h) - t, 0.0)


def mac(mh, ml, acc, f):
    """mul2_mac: (h + l) acc + f."""
    return mh * acc + (ml * acc + f)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def mul2_mul(ah, al, bh, bl):
    h, e = _two_prod(ah, bh)
    return h, e + (ah * bl + al * bh)


def wg_scan(v, ph, pl, rev):
    """wg_scan_pair over the last axis (a multiple of 64 threads), multipliers as h + l: the exclusive
    (ev, eh, el) and the total tv."""
    if rev:
        ev, eh, el, tv = wg_scan(v[..., ::-1], ph[..., ::-1], pl[..., ::-1], False)
        return ev[..., ::-1], eh[..., ::-1], el[..., ::-1], tv
    sh = v.shape
    w64 = sh[:-1] + (sh[-1] // 64, 64)
    v, ph, pl = v.reshape(w64).copy(), ph.reshape(w64).copy(), pl.reshape(w64).copy()
    off = 1
    while off < 64:
        lv, lh, ll = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
        lv[..., off:], lh[..., off:], ll[..., off:] = v[..., :-off], ph[..., :-off], pl[..., :-off]
        v = mac(ph, pl, lv, v)
        ph, pl = mul2_mul(ph, pl, lh, ll)
        off *= 2
    xv, xh, xl = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
    xv[..., 1:], xh[..., 1:], xl[..., 1:] = v[..., :-1], ph[..., :-1], pl[..., :-1]
    tv, th, tl = np.zeros(sh[:-1]), np.ones(sh[:-1]), np.zeros(sh[:-1])
    ev, eh, el = np.empty_like(v), np.empty_like(v), np.empty_like(v)
    for w in range(v.shape[-2]):
        ev[..., w, :] = mac(xh[..., w, :], xl[..., w, :], tv[..., None], xv[..., w, :])
        eh[..., w, :], el[..., w, :] = mul2_mul(th[..., None], tl[..., None], xh[..., w, :], xl[..., w, :])
        tv = mac(ph[..., w, 63], pl[..., w, 63], tv, v[..., w, 63])
        th, tl = mul2_mul(th, tl, ph[..., w, 63], pl[..., w, 63])
    return ev.reshape(sh), eh.reshape(sh), el.reshape(sh), tv


def blocked_solve(f, c0, c1, nblk, sl, nseg, one_line, NTI):
    """f [nlines, m] -> x: the three phases. one_line: k_tri1 (the threads' scan); NTI: threads of k_blk_iface's
    workgroup per line (runs of blocks per thread, the same scan), 0 for k_trib_iface (a thread a line)."""
    nl, m = f.shape
    _, t, D = consts(c0, c1)
    rh, rl = mul2(t)
    lo = [(m * k) // nblk for k in range(nblk + 1)]
    nhi = max(lo[k + 1] - lo[k] for k in range(nblk))
    assert nseg * sl >= nhi
    # gather every block's rows into [line, block, segment, row], zero past a segment's rows
    g = np.zeros((nl, nblk, nseg * sl))
    ln = np.zeros((nblk, nseg), dtype=int)
    for k in range(nblk):
        n = lo[k + 1] - lo[k]
        g[:, k, :n] = f[:, lo[k]:lo[k + 1]]
        ln[k] = np.clip(n - np.arange(nseg) * sl, 0, sl)
    g = g.reshape(nl, nblk, nseg, sl)
    rrh, rrl = rh[:, None, None], rl[:, None, None]
    # both recursions over every segment from zero
    fl, bl = np.zeros((nl, nblk, nseg)), np.zeros((nl, nblk, nseg))
    for i in range(sl):
        fl = np.where(i < ln[None], mac(rrh, rrl, fl, g[..., i]), fl)
        bl = mac(rrh, rrl, bl, g[..., sl - 1 - i])
    # the segments' multipliers: r^sl, r^rem for the one after the whole ones, 1 for an empty one
    mh, ml = np.ones((nl, nblk, nseg)), np.zeros((nl, nblk, nseg))
    for length in np.unique(ln):
        h, l = mul2(tpow(t, int(length)))
        mh[:, ln == length], ml[:, ln == length] = h[:, None], l[:, None]
    if one_line:
        fev, feh, fel, ftv = wg_scan(fl, mh, ml, False)
        bev, beh, bel, btv = wg_scan(bl, mh, ml, True)
    else:   # one thread per line walks the segments
        z = lambda: np.zeros((nl, nblk, nseg))   # noqa: E731
        fev, bev, fel, bel, feh, beh = z(), z(), z(), z(), z() + 1.0, z() + 1.0
        acc, bcc = np.zeros((nl, nblk)), np.zeros((nl, nblk))
        for k in range(nseg):
            kr = nseg - 1 - k
            fev[..., k], bev[..., kr] = acc, bcc
            acc = mac(mh[..., k], ml[..., k], acc, fl[..., k])
            bcc = mac(mh[..., kr], ml[..., kr], bcc, bl[..., kr])
        ftv, btv = acc, bcc
    # ---- the interface: every block's carries from the blocks' pairs (ftv, btv) [line, block] ----
    nlo = m // nblk
    tlo = tpow(t, nlo)
    thi = (tlo + t) - tlo * t
    (hlo, llo), (hhi, lhi) = mul2(tlo), mul2(thi)
    short = np.array([lo[k + 1] - lo[k] == nlo for k in range(nblk)])
    bh, bl_ = np.where(short[None], hlo[:, None], hhi[:, None]), np.where(short[None], llo[:, None], lhi[:, None])
    tm = tpow(t, m)
    pm, idet = 1.0 - tm, 1.0 / (tm * (2.0 - tm))   # r^m, 1 / (1 - r^2m)
    lrf, lrb = np.zeros((nl, nblk)), np.zeros((nl, nblk))
    if NTI:
        per = cdiv(nblk, NTI)
        k0 = np.minimum(np.arange(NTI) * per, nblk)
        k1 = np.minimum(k0 + per, nblk)
        acc, bcc = np.zeros((nl, NTI)), np.zeros((nl, NTI))
        pph, ppl = np.ones((nl, NTI)), np.zeros((nl, NTI))
        for j in range(per):
            k = k0 + j
            on = k < k1
            kk = np.where(on, k, 0)
            acc = np.where(on, mac(bh[:, kk], bl_[:, kk], acc, ftv[:, kk]), acc)
            nh, nl_ = mul2_mul(pph, ppl, bh[:, kk], bl_[:, kk])
            pph, ppl = np.where(on, nh, pph), np.where(on, nl_, ppl)
            k = k1 - 1 - j
            on = k >= k0
            kk = np.where(on, k, 0)
            bcc = np.where(on, mac(bh[:, kk], bl_[:, kk], bcc, btv[:, kk]), bcc)
        xfv, xfh, xfl, FT = wg_scan(acc, pph, ppl, False)
        xbv, xbh, xbl, BT = wg_scan(bcc, pph, ppl, True)
        fm1, bm = (BT + pm * FT) * idet, (FT + pm * BT) * idet
        fcur, bcur = mac(xfh, xfl, fm1[:, None], xfv), mac(xbh, xbl, bm[:, None], xbv)
        for j in range(per):
            k = k0 + j
            for tt in np.nonzero(k < k1)[0]:
                lrf[:, k[tt]] = fcur[:, tt]
                fcur[:, tt] = mac(bh[:, k[tt]], bl_[:, k[tt]], fcur[:, tt], ftv[:, k[tt]])
            k = k1 - 1 - j
            for tt in np.nonzero(k >= k0)[0]:
                lrb[:, k[tt]] = bcur[:, tt]
                bcur[:, tt] = mac(bh[:, k[tt]], bl_[:, k[tt]], bcur[:, tt], btv[:, k[tt]])
    else:   # k_trib_iface: one thread per line walks the blocks, twice
        acc = np.zeros(nl)
        for k in range(nblk):
            acc = mac(bh[:, k], bl_[:, k], acc, ftv[:, k])
        bcc = np.zeros(nl)
        for k in range(nblk - 1, -1, -1):
            bcc = mac(bh[:, k], bl_[:, k], bcc, btv[:, k])
        fcur, bcur = (bcc + pm * acc) * idet, (acc + pm * bcc) * idet
        for k in range(nblk):
            lrf[:, k] = fcur
            fcur = mac(bh[:, k], bl_[:, k], fcur, ftv[:, k])
        for k in range(nblk - 1, -1, -1):
            lrb[:, k] = bcur
            bcur = mac(bh[:, k], bl_[:, k], bcur, btv[:, k])
    # ---- phase 3: every segment's carries from its block's, then the rerun ----
    fin = mac(feh, fel, lrf[..., None], fev)
    bin_ = mac(beh, bel, lrb[..., None], bev)
    if not one_line:   # the line's thread walks the segments again from the block's carries
        acc, bcc = lrf.copy(), lrb.copy()
        for k in range(nseg):
            kr = nseg - 1 - k
            fin[..., k], bin_[..., kr] = acc, bcc
            acc = mac(mh[..., k], ml[..., k], acc, fl[..., k])
            bcc = mac(mh[..., kr], ml[..., kr], bcc, bl[..., kr])
    bv = bin_.copy()
    for i in range(sl - 1, -1, -1):
        on = i < ln[None]
        bv = np.where(on, mac(rrh, rrl, bv, g[..., i]), bv)
        g[..., i] = np.where(on, bv, g[..., i])
    out = np.zeros_like(g)
    fv = fin
    for i in range(sl):
        on = i < ln[None]
        gn = np.where(i + 1 < ln[None], g[..., min(i + 1, sl - 1)], bin_)
        out[..., i] = np.where(on, mac(rrh, rrl, fv, g[..., i]) / D[:, None, None], 0.0)
        fv = np.where(on, mac(rrh, rrl, fv - gn, g[..., i]), fv)
    out = out.reshape(nl, nblk, nseg * sl)
    x = np.empty_like(f)
    for k in range(nblk):
        x[:, lo[k]:lo[k + 1]] = out[:, k, :lo[k + 1] - lo[k]]
    return x


def model_solve(m, deltas, sigma, b, blocks=0, weighted=True):
    """(I + sigma D^T D) x = b as the library solves it on a long last dimension: float64 cosine transforms along
    dim 0 (2-D), the blocked line solve along the last dimension."""
    p = len(m)
    assert p in (1, 2)
    cS = {}
    for blk in block_table(p, deltas if weighted else None, "cpp", unit_weights=not weighted):
        key = tuple(sorted(blk.Sp))
        cS[key] = cS.get(key, 0.0) + blk.w * blk.w
    nblk, tq, sl, nseg = plan(m, blocks)
    if p == 1:
        x = blocked_solve(np.asarray(b, float)[None, :], np.array([1.0]), np.array([sigma * cS[(0,)]]), nblk, sl, nseg,
                          True, 1024)
        return x[0]
    m0, m1 = int(m[0]), int(m[1])
    lam0 = 4.0 * np.sin(np.pi * np.arange(m0) / (2.0 * m0)) ** 2
    c0 = 1.0 + sigma * cS.get((0,), 0.0) * lam0
    c1 = sigma * (cS.get((1,), 0.0) + cS.get((0, 1), 0.0) * lam0)
    B = np.asarray(b, float).reshape(m0, m1, order="F")
    F = sfft.dct(B, type=2, norm="ortho", axis=0)
    X = blocked_solve(F, c0, c1, nblk, sl, nseg, False, 64 if m0 < WAVE_IFACE_BELOW else 0)
    return sfft.idct(X, type=2, norm="ortho", axis=0).ravel(order="F")


def test_plan_block_and_segment_shapes():
    assert plan([4097]) == (2, 0, 16, 256) and plan([1 << 20]) == (256, 0, 16, 256)
    assert plan([1000], 3) == (3, 0, 16, 256) and plan([37], 2) == (2, 0, 16, 256)
    assert plan([10000], 2) is None and plan([37], 38) is None and plan([37], 1) is None
    assert plan([64, 64, 300], 4) == (4, 64, 32, 3)          # 75-row blocks: 32 + 32 + 11
    assert plan([128, 128, 135], 2) == (2, 64, 32, 3)        # 67 / 68
    assert plan([8, 8, 8, 100], 3) == (3, 16, 32, 2)
    assert plan([4096, 67], 2) == (2, 16, 32, 2)
    assert plan([2, 5000])[1] == 4 and plan([3, 4100])[1] == 4
    assert plan([64, 4100])[1] == 16 and plan([1024, 4099])[:2] == (17, 64)
    assert plan([128, 128, 8192]) == (32, 64, 32, 8)
    for m in ([2, 5000], [3, 4100], [64, 4100], [1024, 4099], [16, 16, 4100], [8, 8, 8, 4100], [48, 4100]):
        nb, tq, sl, nseg = plan(m)
        assert 2 <= nb and cdiv(m[-1], nb) <= sl * nseg and nseg <= {64: 8, 16: 32, 4: 64}[tq]


def test_wg_scan_is_the_sequential_weighted_scan():
    rng = np.random.default_rng(5)
    v, p = rng.standard_normal((3, 256)), rng.uniform(0.2, 1.0, (3, 256))
    for rev in (False, True):
        ev, eh, el, tv = wg_scan(v, p, np.zeros_like(p), rev)
        ep = eh + el
        order = range(255, -1, -1) if rev else range(256)
        acc, pa = np.zeros(3), np.ones(3)
        for i in order:
            np.testing.assert_allclose(ev[:, i], acc, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(ep[:, i], pa, rtol=1e-12)
            acc, pa = acc * p[:, i] + v[:, i], pa * p[:, i]
        np.testing.assert_allclose(tv, acc, rtol=1e-12, atol=1e-13)


SIGMAS = [0.0, 1e-3, 3.7, 2e5]
AUTO_SHAPES = [[4097], [4099], [8192], [65537], [1 << 20], [64, 4100], [1024, 4099], [2, 5000], [3, 4100]]
FORCED = [([1000], 3), ([37], 2), ([4096, 67], 2)]


def _check(m, blocks, weighted=True):
    rng = np.random.default_rng(sum(m) + blocks)
    b = rng.standard_normal(int(np.prod(m))) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    fwd_ld, fwd_64 = SLD.forward_ld(m, b), SLD.forward_ld(m, b, np.float64)
    sym_ld = SLD.dtd_symbol_ld(m, deltas, 0, weighted)
    sym_64 = SLD.dtd_symbol_ld(m, deltas, 0, weighted, np.float64)
    for sigma in SIGMAS:
        x_ld = SLD.solve_from_forward(fwd_ld, sym_ld, sigma)
        x_64 = SLD.solve_from_forward(fwd_64, sym_64, sigma)
        x = model_solve(m, deltas, sigma, b, blocks, weighted)
        scale = float(np.max(np.abs(x_ld)))
        e64 = float(np.max(np.abs(x_64 - x_ld))) / scale
        err = float(np.max(np.abs(x - x_ld))) / scale
        print(f"m={m} blocks={blocks} sigma={sigma:g}: err {err:.2e}, e64 {e64:.2e}, ratio {err / e64:.2f}")
        assert err <= min(1e-12, 32.0 * e64), (m, blocks, sigma, err, e64)


@pytest.mark.parametrize("m", AUTO_SHAPES, ids=lambda m: "x".join(map(str, m)))
def test_blocked_model_matches_long_double_auto(m):
    _check(m, 0)


@pytest.mark.parametrize("m,blocks", FORCED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_blocked_model_matches_long_double_forced(m, blocks):
    _check(m, blocks)


def test_blocked_model_unit_weights():
    _check([4099], 0, weighted=False)
    _check([48, 4100], 0, weighted=False)


def test_thread_per_line_interface_matches_the_wave_form():
    """k_trib_iface (>= 8192 lines) against k_blk_iface<1> on the same lines: the same carries to rounding."""
    rng = np.random.default_rng(11)
    f = rng.standard_normal((5, 1111)) + 2.0
    c0, c1 = np.full(5, 1.0), np.array([0.0, 1e-3, 1.0, 50.0, 2e5])
    a = blocked_solve(f, c0, c1, 7, 32, 5, False, 0)
    b = blocked_solve(f, c0, c1, 7, 32, 5, False, 64)
    assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(a))
