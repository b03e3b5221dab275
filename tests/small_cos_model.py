"""Shared by tests/test_small_cos_host.py and tests/test_gpu_small_cos*.py: the transcription of the rules of the
batched fits' in-workgroup cosine solve (multivartv_amd/csrc/mvtv_small_cos.hip, mvtv_internal.h small_cos_shape,
small_cos_zlds, small_cos_lds_bytes) and a float64 numpy model of the kernel's index logic.

Rules. The line dimension is the longest, the last of them on a tie; every other dimension is transformed densely with
an m_j x m_j table at row pitch m_j | 1. A line gets tpl threads, the largest power of two with nlines * tpl <= NT, and
thread s of them the rows [s sl, (s + 1) sl), sl = ceil(m_line / tpl). z stays in LDS while nb * N <= COS_Z_LDS_WORDS.

Model. model_solve: dense products with the tables (long double, rounded), then per line the factorised operator of
DESIGN.md §4.1 as the kernel runs it: both recursions over each segment from zero, the weighted scan over the line's
threads (shuffle steps inside a 64-lane wave, then the line's waves in order), the mirror closure, the rerun from the
carries; r as h + l pairs from the cancellation-free t = 1 - r (plain_r = True: one rounded double and its powers).
"""
import numpy as np

import small_batch_cases as S
from oracle.mvtv_oracle import block_table

LD = np.longdouble
COS_Z_LDS_WORDS = 11264   # kSmallCosZLds
COS_MAX_T = 64            # kSmallCosMaxT
LDS_LIMIT = 160 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def line_dim(m):
    ld = 0
    for j in range(1, len(m)):
        if m[j] >= m[ld]:
            ld = j
    return ld


def plan(m):
    """small_cos_shape: dict(ld, nt, nlines, tpl, sl, toff, pitch, tab_words)."""
    m = [int(v) for v in m]
    N, ld = int(np.prod(m)), line_dim(m)
    nt, nlines = S.nt_rule(N), N // m[ld]
    assert nlines <= nt
    tpl = 1
    while tpl * 2 * nlines <= nt:
        tpl *= 2
    toff, pitch, off = {}, {}, 0
    for j in range(len(m)):
        if j == ld:
            continue
        toff[j], pitch[j] = off, m[j] | 1
        off += m[j] * pitch[j]
    return dict(ld=ld, nt=nt, nlines=nlines, tpl=tpl, sl=cdiv(m[ld], tpl), toff=toff, pitch=pitch, tab_words=off)


def lds_bytes(m, nb, loop):
    """small_cos_lds_bytes."""
    N, pl = int(np.prod(m)), plan(m)
    z = nb * N if (loop and nb * N <= COS_Z_LDS_WORDS) else 0
    return 8 * (N + 9 * (pl["nt"] // 64) + pl["tab_words"] + z)


def solve_name(m):
    return f"k_solve_cos<{len(m)}, {S.nt_rule(int(np.prod(m)))}>"


def loop_name(m, pc, order="cpp", weighted=True):
    """The k_admm_cos instantiation the launch log shows for mesh m."""
    N, p = int(np.prod(m)), len(m)
    zlds = S.n_blocks(p, order, weighted) * N <= COS_Z_LDS_WORDS
    return f"k_admm_cos<{p}, {S.nt_rule(N)}, {'true' if zlds else 'false'}, {'true' if pc else 'false'}>"


def reachable_loops():
    """Every (P, NT, ZLDS) some admitted mesh reaches, as S.reachable_instantiations() with this file's z rule."""
    out = set()
    for p in (1, 2, 3, 4):
        nbs = {S.n_blocks(p, o, w) for o in ("cpp", "py") for w in (True, False)}
        cap = S.MAX_N4 if p == 4 else S.MAX_N
        for N in range(2 ** p, cap + 1):
            for nb in nbs:
                out.add((p, S.nt_rule(N), nb * N <= COS_Z_LDS_WORDS))
    return out


# 2-D at NT = 1024 with z in LDS is reached by no mesh of S.SHAPES under this file's z rule (64 x 64, 2 x 2048 and
# 2048 x 2 hold 12288 edge words): 40 x 50 does (6000).
EXTRA_SHAPES = [[40, 50]]


def _cS(m, deltas, order, weighted, dtype):
    p = len(m)
    oname = order if isinstance(order, str) else ("cpp" if order == 0 else "py")
    cS = {}
    for blk in block_table(p, deltas if weighted else None, oname, unit_weights=not weighted):
        key = tuple(sorted(blk.Sp))
        w = dtype(blk.w)
        cS[key] = cS.get(key, dtype(0.0)) + w * w
    return cS


def tables(m):
    """Per transformed dimension the orthonormal DCT-II matrix C[k][n], long double rounded to double."""
    ld = line_dim(m)
    pi = LD(4.0) * np.arctan(LD(1.0))
    out = {}
    for j, mj in enumerate(m):
        if j == ld:
            continue
        k = np.arange(mj)[:, None]
        n = np.arange(mj)[None, :]
        arg = ((2 * n + 1) * k) % (4 * mj)
        sc = np.where(k == 0, np.sqrt(LD(1.0) / LD(mj)), np.sqrt(LD(2.0) / LD(mj)))
        out[j] = (sc * np.cos(pi * arg.astype(LD) / LD(2 * mj))).astype(np.float64)
    return out


def line_ab(m, deltas, order="cpp", weighted=True):
    """a, b per line as arrays over the mesh with the line dimension dropped (long double, rounded)."""
    p, ld = len(m), line_dim(m)
    cS = _cS(m, deltas, order, weighted, LD)
    pi = LD(4.0) * np.arctan(LD(1.0))
    lam = [LD(4.0) * np.sin(pi * np.arange(mj, dtype=LD) / LD(2 * mj)) ** 2 for mj in m]
    shape = [mj for j, mj in enumerate(m) if j != ld]
    a, b = np.zeros(shape or [1], dtype=LD), np.zeros(shape or [1], dtype=LD)
    others = [j for j in range(p) if j != ld]
    for Sset, c in cS.items():
        term = np.full([1] * max(len(others), 1), c, dtype=LD)
        for j in Sset:
            if j == ld:
                continue
            sh = [1] * len(others)
            sh[others.index(j)] = m[j]
            term = term * lam[j].reshape(sh)
        if ld in Sset:
            b = b + term
        else:
            a = a + term
    return a.astype(np.float64), b.astype(np.float64)


# ---- the multipliers (mvtv_device.h tpow, Mul2) ----
def tpow(t, n):
    y, x = np.zeros_like(t), t.copy()
    while n:
        if n & 1:
            y = (y + x) - y * x
        x = (x + x) - x * x
        n >>= 1
    return y


def mul2(t):
    h = 1.0 - t
    return h, np.where(h >= 0.5, (1.0 - h) - t, 0.0)


def mac(mh, ml, acc, f):
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


def seg_scan(v, ph, pl, rev):
    """seg_scan over the last axis (a line's tpl threads, a power of two): the exclusive (ev, eh, el) and the line's
    total tv. Shuffle steps inside a wave (or inside the line where it is narrower), then the line's waves in order."""
    if rev:
        ev, eh, el, tv = seg_scan(v[..., ::-1], ph[..., ::-1], pl[..., ::-1], False)
        return ev[..., ::-1], eh[..., ::-1], el[..., ::-1], tv
    sh = v.shape
    tpl = sh[-1]
    gl = min(tpl, 64)
    w64 = sh[:-1] + (tpl // gl, gl)
    v, ph, pl = v.reshape(w64).copy(), ph.reshape(w64).copy(), pl.reshape(w64).copy()
    off = 1
    while off < gl:
        lv, lh, ll = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
        lv[..., off:], lh[..., off:], ll[..., off:] = v[..., :-off], ph[..., :-off], pl[..., :-off]
        on = np.arange(gl) >= off
        nv = mac(ph, pl, lv, v)
        nh, nl = mul2_mul(ph, pl, lh, ll)
        v, ph, pl = np.where(on, nv, v), np.where(on, nh, ph), np.where(on, nl, pl)
        off *= 2
    xv, xh, xl = np.zeros_like(v), np.ones_like(v), np.zeros_like(v)
    xv[..., 1:], xh[..., 1:], xl[..., 1:] = v[..., :-1], ph[..., :-1], pl[..., :-1]
    if tpl <= 64:
        return xv.reshape(sh), xh.reshape(sh), xl.reshape(sh), v[..., 0, -1]
    tv, th, tl = np.zeros(sh[:-1]), np.ones(sh[:-1]), np.zeros(sh[:-1])
    ev, eh, el = np.empty_like(v), np.empty_like(v), np.empty_like(v)
    for w in range(v.shape[-2]):
        ev[..., w, :] = mac(xh[..., w, :], xl[..., w, :], tv[..., None], xv[..., w, :])
        eh[..., w, :], el[..., w, :] = mul2_mul(th[..., None], tl[..., None], xh[..., w, :], xl[..., w, :])
        tv = mac(ph[..., w, -1], pl[..., w, -1], tv, v[..., w, -1])
        th, tl = mul2_mul(th, tl, ph[..., w, -1], pl[..., w, -1])
    return ev.reshape(sh), eh.reshape(sh), el.reshape(sh), tv


def line_solve(f, c0, c1, tpl, sl, plain_r=False):
    """f [nlines, m] -> x: (c0 I + c1 L) x = f per line, as cos_solve's line part."""
    nl, m = f.shape
    D = np.sqrt(c0 * (c0 + 4.0 * c1))
    den = 1.0 / (c0 + 2.0 * c1 + D)
    t = (c0 + D) * den
    if plain_r:
        rp = 2.0 * c1 * den
        rh, rl = rp, np.zeros_like(rp)
        pw = lambda n: (rp ** n, np.zeros_like(rp))   # noqa: E731
        tm = 1.0 - rp ** m
    else:
        rh, rl = mul2(t)
        pw = lambda n: mul2(tpow(t, n))   # noqa: E731
        tm = tpow(t, m)
    ln = np.clip(m - np.arange(tpl) * sl, 0, sl)
    g = np.zeros((nl, tpl * sl))
    g[:, :m] = f
    g = g.reshape(nl, tpl, sl)
    rrh, rrl = rh[:, None], rl[:, None]
    fl, bl = np.zeros((nl, tpl)), np.zeros((nl, tpl))
    for i in range(sl):
        on = i < ln[None]
        fl = np.where(on, mac(rrh, rrl, fl, g[..., i]), fl)
        idx = np.clip(ln - 1 - i, 0, sl - 1)
        bl = np.where(on, mac(rrh, rrl, bl, np.take_along_axis(g, np.broadcast_to(idx[None, :, None], (nl, tpl, 1)),
                                                               axis=2)[..., 0]), bl)
    mh, ml = np.ones((nl, tpl)), np.zeros((nl, tpl))
    for length in np.unique(ln):
        h, l = pw(int(length))
        mh[:, ln == length], ml[:, ln == length] = h[:, None], l[:, None]
    pm, idet = 1.0 - tm, 1.0 / (tm * (2.0 - tm))
    if tpl > 1:
        fev, feh, fel, ftv = seg_scan(fl, mh, ml, False)
        bev, beh, bel, btv = seg_scan(bl, mh, ml, True)
        fin = mac(feh, fel, ((pm * ftv + btv) * idet)[:, None], fev)
        bin_ = mac(beh, bel, ((pm * btv + ftv) * idet)[:, None], bev)
    else:
        fin, bin_ = (pm[:, None] * fl + bl) * idet[:, None], (pm[:, None] * bl + fl) * idet[:, None]
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
        out[..., i] = np.where(on, mac(rrh, rrl, fv, g[..., i]) / D[:, None], 0.0)
        fv = np.where(on, mac(rrh, rrl, fv - gn, g[..., i]), fv)
    return out.reshape(nl, tpl * sl)[:, :m]


def model_solve(m, deltas, sigma, b, shift=1.0, order="cpp", weighted=True, plain_r=False):
    """(shift I + sigma D^T D) x = b as k_solve_cos computes it, in float64."""
    m = [int(v) for v in m]
    pl = plan(m)
    ld, p = pl["ld"], len(m)
    X = np.asarray(b, dtype=np.float64).reshape(m, order="F").copy()
    T = tables(m)
    for j in range(p):
        if j != ld:
            X = np.moveaxis(np.tensordot(T[j], X, axes=([1], [j])), 0, j)
    a, bb = line_ab(m, deltas, order, weighted)
    lines = np.moveaxis(X, ld, -1).reshape(-1, m[ld])   # C order over the other dimensions, as a.ravel()
    c0 = shift + sigma * a.ravel()
    c1 = sigma * bb.ravel()
    xs = line_solve(lines, c0, c1, pl["tpl"], pl["sl"], plain_r)
    shape_o = [mj for j, mj in enumerate(m) if j != ld]
    X = np.moveaxis(xs.reshape(shape_o + [m[ld]]), -1, ld)
    for j in range(p - 1, -1, -1):
        if j != ld:
            X = np.moveaxis(np.tensordot(T[j].T, X, axes=([1], [j])), 0, j)
    return X.ravel(order="F")
