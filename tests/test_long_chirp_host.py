"""Host model of the chirp-z cosine transform of a leading mesh dimension of any length (k_chc / k_chr / k_cho,
mvtv_spectral.hip; mvtv_problem_dct_chirp).

A float64 numpy transcription of the passes' index logic: the library's convolution length M = a b (dct_chirp_auto),
the Makhoul order folded into the load, the exact chirp index n^2 mod 2m, the zero padding to M, the line as an a x b
matrix (sample n = n1 b + n2, frequency k1 + a k2 of the length-M transform), the inter-pass twiddle W_M^{n2 k1}, the
filter spectrum H stored at position b k1 + k2 (the order in which the fused row pass meets the frequencies), the
inverse passes back to natural sample order, the partner of Z[k] in the mirror column (m - n2) mod b of the column
tile's orbit (row (m - k) / b), the quarter-wave factor, the inverse transform as the conjugate of a forward one, and
the launch shapes (``plan`` / ``launches``, the transcription of launch_dct_chirp, which tests/test_gpu_long_chirp.py
imports). Checked against the long-double cosine-transform solve (oracle/spectral_ld.py) with test_gpu_dispatch.py's
forward-error rule. No GPU."""
import numpy as np
import pytest
import scipy.fft as sfft

from oracle import spectral_ld as SLD
from test_long_dct_host import cdiv, factor_ok, radix_plan, sub_fft

SPLIT_MAX = 4096    # kSplitMax: the longest factor
SLOTS = 4104        # dsp::SLOTS: complex LDS slots of a workgroup
GMAX = 64           # dsp::GMAX (the row pass takes single rows: up to 2 GMAX of them)
K_BOUND, RTOL_DIRECT = 32.0, 1e-12   # tests/test_gpu_dispatch.py
LD = np.longdouble
PI = LD(4.0) * np.arctan(LD(1.0))


def smooth(n):
    for q in (2, 3, 5, 7):
        while n % q == 0:
            n //= q
    return n == 1


def chirp_auto(m):
    """dct_chirp_auto: the smallest 2-3-5-7-smooth M >= 2m - 1 with a factorisation into two factors <= 4096, a the
    largest such divisor <= sqrt(M); None: no such M."""
    M = max(4, 2 * m - 1)
    while M <= SPLIT_MAX * SPLIT_MAX:
        if smooth(M):
            best, d = 0, 2
            while d * d <= M:
                if M % d == 0 and M // d <= SPLIT_MAX:
                    best = d
                d += 1
            if best:
                return best, M // best
        M += 1
    return None


def orbits(m, b):
    """chirp_col's rule: the orbits (u, u') of the column involution u -> (m - u) mod b, in tile order."""
    r = m % b
    nlo = r // 2 + 1
    norb = nlo + (r + b) // 2 - r
    out = []
    for t in range(norb):
        out.append((t, r - t) if t < nlo else (r + 1 + (t - nlo), b - 1 - (t - nlo)))
    return out


def plan(mesh, d, ab=None):
    """launch_dct_chirp's shapes for dimension d of mesh under the factors ab (None: the library's)."""
    m = int(mesh[d])
    a, b = ab or chirp_auto(m)
    nlines = int(np.prod(mesh)) // m
    nclt = cdiv(nlines, 2)
    norb = len(orbits(m, b))
    tq = 2 if d == 0 else 16
    while tq > 2 and (tq // 2) * 2 * (a + 1) > SLOTS:
        tq //= 2
    hmax = min(norb, max(1, SLOTS // ((tq // 2) * 2 * (a + 1))))
    nct = cdiv(norb, hmax)
    Ch = cdiv(norb, nct)
    G = min(2 * GMAX, max(1, SLOTS // (b + 1)))
    return dict(a=a, b=b, M=a * b, tq=tq, Ch=Ch, nct=nct, norb=norb, G=G, grid_c=cdiv(nclt, tq // 2) * nct,
                grid_r=cdiv(nclt * a, G), lds_c=(tq // 2) * 2 * Ch * (a + 1) * 16, lds_r=G * (b + 1) * 16)


def launches(mesh, d, ab=None, inverse=False, formb=False):
    """[(kernel, grid, block)] of one chirp pass along d, in launch order."""
    s = plan(mesh, d, ab)
    t = lambda v: "true" if v else "false"   # noqa: E731
    return [(f"k_chc<{t(inverse)}, {t(d == 0)}, {t(formb and not inverse)}>", s["grid_c"], 512),
            ("k_chr", s["grid_r"], 512),
            (f"k_cho<{t(inverse)}, {t(d == 0)}>", s["grid_c"], 512)]


def solve_launches(mesh, chirps, formb=False):
    """The chirp launches of one spectral solve: forward along the chirp dims ascending (b formed on load by the
    first pass of the solve, which is dim 0's), then inverse descending. chirps: {dim: (a, b) or None}."""
    out = []
    for d in sorted(chirps):
        out += launches(mesh, d, chirps[d], False, formb and d == 0)
    for d in sorted(chirps, reverse=True):
        out += launches(mesh, d, chirps[d], True)
    return out


# ---- the tables --------------------------------------------------------------------------------------------------
def tables(m, a, b):
    """chirp_tables: c[n] = e^{-i pi n^2/m} with n^2 mod 2m exact, the quarter wave, and H = FFT_M(h) / M of the
    wrapped h[j] = conj c[|j|] at position b k1 + k2 for frequency k1 + a k2; long double, rounded once."""
    M = a * b
    n = np.arange(m, dtype=np.int64)
    ang = -PI * ((n * n) % (2 * m)).astype(LD) / LD(m)
    c = np.cos(ang) + 1j * np.sin(ang)
    h = np.zeros(M, dtype=np.clongdouble)
    h[:m] = np.conj(c)
    h[M - m + 1:] = np.conj(c[1:][::-1])   # wraps onto the head when M < 2m - 1: the M = 2m - 2 variant
    H = sfft.fft(h) / LD(M)
    k1, k2 = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    Ht = H[k1 + a * k2].ravel()
    qa = -PI * n.astype(LD) / LD(2 * m)
    q = np.cos(qa) + 1j * np.sin(qa)
    return c.astype(np.complex128), q.astype(np.complex128), Ht.astype(np.complex128)


def wM(M, J):
    """W_M^J rounded to float64 from a long-double evaluation (dd_tw's hi + lo product is one rounded value)."""
    ang = -2.0 * PI * (np.asarray(J, dtype=np.int64) % M).astype(LD) / LD(M)
    return np.cos(ang).astype(np.float64) + 1j * np.sin(ang).astype(np.float64)


class Bug:
    """A deliberate index error for the tests with teeth."""
    h_off = 0          # the filter spectrum read at position b k1 + k2 + this
    partner_off = 0    # the k <-> m - k partner taken from the mirror column + this


def convolve(y, m, a, b, Ht, bug=Bug):
    """The three passes on one packed line: y (m values, already times c) -> w (m values) = y * h circularly."""
    M = a * b
    pad = np.zeros(M, dtype=np.complex128)
    pad[:m] = y                                              # zero for m <= n < M
    S = sub_fft(pad.reshape(a, b).T, False).T                # k_chc: [k1][n2], length-a FFTs of the columns
    k1, n2 = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    tw = wM(M, n2 * k1)
    S = S * tw
    R = sub_fft(S, False)                                    # k_chr: [k1][k2]
    R = R * Ht[(k1 * b + n2 + bug.h_off) % M]
    R = sub_fft(R, True) * np.conj(tw)                       # [k1][n2], unnormalised inverse (H carries 1 / M)
    w = sub_fft(R.T, True).T.ravel()                         # k_cho: [n1][n2] = sample n
    return w[:m]


def forward_pair(xa, xb, ab, bug=Bug):
    """Unnormalised DCT-II of the real lines xa, xb (length m) by k_chc, k_chr, k_cho: natural frequency order."""
    m = xa.size
    a, b = ab
    c, q, Ht = tables(m, a, b)
    n = np.arange(m)
    src = np.where(2 * n < m, 2 * n, 2 * (m - 1 - n) + 1)     # v[n] = x[2n], v[m-1-n] = x[2n+1]
    v = xa[src] + 1j * xb[src]
    Z = c * convolve(v * c, m, a, b, Ht, bug)
    # Z[m - k]: the mirror column of k's orbit, row (m - k) / b; k = 0 pairs with itself
    mirror = np.empty(b, dtype=np.int64)
    for u, up in orbits(m, b):
        mirror[u], mirror[up] = up, u
    kp = np.where(n == 0, 0, m - n)
    pos = (kp // b) * b + (mirror[n % b] + bug.partner_off) % b
    pos = np.where(n == 0, 0, pos)
    Z2 = np.where(pos < m, Z[np.minimum(pos, m - 1)], 0.0)
    A = 0.5 * (Z + np.conj(Z2))
    B = -0.5j * (Z - np.conj(Z2))
    return (q * A).real, (q * B).real


def inverse_pair(Xa, Xb, ab):
    """Unnormalised DCT-III (m x the inverse of forward_pair): the inverse DFT as conj(DFT(conj V))."""
    m = Xa.size
    a, b = ab
    c, q, Ht = tables(m, a, b)
    k = np.arange(m)
    kp = np.where(k == 0, 0, m - k)

    def V(X):
        Xm = np.where(k == 0, 0.0, X[kp])                    # X[m] = 0
        return np.conj(q) * (X - 1j * Xm)
    Z = V(Xa) + 1j * V(Xb)
    z = np.conj(c * convolve(np.conj(Z) * c, m, a, b, Ht))
    src = np.where(2 * k < m, 2 * k, 2 * (m - 1 - k) + 1)
    xa, xb = np.empty(m), np.empty(m)
    xa[src], xb[src] = z.real, z.imag
    return xa, xb


def model_solve(mesh, ab, deltas, sigma, bvec, bug=Bug, forward_only=False):
    """(I + sigma D^T D) x = b on a 2-D mesh: the chirp passes along dim 0 (line pairs, an unpaired last line with a
    zero partner), the last dimension by float64 cosine transforms. forward_only: the way back by pocketfft."""
    m0, m1 = mesh
    x = np.asarray(bvec, dtype=np.float64).reshape(mesh, order="F")
    C = np.empty_like(x)
    for j in range(0, m1, 2):
        xb = x[:, j + 1] if j + 1 < m1 else np.zeros(m0)
        ca, cb = forward_pair(x[:, j], xb, ab, bug)
        C[:, j] = ca
        if j + 1 < m1:
            C[:, j + 1] = cb
    sym = SLD.dtd_symbol_ld(mesh, deltas, "cpp", True, np.float64)
    T = sfft.dct(C, type=2, axis=1, norm="ortho") / (1.0 + sigma * sym)
    Y = sfft.idct(T, type=2, axis=1, norm="ortho")
    out = np.empty_like(x)
    for j in range(0, m1, 2):
        yb = Y[:, j + 1] if j + 1 < m1 else np.zeros(m0)
        ya, yb = inverse_pair(Y[:, j], yb, ab)
        out[:, j] = ya
        if j + 1 < m1:
            out[:, j + 1] = yb
    return out.ravel(order="F") / m0


# ---- tests -----------------------------------------------------------------------------------------------------------
def test_the_librarys_convolution_length():
    assert chirp_auto(4099) == (84, 98) and chirp_auto(4100) == (84, 98)          # M = 8232
    assert chirp_auto(5003) == (96, 105) and chirp_auto(5504) == (105, 105)       # 10080, 11025
    assert chirp_auto(8256) == (120, 140)                                         # 16800
    assert chirp_auto(65537) == (324, 405)                                        # 131220
    assert chirp_auto(100003) == (448, 448)                                       # 200704
    assert chirp_auto(2) == (2, 2) and chirp_auto(23) == (5, 9)                   # M = 45 = 2m - 1 exactly
    assert chirp_auto((4096 * 4096 + 1) // 2) == (4096, 4096)
    assert chirp_auto((4096 * 4096 + 1) // 2 + 1) is None
    for m in (4099, 8256, 65537):
        a, b = chirp_auto(m)
        assert a * b >= 2 * m - 1 and factor_ok(a) and factor_ok(b) and a <= b


def test_orbits_partition_the_columns_and_hold_the_partner():
    for m, b in ((4099, 98), (4100, 98), (23, 9), (22, 8), (13, 16), (13, 2), (100, 20), (64, 16), (4099, 3),
                 (4099, 4096), (37, 15), (37, 10), (8256, 140)):
        orb = orbits(m, b)
        cols = [u for u, _ in orb] + [up for u, up in orb if up != u]
        assert sorted(cols) == list(range(b)), (m, b)
        for u, up in orb:
            assert u <= up and (m - u) % b == up and (m - up) % b == u


def test_chirp_index_is_exact_where_a_float_square_is_not():
    m = 100003
    n = np.arange(m, dtype=np.int64)
    exact = (n * n) % (2 * m)
    assert int(exact[-1]) == ((m - 1) ** 2) % (2 * m)
    assert np.max(n * n) < 2 ** 63 and np.max(n.astype(np.float64) ** 2) > 2 ** 33


@pytest.mark.parametrize("m,ab", [(23, (5, 9)), (22, (6, 8)), (37, (5, 15)), (37, (8, 10)), (13, (2, 16)),
                                  (13, (16, 2)), (100, (10, 20)), (64, (8, 16)), (11, (3, 7)), (45, (9, 10)),
                                  (24, (7, 7)), (4099, None), (4100, None), (8198, None), (4099, (3, 4096)),
                                  (4099, (4096, 3))])
def test_forward_matches_the_cosine_sum_and_the_inverse_undoes_it(m, ab):
    ab = ab or chirp_auto(m)
    rng = np.random.default_rng(m * 31 + ab[0])
    xa, xb = rng.standard_normal(m) + 2.0, rng.standard_normal(m) + 2.0
    Xa, Xb = forward_pair(xa, xb, ab)
    for X, x in ((Xa, xa), (Xb, xb)):
        ref = 0.5 * sfft.dct(x.astype(LD), type=2)   # sum x[n] cos(pi (2n + 1) k / 2m)
        assert np.max(np.abs(X - ref)) <= 64 * np.finfo(float).eps * np.max(np.abs(ref))
    ya, yb = inverse_pair(Xa, Xb, ab)
    assert np.max(np.abs(ya / m - xa)) <= 1e-12 and np.max(np.abs(yb / m - xb)) <= 1e-12


SOLVES = [([23, 2], (5, 9)), ([22, 2], (6, 8)), ([22, 3], (6, 8)), ([22, 5], (5, 9)), ([37, 4], (5, 15)),
          ([37, 4], (8, 10)), ([13, 40], (2, 16)), ([13, 40], (16, 2)), ([100, 7], (10, 20)), ([64, 2], (8, 16)),
          ([4099, 3], None), ([4100, 2], None), ([8256, 2], None), ([8198, 2], None)]


def _errs(mesh, ab, sigma, bug=Bug):
    ab = ab or chirp_auto(mesh[0])
    N = int(np.prod(mesh))
    b = np.random.default_rng(2000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in mesh]
    x_ld = SLD.spectral_solve_ld(mesh, deltas, sigma, b, "cpp", True)
    x64 = SLD.spectral_solve_ld(mesh, deltas, sigma, b, "cpp", True, np.float64)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(model_solve(mesh, ab, deltas, sigma, b, bug) - x_ld))) / scale
    return err, e64


@pytest.mark.parametrize("sigma", [0.0, 1e-3, 3.7, 2e5])
@pytest.mark.parametrize("mesh,ab", SOLVES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, (list, tuple)) else "auto")
def test_model_solve_forward_error(mesh, ab, sigma):
    err, e64 = _errs(mesh, ab, sigma)
    print(f"chirp model {mesh} {ab} sigma={sigma:g}: e64 {e64:.2e} model {err:.2e} ratio {err / e64:.2f}")
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


@pytest.mark.parametrize("mesh,ab", [([22, 3], (6, 8)), ([37, 4], (5, 15)), ([4099, 2], None)],
                         ids=["22x3", "37x4", "4099x2"])
def test_index_errors_are_caught_by_orders_of_magnitude(mesh, ab):
    class Hoff(Bug):
        h_off = 1

    class Col(Bug):
        partner_off = 1
    bound = min(RTOL_DIRECT, K_BOUND * _errs(mesh, ab, 3.7)[1])
    for bug in (Hoff, Col):
        err, _ = _errs(mesh, ab, 3.7, bug)
        assert err >= 1e3 * bound, (bug.__name__, err, bound)


@pytest.mark.parametrize("mesh,ab", [([24, 3], (5, 9)), ([33, 4], (7, 9)), ([64, 2], (5, 25))],
                         ids=["24x3", "33x4", "64x2"])
def test_a_convolution_too_short_wraps_around(mesh, ab):
    """M = 2m - 3: the lag m - 1 lands on the lag -(m - 2), whose filter value differs."""
    assert ab[0] * ab[1] == 2 * mesh[0] - 3
    err, e64 = _errs(mesh, ab, 3.7)
    assert err >= 1e3 * min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


@pytest.mark.parametrize("mesh,ab", [([22, 3], (6, 7)), ([37, 4], (8, 9)), ([64, 2], (9, 14))],
                         ids=["22x3", "37x4", "64x2"])
def test_m_equal_2m_minus_2_does_not_wrap(mesh, ab):
    """M = 2m - 2 was expected to wrap around; it does not. The only coincidence is of the lags m - 1 and -(m - 1),
    and the filter is symmetric, h[j] = h[-j] = conj c[|j|], so both carry the same value: the model stays at the
    rounding level (22 x 3: 5.0e-16 against e64 3.3e-16 at sigma = 3.7). The library keeps the documented M >= 2m - 1."""
    assert ab[0] * ab[1] == 2 * mesh[0] - 2
    err, e64 = _errs(mesh, ab, 3.7)
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


def test_shapes_of_the_named_cases():
    """What each case of tests/test_gpu_long_chirp.py is for, from the plan alone."""
    s = plan([4099, 2], 0)
    assert (s["a"], s["b"], s["tq"], s["norb"], s["Ch"], s["nct"], s["grid_c"], s["G"], s["grid_r"]) == \
        (84, 98, 2, 49, 17, 3, 3, 41, 3)
    assert plan([4099, 3], 0)["grid_c"] == 6                      # the unpaired last line has tiles of its own
    assert plan([4100, 600], 0)["grid_c"] == 900 and plan([4100, 600], 0)["grid_r"] == cdiv(300 * 84, 41)
    assert plan([65537, 2], 0)["M"] == 131220 and plan([65537, 2], 0)["G"] == 10
    # a factor of 4096: more than 64 KB of dynamic LDS (one orbit of 2 x 4097 slots; one row of 4097)
    assert plan([4099, 2], 0, (4096, 3))["lds_c"] == 2 * 4097 * 16 and plan([4099, 2], 0, (4096, 3))["Ch"] == 1
    assert plan([4099, 2], 0, (3, 4096))["lds_r"] == 4097 * 16 and plan([4099, 2], 0, (3, 4096))["G"] == 1
    assert plan([4099, 2], 0, (3, 4096))["lds_c"] <= 4104 * 16
    # strided passes: 8 adjacent line pairs (128-B rows)
    assert plan([22, 22, 3], 1, (6, 8))["tq"] == 16 and plan([11, 11, 11, 3], 2, (3, 7))["tq"] == 16
    assert launches([22, 22, 3], 1, (6, 8), inverse=True)[0][0] == "k_chc<true, false, false>"
    assert [n for n, _, _ in solve_launches([4099, 2], {0: None}, formb=True)] == [
        "k_chc<false, true, true>", "k_chr", "k_cho<false, true>", "k_chc<true, true, false>", "k_chr",
        "k_cho<true, true>"]
    used = set()
    for m, ab in ((4099, None), (8256, None), (5504, None), (23, (5, 9)), (22, (6, 8)), (13, (2, 16))):
        a, b = ab or chirp_auto(m)
        used |= set(radix_plan(a) + radix_plan(b))
    assert used == {2, 3, 4, 5, 7, 8}


def test_launches_of_the_named_cases():
    """The launch lists tests/test_gpu_long_chirp.py asserts against the launch log, from the plan alone."""
    assert launches([4099, 2], 0) == [("k_chc<false, true, false>", 3, 512), ("k_chr", 3, 512),
                                      ("k_cho<false, true>", 3, 512)]
    assert launches([4099, 3], 0, inverse=True) == [("k_chc<true, true, false>", 6, 512), ("k_chr", 5, 512),
                                                    ("k_cho<true, true>", 6, 512)]
    assert launches([4100, 600], 0, formb=True)[0] == ("k_chc<false, true, true>", 900, 512)
    assert plan([65537, 2], 0)["M"] == 131220 and plan([8256, 4], 0)["M"] == 16800
    assert launches([22, 22, 3], 1, (6, 8))[0][0] == "k_chc<false, false, false>"
    assert len(solve_launches([11, 11, 11, 3], {0: (3, 7), 1: (4, 6), 2: (5, 5)})) == 18
