"""Host model of the two-pass ("four-step") cosine transform of a leading mesh dimension (k_dsc / k_dsr,
mvtv_spectral.hip).

A float64 numpy transcription of the passes' index logic: the factor split m = a b (dct_split_auto), the Makhoul
order folded into the column pass's load, the line as an a x b matrix (sample n = n1 b + n2, frequency k = k1 + a k2),
the inter-pass twiddle W_m^{n2 k1} read at index J = 4 n2 k1 of the powers of e^{-2 pi i/4m} (T1[J >> 12] T2[J & 4095]
with hi + lo entries), the quarter-wave twiddle at J = k, the partner of Z[k] at (a - k1, b - 1 - k2) (row 0:
(0, b - k2)), the frequency order position b k1 + k2 <-> k = k1 + a k2 with the lam table stored in it, and the launch
shapes (``plan``, the transcription of launch_dct_split, which tests/test_gpu_long_dct.py imports). Checked against the
long-double cosine-transform solve (oracle/spectral_ld.py) with test_gpu_dispatch.py's forward-error rule. No GPU."""
import numpy as np
import pytest

from oracle import spectral_ld as SLD

SPLIT_MAX = 4096    # kSplitMax: the longest factor
SLOTS = 4104        # dsp::SLOTS: complex LDS slots of a workgroup
GMAX = 64           # dsp::GMAX
K_BOUND, RTOL_DIRECT = 32.0, 1e-12   # tests/test_gpu_dispatch.py


def cdiv(a, b):
    return (a + b - 1) // b


def radix_plan(n):
    """dct_radix_plan: radices in stage order (8s first), None for a length with another prime factor."""
    rad = []
    for r in (8, 4, 2, 3, 5, 7):
        while n % r == 0 and n > 1:
            rad.append(r)
            n //= r
    return rad if n == 1 and len(rad) <= 8 else None


def factor_ok(n):
    return 2 <= n <= SPLIT_MAX and radix_plan(n) is not None


def auto_split(m):
    """dct_split_auto: the largest a <= sqrt(m) with both factors 2-3-5-7-smooth and m / a <= 4096; 0: none."""
    best, a = 0, 2
    while a * a <= m:
        if m % a == 0 and factor_ok(a) and factor_ok(m // a):
            best = a
        a += 1
    return best


def digit_rev(n):
    """Position of sample k in the mixed-radix plan's digit-reversed input order (dct_split_setup's rule)."""
    rad = radix_plan(n)
    out = np.zeros(n, dtype=np.int64)
    for k in range(n):
        r, pos = k, 0
        for st in range(len(rad) - 1, -1, -1):
            pos += (r % rad[st]) * int(np.prod(rad[:st], dtype=np.int64))
            r //= rad[st]
        out[k] = pos
    return out


def plan(mesh, d, a=0):
    """launch_dct_split's shapes for dimension d of mesh: dict with the factors, the column pass's tile (tq lines x C
    columns, nct column tiles, grid_c) and the row pass's (G row pairs of npr a line pair, grid_r); None: no split."""
    m = int(mesh[d])
    a = a or (auto_split(m) if m > SPLIT_MAX else 0)
    if not a:
        return None
    b = m // a
    nlines = int(np.prod(mesh)) // m
    nclt = cdiv(nlines, 2)
    tq = 2 if d == 0 else 16
    while tq > 2 and (tq // 2) * (a + 1) > SLOTS:
        tq //= 2
    cmax = min(b, max(1, SLOTS // ((tq // 2) * (a + 1))))
    nct = cdiv(b, cmax)
    C = cdiv(b, nct)
    npr = a // 2 + 1
    G = min(GMAX, max(1, SLOTS // (2 * (b + 1))))
    return dict(a=a, b=b, tq=tq, C=C, nct=nct, grid_c=cdiv(nlines, tq) * nct, G=G, npr=npr,
                grid_r=cdiv(nclt * npr, G), lds_c=(tq // 2) * C * (a + 1) * 16, lds_r=2 * G * (b + 1) * 16)


def launches(mesh, d, a=0, inverse=False, formb=False):
    """[(kernel, grid, block)] of one split pass along d, in launch order."""
    s = plan(mesh, d, a)
    t = lambda v: "true" if v else "false"   # noqa: E731
    col = (f"k_dsc<{t(inverse)}, {t(d == 0)}, {t(formb and not inverse)}>", s["grid_c"], 512)
    row = (f"k_dsr<{t(inverse)}, {t(d == 0)}>", s["grid_r"], 512)
    return [row, col] if inverse else [col, row]


def solve_launches(mesh, splits, formb=False):
    """The split launches of one spectral solve: forward along the split dims ascending (b formed on load by the
    first pass of the solve, which is dim 0's), then inverse descending. splits: {dim: a} (0 = automatic)."""
    out = []
    for d in sorted(splits):
        out += launches(mesh, d, splits[d], False, formb and d == 0)
    for d in sorted(splits, reverse=True):
        out += launches(mesh, d, splits[d], True)
    return out


# ---- the passes ------------------------------------------------------------------------------------------------------
class Bug:
    """A deliberate index error for the tests with teeth."""
    twiddle_off = 0      # inter-pass twiddle read at n2 k1 + this
    partner_row_off = 0  # the k <-> m - k partner taken from row a - k1 + this
    natural_lam = False  # the dimension's lam table left in natural order


def w4(m, J):
    """e^{-2 pi i J / 4m} rounded to float64 from a long-double evaluation (the kernels' hi + lo product carries its
    rounding errors, so a twiddle is one rounded value)."""
    pi = np.longdouble(4.0) * np.arctan(np.longdouble(1.0))
    J = np.asarray(J, dtype=np.int64)
    hi, lo = J >> 12, J & 4095    # the two table indices; their sum of angles is the angle of J
    ang = -2.0 * pi * ((hi * 4096 + lo) % (4 * m)).astype(np.longdouble) / np.longdouble(4 * m)
    return np.cos(ang).astype(np.float64) + 1j * np.sin(ang).astype(np.float64)


def sub_fft(x, inverse):
    """The length-n FFTs of the LDS stages over the last axis, input gathered through the digit-reversed order and
    back (DIT: reversed in, natural out; DIF inverse: natural in, reversed out, un-reversed by the store)."""
    n = x.shape[-1]
    rev = digit_rev(n)
    if not inverse:
        lds = np.empty_like(x)
        lds[..., rev] = x                      # load: sample k to its digit-reversed place
        return np.fft.fft(lds[..., rev], axis=-1)   # the DIT stages take the reversed order, natural out
    y = np.fft.ifft(x, axis=-1) * n            # unnormalised
    lds = np.empty_like(y)
    lds[..., rev] = y                          # DIF leaves sample n1 at rev[n1]
    return lds[..., rev]                       # the store reads rev[n1]


def forward_pair(xa, xb, a, bug=Bug):
    """Unnormalised DCT-II of the real lines xa, xb (length m = a b) by k_dsc then k_dsr: the coefficients of
    frequency k = k1 + a k2 at position b k1 + k2."""
    m = xa.size
    b = m // a
    n = np.arange(m)
    src = np.where(2 * n < m, 2 * n, 2 * (m - 1 - n) + 1)     # v[n] = x[2n], v[m-1-n] = x[2n+1]
    v = (xa[src] + 1j * xb[src]).reshape(a, b)                # [n1][n2]
    y = sub_fft(v.T, False).T                                 # [k1][n2]: length-a FFTs of the columns
    k1, n2 = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    y = y * w4(m, 4 * (n2 * k1 + bug.twiddle_off))
    Z = sub_fft(y, False)                                     # [k1][k2]: length-b FFTs of the rows
    k2 = n2
    rowp = np.where(k1 == 0, 0, (a - k1 + bug.partner_row_off) % a)
    k2p = np.where(k1 == 0, (b - k2) % b, b - 1 - k2)
    Z2 = Z[rowp, k2p]                                         # Z[m - k]
    q = w4(m, k1 + a * k2)                                    # e^{-i pi k / 2m}
    A = 0.5 * (Z + np.conj(Z2))
    B = -0.5j * (Z - np.conj(Z2))
    return (q * A).real.ravel(), (q * B).real.ravel()


def inverse_pair(Xa, Xb, a):
    """Unnormalised DCT-III (m x the inverse of forward_pair) by k_dsr<INV> then k_dsc<INV>."""
    m = Xa.size
    b = m // a
    k1, k2 = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    rowp = np.where(k1 == 0, 0, a - k1)
    k2p = np.where(k1 == 0, (b - k2) % b, b - 1 - k2)
    k = k1 + a * k2
    qc = np.conj(w4(m, k))

    def V(X):
        X = X.reshape(a, b)
        Xm = np.where(k == 0, 0.0, X[rowp, k2p])              # X[m] = 0
        return qc * (X - 1j * Xm)
    Z = V(Xa) + 1j * V(Xb)
    y = sub_fft(Z, True)                                      # [k1][n2]
    y = y * np.conj(w4(m, 4 * (k2 * k1)))                     # n2 k1 (k2 holds the column index here)
    v = sub_fft(y.T, True).T.ravel()                          # [n1][n2]
    n = np.arange(m)
    src = np.where(2 * n < m, 2 * n, 2 * (m - 1 - n) + 1)
    xa, xb = np.empty(m), np.empty(m)
    xa[src], xb[src] = v.real, v.imag
    return xa, xb


def lam_table(m, a):
    """The dimension's eigenvalues in the order of the forward pass: position b k1 + k2 holds k = k1 + a k2."""
    pos = np.arange(m)
    b = m // a
    return pos // b + a * (pos % b)


def model_solve(mesh, a, deltas, sigma, bvec, bug=Bug):
    """(I + sigma D^T D) x = b on a 2-D mesh: the split passes along dim 0 (line pairs, an unpaired last line with a
    zero partner), the last dimension by float64 cosine transforms with the symbol rows in the split's order."""
    import scipy.fft as sfft
    m0, m1 = mesh
    x = np.asarray(bvec, dtype=np.float64).reshape(mesh, order="F")
    C = np.empty_like(x)
    for j in range(0, m1, 2):
        xb = x[:, j + 1] if j + 1 < m1 else np.zeros(m0)
        ca, cb = forward_pair(x[:, j], xb, a, bug)
        C[:, j] = ca
        if j + 1 < m1:
            C[:, j + 1] = cb
    sym = SLD.dtd_symbol_ld(mesh, deltas, "cpp", True, np.float64)
    order = np.arange(m0) if bug.natural_lam else lam_table(m0, a)
    T = sfft.dct(C, type=2, axis=1, norm="ortho") / (1.0 + sigma * sym[order, :])
    Y = sfft.idct(T, type=2, axis=1, norm="ortho")
    out = np.empty_like(x)
    for j in range(0, m1, 2):
        yb = Y[:, j + 1] if j + 1 < m1 else np.zeros(m0)
        ya, yb = inverse_pair(Y[:, j], yb, a)
        out[:, j] = ya
        if j + 1 < m1:
            out[:, j + 1] = yb
    return out.ravel(order="F") / m0


# ---- tests -----------------------------------------------------------------------------------------------------------
def test_factorisation():
    assert auto_split(8192) == 64 and auto_split(5000) == 50 and auto_split(6561) == 81
    assert auto_split(4608) == 64 and auto_split(8400) == 84 and auto_split(1 << 20) == 1024
    assert auto_split(1 << 24) == 4096 and auto_split(1 << 25) == 0   # a factor would pass 4096
    assert auto_split(4099) == 0 and auto_split(4100) == 0           # a prime factor >= 11
    assert not factor_ok(11) and not factor_ok(8192) and factor_ok(4096) and not factor_ok(1)


def test_digit_reversal_is_a_permutation():
    for n in (2, 6, 8, 64, 81, 84, 100, 125, 4096):
        r = digit_rev(n)
        assert sorted(r) == list(range(n))


@pytest.mark.parametrize("m,a", [(64, 8), (48, 2), (48, 24), (60, 6), (105, 7), (1000, 8), (1000, 125), (45, 5),
                                 (45, 9), (12, 2), (12, 3), (12, 4), (8192, 64), (6561, 81)])
def test_forward_matches_the_cosine_sum_and_the_inverse_undoes_it(m, a):
    rng = np.random.default_rng(m * 31 + a)
    xa, xb = rng.standard_normal(m) + 2.0, rng.standard_normal(m) + 2.0
    import scipy.fft as sfft
    Xa, Xb = forward_pair(xa, xb, a)
    order = lam_table(m, a)
    for X, x in ((Xa, xa), (Xb, xb)):
        ref = 0.5 * sfft.dct(x.astype(np.longdouble), type=2)[order]   # sum x[n] cos(pi (2n + 1) k / 2m)
        assert np.max(np.abs(X - ref)) <= 64 * np.finfo(float).eps * np.max(np.abs(ref))
    ya, yb = inverse_pair(Xa, Xb, a)
    assert np.max(np.abs(ya / m - xa)) <= 1e-13 and np.max(np.abs(yb / m - xb)) <= 1e-13


SOLVES = [([64, 2], 8), ([64, 3], 8), ([48, 40], 2), ([48, 40], 24), ([60, 7], 6), ([105, 4], 7), ([1000, 9], 8),
          ([1000, 9], 125), ([4096, 5], 64), ([8192, 2], 0), ([8192, 3], 0), ([6561, 2], 0), ([5000, 8], 0)]


def _errs(mesh, a, sigma, bug=Bug):
    a = a or auto_split(mesh[0])
    N = int(np.prod(mesh))
    b = np.random.default_rng(2000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in mesh]
    x_ld = SLD.spectral_solve_ld(mesh, deltas, sigma, b, "cpp", True)
    x64 = SLD.spectral_solve_ld(mesh, deltas, sigma, b, "cpp", True, np.float64)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(model_solve(mesh, a, deltas, sigma, b, bug) - x_ld))) / scale
    return err, e64


@pytest.mark.parametrize("sigma", [0.0, 1e-3, 3.7, 2e5])
@pytest.mark.parametrize("mesh,a", SOLVES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_model_solve_forward_error(mesh, a, sigma):
    err, e64 = _errs(mesh, a, sigma)
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


@pytest.mark.parametrize("mesh,a", [([64, 3], 8), ([60, 7], 6), ([8192, 2], 0)], ids=["64x3", "60x7", "8192x2"])
def test_index_errors_are_caught_by_orders_of_magnitude(mesh, a):
    class Tw(Bug):
        twiddle_off = 1

    class Row(Bug):
        partner_row_off = 1

    class Lam(Bug):
        natural_lam = True
    bound = min(RTOL_DIRECT, K_BOUND * _errs(mesh, a, 3.7)[1])
    for bug in (Tw, Row):
        err, _ = _errs(mesh, a, 3.7, bug)
        assert err >= 1e6 * bound, (bug.__name__, err, bound)
    err, _ = _errs(mesh, a, 3.7, Lam)   # a wrong eigenvalue per frequency: large at a sigma where the symbol matters
    assert err >= 1e3 * bound, (err, bound)


def test_shapes_of_the_named_cases():
    """What each case of tests/test_gpu_long_dct.py is for, from the plan alone."""
    s = plan([8192, 2], 0)
    assert (s["a"], s["b"], s["tq"], s["C"], s["nct"], s["grid_c"], s["G"], s["grid_r"]) == (64, 128, 2, 43, 3, 3, 15, 3)
    assert plan([8192, 3], 0)["grid_c"] == 6                       # the unpaired last line has a tile of its own
    assert plan([8192, 600], 0)["grid_c"] == 900 and plan([8192, 600], 0)["grid_r"] == 660
    for m, a in ((4608, 64), (5000, 50), (8400, 84), (6561, 81)):   # every radix between them
        assert plan([m, 2], 0)["a"] == a
    used = set()
    for m in (4608, 5000, 8400):
        s = plan([m, 2], 0)
        used |= set(radix_plan(s["a"]) + radix_plan(s["b"]))
    assert used == {2, 3, 4, 5, 7, 8}
    s = plan([1 << 20, 2], 0)
    assert (s["a"], s["b"], s["C"], s["G"]) == (1024, 1024, 4, 2)
    assert plan([4096, 5], 0, 64)["grid_c"] == 3 * 2                # 64 columns in two tiles of 32 a line pair
    # strided passes: 16 adjacent lines (128-B rows) while a line of a fits, one row pair a workgroup past b = 2051
    assert plan([64, 64, 3], 1, 8)["tq"] == 16 and plan([12, 12, 12, 3], 2, 3)["tq"] == 16
    assert plan([4096, 5], 0, 64)["lds_r"] <= 65536 and plan([8192, 2], 0, 2)["lds_r"] == 2 * 4097 * 16
    assert plan([8192, 3], 0, 4096)["lds_c"] == 4097 * 16 and plan([8192, 3], 0, 4096)["C"] == 1
    assert plan([48, 40], 0) is None and plan([4100, 4100], 0) is None
