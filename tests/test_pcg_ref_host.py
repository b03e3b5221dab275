"""The GPU checks of tests/test_gpu_pcg_scalars.py and tests/test_gpu_stencil_march.py have teeth, shown on the
CPU. No GPU.

PCG side: the k-th iterate of the spectrally preconditioned PCG (tests/pcg_ref.py) in float64 and in long double
agree to 1e-12 of max|x| for k <= 6, and the same float64 run with one 256-cell workgroup's share dropped from p.q is
off by at least 1e-4: the 1e-11 bound of the GPU tests sits between the two with room on both sides (measured: the
gap at most 2e-14, the mutation at least 2e-4).

Operator side: the componentwise bound c u (|W| |x| + sigma a) of tests/stencil_ref.py is violated by one stencil
weight class off by 1e-13 relative and by one tile-edge column that mirrors its right neighbour instead of loading it,
while float64 evaluations of the correct operator (the separable form of oracle/stencil_ld.py and a model of the
kernels' K-weighted class sums) stay within it, the separable one at a ratio of at most 8."""
import functools

import numpy as np
import pytest
import scipy.fft as sfft

import pcg_ref as PR
import stencil_ref as R
from oracle import spectral_ld as SLD
from oracle import stencil_ld as SL

LD = np.longdouble
MESHES = [[270, 41], [40, 40, 36], [12, 12, 12, 40]]
KS = (1, 2, 3, 4, 6)


def dct_solve(m, dtype):
    """solve(s, b) = (I + s D^T D)^-1 b by cosine transforms in ``dtype`` (oracle/spectral_ld.py)"""
    p = len(m)
    sym = SLD.dtd_symbol_ld(m, R.DELTAS[:p], "cpp", True, dtype)
    shape = [int(v) for v in m]

    def solve(s, b):
        t = sfft.dctn(np.asarray(b, dtype=dtype).reshape(shape, order="F"), type=2, norm="ortho")
        t = t / (dtype(1.0) + dtype(s) * sym)
        return sfft.idctn(t, type=2, norm="ortho").ravel(order="F")

    return solve


@functools.lru_cache(maxsize=None)
def _runs(m, kind):
    m = list(m)
    p, n = len(m), int(np.prod(m))
    blocks = R.blocks_of(p)
    W, sigma = (PR.fold_weights(n, 7), 6.0) if kind == "fold" else (PR.count_weights(n, 8), 0.04 if p == 2 else 0.1)
    rng = np.random.default_rng(9)
    x0 = PR.theta0(m, 10)
    b = W * rng.standard_normal(n) + sigma * SL.apply_dtd(m, blocks, x0, dtype=np.float64)
    out = {}
    for dtype in (np.float64, LD):
        A = functools.partial(SL.apply_A, m, blocks, W, sigma, dtype=dtype)
        Minv, scaled = PR.spectral_preconditioner(m, blocks, W, sigma, dct_solve(m, dtype), dtype)
        out[dtype] = PR.pcg_iterates(A, Minv, b.astype(dtype), x0.astype(dtype), max(KS))[0]
        if dtype is np.float64:
            lo_i = (n // 2 // 256) * 256   # one workgroup's 256 consecutive cells, mid-mesh
            drop = lambda pp, qq: pp @ qq - pp[lo_i:lo_i + 256] @ qq[lo_i:lo_i + 256]   # noqa: E731
            out["mutated"] = PR.pcg_iterates(A, Minv, b, x0, max(KS), pq=drop)[0]
    return out, scaled


@pytest.mark.parametrize("kind", ["fold", "counts"])
@pytest.mark.parametrize("m", MESHES, ids=lambda m: "x".join(str(v) for v in m))
def test_iterate_bound_sits_between_rounding_and_a_lost_partial(m, kind):
    out, scaled = _runs(tuple(m), kind)
    assert scaled == (kind == "counts")   # both sides of the std(W) >= 0.1 dbar switch
    for k in KS:
        xl = out[LD][k - 1]
        scale = float(np.max(np.abs(xl)))
        gap = float(np.max(np.abs(out[np.float64][k - 1] - xl))) / scale
        off = float(np.max(np.abs(out["mutated"][k - 1] - xl))) / scale
        print(f"{m} {kind} k={k}: float64 to long double {gap:.2e}, one workgroup's p.q dropped {off:.2e}")
        assert gap <= 1e-12, k
        assert off >= 1e-4, k


# one shape per p with a tile edge inside dim 0 (256 columns for k_apply2d, 64 for k_apply3d / k_apply4d)
TEETH = [([300, 9], 255), ([65, 65, 7], 63), ([65, 65, 65, 2], 63)]


@pytest.mark.parametrize("m,col", TEETH, ids=["p2", "p3", "p4"])
@pytest.mark.parametrize("wkind", ["I", "diag"])
def test_operator_bound_has_teeth(m, col, wkind):
    p = len(m)
    c = R.c_bound(p)
    blocks = R.blocks_of(p)
    x, dtd, a = R.reference(tuple(m))
    W = None if wkind == "I" else R.make_w(m)
    v = R.class_sums(m, x)
    vbad = R.class_sums(m, x, wrong_mirror_col=col)
    for sigma in (0.37, 25.6):
        q64 = SL.apply_A(m, blocks, W, sigma, x, dtype=np.float64)
        r64 = R.ratio(q64, W, sigma, x, dtd, a)[0]
        K = R.stencil_weights(p, blocks, sigma, W is None)
        rk = R.ratio(R.model_apply(K, v, x, W), W, sigma, x, dtd, a)[0]
        least = np.inf
        # a weight class off by 1e-13 relative (900 u): the centre, the dim-0 neighbours, and the corners, whose
        # share of an output is the smallest of all classes
        for t in (0, 1, (1 << p) - 1):
            Kt = K.copy()
            Kt[t] *= 1.0 + 1e-13
            least = min(least, R.ratio(R.model_apply(Kt, v, x, W), W, sigma, x, dtd, a)[0])
        rm = R.ratio(R.model_apply(K, vbad, x, W), W, sigma, x, dtd, a)[0]
        print(f"{m} W={wkind} sigma={sigma}: separable float64 {r64:.2f}, class-sum model {rk:.2f}, bound {c}; "
              f"a weight class + 1e-13: at least {least:.0f}; wrong mirror at column {col}: {rm:.2e}")
        assert r64 <= 8.0
        assert rk <= c
        assert least > c
        assert rm > c
