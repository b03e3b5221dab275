"""The marching stencil operators (k_apply2d / k_apply3d / k_apply3d2 / k_apply4d, mvtv_cg3d.hip) against the
long-double W + sigma D^T D (oracle/stencil_ld.py), in the launch configurations the real runs use: several in-plane
tiles, partial tiles of one column or one lane, chunks of the marched dimension of two and three planes with a ragged
last one (the carried s1m / s0c / s1c, the z0 > 0 reload of plane z0 - 1), grids padded for the XCD remap, W = I
(the centre weight + 1) and W with zeros. The shapes and what each is for: tests/test_stencil_tiling_host.py.

Every Problem.apply_A call must be one launch of the expected instantiation with the transcribed grid, and its output
must satisfy, componentwise,

    |q_gpu - q_ld| <= c u (|W| |x| + sigma a),   c = 2 (3^p + 2^p + p + 4),   u = 2^-53

(derivation and a: tests/stencil_ref.py; the bound's teeth: tests/test_pcg_ref_host.py) and the suite's RTOL_OP of
max|q|. The largest ratio to u (|W| |x| + sigma a) per case goes to $MVTV_PARITY_LOG."""
import numpy as np
import pytest

import stencil_ref as R
import test_stencil_tiling_host as T
from conftest import log_parity

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL_OP = 1e-13   # test_gpu_parity.RTOL_OP
SIGMAS = (0.0, 0.37, 25.6)
# the launch log's names, read from a logged run: the first template argument is the WMode (0 W_NONE, which W = I
# takes with + 1 on the centre weight; 2 W_DIAG), the second DOT
WMODE_ARG = {"I": 0, "diag": 2}

# (case of test_stencil_tiling_host.CASES, block order, unit weights): every case in cpp order with the deltas of
# stencil_ref.DELTAS, and one per p in py order (no all-ones block) and one with unit weights
RUNS = [(name, "cpp", False) for name in T.CASES] + \
       [("2d-a", "py", False), ("3d2-b", "py", False), ("4d-c", "py", False),
        ("2d-b", "cpp", True), ("3d1-a", "cpp", True), ("4d-a", "cpp", True)]


def _sigmas(m):
    """every mesh at least two of the project's sigmas; all three below a million nodes"""
    return SIGMAS if int(np.prod(m)) <= 1_000_000 else SIGMAS[1:]


@pytest.mark.parametrize("wkind", ["I", "diag"])
@pytest.mark.parametrize("name,order,unit", RUNS, ids=[f"{n}-{o}{'-unit' if u else ''}" for n, o, u in RUNS])
def test_marching_operator(name, order, unit, wkind):
    m = T.CASES[name]
    p = len(m)
    x, dtd, a = R.reference(tuple(m), order, unit)
    W = None if wkind == "I" else R.make_w(m)
    kernel = f"{T.kernel_of(m)}<{WMODE_ARG[wkind]}, false>"
    grid = T.tiling(m)[5]
    c = R.c_bound(p)
    worst = {}
    with mv.Problem(m, np.zeros(x.size), wdiag=W, deltas=R.DELTAS[:p],
                    order=mv.ORDER_CPP if order == "cpp" else mv.ORDER_PY, weighted=not unit) as P:
        for sigma in _sigmas(m):
            with launch_log() as log:
                q = P.apply_A(sigma, x)
            assert [(n, g[0], b[0]) for n, g, b in log] == [(kernel, grid, 256)], sigma
            ratio, qmax, emax = R.ratio(q, W, sigma, x, dtd, a)
            print(f"{name} {order} unit={unit} W={wkind} sigma={sigma}: ratio to u {ratio:.3f} (bound {c}), "
                  f"max err / max|q| {emax / qmax:.3e}")
            worst[f"ratio_s{sigma:g}"] = ratio
            assert ratio <= c, sigma
            assert emax <= RTOL_OP * qmax, sigma
    log_parity(f"stencil_march/{name}/{order}{'/unit' if unit else ''}/W={wkind}", bound=c, **worst)
