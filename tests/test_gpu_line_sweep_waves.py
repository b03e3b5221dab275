"""The marching line sweeps (k_sweep) at the chunk shapes where the plane prefetch and the up sweep's
two-level exponent take another path.

Meshes 512 x 512 x m_2 with forced sweeps, `P.line_sweep(1, chunks)`, as tests/test_gpu_line_sweep.py. The cases:
chunks of 3 planes and of 1 plane (a chunk whose prefetch has no next plane, a chunk that is its own top and bottom),
chunks of 9, 8 | 9 and 16 | 17 planes (the exponent hi - i = 8 a + b starts on, one past and two multiples past a
multiple of 8: Bin reloaded in the first step, in the second, twice), a chunk of 15 planes (the chunk starts at b = 7,
where the step's own rebuild must rest), and chunks of 65 planes (a >= 8, longer than the 64 of the 512^3 benchmark).
sigma = 1e-40 makes r about 1e-40, so r^8 underflows inside the powering; sigma = 0 makes r = 0.

Forward error as tests/test_gpu_line_sweep.py::test_forced_sweeps_forward_error: b = randn + 2, delta = (1 + 2e-4) / m,
against the long-double reference oracle/spectral_ld.py with the bound min(1e-12, 32 e64), e64 from the float64
evaluation of the same formula. Every case is solved twice and the two results must agree bit for bit: the exchange
buffer's slots are written and read by different threads between barriers, and Bin's reload lands in registers a
step after it is issued, so a missing barrier or wait shows as a difference between two runs before it shows as an
error above the bound.
"""
import functools
import os

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd._lib import launch_log  # noqa: E402

pytestmark = pytest.mark.gpu

K_BOUND = 32.0
RTOL_DIRECT = 1e-12
SIGMAS = (0.0, 1e-40, 3.7, 2e5)
WORKERS = min(16, os.cpu_count() or 1)
M01 = 512

# (m_2, chunks)
CASES = [(3, 1), (3, 3), (9, 1), (15, 1), (17, 2), (33, 2), (130, 2)]

DOWN, IFACE, UP = "k_sweep<9, false>", "k_trisr_iface", "k_sweep<9, true>"


@functools.lru_cache(maxsize=1)
def _case(m2):
    """one mesh's problem, right-hand side and the references' forward transforms and symbols"""
    m = (M01, M01, m2)
    N = int(np.prod(m))
    b = np.random.default_rng(3 * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP)
    assert P.spectral_ok()
    ref = {}
    for name, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[name] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, 0, True, dtype))
    return P, b, ref


@functools.lru_cache(maxsize=4)
def _reference(m2, sigma):
    """x_ld, its scale and e64 of one mesh and sigma, shared by the mesh's chunk counts"""
    _, _, ref = _case(m2)
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    x_ld.setflags(write=False)
    return x_ld, scale, e64


@pytest.mark.parametrize("sigma", SIGMAS, ids=lambda s: f"{s:g}")
@pytest.mark.parametrize("m2,chunks", CASES, ids=lambda v: str(v))
def test_sweeps_forward_error_and_repeat(m2, chunks, sigma):
    P, b, _ = _case(m2)
    P.line_sweep(1, chunks)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    names = [n for n, _, _ in log]
    assert names[1:4] == [DOWN, IFACE, UP], names
    for k in (1, 3):
        assert log[k][1] == ((M01 // 16) * chunks, 1, 1) and log[k][2] == (512, 1, 1), log[k]
    x2 = P.solve_spectral(sigma, b)
    x_ld, scale, e64 = _reference(m2, sigma)
    err = float(np.max(np.abs(x - x_ld))) / scale
    nd = int(np.count_nonzero(x.view(np.uint64) != x2.view(np.uint64)))
    print(f"two-level sweep 512x512x{m2} chunks {chunks} sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e} "
          f"ratio {err / max(e64, 1e-300):.1f}, words differing between two solves {nd}")
    log_parity(f"two-level sweep 512x512x{m2} C={chunks} sigma={sigma:g}", e64=e64, err=err, repeat_diff=nd)
    assert nd == 0
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)
