"""The marching line sweeps of the 3-D spectral solve (k_sweep) in checked tests.

Meshes. A 3-D problem needs m_0 = m_1 (the mixed-partial rule, tests/test_gpu_parity.py::test_dim_mismatch_raises) and
every m_j >= 2, and the sweeps are instantiated for m_1 = 512, so every mesh here is 512 x 512 x m_2: 32 tiles a
plane. The cases vary what the sweeps add, the planes of dim 2 and their chunks: degenerate lines whose chunk's top plane
is its bottom (m_2 = 2 with 1 and 2 chunks), chunks of 2, 2, 3 planes (7 / 3), every plane a chunk (40 / 40), uneven
chunks (33 with 1, 4, 16) and the cost model's own count on a mesh that cannot fill the GPU (33 / 0).

Forward error as tests/test_gpu_dispatch.py: b = randn + 2, delta = (1 + 2e-4) / m, against the long-double reference
oracle/spectral_ld.py with the bound min(1e-12, 32 e64), e64 from the float64 evaluation of the same formula.
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
SIGMAS = (0.0, 1e-3, 3.7, 2e5)
WORKERS = min(16, os.cpu_count() or 1)
M01 = 512

# (m_2, chunks): line_sweep(1, chunks)
FORCED = [(2, 1), (2, 2), (7, 3), (40, 40), (33, 1), (33, 4), (33, 16), (33, 0)]

DOWN, IFACE, UP = "k_sweep<9, false>", "k_trisr_iface", "k_sweep<9, true>"


def _names(log):
    return [n for n, _, _ in log]


def check_old_log(log):
    """the five-pass solve: dim-0 forward, strided dim-1 forward, the dim-2 line solve, dim-1 inverse, dim-0 inverse"""
    names = _names(log)
    assert len(names) == 5, names
    assert names[0].startswith("k_dct8<9, 0, true, false,") and names[4].startswith("k_dct8<9, 1, true, false,"), names
    assert names[1].startswith("k_dct8<9, 0, false, false,") and names[3].startswith("k_dct8<9, 1, false, false,"), names
    assert names[2].startswith(("k_trir<", "k_trigr<", "k_dct")), names
    assert not any(n.startswith("k_sweep") for n in names)


def check_sweep_log(log, old, chunks=None):
    """first pass, down sweep, interface, up sweep, dim-0 inverse; the two dim-0 passes as the five-pass solve's"""
    names = _names(log)
    assert names == [old[0][0], DOWN, IFACE, UP, old[4][0]], names
    assert log[0][1:] == old[0][1:] and log[4][1:] == old[4][1:]
    for k in (1, 3):
        assert log[k][2] == (512, 1, 1) and log[k][1][1:] == (1, 1) and log[k][1][0] % (M01 // 16) == 0, log[k]
        if chunks:
            assert log[k][1][0] == (M01 // 16) * chunks, log[k]
    assert log[1][1] == log[3][1]
    assert log[2][1] == (M01 * M01 // 256, 1, 1) and log[2][2] == (256, 1, 1), log[2]
    return log[1][1][0] // (M01 // 16)


@functools.lru_cache(maxsize=1)
def _case(m2):
    """one mesh's problem, right-hand side, references' forward transforms and symbols, and its five-pass launch log"""
    m = (M01, M01, m2)
    N = int(np.prod(m))
    b = np.random.default_rng(3 * 1000003 + N).standard_normal(N) + 2.0
    deltas = [(1.0 + 2e-4) / v for v in m]
    P = mv.Problem(list(m), b, deltas=deltas, order=mv.ORDER_CPP)
    assert P.spectral_ok()
    ref = {}
    for name, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[name] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, deltas, 0, True, dtype))
    P.line_sweep(0)
    with launch_log() as old:
        P.solve_spectral(1e-3, b)
    check_old_log(old)
    return P, b, ref, list(old)


@pytest.mark.parametrize("sigma", SIGMAS, ids=lambda s: f"{s:g}")
@pytest.mark.parametrize("m2,chunks", FORCED, ids=lambda v: str(v))
def test_forced_sweeps_forward_error(m2, chunks, sigma):
    P, b, ref, old = _case(m2)
    P.line_sweep(1, chunks)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    used = check_sweep_log(log, old, chunks or None)
    assert 1 <= used <= m2
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    e64 = float(np.max(np.abs(x64 - x_ld))) / scale
    err = float(np.max(np.abs(x - x_ld))) / scale
    print(f"line sweep 512x512x{m2} chunks {chunks} ({used}) sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e} "
          f"ratio {err / max(e64, 1e-300):.1f}")
    log_parity(f"line sweep 512x512x{m2} C={used} sigma={sigma:g}", e64=e64, err=err)
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


def test_sweeps_off_is_the_five_pass_log():
    P, b, _, old = _case(33)
    P.line_sweep(1, 4)
    P.line_sweep(0)
    with launch_log() as log:
        P.solve_spectral(3.7, b)
    check_old_log(log)
    assert [(n, g, bl) for n, g, bl in log] == [(n, g, bl) for n, g, bl in old]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


ADMM_M = [M01, M01, 12]
ADMM_LAM, ADMM_RHO0, ADMM_ITERS = 0.8, 0.004, 4   # rho0 = lam / 200: adapt_step doubles rho in the first iterations


def test_sweeps_in_admm_loop():
    """W = I, 4 fixed iterations from a rho0 that adapt_step changes, sweeps forced (3 chunks), against the C oracle's
    loop with scipy.fft's exact solve (tests/test_gpu_dispatch.py::test_first_pass_in_admm_loop): rho exact, theta and
    u to 1e-10; and against the same run without the sweeps: rho exact, theta to 1e-12 max|theta|."""
    from multivartv_amd.synth import towers
    from oracle import c_oracle
    m = ADMM_M
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(y.size, y.mean())
    out = {}
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        assert P.spectral_ok()
        for mode in (1, 0):
            P.line_sweep(mode, 3 if mode else 0)
            P.state_set(th0, None, ADMM_RHO0)
            with launch_log() as log:
                st = P.run(ADMM_LAM, fixed_iters=ADMM_ITERS)
            assert st["theta_solver"] == mv.SOLVER_SPECTRAL and st["iters"] == ADMM_ITERS
            names = _names(log)
            if mode:
                assert names.count(DOWN) >= ADMM_ITERS and names.count(DOWN) == names.count(UP) == names.count(IFACE)
                assert not any(n.startswith("k_trir") or n.startswith("k_dct8<9, 0, false") for n in names), set(names)
            else:
                assert not any(n.startswith("k_sweep") for n in names)
            out[mode] = P.state_get(want_u=True)
    (tg, ug, rg), (t0, _, r0) = out[1], out[0]
    th, u = th0.copy(), np.zeros(c_oracle.num_edges(m))
    ref = c_oracle.admm_rcpp_spectral(m, y, ADMM_LAM, th, u, ADMM_RHO0, deltas, fixed_iters=ADMM_ITERS, workers=WORKERS)
    assert ref["rho"] != ADMM_RHO0
    assert rg == ref["rho"] and r0 == ref["rho"]
    et, eu = _rel(tg, th), float(np.max(np.abs(ug - u)) / max(1.0, np.max(np.abs(u))))
    e0 = _rel(tg, t0)
    print(f"line sweep admm: theta {et:.2e} u {eu:.2e} against the oracle, theta {e0:.2e} against the five-pass solve")
    log_parity("line sweep admm 512x512x12", theta=et, u=eu, theta_vs_off=e0)
    assert et <= 1e-10
    assert eu <= 1e-10
    assert e0 <= 1e-12


def test_sweeps_as_pcg_preconditioner():
    """W = a 0 / 1 fold mask: PCG with the cosine-transform preconditioner, w0 = mean(W); the sweeps run inside it.
    Against the same run without them: the PCG iteration count within 1, theta to 1e-9 max|theta|."""
    from multivartv_amd.synth import towers
    m = ADMM_M
    y = towers(m, seed=3)
    W = (np.random.default_rng(3).permutation(y.size) % 5 != 0).astype(float)
    oty = W * y
    deltas = [(1.0 + 2e-4) / v for v in m]
    th0 = np.full(W.size, oty.sum() / W.sum())
    out = {}
    with mv.Problem(m, oty, wdiag=W, deltas=deltas, order=mv.ORDER_CPP) as P:
        for mode in (1, 0):
            P.line_sweep(mode, 3 if mode else 0)
            with launch_log() as log:
                tg, ug, rg, st = P.admm(0.5, th0, u=np.zeros(P.E), rho=0.1, fixed_iters=2, pcg_rtol=1e-13,
                                        theta_solver=mv.SOLVER_PCG_SPECTRAL)
            assert st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL and st["pcg_unconverged"] == 0
            names = _names(log)
            assert (names.count(DOWN) > 0) == bool(mode) and names.count(DOWN) == names.count(UP)
            assert mode == 0 or not any(n.startswith("k_trir") for n in names)
            out[mode] = (tg, rg, int(st["pcg_iters"]))
    (t1, r1, n1), (t0, r0, n0) = out[1], out[0]
    e = _rel(t1, t0)
    print(f"line sweep pcg: iterations {n1} / {n0}, theta {e:.2e}")
    log_parity("line sweep pcg 512x512x12", theta=e, pcg_iters=n1, pcg_iters_off=n0)
    assert r1 == r0
    assert abs(n1 - n0) <= 1
    assert e <= 1e-9


@pytest.mark.parametrize("sigma", (1e-3, 2e5), ids=lambda s: f"{s:g}")
def test_auto_gate_on_past_2_24_nodes(sigma):
    """512 x 512 x 128 = 2^25 nodes, the smallest power-of-two mesh past the bound: the default mode takes the sweeps;
    x agrees with the five-pass solve of the same problem to 1e-12 max|x|."""
    P, b = _big()
    P.line_sweep(0)
    with launch_log() as old:
        x0 = P.solve_spectral(sigma, b)
    check_old_log(old)
    P.line_sweep(-1)
    with launch_log() as log:
        x = P.solve_spectral(sigma, b)
    used = check_sweep_log(log, list(old))
    assert 128 // used >= 8
    e = _rel(x, x0)
    print(f"line sweep auto 512x512x128 sigma {sigma:g}: {used} chunks, against the five-pass solve {e:.2e}")
    log_parity(f"line sweep auto 512x512x128 sigma={sigma:g}", x_vs_off=e, chunks=used)
    assert e <= 1e-12


@functools.lru_cache(maxsize=1)
def _big():
    m = [M01, M01, 128]
    N = int(np.prod(m))
    b = np.random.default_rng(7).standard_normal(N) + 2.0
    return mv.Problem(m, b, deltas=[(1.0 + 2e-4) / v for v in m], order=mv.ORDER_CPP), b


def test_auto_gate_off_at_2_24_nodes():
    m = [M01, M01, 64]
    N = int(np.prod(m))
    b = np.random.default_rng(8).standard_normal(N) + 2.0
    with mv.Problem(m, b, deltas=[(1.0 + 2e-4) / v for v in m], order=mv.ORDER_CPP) as P:
        with launch_log() as log:
            P.solve_spectral(3.7, b)
        check_old_log(log)
        P.line_sweep(1)
        with launch_log() as log2:
            P.solve_spectral(3.7, b)
        check_sweep_log(log2, list(log))
