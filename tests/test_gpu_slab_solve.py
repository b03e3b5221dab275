"""The slab path's line solve, isolated: every k_trisr tile launch_tri_slab can pick, pinned by its launch and checked
against the long-double solve.

The θ-solve of a slab rank is local transforms along dims 0..p-2 around the substructured line solves of the last
dimension: k_trisr<1, ...> (every block's two sums), an all-to-all, k_trisr_iface (the chunk owner's scan over the
ranks with the mirror closure), an all-to-all back, k_trisr<3, ...> (the recursions rerun from the carries). The ADMM
loop tests run it at rho = lambda / 5, where r^n of a block is negligible and a wrong interface is invisible
(tests/test_line_solve_host.py::test_uneven_blocks_see_a_wrong_block_multiplier), and on meshes that reach three of
the twelve instantiations.

Isolating recipe: mvtv_slab_run starts from theta_0 everywhere, u_0 = 0 and g_alpha = D^T D theta_0. With
theta_0 = 0.0 the first right-hand side is exactly O^T y, so one fixed iteration from rho_0 = sigma leaves
theta_1 = (W + sigma D^T D)^-1 O^T y in the resident state (the edge pass that follows does not touch theta), for any
sigma > 0. The ranks are the in-process loopback group, one host thread each, every thread inside its own launch log;
world 1 runs the distributed path under MVTV_SLAB_DISTRIBUTED=1.

Each case of CASES is a mesh, a world size and the (k_trisr template arguments after the phase, grid, block) expected
from every rank, as literals read off launch_tri_slab: lines = prod m_j (j < p - 1), a rank's n owned planes split into
nseg segments of sl rows, phases 1 and 3 on grid ceil(lines / TQ) with TQ * nseg threads, the interface on
ceil((lines / world) / 256) workgroups of 256. Inputs and bound are tests/test_gpu_dispatch.py's: b = randn + 2,
delta_j = (1 + 2e-4) / m_j, C++ block order, max|theta - x_ld| <= min(1e-12, 32 e64) max|x_ld| at
sigma in {1e-3, 3.7, 2e5} (sigma = 0 is refused: rho_0 > 0), x_ld = oracle.spectral_ld in long double and e64 the
error of the same formula in float64.

W = 2 I (W_CASES): the w0 argument of the three kernels. The theta-solve is then PCG whose preconditioner is this line
solve with w0 = mean W = 2, the exact inverse, and theta = (I + (sigma / 2) D^T D)^-1 b; bound 1e-12 of max|x_ld| (the
e64 yardstick does not model the PCG update), pcg_rtol = 1e-13. The PCG repairs a wrong preconditioner at the price of
iterations, so the count is bounded too: at most 2 (reasoning at the assertion; 1 measured).

test_every_k_trisr_instantiation_has_a_case needs no GPU.
"""
import functools
import threading

import numpy as np
import pytest

from conftest import log_parity
from oracle import spectral_ld as S
from test_gpu_dispatch import K_BOUND, RTOL_DIRECT, WORKERS

mv = pytest.importorskip("multivartv_amd")
from multivartv_amd import slab  # noqa: E402
from multivartv_amd._lib import launch_log  # noqa: E402

gpu = pytest.mark.gpu

SIGMAS = (1e-3, 3.7, 2e5)
W_SIGMAS = (1e-3, 3.7)
W0 = 2.0

# (mesh, world, [(k_trisr<PHASE, ...> arguments after the phase, grid, block) per rank; one entry: every rank],
#  grid of k_trisr_iface)
CASES = [
    # ---- 64-line tiles, <= 4 segments of <= 4 rows
    ((96, 96, 16), 4, [("4, 64, 4", 144, 256)], 9),        # 4 planes -> 4 one-row segments
    ((96, 96, 32), 2, [("4, 64, 4", 144, 256)], 18),       # 16 -> 4 x 4: the row registers full
    ((96, 96, 24), 8, [("4, 64, 4", 144, 192)], 5),        # 3 -> 3 x 1; 8-block interface scan, its last workgroup half full
    ((21, 21, 21, 12), 3, [("4, 64, 4", 145, 256)], 13),   # 4-D, 9261 lines: ragged last tile, chunk 3087 cuts tiles
    ((96, 96, 8), 8, [("4, 64, 4", 144, 64)], 5),          # one owned plane: a single one-row segment
    # ---- 64-line tiles, <= 16-row segments, the segment arrays sized 4 / 8 / 16
    ((96, 96, 64), 2, [("16, 64, 4", 144, 256)], 18),      # 32 -> 4 x 8
    ((100, 100, 10), 2, [("16, 64, 8", 157, 320)], 20),    # 5 -> 5 x 1; 10000 lines: ragged tile, chunk 5000 cuts a tile
    ((96, 96, 128), 1, [("16, 64, 8", 144, 512)], 36),     # 128 -> 8 x 16: the row registers full
    ((96, 96, 26), 2, [("16, 64, 16", 144, 832)], 18),     # 13 -> 13 x 1
    ((96, 96, 256), 1, [("16, 64, 16", 144, 1024)], 36),   # 256 -> 16 x 16: the largest wide block
    # ---- uneven blocks: 18 -> 6 x 3 on the wide tile, 19 -> 19 x 1 on the narrow one
    ((96, 96, 37), 2, [("16, 64, 8", 144, 384), ("16, 16, 64", 576, 304)], 18),
    # ---- 16-line tiles
    ((24, 24, 5), 2, [("16, 16, 64", 36, 32), ("16, 16, 64", 36, 48)], 2),   # the shortest uneven blocks: 2 and 3
    ((50, 74), 2, [("16, 16, 64", 4, 592)], 1),            # 2-D, 50 lines: ragged tile, chunk 25; 37 -> 37 x 1
    ((13, 13, 62), 1, [("16, 16, 64", 11, 496)], 1),       # Bluestein leading dims; 62 -> 31 x 2
    ((4, 4, 2112), 2, [("32, 16, 64", 1, 528)], 1),        # 1056 -> 33 x 32: 32-row segments
    ((6, 6, 2050), 2, [("32, 16, 64", 3, 656)], 1),        # 1025 -> 41 x 25, ragged tile
    ((16, 16, 2048), 1, [("32, 16, 64", 16, 1024)], 1),    # 2048 -> 64 x 32: 64 segments, 1024 threads
]
# (24 x 24 x 5: blocks of 2 and 3 planes, where r^n of a block is not negligible even at sigma = 1e-3)
W_CASES = [((96, 96, 64), 2), ((96, 96, 37), 2), ((50, 74), 2), ((24, 24, 5), 2)]

# every instantiation launch_tri_slab can launch
REACHABLE = [f"k_trisr<{ph}, {t}>" for ph in (1, 3)
             for t in ("4, 64, 4", "16, 64, 4", "16, 64, 8", "16, 64, 16", "16, 16, 64", "32, 16, 64")]

_BY_KEY = {(m, world): (tiles, iface) for m, world, tiles, iface in CASES}


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return f"w{v}" if isinstance(v, int) else f"{v:g}"


def _rank_tiles(m, world):
    tiles, _ = _BY_KEY[(m, world)]
    return tiles * world if len(tiles) == 1 else tiles


def expected_log(m, world, rank):
    """the k_trisr launches of one theta-solve on `rank`"""
    args, grid, block = _rank_tiles(m, world)[rank]
    return [(f"k_trisr<1, {args}>", grid, block), ("k_trisr_iface", _BY_KEY[(m, world)][1], 256),
            (f"k_trisr<3, {args}>", grid, block)]


def test_every_k_trisr_instantiation_has_a_case():
    """The union of the kernels the cases pin (each asserts its own against the launch log) is the whole list."""
    assert len(set(REACHABLE)) == len(REACHABLE) == 12
    assert len(_BY_KEY) == len(CASES)
    covered = set()
    for m, world, tiles, _ in CASES:
        assert len(tiles) in (1, world) and int(np.prod(m[:-1])) % world == 0 and m[-1] >= world
        for r in range(world):
            covered |= {n for n, _, _ in expected_log(m, world, r) if n != "k_trisr_iface"}
    assert covered == set(REACHABLE), sorted(set(REACHABLE) - covered) + sorted(covered - set(REACHABLE))
    assert all(k in _BY_KEY for k in W_CASES)


def _deltas(m):
    return [(1.0 + 2e-4) / v for v in m]


@functools.lru_cache(maxsize=1)
def _reference(m):
    """b and the forward transforms and symbols of the long-double reference and of its float64 evaluation: once per
    mesh (the parameters run mesh-major), shared by every sigma and left unchanged."""
    N = int(np.prod(m))
    b = np.random.default_rng(len(m) * 1000003 + N).standard_normal(N) + 2.0
    b.setflags(write=False)
    ref = {}
    for name, dtype in (("ld", np.longdouble), ("f64", np.float64)):
        ref[name] = (S.forward_ld(m, b, dtype, workers=WORKERS), S.dtd_symbol_ld(m, _deltas(m), "cpp", True, dtype))
    return b, ref


def _errors(m, sigma, theta):
    """(e64, the GPU's error), both relative to max|x_ld|"""
    b, ref = _reference(m)
    x_ld = S.solve_from_forward(*ref["ld"], sigma, workers=WORKERS)
    x64 = S.solve_from_forward(*ref["f64"], sigma, workers=WORKERS)
    scale = float(np.max(np.abs(x_ld)))
    assert scale >= abs(float(b.mean())) * (1.0 - 1e-12)   # the mean of b passes through unchanged
    return float(np.max(np.abs(x64 - x_ld))) / scale, float(np.max(np.abs(theta - x_ld))) / scale


def solve(m, world, sigma, w0=None, **run_kw):
    """One theta-solve on every rank of a loopback group: (stats, k_trisr launches) per rank and theta assembled from
    the owned planes. The caller sets MVTV_SLAB_DISTRIBUTED at world 1."""
    b, _ = _reference(m)
    comms = slab.Comm.local_group(world)
    zb = slab.plane_bounds(int(m[-1]), world)
    pl = int(np.prod(m[:-1]))
    own = [b[zb[r] * pl:zb[r + 1] * pl] for r in range(world)]
    if w0 is None:
        ranks = [slab.SlabADMM(list(m), own[r], _deltas(m), 0.0, comms[r], device=0) for r in range(world)]
    else:
        ranks = [slab.SlabADMM(list(m), w0 * own[r], _deltas(m), 0.0, comms[r], device=0,
                               w_owned=np.full(own[r].size, w0)) for r in range(world)]
    out, err = [None] * world, [None] * world

    def work(r):
        try:
            with launch_log() as log:
                st = ranks[r].run(1.0, rho0=sigma, fixed_iters=1, **run_kw)
            assert log and not log[0][0].startswith("#"), log[:1]
            assert all(g[1:] == (1, 1) and bl[1:] == (1, 1) for _, g, bl in log)
            out[r] = (st, [(n, g[0], bl[0]) for n, g, bl in log if n.startswith("k_trisr")])
        except Exception as e:   # noqa: BLE001 (re-raised below)
            err[r] = e

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    theta = None
    if not any(err):
        theta = np.concatenate([s.theta_owned() for s in ranks])
    for s in ranks:
        s.close()
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    return out, theta


def _set_world(monkeypatch, world):
    if world == 1:
        monkeypatch.setenv("MVTV_SLAB_DISTRIBUTED", "1")
    else:
        monkeypatch.delenv("MVTV_SLAB_DISTRIBUTED", raising=False)


def _kernels(m, world):
    return " | ".join(sorted({n for r in range(world) for n, _, _ in expected_log(m, world, r)}))


@gpu
@pytest.mark.parametrize("m,world,sigma", [(m, w, s) for m, w, _, _ in CASES for s in SIGMAS], ids=_id)
def test_launches_and_forward_error(m, world, sigma, monkeypatch):
    _set_world(monkeypatch, world)
    out, theta = solve(m, world, sigma)
    for r, (st, log) in enumerate(out):
        assert st["iters"] == 1 and st["theta_solver"] == mv.SOLVER_SPECTRAL, (r, st)
        assert log == expected_log(m, world, r), (r, log)
    e64, err = _errors(m, sigma, theta)
    print(f"slab solve {_id(m)} w{world} sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e} ratio {err / max(e64, 1e-300):.1f}")
    log_parity(f"slab solve {_id(m)} w{world} sigma={sigma:g}", e64=e64, err=err, kernels=_kernels(m, world))
    assert err <= min(RTOL_DIRECT, K_BOUND * e64), (err, e64)


@gpu
@pytest.mark.parametrize("m,world,sigma", [(m, w, s) for m, w in W_CASES for s in W_SIGMAS], ids=_id)
def test_w0_through_the_pcg_preconditioner(m, world, sigma, monkeypatch):
    """W = 2 I: w_std = 0, so the unscaled PCG runs and its preconditioner, the slab line solve with w0 = 2, is the
    exact inverse of the operator."""
    _set_world(monkeypatch, world)
    out, theta = solve(m, world, sigma, w0=W0, pcg_rtol=1e-13)
    for r, (st, log) in enumerate(out):
        assert st["iters"] == 1 and st["theta_solver"] == mv.SOLVER_PCG_SPECTRAL, (r, st)
        assert st["pcg_iters"] >= 1 and st["pcg_unconverged"] == 0, (r, st)
        want = expected_log(m, world, r)   # every preconditioner solve launches the same three
        assert len(log) >= 3 and len(log) % 3 == 0 and log == want * (len(log) // 3), (r, log[:6])
    e64, err = _errors(m, sigma / W0, theta)
    pcg_iters = int(out[0][0]["pcg_iters"])
    print(f"slab solve W=2I {_id(m)} w{world} sigma {sigma:g}: e64 {e64:.2e} gpu {err:.2e} "
          f"ratio {err / max(e64, 1e-300):.1f} pcg_iters {pcg_iters}")
    log_parity(f"slab solve W=2I {_id(m)} w{world} sigma={sigma:g}", e64=e64, err=err,
               ratio=err / max(e64, 1e-300), pcg_iters=pcg_iters, kernels=_kernels(m, world))
    assert err <= RTOL_DIRECT, (err, e64)
    # The PCG absorbs a wrong preconditioner into more iterations, so theta alone cannot show one. An exact inverse
    # known to a relative error eps_M contracts the residual by about cond * eps_M per iteration. A line solve within
    # the bound of test_launches_and_forward_error has eps_M <= 32 e64 < 6e-14 (e64 < 1.7e-15 on these meshes), and
    # cond = 1 + (sigma / 2) max sym < 120 here (asserted), so one iteration leaves at most 7e-12 of the residual and
    # two 5e-23, below pcg_rtol = 1e-13; a preconditioner off by 1e-7 would need three.
    sym_max = float(np.max(_reference(m)[1]["f64"][1]))
    assert 1.0 + sigma / W0 * sym_max < 120.0 and K_BOUND * e64 < 6e-14, (sym_max, e64)
    assert all(st["pcg_iters"] <= 2 for st, _ in out), [st["pcg_iters"] for st, _ in out]
