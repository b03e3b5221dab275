"""The ADMM loop of mvtv_admm.cpp (one iteration body shared by the device-controlled loop, the host-controlled loop
and the slab loop of mvtv_slab.cpp) on the smallest meshes that reach each branch of its edge pass.

(a) test_resumed_run_against_reference: both one-GPU loops (the device-controlled one, and the host-controlled one
under MVTV_ADMM_SYNC=1) against the CPU references, in two calls: admm(fixed_iters=3), an odd count, so the run ends on
the swapped parity of the D^T u and z ping-pongs, then run(fixed_iters=2) with no state_set, which starts from the z
form of u and the kept D^T u (state_get does not see that buffer: only the resumed run shows whether the epilogue left
it in the right place). Meshes: [37] (k_edge_update + k_gather), [12, 10] (k_admm2d), [8, 8, 11] (k_admm3a),
[5, 5, 5, 6] (k_admm4a + k_gather4b), asserted from the launch log. Data towers(m), delta_j = (1 + 2e-4) / m_j, C++
block order, theta_0 = mean y. Variants: A at lambda = 300 (rho 300 -> 30 -> 3 inside the first call), B at
lambda = 0.5 from rho_0 = 0.01 (rho doubles in the first iterations), C at tune = 2. References, chained the same way
from their own first call: oracle/variants_spectral.py for A and C, the C oracle's loop for B (theta, u and rho carried
over). Bounds (test_gpu_variants_fused.py): iterations and rho exactly, theta to 1e-9 of max|theta_ref|, u to 1e-9 of
max(1, max|u_ref|). Before any GPU comparison the references alone must show that no adaptation decision sits within
1e-6 (relative) of its threshold: A's adapt_hi / adapt_lo, and for B r / s against 10 and 1 / 10 after every iteration
(prefix runs of the C oracle). Measured on one MI355X over the 24 cases: theta within 6.1e-14, u within 1.3e-13, the
same figures before and after the loop moved to mvtv_admm.cpp.

(b) test_launch_sequence_and_timing_table: the kernel launches of a 3-iteration variant-B run (name with template
arguments, block, and grid where the launcher does not size it by the CU count) and the `launches` column of the
per-kernel timing table, entry for entry against a table recorded from the library of the commit before the loop was
rewritten (PARENT). Configurations: the four meshes under both one-GPU loops; [8, 8, 11] and [5, 5, 5, 6] as a slab
group of one rank, [12, 10] as a slab group of two (a ghosted 2-D slab takes the generic edge update and gather with
the z halo between them). The launch log belongs to the calling thread and the timing table to a rank's problem, so
the slab cases drive the ranks as slab.run_local_group does (loopback transport, one host thread per rank) with the
log and the timing switched on inside each thread.
"""
import functools
import threading

import numpy as np
import pytest

from conftest import log_parity

mv = pytest.importorskip("multivartv_amd")
c_oracle = pytest.importorskip("oracle.c_oracle")
from multivartv_amd import slab  # noqa: E402
from multivartv_amd._lib import launch_log  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402
from oracle import variants_spectral as V  # noqa: E402

gpu = pytest.mark.gpu

MESHES = {(37,): ("k_edge_update<", "k_gather<"), (12, 10): ("k_admm2d<",), (8, 8, 11): ("k_admm3a<",),
          (5, 5, 5, 6): ("k_admm4a<", "k_gather4b<")}
LOOPS = ("device", "host")
LAM = {"A": 300.0, "B": 0.5, "C": 2.0}
RHO0_B = 0.01
MARGIN = 1e-6
N1, N2 = 3, 2   # iterations of the first call (odd) and of the resumed one


def _mid(m):
    return "x".join(map(str, m))


def _deltas(m):
    return [(1.0 + 2e-4) / v for v in m]


@functools.lru_cache(maxsize=None)
def _data(m):
    y = towers(list(m))
    y.setflags(write=False)
    return y, float(y.mean())


def _margin(value, threshold):
    return abs(value / threshold - 1.0) if np.isfinite(value) else np.inf


def _b_call(m, y, th, u, rho, n):
    """n iterations of the C oracle's variant-B loop from (th, u, rho); the margins of every adaptation decision from
    its prefix runs of 1 .. n iterations."""
    margins, out = [], None
    for k in range(1, n + 1):
        t, v = th.copy(), u.copy()
        rs = c_oracle.admm_rcpp(list(m), y, LAM["B"], t, v, rho, _deltas(m), fixed_iters=k, pcg_rtol=1e-13)
        ratio = rs["r_norm"] / rs["s_norm"] if rs["s_norm"] > 0.0 else np.inf
        margins += [_margin(ratio, 10.0), _margin(ratio, 0.1)]
        out = (t, v, rs["rho"], rs["iters"])
    return out, margins


@functools.lru_cache(maxsize=None)
def _reference(m, variant):
    """((theta, u, rho, iters) after the first call, the same after the resumed one), computed once per mesh and
    variant and shared by both loops; the conditions on the reference alone are asserted here."""
    y, ymean = _data(m)
    th0 = np.full(y.size, ymean)
    if variant == "B":
        first, mg1 = _b_call(m, y, th0, np.zeros(c_oracle.num_edges(list(m))), RHO0_B, N1)
        second, mg2 = _b_call(m, y, first[0], first[1], first[2], N2)
        assert min(mg1 + mg2) >= MARGIN, (mg1, mg2)
        assert first[2] > RHO0_B, first[2]   # rho did rise inside the first call
    else:
        fn = V.admm_cpp_spectral if variant == "A" else V.admm_py_spectral
        r1 = fn(list(m), y, LAM[variant], th0, ymean, _deltas(m), order="cpp", fixed_iters=N1)
        r2 = fn(list(m), y, LAM[variant], r1.theta, ymean, _deltas(m), order="cpp", fixed_iters=N2, u0=r1.u)
        if variant == "A":
            mg = [min(h["adapt_hi"], h["adapt_lo"]) for h in r1.history + r2.history]
            assert min(mg) >= MARGIN, mg
            assert r1.rho <= 3.0, r1.history   # rho did fall inside the first call (300 -> 30 -> 3, some meshes -> 0)
        first, second = (r1.theta, r1.u, r1.rho, r1.iters), (r2.theta, r2.u, r2.rho, r2.iters)
    for part in first[:2] + second[:2]:
        part.setflags(write=False)
    return first, second


def _errors(th, u, ref):
    return (float(np.max(np.abs(th - ref[0])) / np.max(np.abs(ref[0]))),
            float(np.max(np.abs(u - ref[1])) / max(1.0, np.max(np.abs(ref[1])))))


@gpu
@pytest.mark.parametrize("variant", ("A", "B", "C"))
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("m", list(MESHES), ids=_mid)
def test_resumed_run_against_reference(m, loop, variant, monkeypatch):
    first, second = _reference(m, variant)
    if loop == "host":
        monkeypatch.setenv("MVTV_ADMM_SYNC", "1")
    else:
        monkeypatch.delenv("MVTV_ADMM_SYNC", raising=False)
    y, ymean = _data(m)
    th0 = np.full(y.size, ymean)
    lam = LAM[variant]
    code = {"A": mv.VARIANT_CPP, "B": mv.VARIANT_RCPP, "C": mv.VARIANT_PY}[variant]
    kw = dict(variant=code) if variant == "B" else dict(variant=code, ymean=ymean)
    with mv.Problem(list(m), y, deltas=_deltas(m), order=mv.ORDER_CPP) as P:
        with launch_log() as log:
            if variant == "B":
                th1, u1, rho1, st1 = P.admm(lam, th0, u=np.zeros(P.E), rho=RHO0_B, fixed_iters=N1, **kw)
            else:
                th1, u1, rho1, st1 = P.admm(lam, th0, fixed_iters=N1, **kw)
            st2 = P.run(lam, fixed_iters=N2, **kw)
            th2, u2, rho2 = P.state_get()
    assert log and not log[0][0].startswith("#"), log[:1]
    names = {n for n, _, _ in log}
    for prefix in MESHES[m]:
        assert any(n.startswith(prefix) for n in names), (prefix, sorted(names))
    assert st1["theta_solver"] == st2["theta_solver"] == mv.SOLVER_SPECTRAL

    e1, e2 = _errors(th1, u1, first), _errors(th2, u2, second)
    rec = dict(theta_first=e1[0], u_first=e1[1], theta_resumed=e2[0], u_resumed=e2[1], rho_first=float(first[2]),
               rho_resumed=float(second[2]))
    print(_mid(m), loop, variant, rec)
    log_parity(f"admm loops {_mid(m)}-{loop}-{variant}", **rec)
    assert st1["iters"] == first[3] == N1 and st2["iters"] == second[3] == N2
    assert rho1 == first[2] and st1["rho"] == first[2]
    assert rho2 == second[2] and st2["rho"] == second[2]
    assert e1[0] <= 1e-9 and e1[1] <= 1e-9, e1
    assert e2[0] <= 1e-9 and e2[1] <= 1e-9, e2


# ------------------------------------------------------------------------------ (b) launches and the timing table
CU_SIZED = ("k_admm3a<", "k_plane8<")   # launchers that size the grid by the device's CU count: grid not compared
CONFIGS = ([("one", m, loop) for m in MESHES for loop in LOOPS]
           + [("slab", (8, 8, 11), 1), ("slab", (5, 5, 5, 6), 1), ("slab", (12, 10), 2)])


def _cid(cfg):
    return f"{cfg[0]}-{_mid(cfg[1])}-{cfg[2]}"


def _entries(log):
    assert log and not log[0][0].startswith("#"), log[:1]
    assert all(g[1:] == (1, 1) and b[1:] == (1, 1) for _, g, b in log)
    return [(n, None if n.startswith(CU_SIZED) else g[0], b[0]) for n, g, b in log]


def _launches(P):
    return {k: v["launches"] for k, v in P.timings().items() if v["launches"]}


def record(cfg):
    """[(launch entries, {timing row: launches})] of the configuration's run, one pair per rank. The caller sets
    MVTV_ADMM_SYNC for the host-controlled loop."""
    kind, m, _ = cfg
    y, ymean = _data(m)
    if kind == "one":
        with mv.Problem(list(m), y, deltas=_deltas(m), order=mv.ORDER_CPP) as P:
            P.timing(True)
            with launch_log() as log:
                P.admm(LAM["B"], np.full(y.size, ymean), u=np.zeros(P.E), rho=RHO0_B, fixed_iters=N1)
            return [(_entries(log), _launches(P))]
    world = cfg[2]
    comms = slab.Comm.local_group(world)
    b = slab.plane_bounds(int(m[-1]), world)
    pl = int(np.prod(m[:-1]))
    ranks = [slab.SlabADMM(list(m), y[b[r] * pl:b[r + 1] * pl], _deltas(m), ymean, comms[r], device=0)
             for r in range(world)]
    out, err = [None] * world, [None] * world

    def work(r):
        try:
            ranks[r].P.timing(True)
            with launch_log() as log:
                ranks[r].run(LAM["B"], rho0=RHO0_B, fixed_iters=N1)
            out[r] = (_entries(log), _launches(ranks[r].P))
        except Exception as e:   # noqa: BLE001 (re-raised below)
            err[r] = e

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in ranks:
        s.close()
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    return out


# The table, recorded by record() from the library of commit PARENT (one MI355X), the last before the loop moved to
# mvtv_admm.cpp. A run is: the set-up launches, three iterations (theta-solve, then the edge pass reading an explicit
# u in the first iteration, u from z after it; the slab loop ends an iteration with k_admm_control, which the one-GPU
# loops fold into their last k_finalize), the launches after the loop (twin blocks filled, u exported).
PARENT = "0da8e3e"
FIN, CTRL = ("k_finalize", 1, 1024), ("k_admm_control", 1, 1)
IMPORT4 = (2, 3, 3, 2, 3, 2, 2, 2, 3, 2, 2, 2, 2, 2, 2)   # grids of the 15 blocks' import / export at 5 x 5 x 5 x 6
IMPORT3 = (2, 3, 3, 3, 3, 3, 3)


def _k(name, grids):
    return [(name, g, 256) for g in grids]


def _run(pre, solve, edge, post, ctrl=False):
    its = [solve + [(n.replace("UM", str(um)), g, b) for n, g, b in edge] + ([CTRL] if ctrl else []) for um in (0, 1, 1)]
    return pre + its[0] + its[1] + its[2] + post


SOLVE = {
    (37,): [("k_dctb8<7, 2, true, true, 16>", 1, 128)],
    (12, 10): [("k_dctg<0, true, true>", 5, 512), ("k_dctg<2, false, false>", 6, 512), ("k_dctg<1, true, false>", 5, 512)],
    (8, 8, 11): [("k_dct8<3, 0, true, true, 16, 0>", 6, 8), ("k_dct8<3, 0, false, false, 16, 0>", 11, 8),
                 ("k_dctb8<5, 2, false, false, 32>", 2, 64), ("k_dct8<3, 1, false, false, 16, 0>", 11, 8),
                 ("k_dct8<3, 1, true, false, 16, 0>", 6, 8)],
    (5, 5, 5, 6): [("k_dctg<0, true, true>", 75, 512)] + [("k_dctg<0, false, false>", 75, 512)] * 2
                  + [("k_dctg<2, false, false>", 63, 512)] + [("k_dctg<1, false, false>", 75, 512)] * 2
                  + [("k_dctg<1, true, false>", 75, 512)],
    # a rank of the two-rank 2-D slab: dim 0 forward, the substructured line solves, dim 0 back (first and last owned
    # plane, then the interior)
    "slab2": [("k_dctg<0, true, true>", 3, 512), ("k_trisr<1, 16, 16, 64>", 1, 80), ("k_trisr_iface", 1, 256),
              ("k_trisr<3, 16, 16, 64>", 1, 80), ("k_dctg<1, true, false>", 1, 512), ("k_dctg<1, true, false>", 1, 512),
              ("k_dctg<1, true, false>", 2, 512)],
}
EDGE = {
    (37,): [("k_edge_update<1, 0, UM, false>", 1, 256), FIN, ("k_gather<1, 0, 1, true>", 1, 256), FIN],
    (12, 10): [("k_admm2d<0, UM, false, 3>", 8, 256), FIN],
    (8, 8, 11): [("k_admm3a<0, UM, false, 7, true>", None, 1024), FIN],
    (5, 5, 5, 6): [("k_admm4a<0, UM, false, 15, true>", 32, 768), FIN, ("k_gather4b<1, true>", 8, 256), FIN],
    "slab2": [("k_edge_update<2, 0, UM, false>", 1, 256), FIN, ("k_gather<2, 0, 1, true>", 1, 256), FIN],
}
ONE = {   # mesh: (set-up, after the loop, timing rows of the device-controlled loop)
    (37,): (_k("k_edges_import", (1,)) + [("k_gather<1, 0, 0, false>", 1, 256), ("k_apply_A<1, 0, false, false>", 1, 256)],
            _k("k_edges_export", (1,)),
            {"dct_first": 3, "edge_update": 3, "gather_Dt": 4, "other": 1, "reduce": 6}),
    (12, 10): (_k("k_edges_import", (1, 1, 1)) + [("k_gather<2, 0, 0, false>", 1, 256), ("k_apply2d<0, false>", 8, 256)],
               _k("k_edges_export", (1, 1, 1)),
               {"admm_fused": 3, "dct": 6, "dct_first": 3, "gather_Dt": 1, "other": 1, "reduce": 3}),
    (8, 8, 11): (_k("k_edges_import", IMPORT3)
                 + [("k_gather3d<0, 0, false, 256, 7>", 24, 256), ("k_apply3d2<0, false>", 24, 256)],
                 _k("k_edges_copy_block", (3,)) + _k("k_edges_export", IMPORT3),
                 {"admm_fused": 3, "dct": 12, "dct_first": 1, "dct_first_fold": 2, "gather_Dt": 1, "other": 1,
                  "reduce": 3}),
    (5, 5, 5, 6): (_k("k_edges_import", IMPORT4) + [("k_gather4a<0, 0, 15, 8>", 32, 512),
                                                    ("k_gather4b<0, false>", 8, 256), ("k_apply4d<0, false>", 64, 256)],
                   _k("k_edges_copy_block", (3,) * 4) + _k("k_edges_export", IMPORT4),
                   {"admm_fused4": 3, "dct": 18, "dct_first": 3, "gather4_b": 3, "gather_Dt": 1, "other": 1,
                    "reduce": 6}),
}
# the host-controlled loop passes its scalars by value and never folds the right-hand side: at 8 x 8 x 11 (m_0 a power
# of two) its three first passes all count as dct_first; everything else as the device-controlled loop
HOST_ROWS = {(8, 8, 11): {"admm_fused": 3, "dct": 12, "dct_first": 3, "gather_Dt": 1, "other": 1, "reduce": 3}}
TABLE = {}
for _m, (_pre, _post, _rows) in ONE.items():
    TABLE[_cid(("one", _m, "device"))] = [(_run(_pre, SOLVE[_m], EDGE[_m], _post), _rows)]
    TABLE[_cid(("one", _m, "host"))] = [(_run(_pre, SOLVE[_m], EDGE[_m], _post), HOST_ROWS.get(_m, _rows))]
# the slab loop: theta_0 and u_0 = 0 filled on the device, no import or export; its reductions are not timed
TABLE[_cid(("slab", (8, 8, 11), 1))] = [
    (_run([("k_fill", 3, 256), ("k_apply3d2<0, false>", 24, 256)], SOLVE[(8, 8, 11)], EDGE[(8, 8, 11)],
          _k("k_edges_copy_block", (3,)), ctrl=True),
     {"admm_fused": 3, "dct": 12, "dct_first": 1, "dct_first_fold": 2})]
TABLE[_cid(("slab", (5, 5, 5, 6), 1))] = [
    (_run([("k_fill", 3, 256), ("k_apply4d<0, false>", 64, 256)], SOLVE[(5, 5, 5, 6)], EDGE[(5, 5, 5, 6)],
          _k("k_edges_copy_block", (3,) * 4), ctrl=True),
     {"admm_fused4": 3, "dct": 18, "dct_first": 3, "gather4_b": 3})]
TABLE[_cid(("slab", (12, 10), 2))] = [
    (_run([("k_fill", 1, 256), ("k_apply_A<2, 0, false, false>", 1, 256)], SOLVE["slab2"], EDGE["slab2"], [], ctrl=True),
     {"dct": 15, "dct_first": 3, "edge_update": 3, "gather_Dt": 3})] * 2


@gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cid)
def test_launch_sequence_and_timing_table(cfg, monkeypatch):
    if cfg[0] == "one" and cfg[2] == "host":
        monkeypatch.setenv("MVTV_ADMM_SYNC", "1")
    else:
        monkeypatch.delenv("MVTV_ADMM_SYNC", raising=False)
    got, want = record(cfg), TABLE[_cid(cfg)]
    assert len(got) == len(want)
    for r, ((log, launches), (wlog, wlaunches)) in enumerate(zip(got, want)):
        assert len(log) == len(wlog), (r, len(log), len(wlog))
        for i, (g, w) in enumerate(zip(log, wlog)):
            assert g == tuple(w), (r, i, g, w)
        assert launches == wlaunches, (r, launches, wlaunches)
