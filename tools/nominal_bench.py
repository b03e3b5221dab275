"""GPU measurement of the nominal block orders against the reference order: ADMM iterations a second and the fused
edge pass's time per launch (HIP-event timing of the kernel's own dispatch, mvtv_timing_*), for legs
MESH:ORDER run in turn REPS times in one process. Each leg warms up with 5 iterations, then runs
Problem.run(fixed_iters=20) timed by the wall clock (it/s, timing off) and once more with kernel timing on.
One JSON line a leg and repetition.

usage: nominal_bench.py [--reps R] [MESH:ORDER ...]     default: 512x512x512:0 512x512x512:2 640x480x256:2"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import multivartv_amd as mv  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402

args = sys.argv[1:]
reps = 3
if args[:1] == ["--reps"]:
    reps, args = int(args[1]), args[2:]
legs = args or ["512x512x512:0", "512x512x512:2", "640x480x256:2"]
ITERS = 20


def open_leg(leg):
    mesh, order = leg.split(":")
    m = [int(v) for v in mesh.split("x")]
    y = towers(m)
    P = mv.Problem(m, y, deltas=[(1.0 + 2e-4) / v for v in m], order=int(order), device=0)
    P.state_set(np.full(y.size, y.mean()), None, 0.2)
    P.run(1.0, fixed_iters=5)
    return P


for rep in range(reps):
    for leg in legs:
        # one problem at a time: a 512^3 problem holds two edge buffers of 7 N words
        P = open_leg(leg)
        t0 = time.perf_counter()
        st = P.run(1.0, fixed_iters=ITERS)
        wall = time.perf_counter() - t0
        P.timing(True)
        P.run(1.0, fixed_iters=ITERS)
        T = P.timings()
        P.timing(False)
        fused = T["admm_fused"] if T["admm_fused"]["launches"] else T["admm_fused4"]
        rec = dict(leg=leg, rep=rep, N=P.N, E=P.E, iters=st["iters"], it_per_s=ITERS / wall,
                   theta_solver=st["theta_solver"], fused_ms=fused["ms"] / max(fused["launches"], 1),
                   fused_launches=fused["launches"], fused_bytes=fused["bytes_per_launch"],
                   kernels_ms={k: v["ms"] / v["launches"] for k, v in T.items() if v["launches"]})
        rec["fused_GBps"] = rec["fused_bytes"] / (rec["fused_ms"] * 1e-3) / 1e9 if rec["fused_ms"] else 0.0
        print(json.dumps(rec), flush=True)
        P.close()
