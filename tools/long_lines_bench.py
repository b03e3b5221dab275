#!/usr/bin/env python3
"""ADMM iterations per second (variant B, fixed iterations, towers input, AUTO theta-solve) on one mesh: the timing
script of the long-last-dimension measurements (profiles/long_lines/).

    python tools/long_lines_bench.py --m 16777216 --steps 20 --warmup 3
    python tools/long_lines_bench.py --m 512 512 512 --blocks 8        # the blocked solve forced (3N against 2N)
    MVTV_LIB_PATH=/path/to/another/libmvtv.so python tools/long_lines_bench.py --m 1024 16384 --steps 5

Prints one JSON line: the mesh, the solver that ran, iterations, seconds of the timed run (the library's own wall
time of the call, stream drained) and it/s. A library without mvtv_problem_line_blocks (an older build, for an A/B)
is loaded too; --blocks then fails."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from multivartv_amd import _lib  # noqa: E402

if not hasattr(ctypes.CDLL(_lib.LIB_PATH), "mvtv_problem_line_blocks"):
    _lib.SIGNATURES.pop("mvtv_problem_line_blocks", None)

import multivartv_amd as mv  # noqa: E402
from multivartv_amd.synth import towers  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=0, help="Problem.line_blocks(blocks) before the runs")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    m = list(a.m)
    y = towers(m)
    deltas = [(1.0 + 2e-4) / v for v in m]
    with mv.Problem(m, y, deltas=deltas, order=mv.ORDER_CPP) as P:
        if a.blocks:
            P.line_blocks(a.blocks)
        P.state_set(np.full(y.size, y.mean()), None, a.lam / 5)
        if a.warmup:
            P.run(a.lam, fixed_iters=a.warmup)
        st = P.run(a.lam, fixed_iters=a.steps)
    print(json.dumps(dict(tag=a.tag, lib=os.path.basename(os.path.dirname(_lib.LIB_PATH)), m=m, blocks=a.blocks,
                          theta_solver=st["theta_solver"], iters=st["iters"], seconds=st["seconds"],
                          its_per_s=st["iters"] / st["seconds"], pcg_iters=st["pcg_iters"])))


if __name__ == "__main__":
    main()
