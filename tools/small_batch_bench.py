#!/usr/bin/env python3
"""Small-mesh fits, batched against one after another: the timing script of DESIGN.md §4.5 (profiles/small_batch/).

    python tools/small_batch_bench.py cv --m 10 10 --n 100 --repeats 3          # mvtv()'s 5-fold CV over 100 lambdas
    python tools/small_batch_bench.py sweep --m 10 10 --n 100 --repeats 3       # nbatch independent single fits

cv: cv.mbs_impl(folds, n_lambda) on n scattered points, three legs interleaved in one process (leg A of repeat 1, leg B
of repeat 1, ..., so a drift of the box hits every leg alike): unbatched, concurrent=4, batched=True. One JSON line per
(leg, repeat): wall seconds of the whole call, and ADMM it/s = the paths' total iterations / wall. The iteration total
(and the mean PCG iterations per theta-solve, the baseline of the cosine follow-up) comes from one untimed
Problem.path_batch call over the same six paths; the unbatched legs' own counts differ from it by a few iterations
where their theta-solve stops elsewhere (pcg_rtol 1e-10, spectral preconditioner).

The legs batched_cos1 / batched_cos2 are batched=True with batch_cosine=1 / 2 (the in-workgroup cosine theta-solve,
mvtv_problem_batch_cosine); each batched leg's line carries its own mean PCG iterations per theta-solve.

The leg device_cv is batched=True with device_cv=True: the paths and the fold-MSE matrix through one Problem.cv_batch call
(mvtv_cv_batch: member setup and scoring on the GPU; profiles/cv_batch/). Every leg's untimed warm-up
call (three lambdas) is reported too, as `warmup` lines: the first call of a leg pays for the kernels' loading.

    python tools/small_batch_bench.py folds --m 20 --n 100 --fold-list 5 20 0 --legs batched device_cv

folds: the cv mode once per fold count of --fold-list (0: leave-one-out, folds = n), same legs, same method.

sweep: nbatch in --nbatch independent fits at one lambda (own data per member, cold start) through one
Problem.path_batch call, against the same fits through Problem.admm one after another (the parent path; at most
--seq-cap of them are run and the per-fit time is reported, so `seq_seconds` of a larger nbatch is that times nbatch).
--cos-modes 0 1 2 runs each path_batch call once per batch_cosine mode, interleaved (one line each, `cos_mode`);
--identity puts the data on the mesh nodes (W = I), the members mode 1's exact solve takes.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import multivartv_amd as mv  # noqa: E402
from multivartv_amd import cv  # noqa: E402
from multivartv_amd.utils import create_deltas, interp_weights  # noqa: E402


def scattered(n, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, size=(n, p))
    f = np.where(np.all(x > 0.6, axis=1), 1.0, 0.0)
    return x, f + 0.3 * rng.standard_normal(n)


def members_of(x, y, m, folds, seed):
    """(O^T y, W, mean y) of the final path and of each fold's training set, as cv.mbs_impl builds them."""
    mesh = cv.create_mesh(x, m)
    axes = cv.tensor_axes(mesh, m)
    deltas = create_deltas(x, m)
    N = int(np.prod(m))
    P = mv.Problem(m, np.zeros(N), deltas=deltas, order=mv.ORDER_CPP, weighted=True)
    fi = cv.kfoldinds(len(y), folds, seed)
    out = []
    for f in [None] + list(range(folds)):
        tr = slice(None) if f is None else fi != f
        W, oty = interp_weights(P.nearest(axes, x[tr]), N, y[tr])
        out.append((oty, W, float(y[tr].mean())))
    return P, out


def run_cv(a, folds=None):
    folds = a.folds if folds is None else folds
    m, p = list(a.m), len(a.m)
    x, y = scattered(a.n, p, a.seed)
    P, mem = members_of(x, y, m, folds, 0)
    P.set_data(mem[0][0], mem[0][1])
    lams = cv.create_lambdas(a.n_lambda, P)
    N = P.N
    _, _, _, stats, _ = P.path_batch(np.stack([q[0] for q in mem]), lams, np.stack([np.full(N, q[2]) for q in mem]),
                                     np.full(len(mem), lams[0] / 5.0), wdiag=np.stack([q[1] for q in mem]),
                                     want_thetas=False)
    iters = sum(s["iters"] for row in stats for s in row)
    pcg = sum(s["pcg_iters"] for row in stats for s in row)
    base = dict(mode="cv", m=m, n=a.n, folds=folds, n_lambda=a.n_lambda, admm_iters=iters,
                pcg_per_solve=pcg / max(iters, 1), maxiter_hits=sum(s["status"] == 1 for row in stats for s in row))
    legs = {"unbatched": {}, "concurrent4": dict(concurrent=4), "batched": dict(batched=True),
            "batched_cos1": dict(batched=True, batch_cosine=1), "batched_cos2": dict(batched=True, batch_cosine=2),
            "device_cv": dict(batched=True, device_cv=True)}
    legs = {k: v for k, v in legs.items() if k in a.legs}
    leg_pcg = {}
    for leg, kw in legs.items():   # the cosine legs' own counts, untimed
        if kw.get("batch_cosine"):
            P.batch_cosine(kw["batch_cosine"])
            _, _, _, st, _ = P.path_batch(np.stack([q[0] for q in mem]), lams, np.stack([np.full(N, q[2]) for q in mem]),
                                          np.full(len(mem), lams[0] / 5.0), wdiag=np.stack([q[1] for q in mem]),
                                          want_thetas=False)
            leg_pcg[leg] = dict(admm_iters=sum(s["iters"] for row in st for s in row),
                                pcg_per_solve=sum(s["pcg_iters"] for row in st for s in row) / max(iters, 1))
    P.close()
    for leg, kw in legs.items():   # warm-up: kernels loaded, allocator warm
        t0 = time.perf_counter()
        cv.mbs_impl(x, y, m, lambdas=lams[:3], folds=folds, group=False, **kw)
        print(json.dumps(dict(mode="cv", warmup=True, m=m, n=a.n, folds=folds, n_lambda=3, leg=leg,
                              seconds=time.perf_counter() - t0)), flush=True)
    for rep in range(a.repeats):
        for leg, kw in legs.items():
            t0 = time.perf_counter()
            out = cv.mbs_impl(x, y, m, lambdas=lams, folds=folds, group=False, **kw)
            dt = time.perf_counter() - t0
            print(json.dumps(dict(base, **leg_pcg.get(leg, {}), leg=leg, rep=rep, seconds=dt, its_per_s=iters / dt,
                                  best=out["lambda_minmse_ind"])), flush=True)


def run_sweep(a):
    m, p = list(a.m), len(a.m)
    N = int(np.prod(m))
    x0, _ = scattered(a.n, p, a.seed)
    deltas = create_deltas(x0, m)
    mesh = cv.create_mesh(x0, m)
    axes = cv.tensor_axes(mesh, m)
    P = mv.Problem(m, np.zeros(N), deltas=deltas, order=mv.ORDER_CPP, weighted=True)
    nmax = max(a.nbatch)
    mem = []
    for b in range(nmax):   # the same points, own responses per member
        rng = np.random.default_rng(1000 + b)
        if a.identity:   # the data on the mesh nodes: W = I
            y = np.where(np.all(mesh > 0.6, axis=1), 1.0, 0.0) + 0.3 * rng.standard_normal(N)
            mem.append((y, np.ones(N), float(y.mean())))
            continue
        y = np.where(np.all(x0 > 0.6, axis=1), 1.0, 0.0) + 0.3 * rng.standard_normal(a.n)
        W, oty = interp_weights(P.nearest(axes, x0), N, y)
        mem.append((oty, W, float(y.mean())))
    oty = np.stack([q[0] for q in mem])
    W = np.stack([q[1] for q in mem])
    th0 = np.stack([np.full(N, q[2]) for q in mem])
    rho0 = np.full(nmax, a.lam / 5.0)
    for cm in a.cos_modes:   # warm-up
        P.batch_cosine(cm)
        P.path_batch(oty[:2], [a.lam], th0[:2], rho0[:2], wdiag=W[:2], want_thetas=False)
    P.set_data(oty[0], W[0])
    P.admm(a.lam, th0[0], rho=a.lam / 5.0, return_u=False)
    for rep in range(a.repeats):
        nseq = min(a.seq_cap, nmax)
        t0 = time.perf_counter()
        seq_iters = 0
        for b in range(nseq):
            P.set_data(oty[b], W[b])
            seq_iters += P.admm(a.lam, th0[b], rho=a.lam / 5.0, return_u=False)[3]["iters"]
        per_fit = (time.perf_counter() - t0) / nseq
        for nb in a.nbatch:
            for cm in a.cos_modes:
                P.batch_cosine(cm)
                t0 = time.perf_counter()
                _, _, _, stats, _ = P.path_batch(oty[:nb], [a.lam], th0[:nb], rho0[:nb], wdiag=W[:nb], want_thetas=True)
                dt = time.perf_counter() - t0
                iters = sum(s[0]["iters"] for s in stats)
                pcg = sum(s[0]["pcg_iters"] for s in stats)
                print(json.dumps(dict(mode="sweep", m=m, n=a.n, lam=a.lam, rep=rep, nbatch=nb, cos_mode=cm,
                                      identity=bool(a.identity), seconds=dt, admm_iters=iters, its_per_s=iters / dt,
                                      pcg_per_solve=pcg / max(iters, 1), seq_fits_timed=nseq,
                                      seq_seconds_per_fit=per_fit, seq_its_per_s=seq_iters / (per_fit * nseq),
                                      speedup=per_fit * nb / dt)), flush=True)
    P.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cv", "folds", "sweep"])
    ap.add_argument("--m", type=int, nargs="+", required=True)
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--fold-list", type=int, nargs="+", default=[5, 20, 0])
    ap.add_argument("--n-lambda", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--nbatch", type=int, nargs="+", default=[1, 6, 64, 256, 1024])
    ap.add_argument("--seq-cap", type=int, default=16)
    ap.add_argument("--legs", nargs="+", default=["unbatched", "concurrent4", "batched"])
    ap.add_argument("--cos-modes", type=int, nargs="+", default=[0], choices=[0, 1, 2])
    ap.add_argument("--identity", action="store_true")
    a = ap.parse_args()
    if a.mode == "folds":
        for f in a.fold_list:
            run_cv(a, a.n if f == 0 else f)
    else:
        (run_cv if a.mode == "cv" else run_sweep)(a)


if __name__ == "__main__":
    main()
