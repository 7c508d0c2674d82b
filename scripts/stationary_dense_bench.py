#!/usr/bin/env python
"""Measurements behind DESIGN.md section 14: prints ONE JSON object.

For Float64 and n = 1024, 4096, 16384 (strictly diagonally dominant, non-symmetric), per iteration of each dense stationary method:
microseconds between two HIP events on the context's stream (median, minimum and maximum of --reps after --warmup), and

  jacobi        one copy of x and ONE row-owned sweep over all n^2 entries: n^2 * 8 B / time as a share of 8 TB/s -- the row-owned sweep alone;
  gauss_seidel  the upper phase (a row-owned sweep over n^2 / 2 entries) + the forward substitution in the panel form (ceil(n / W) launches
                over the other n^2 / 2); `forward_us_estimate` = this minus half the Jacobi time;
  sor, ssor     the same with the relaxed update (ssor: + one copy of x and a full row-owned sweep);
  sparse_route  the same matrix uploaded as CSR and swept by the sparse gauss_seidel_ (what the package could do before the dense entries
                existed), at the sizes up to --sparse-max where its one-row levels finish in seconds;
  cpu_checker   tests/stationary_ref/stationary_dense_ref.c (gcc -O2) on one core, one Gauss-Seidel iteration.

Usage: python scripts/stationary_dense_bench.py [--reps 7] [--warmup 2] [--sizes 1024,4096,16384] > profiles/stationary_dense_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

PEAK = 8.0e12               # bytes / s, the HBM peak the shares are quoted against


def timed(ctx, fn, reps, warmup):
    """microseconds of fn() between two HIP events on the context's stream, one figure per repetition"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = []
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if it >= warmup:
                    out.append(e0.elapsed_time(e1) * 1e3)
    finally:
        ctx.set_stream(None)
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def matrix(n, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.random((n, n)) - 0.5
    A[np.arange(n), np.arange(n)] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.5 * n + 1.0)      # above any off-diagonal row sum (entries in [-0.5, 0.5))
    return np.asfortranarray(A)


def bench_size(pkg, ctx, ref, n, reps, warmup, sparse_max):
    A = matrix(n)
    rng = np.random.default_rng(1)
    b = rng.standard_normal(n)
    M = pkg.HipMatrix(n, n, np.float64, ctx)
    padded = A if M.ld == n else np.asfortranarray(np.vstack([A, np.zeros((M.ld - n, n))]))
    M.buf.copy_from_host(padded.ravel(order="F"))
    del padded
    O = pkg.DenseStationaryOperator(M)
    info = O.info()
    x, t, bd = pkg.HipVector(n, ctx=ctx).fill_(0), pkg.HipVector(n, ctx=ctx).fill_(0), pkg.HipVector.from_numpy(b, ctx)
    nbytes = 8.0 * n * n
    res = {"n": n, "ld": M.ld, "W": info["W"], "R": info["R"], "launches_forward": info["launches_forward"], "form": info["form"],
           "row_sweep_workgroups": -(-n // info["R"])}
    steps = {"jacobi": (lambda: O.jacobi_step_(x, t, bd), 1.0), "gauss_seidel": (lambda: O.gs_step_(x, bd), 1.0),
             "sor": (lambda: O.sor_step_(x, t, bd, 1.25), 1.0), "ssor": (lambda: O.ssor_step_(x, t, bd, 1.25), 2.0)}
    for name, (fn, passes) in steps.items():
        x.fill_(0)
        us = timed(ctx, fn, reps, warmup)
        s = stats(us)
        s["share_of_8TBps"] = round(passes * nbytes / (s["median_us"] * 1e-6) / PEAK, 4)
        res[name] = s
    res["gauss_seidel"]["forward_us_estimate"] = round(res["gauss_seidel"]["median_us"] - res["jacobi"]["median_us"] / 2, 1)
    res["gauss_seidel"]["forward_us_per_launch_estimate"] = round(res["gauss_seidel"]["forward_us_estimate"] / info["launches_forward"], 2)
    # the iterate the timed loop leaves is a Gauss-Seidel iterate of a convergent system: a sanity check against the direct solution
    x.fill_(0)
    for _ in range(30):
        O.gs_step_(x, bd)
    if n <= 4096:
        exact = np.linalg.solve(A, b)
        res["gauss_seidel_30_iterations_relative_error"] = float(np.linalg.norm(x.to_numpy() - exact) / np.linalg.norm(exact))
    if n <= sparse_max:
        import scipy.sparse as sp
        t0 = time.perf_counter()
        S = pkg.HipCSR.from_scipy(sp.csc_matrix(A), ctx)
        Os = pkg.StationaryOperator(S)
        setup = time.perf_counter() - t0
        it = pkg.GaussSeidelIterable(Os, x, bd, 1)
        us = timed(ctx, it._step, max(3, reps // 2), 1)
        res["sparse_route"] = dict(stats(us), setup_s=round(setup, 3), levels_forward=Os.info()["levels_forward"], launches_forward=Os.info()["launches_forward"])
    t0 = time.perf_counter()
    ref.gauss_seidel(A, b, np.zeros(n), 1)
    t1 = time.perf_counter()
    ref.gauss_seidel(A, b, np.zeros(n), 11)
    t2 = time.perf_counter()
    res["cpu_checker"] = {"gauss_seidel_us_per_iteration": round(((t2 - t1) - (t1 - t0)) / 10 * 1e6, 1)}      # the difference removes the copy of A
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--sparse-max", type=int, default=1024)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    import stationary_dense_host as dh
    ref = dh.build(tempfile.mkdtemp())
    ctx = pkg.default_context()
    res = {"device": ctx.info()["arch"], "dtype": "float64", "peak_TBps": PEAK / 1e12, "reps": args.reps, "sizes": []}
    for n in (int(v) for v in args.sizes.split(",")):
        res["sizes"].append(bench_size(pkg, ctx, ref, n, args.reps, args.warmup, args.sparse_max))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
