#!/usr/bin/env python
"""Measurements behind DESIGN.md section 16: prints ONE JSON object.

For Float64 and Float32 and n = 1024 (launches dominate), 4096 (cache-sized) and 16384 (HBM-bound: 2.1 GB at Float64), on a seeded n x n
matrix without zero entries, microseconds per call between two HIP events on the context's stream -- every timed window holds enough
back-to-back calls to last tens of milliseconds, the routes alternate inside every repetition, median / minimum / maximum of --reps windows
after --warmup.  Per width b of --widths:

  vec_b     b calls of mik_dense_mul on the columns of X, one handle (the route before the block product; its code is unchanged)
  mm_b      mik_dense_mm(b) as the library routes it (a last group below its threshold goes through the vector kernels)
  blk_b     mik_dense_mm(b) with the block kernel forced at every width (mik_dev_dense_block_min_width = 1): what the threshold is chosen from

`vec_1_again` is a second, identical route of one mik_dense_mul: its distance from vec_1 is the spread between two identical routes of the
same run.  `speedup` = vec_b / mm_b; `byte_ratio` = b / (ceil(b / GW) * (1 + 2 GW / C)), the matrix bytes the vector route moves over those of
the block route with its workspace traffic; `fraction_of_byte_ratio` = speedup / byte_ratio.

--lobpcg N: one lobpcg of block 8 with at most --lobpcg-iters iterations on the N x N matrix as a HipMatrix and as a full HipCSR, wall time.

Usage: python scripts/dense_block_bench.py [--reps 9] [--warmup 2] [--sizes 1024,4096,16384] [--widths 1,2,3,4,6,8,9,32] [--lobpcg 4096]
       > profiles/dense_block_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

_vp = C.c_void_p


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def windows(ctx, routes, reps, warmup):
    """microseconds per call of every route {name: (fn, calls per window)}: the calls between two HIP events, the routes alternating inside
    every repetition"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = {name: [] for name in routes}
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                for name, (fn, inner) in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(inner):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    if it >= warmup:
                        out[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    finally:
        ctx.set_stream(None)
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def matrix(pkg, ctx, dtype, n):
    rng = np.random.default_rng(n)
    A = np.asfortranarray((rng.random((n, n), dtype=np.float32) + 0.25).astype(dtype))           # no zero entries
    M = pkg.HipMatrix(n, n, dtype, ctx)
    assert M.ld == n
    M.buf.copy_from_host(A.reshape(-1, order="F"))
    return A, M


def bench(pkg, ctx, dtype, n, widths, reps, warmup, chunk, gw):
    dtype = np.dtype(dtype)
    es = dtype.itemsize
    L = pkg.lib()
    A, M = matrix(pkg, ctx, dtype, n)
    del A
    rng = np.random.default_rng(n + 1)
    X = pkg.HipMatrix.from_numpy((rng.random((n, 32)) - 0.5).astype(dtype), ctx)
    Y = pkg.HipMatrix(n, 32, dtype, ctx)
    h = M.dense
    M.reserve_block_()
    xs, ys = [_vp(X.col(j).ptr) for j in range(32)], [_vp(Y.col(j).ptr) for j in range(32)]
    xp, yp = _vp(X.buf.ptr), _vp(Y.buf.ptr)

    def vec(b):
        def run():
            for j in range(b):
                L.mik_dense_mul(h, 0, xs[j], ys[j])
        return run

    def mm(b, forced):
        def run():
            if forced:
                L.mik_dev_dense_block_min_width(h, 1)
            L.mik_dense_mm(h, b, xp, X.ld, yp, Y.ld)
            if forced:
                L.mik_dev_dense_block_min_width(h, 0)
        return run

    def inner(b_reads):                                                  # ~40 ms per window at 3 TB/s, bounded for the launch-bound sizes
        return int(min(2000, max(2, round(40e-3 / (b_reads * n * n * es / 3.0e12)))))

    routes = {}
    for b in widths:
        groups = -(-b // gw)
        routes[f"vec_{b}"] = (vec(b), inner(b))
        routes[f"mm_{b}"] = (mm(b, False), inner(groups))
        if b % gw:
            routes[f"blk_{b}"] = (mm(b, True), inner(groups))
    routes["vec_1_again"] = (vec(1), inner(1))
    for fn, _ in routes.values():                                        # every route once, checked
        fn()
    Y.col(0).to_numpy()
    us = windows(ctx, routes, reps, warmup)
    res = {"dtype": dtype.name, "n": n, "matrix_bytes": n * n * es, "routes": {k: dict(stats(v), calls_per_window=routes[k][1]) for k, v in us.items()}}
    res["spread_between_identical_routes"] = round(abs(res["routes"]["vec_1"]["median_us"] - res["routes"]["vec_1_again"]["median_us"]) /
                                                   res["routes"]["vec_1"]["median_us"], 4)
    res["widths"] = []
    for b in widths:
        v, m = res["routes"][f"vec_{b}"]["median_us"], res["routes"][f"mm_{b}"]["median_us"]
        ratio = b / (-(-b // gw) * (1 + 2 * gw / chunk))
        row = {"b": b, "vec_us": v, "mm_us": m, "speedup": round(v / m, 3), "byte_ratio": round(ratio, 3), "fraction_of_byte_ratio": round(v / m / ratio, 3)}
        if f"blk_{b}" in res["routes"]:
            row["blk_us"] = res["routes"][f"blk_{b}"]["median_us"]
            row["blk_speedup"] = round(v / row["blk_us"], 3)
        res["widths"].append(row)
    return res


def lobpcg_case(pkg, ctx, n, iters):
    """wall seconds of lobpcg (block 8, at most `iters` iterations, the default tolerance) on a HipMatrix and on the same matrix as a full HipCSR"""
    dtype = np.dtype(np.float64)
    rng = np.random.default_rng(n)
    R = rng.random((n, n))
    A = np.asfortranarray(R + R.T + 20 * np.eye(n))
    del R
    X0 = np.random.default_rng(1).random((n, 8))
    M = pkg.HipMatrix(n, n, dtype, ctx)
    M.buf.copy_from_host(A.reshape(-1, order="F"))
    t0 = time.perf_counter()
    rowptr = np.arange(0, n * n + 1, n, dtype=np.int32)
    S = pkg.HipCSR(n, n, rowptr, np.tile(np.arange(n, dtype=np.int32), n), np.ascontiguousarray(A).reshape(-1), index_base=0, is_csc=False, ctx=ctx)
    res = {"n": n, "block": 8, "maxiter": iters, "csr_upload_s": round(time.perf_counter() - t0, 2)}
    out = {}
    for name, op in (("dense", M), ("csr", S), ("dense", M), ("csr", S)):          # the first pair warms up
        t0 = time.perf_counter()
        r = pkg.lobpcg(op, True, X0, maxiter=iters, dense=name == "dense")
        r.X.to_numpy()
        out[name] = time.perf_counter() - t0
        res[name + "_lambda_max"], res[name + "_iterations"] = float(r.lam[0]), int(r.iterations)
    res["dense_s"], res["csr_s"] = round(out["dense"], 4), round(out["csr"], 4)
    res["dense_over_csr_time"] = round(out["dense"] / out["csr"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--widths", default="1,2,3,4,6,8,9,32")
    ap.add_argument("--lobpcg", type=int, default=4096)
    ap.add_argument("--lobpcg-iters", type=int, default=20)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    c, r, g = C.c_int(), C.c_int(), C.c_int()
    pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r))
    pkg.lib().mik_dense_block_shape(C.byref(g))
    widths = [int(v) for v in args.widths.split(",")]
    res = {"device": ctx.info()["arch"], "chunk": c.value, "rows_per_workgroup": r.value, "group_width": g.value, "reps": args.reps,
           "warmup": args.warmup, "cases": []}
    for n in (int(v) for v in args.sizes.split(",") if v):
        for dtype in (np.float64, np.float32):
            log(f"n = {n} {np.dtype(dtype).name}")
            res["cases"].append(bench(pkg, ctx, dtype, n, widths, args.reps, args.warmup, c.value, g.value))
            log("  " + json.dumps(res["cases"][-1]["widths"]))
    if args.lobpcg:
        res["lobpcg"] = lobpcg_case(pkg, ctx, args.lobpcg, args.lobpcg_iters)
        log("  " + json.dumps(res["lobpcg"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
