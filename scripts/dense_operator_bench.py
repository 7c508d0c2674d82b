#!/usr/bin/env python
"""Measurements behind DESIGN.md section 15: prints ONE JSON object.

For Float64 and Float32 and n = 4096 (cache-sized: the matrix fits the 256 MB Infinity Cache) and n = 16384 (HBM-bound: 2.1 GB at Float64),
on a seeded n x n matrix without zero entries, microseconds per call between two HIP events on the context's stream -- every timed window
holds enough back-to-back calls to last tens of milliseconds, the four routes alternate inside every repetition, median / minimum / maximum
of --reps windows after --warmup:

  dense_n   mik_dense_mul, y = A x   (k_dense_n + k_dense_n_combine)
  dense_t   mik_dense_mul, y = A' x  (k_dense_t + k_finalize_store)
  csr       mik_spmv on the same matrix uploaded as a full HipCSR (12 B per Float64 entry): the only route before the dense operator
  copy      mik_copy of n * n elements: the copy ceiling of the same run (it reads AND writes that many bytes)

`matrix_TBps` = n * n * sizeof(T) / time; `share_of_copy` = that rate over the copy's (2 * n * n * sizeof(T) / its time).

Usage: python scripts/dense_operator_bench.py [--reps 9] [--warmup 2] [--sizes 4096,16384] [--csr-max 16384] > profiles/dense_operator_bench.json
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


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def windows(ctx, routes, inner, reps, warmup):
    """microseconds per call of every route: `inner` calls between two HIP events, the routes alternating inside every repetition"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = {name: [] for name in routes}
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                for name, fn in routes.items():
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


def bench(pkg, ctx, dtype, n, reps, warmup, csr_max):
    dtype = np.dtype(dtype)
    es = dtype.itemsize
    rng = np.random.default_rng(n)
    A = np.asfortranarray((rng.random((n, n), dtype=np.float32) + 0.25).astype(dtype))           # no zero entries
    M = pkg.HipMatrix(n, n, dtype, ctx)
    assert M.ld == n
    M.buf.copy_from_host(A.reshape(-1, order="F"))
    x = pkg.HipVector.from_numpy((rng.random(n) - 0.5).astype(dtype), ctx)
    y = pkg.HipVector(n, dtype, ctx)
    src, dst = pkg.HipVector(n * n, dtype, ctx), pkg.HipVector(n * n, dtype, ctx)
    routes = {"dense_n": lambda: pkg.mul_(y, M, x), "dense_t": lambda: pkg.mul_(y, M.adj, x), "copy": lambda: dst.copyto_(src)}
    res = {"dtype": dtype.name, "n": n, "matrix_bytes": n * n * es}
    if n <= csr_max:
        t0 = time.perf_counter()
        rowptr = np.arange(0, n * n + 1, n, dtype=np.int64)
        S = pkg.HipCSR(n, n, rowptr.astype(np.int32) if n * n < 2 ** 31 else rowptr, np.tile(np.arange(n, dtype=np.int32 if n * n < 2 ** 31 else np.int64), n),
                       np.ascontiguousarray(A).reshape(-1), index_base=0, is_csc=False, ctx=ctx)
        res["csr_upload_s"] = round(time.perf_counter() - t0, 2)
        res["csr_kernel"], res["csr_stored_bytes"] = S.spmv_kernel(), S.spmv_stored_bytes()
        log(f"  csr uploaded in {res['csr_upload_s']} s, kernel {res['csr_kernel']}")
        ys = pkg.HipVector(n, dtype, ctx)
        routes["csr"] = lambda: pkg.mul_(ys, S, x)
        pkg.mul_(ys, S, x)
        pkg.mul_(y, M, x)
        d = np.abs(ys.to_numpy().astype(np.float64) - y.to_numpy().astype(np.float64)).max()
        res["max_abs_difference_dense_n_vs_csr"] = float(d)                                      # two summation orders of the same product
    del A
    inner = max(2, int(round(40e-3 / (n * n * es / 3.0e12))))                                    # ~40 ms per window at 3 TB/s
    us = windows(ctx, routes, inner, reps, warmup)
    res["calls_per_window"] = inner
    for name, v in us.items():
        s = stats(v)
        s["matrix_TBps"] = round(n * n * es / (s["median_us"] * 1e-6) / 1e12, 3)
        res[name] = s
    copy_rate = 2 * res["copy"]["matrix_TBps"]
    res["copy"]["read_plus_write_TBps"] = round(copy_rate, 3)
    for name in ("dense_n", "dense_t", "csr"):
        if name in res:
            res[name]["share_of_copy"] = round(res[name]["matrix_TBps"] / copy_rate, 3)
    if "csr" in res:
        res["dense_n_over_csr_time"] = round(res["dense_n"]["median_us"] / res["csr"]["median_us"], 3)
        res["dense_t_over_csr_time"] = round(res["dense_t"]["median_us"] / res["csr"]["median_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--csr-max", type=int, default=16384)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    c, r = C.c_int(), C.c_int()
    pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r))
    res = {"device": ctx.info()["arch"], "chunk": c.value, "rows_per_workgroup": r.value, "reps": args.reps, "warmup": args.warmup, "cases": []}
    for n in (int(v) for v in args.sizes.split(",")):
        for dtype in (np.float64, np.float32):
            log(f"n = {n} {np.dtype(dtype).name}")
            res["cases"].append(bench(pkg, ctx, dtype, n, args.reps, args.warmup, args.csr_max))
            log("  " + json.dumps(res["cases"][-1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
