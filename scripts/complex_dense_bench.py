#!/usr/bin/env python
"""Measurements behind DESIGN.md section 18: writes ONE JSON object (default: profiles/complex_dense_bench.json) and prints it.

For ComplexF64 and ComplexF32 and n = 2048 (cache-sized) and n = 8192 (HBM-bound: 1.07 GB at ComplexF64), on a seeded n x n matrix
without zero entries, microseconds per call between two HIP events on the context's stream -- every timed window holds enough back-to-back
calls to last about 40 ms, the routes alternate inside every repetition, median / minimum / maximum of --reps windows after --warmup:

  dense_n   mik_dense_mul, y = A x   (k_cdense_n + k_dense_n_combine over 2 m reals)
  dense_t   mik_dense_mul, y = A' x  (k_cdense_t + k_finalize_store)
  csr       mik_spmv on the same matrix uploaded as a full complex HipCSR (20 B per ComplexF64 entry): the only route before this operator
  real_n    the real mik_dense_mul, y = B x, on a real 2 n x n matrix of the component type: the same bytes
  real_t    ... y = B' x

`matrix_TBps` = matrix bytes / time; `over_csr_time` = time over the csr route's (the bar of section 18: < 1 at n = 8192 for both forms);
`share_of_real` = the route's bytes per second over those of the real kernel of the same form.

Usage: python scripts/complex_dense_bench.py [--reps 9] [--warmup 2] [--sizes 2048,8192] [--out profiles/complex_dense_bench.json]
"""
import argparse
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


def bench(pkg, ctx, dtype, n, reps, warmup):
    dtype = np.dtype(dtype)
    rt = np.dtype(dtype.type(0).real.dtype)
    es = dtype.itemsize
    rng = np.random.default_rng(n)
    A = np.empty((n, n), dtype, order="F")
    A.real = rng.random((n, n), dtype=np.float32).T + 0.25                                       # no zero parts
    A.imag = rng.random((n, n), dtype=np.float32).T + 0.25
    M = pkg.HipMatrix(n, n, dtype, ctx)
    assert M.ld == n
    M.buf.copy_from_host(A.reshape(-1, order="F"))
    x = pkg.HipVector.from_numpy(((rng.random(n) - 0.5) + 1j * (rng.random(n) - 0.5)).astype(dtype), ctx)
    y = pkg.HipVector(n, dtype, ctx)
    # the real matrix of the same bytes: the same device contents read as 2 n x n reals would do, but a separate buffer keeps the routes apart
    B = pkg.HipMatrix(2 * n, n, rt, ctx)
    assert B.ld == 2 * n
    B.buf.copy_from_host(A.reshape(-1, order="F").view(rt))
    xr, yr = pkg.HipVector.from_numpy((rng.random(n) - 0.5).astype(rt), ctx), pkg.HipVector(2 * n, rt, ctx)
    xr2, yr2 = pkg.HipVector.from_numpy((rng.random(2 * n) - 0.5).astype(rt), ctx), pkg.HipVector(n, rt, ctx)
    t0 = time.perf_counter()
    S = pkg.HipCSR(n, n, np.arange(0, n * n + 1, n, dtype=np.int32), np.tile(np.arange(n, dtype=np.int32), n), np.ascontiguousarray(A).reshape(-1),
                   index_base=0, is_csc=False, ctx=ctx)
    res = {"dtype": dtype.name, "n": n, "matrix_bytes": n * n * es, "csr_upload_s": round(time.perf_counter() - t0, 2), "csr_kernel": S.spmv_kernel(),
           "csr_stored_bytes": S.spmv_stored_bytes()}
    log(f"  csr uploaded in {res['csr_upload_s']} s, kernel {res['csr_kernel']}")
    ys = pkg.HipVector(n, dtype, ctx)
    pkg.mul_(ys, S, x)
    pkg.mul_(y, M, x)
    res["max_abs_difference_dense_n_vs_csr"] = float(np.abs(ys.to_numpy().astype(np.complex128) - y.to_numpy().astype(np.complex128)).max())
    del A
    routes = {"dense_n": lambda: pkg.mul_(y, M, x), "dense_t": lambda: pkg.mul_(y, M.adj, x), "csr": lambda: pkg.mul_(ys, S, x),
              "real_n": lambda: pkg.mul_(yr, B, xr), "real_t": lambda: pkg.mul_(yr2, B.adj, xr2)}
    inner = max(2, int(round(40e-3 / (n * n * es / 3.0e12))))                                    # ~40 ms per window at 3 TB/s
    us = windows(ctx, routes, inner, reps, warmup)
    res["calls_per_window"] = inner
    for name, v in us.items():
        s = stats(v)
        s["matrix_TBps"] = round(n * n * es / (s["median_us"] * 1e-6) / 1e12, 3)
        res[name] = s
    for form in ("n", "t"):
        d = res[f"dense_{form}"]
        d["over_csr_time"] = round(d["median_us"] / res["csr"]["median_us"], 3)
        d["share_of_real"] = round(d["matrix_TBps"] / res[f"real_{form}"]["matrix_TBps"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_dense_bench.json"))
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    res = {"device": ctx.info()["arch"], "reps": args.reps, "warmup": args.warmup, "shape": {}, "cases": []}
    for dtype in (np.complex128, np.complex64):
        import ctypes as C
        c, r = C.c_int(), C.c_int()
        pkg.lib().mik_dense_mul_shape_for(pkg._lib.dtype_code(dtype), C.byref(c), C.byref(r))
        res["shape"][np.dtype(dtype).name] = {"chunk": c.value, "rows_per_workgroup": r.value}
    for n in (int(v) for v in args.sizes.split(",")):
        for dtype in (np.complex128, np.complex64):
            log(f"n = {n} {np.dtype(dtype).name}")
            res["cases"].append(bench(pkg, ctx, dtype, n, args.reps, args.warmup))
            log("  " + json.dumps(res["cases"][-1]))
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
