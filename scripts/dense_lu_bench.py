#!/usr/bin/env python
"""Measurements behind DESIGN.md section 23: writes ONE JSON object (profiles/dense_lu_bench.json).

First the bits: factors, pivots and one solve at a small n against tests/dense_ref/dense_lu_ref.c (np.array_equal), both types.  Then, for
Float64 and Float32 and n = 1024, 4096, 8192 (standard normal entries: an interchange at almost every step), medians of --reps after
--warmup, timed between two HIP events on the context's stream unless said otherwise:

  factor   one lu_(A) on a fresh copy (the copy is outside the window).  With --families DIR the split by kernel family is added from the
           kernel statistics of a profiler run of `--only-factor` (see below): panel (search, pick, update), interchange, strip solve,
           trailing update, and the trailing update's multiply-subtract rate against the unfused vector rate of the chip (the spec
           peak / 4: a multiply and a subtract are two issue slots, an FMA counts two flops).
  ldiv     one ldiv_(y, F, x), against one y = A x of the same matrix (mik_dense_mul: the same n^2 elements, no serial dependency) and
           against the route it replaces: download, scipy.linalg.lu_solve on the host, upload (wall clock, float64 factors as
           tests/test_gpu_callbacks.py's DenseSolve holds them).
  gmres    one inner iteration of the fused gmres(restart = 30) with Pl = F through mik_dense_lu_ldiv_fn, against the same run with Pl as a
           Python object that forwards to F.ldiv_ (wall clock over 30 iterations / 30; the solves are bit-identical, so the difference is the
           Python frame and the ctypes callback).

`--only-factor N DTYPE REPS` runs REPS factorisations and exits; under `rocprofv3 --kernel-trace --stats -d DIR -o lu_DTYPE_N
--output-format csv -- python scripts/dense_lu_bench.py --only-factor N DTYPE REPS` it leaves DIR/lu_DTYPE_N_kernel_stats.csv.

Usage: python scripts/dense_lu_bench.py [--reps 5] [--warmup 1] [--sizes 1024,4096,8192] [--families DIR] [--out profiles/dense_lu_bench.json]
"""
import argparse
import csv
import glob
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

SPEC_TFLOPS = {"float64": 78.6, "float32": 157.3}          # vector peak, an FMA counted as two flops
FAMILIES = {"k_lu_search": "panel", "k_lu_pick": "panel", "k_lu_update": "panel", "k_lu_swap": "interchange", "k_lu_strip": "strip_solve",
            "k_lu_trail": "trailing_update"}
REPS_TRACED = 2


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def timed(ctx, fn, reps, warmup, before=None):
    """microseconds of fn() between two HIP events on the context's stream, one figure per repetition; before() runs outside the window"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = []
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                if before is not None:
                    before()
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


def wall(ctx, fn, reps, warmup):
    out = []
    for it in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return out


def upload(pkg, ctx, A):
    n = A.shape[0]
    M = pkg.HipMatrix(n, n, A.dtype, ctx)
    padded = A if M.ld == n else np.asfortranarray(np.vstack([A, np.zeros((M.ld - n, n), A.dtype)]))
    M.buf.copy_from_host(padded.ravel(order="F"))
    return M


def matrix(n, dtype):
    return np.asfortranarray(np.random.default_rng(n).standard_normal((n, n)).astype(dtype))


def check_bits(pkg, ctx, ref):
    import dense_lu_host as lh
    out = {}
    for dtype in (np.float64, np.float32):
        n = 323
        A, b = lh.random(n, dtype), lh.vector(n, dtype)
        LU, ipiv, singular = ref.factor(A)
        F = pkg.lu(upload(pkg, ctx, A))
        ok = singular == 0 and np.array_equal(F.ipiv, ipiv) and np.array_equal(F.factors.to_numpy(), LU) and \
            np.array_equal(F.solve(pkg.HipVector.from_numpy(b, ctx)).to_numpy(), ref.solve(LU, ipiv, b))
        if not ok:
            raise SystemExit(f"dense LU differs from the checker at n = {n}, {np.dtype(dtype)}: nothing is measured")
        out[np.dtype(dtype).name] = {"n": n, "bit_identical_to_checker": True}
    return out


def trailing_pairs(n, W):
    """multiply-subtracts of the trailing updates of one factorisation"""
    return sum((n - k1) ** 2 * W for k1 in range(W, n, W))


def family_split(directory, dtype, n, W):
    found = glob.glob(os.path.join(directory, "**", f"lu_{dtype}_{n}_kernel_stats.csv"), recursive=True)
    if not found:
        return None
    split = {v: 0.0 for v in FAMILIES.values()}
    calls = 0
    with open(found[0]) as f:
        rows = csv.DictReader(f)
        col = {what: next(c for c in rows.fieldnames if what in c.lower()) for what in ("name", "calls", "total")}    # Name, Calls, TotalDurationNs
        assert "ns" in col["total"].lower(), col
        for row in rows:
            for key, fam in FAMILIES.items():
                if key in row[col["name"]]:
                    split[fam] += float(row[col["total"]]) / 1e3 / REPS_TRACED
                    calls += int(row[col["calls"]])
    out = {k + "_us": round(v, 1) for k, v in split.items()}
    out["kernel_sum_us"] = round(sum(split.values()), 1)
    out["launches_traced_per_factorisation"] = calls // REPS_TRACED
    if split["trailing_update"] > 0:
        rate = trailing_pairs(n, W) / (split["trailing_update"] * 1e-6)
        yard = SPEC_TFLOPS[dtype] * 1e12 / 4
        out["trailing_multiply_subtracts_per_s"] = float(f"{rate:.4g}")
        out["unfused_vector_rate_per_s"] = yard
        out["trailing_share_of_unfused_vector_rate"] = round(rate / yard, 4)
    return out


class PythonLdiv:
    def __init__(self, F):
        self.F = F

    def ldiv_(self, y, x=None):
        return self.F.ldiv_(y, x)


def bench(pkg, ctx, n, dtype, reps, warmup, families):
    import scipy.linalg
    name = np.dtype(dtype).name
    A = matrix(n, dtype)
    M = upload(pkg, ctx, A)
    work = pkg.HipMatrix(n, n, dtype, ctx)
    holder = {}

    def fresh():
        work.buf.copyto_(M.buf)

    def factor():
        holder["F"] = None                                   # the previous handle goes first: it refers to `work`
        holder["F"] = pkg.lu_(work)
    res = {"n": n, "dtype": name, "factor": stats(timed(ctx, factor, reps, warmup, before=fresh))}
    F = holder["F"]
    info = F.info()
    res["info"] = info
    if families:
        split = family_split(families, name, n, info["W"])
        if split:
            res["factor"]["families"] = split
    rng = np.random.default_rng(1)
    b = rng.standard_normal(n).astype(dtype)
    x, y = pkg.HipVector.from_numpy(b, ctx), pkg.HipVector(n, dtype, ctx).fill_(0)
    res["ldiv"] = stats(timed(ctx, lambda: F.ldiv_(y, x), 4 * reps, warmup))
    res["ldiv"]["us_per_launch"] = round(res["ldiv"]["median_us"] / info["launches_solve"], 2)
    res["mul"] = stats(timed(ctx, lambda: pkg.mul_(y, M, x), 4 * reps, warmup))
    res["ldiv"]["ratio_to_mul"] = round(res["ldiv"]["median_us"] / res["mul"]["median_us"], 1)
    host_lu = scipy.linalg.lu_factor(A.astype(np.float64))

    def host_route():
        v = scipy.linalg.lu_solve(host_lu, x.to_numpy().astype(np.float64))
        y.copyto_(pkg.HipVector.from_numpy(v.astype(dtype), ctx))
    res["host_route"] = stats(wall(ctx, host_route, reps, warmup))
    res["ldiv"]["ratio_to_host_route"] = round(res["ldiv"]["median_us"] / res["host_route"]["median_us"], 2)
    # fused gmres(restart = 30): Pl = lu of a nearby matrix, 30 inner iterations
    near = pkg.lu(upload(pkg, ctx, (A + 0.01 * rng.standard_normal((n, n)).astype(dtype)).astype(dtype)))
    iters = {}

    def run(P, key):
        _, h = pkg.gmres(M, x, Pl=P, restart=30, maxiter=30, reltol=0.0, log=True)
        iters[key] = h.iters
    lib_us = wall(ctx, lambda: run(near, "library"), reps, warmup)
    py_us = wall(ctx, lambda: run(PythonLdiv(near), "python"), reps, warmup)
    res["gmres30"] = {"inner_iterations": iters, "library_callback_us_per_iteration": round(statistics.median(lib_us) / max(iters["library"], 1), 1),
                      "python_callback_us_per_iteration": round(statistics.median(py_us) / max(iters["python"], 1), 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--families", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_lu_bench.json"))
    ap.add_argument("--only-factor", nargs=3, metavar=("N", "DTYPE", "REPS"), default=None)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    if args.only_factor:
        n, dtype, reps = int(args.only_factor[0]), np.dtype(args.only_factor[1]), int(args.only_factor[2])
        M = upload(pkg, ctx, matrix(n, dtype))
        for _ in range(reps):
            pkg.lu(M)
        ctx.synchronize()
        return
    import dense_lu_host as lh
    ref = lh.build(tempfile.mkdtemp())
    res = {"device": ctx.info()["arch"], "reps": args.reps, "warmup": args.warmup, "spec_vector_TFLOPS": SPEC_TFLOPS, "checked_first": check_bits(pkg, ctx, ref),
           "runs": []}
    for dtype in (np.float64, np.float32):
        for n in (int(v) for v in args.sizes.split(",")):
            res["runs"].append(bench(pkg, ctx, n, dtype, args.reps, args.warmup, args.families))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT), "runs": len(res["runs"])}))


if __name__ == "__main__":
    main()
