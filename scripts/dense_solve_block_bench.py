#!/usr/bin/env python
"""Measurements behind DESIGN.md section 26: writes ONE JSON object (profiles/dense_solve_block_bench.json).

First the bits: at n = 323, for the LU (Float64) and the Cholesky (Float64, ComplexF64), a block solve of G + 1 columns against the
checkers of tests/dense_ref applied column by column and against the vector ldiv_ of every column (same_bits).  Then, for n = 1024, 4096,
8192 and b = 1, 2, 4, 8, 16, 32 columns, ONE block ldiv_(Y, X, cols=b) against b vector ldiv_(y, x) of the same binary on the same handle:
each form between two HIP events on the context's stream, the two forms alternated repetition by repetition, medians of --reps after
--warmup.  `ratio_block_to_vectors` is block / (b vector solves); `ratio_block_to_one_vector` is block / (the b = 1 vector figure) -- the
expectation it tests is that b <= NB columns cost about one vector solve.  Last, one lobpcg run (a dense Float64 operator, cholesky(A) as P,
a block of 8 columns, a fixed number of iterations): the preconditioner routed to one block call against the same factorisation behind an
object that offers vector ldiv_ only (the per-column path), wall clock, alternated, and the two results compared with array_equal.

Usage: python scripts/dense_solve_block_bench.py [--reps 7] [--warmup 2] [--sizes 1024,4096,8192] [--out profiles/dense_solve_block_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import __graft_entry__ as graft  # noqa: E402
from dense_chol_bench import matrix as hermitian  # noqa: E402
from dense_lu_bench import matrix as general, stats, upload  # noqa: E402

WIDTHS = (1, 2, 4, 8, 16, 32)
KINDS = (("lu", np.float64), ("cholesky", np.float64), ("cholesky", np.complex128))


def factor(pkg, ctx, kind, A):
    return (pkg.lu_ if kind == "lu" else pkg.cholesky_)(upload(pkg, ctx, A))


def block_of(pkg, ctx, host):
    M = pkg.HipMatrix(host.shape[0], host.shape[1], host.dtype, ctx)
    pad = np.zeros((M.ld, host.shape[1]), host.dtype, order="F")
    pad[:host.shape[0], :] = host
    M.buf.copy_from_host(pad.ravel(order="F"))
    return M


def download(M):
    return M.buf.to_numpy().reshape((M.ld, M.cols), order="F")[:M.n, :]


def check_bits(pkg, ctx):
    import dense_chol_host as ch
    import dense_lu_host as lh
    import dense_solve_block_host as sb
    tmp = tempfile.mkdtemp()
    lu_ref, chol_ref = lh.build(tmp), ch.build(tmp)
    out = []
    for kind, dtype in KINDS:
        n = 323
        if kind == "lu":
            A = lh.random(n, dtype)
            LU, ipiv, singular = lu_ref.factor(A)
            solve = lambda b: lu_ref.solve(LU, ipiv, b)  # noqa: E731
        else:
            A = ch.hpd(n, dtype)
            L, info = chol_ref.factor(A)
            solve = lambda b: chol_ref.solve(L, b)  # noqa: E731
        F = factor(pkg, ctx, kind, A)
        cols = F.block_plan(1)["G"] + 1
        B = sb.rhs(n, cols, dtype)
        want = sb.per_column(solve, B)
        X, Y = block_of(pkg, ctx, B), block_of(pkg, ctx, np.zeros_like(B))
        F.ldiv_(Y, X)
        got = download(Y)
        y = pkg.HipVector(n, dtype, ctx)
        vec = np.stack([F.ldiv_(y, X.col(j)).to_numpy() for j in range(cols)], axis=1)
        if not (np.isfinite(want).all() and ch.same_bits(got, want) and ch.same_bits(got, vec)):
            raise SystemExit(f"the block solve of {kind} {np.dtype(dtype)} differs from the checker or from the vector solves at n = {n}: nothing is measured")
        out.append({"factorisation": kind, "dtype": np.dtype(dtype).name, "n": n, "columns": cols, "bit_identical_to_checker_and_to_vector_solves": True})
    return out


def alternated(ctx, forms, reps, warmup):
    """microseconds of every form between two HIP events on the context's stream, the forms taking turns within a repetition"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = [[] for _ in forms]
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
                for k, fn in enumerate(forms):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    if it >= warmup:
                        out[k].append(e0.elapsed_time(e1) * 1e3)
    finally:
        ctx.set_stream(None)
    return out


def bench(pkg, ctx, kind, dtype, n, reps, warmup):
    A = general(n, dtype) if kind == "lu" else hermitian(n, dtype)
    F = factor(pkg, ctx, kind, A)
    del A
    rng = np.random.default_rng(1)
    B = rng.standard_normal((n, max(WIDTHS)))
    B = (B + 1j * rng.standard_normal(B.shape) if np.dtype(dtype).kind == "c" else B).astype(dtype)
    X, Y = block_of(pkg, ctx, B), block_of(pkg, ctx, np.zeros_like(B))
    xs, ys = [X.col(j) for j in range(X.cols)], [Y.col(j) for j in range(Y.cols)]
    F.ldiv_(Y, X)                                              # the workspace is allocated here, outside every window
    res = {"factorisation": kind, "dtype": np.dtype(dtype).name, "n": n, "vector_launches": (F.info() if kind == "lu" else F.plan())["launches_solve"], "widths": []}
    one = None
    for b in WIDTHS:
        def block():
            F.ldiv_(Y, X, cols=b)

        def vectors():
            for j in range(b):
                F.ldiv_(ys[j], xs[j])
        tb, tv = alternated(ctx, (block, vectors), reps, warmup)
        row = {"b": b, "plan": F.block_plan(b), "block": stats(tb), "vectors": stats(tv)}
        if b == 1:
            one = row["vectors"]["median_us"]
        row["ratio_block_to_vectors"] = round(row["block"]["median_us"] / row["vectors"]["median_us"], 3)
        row["ratio_block_to_one_vector"] = round(row["block"]["median_us"] / one, 3)
        res["widths"].append(row)
    return res


class VectorOnly:
    """the factorisation behind vector ldiv_ only: lobpcg's per-column path"""

    def __init__(self, F):
        self.F = F

    def ldiv_(self, y, x):
        return self.F.ldiv_(y, x)


def bench_lobpcg(pkg, ctx, n, iterations, reps):
    A = hermitian(n, np.float64)
    M = upload(pkg, ctx, A)
    F = pkg.cholesky(M)
    width = 8
    X0 = np.random.default_rng(3).standard_normal((n, width))
    times, results = {"routed": [], "per_column": []}, {}
    for it in range(reps + 1):
        for name, P in (("routed", F), ("per_column", VectorOnly(F))):
            ctx.synchronize()
            t0 = time.perf_counter()
            results[name] = pkg.lobpcg(M, False, X0, P=P, tol=1e-300, maxiter=iterations, dense=True)
            ctx.synchronize()
            if it:
                times[name].append((time.perf_counter() - t0) * 1e3)
    same = np.array_equal(results["routed"].lam, results["per_column"].lam) and np.array_equal(results["routed"].X.to_numpy(), results["per_column"].X.to_numpy())
    if not same:
        raise SystemExit("lobpcg: the routed and the per-column preconditioner give different results")
    out = {"n": n, "dtype": "float64", "block": width, "iterations": int(results["routed"].iterations), "results_array_equal": True,
           "routed_ms": round(statistics.median(times["routed"]), 2), "per_column_ms": round(statistics.median(times["per_column"]), 2)}
    out["ratio_routed_to_per_column"] = round(out["routed_ms"] / out["per_column_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_solve_block_bench.json"))
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    res = {"device": ctx.info()["arch"], "reps": args.reps, "warmup": args.warmup, "checked_first": check_bits(pkg, ctx), "runs": []}
    for kind, dtype in KINDS:
        for n in (int(v) for v in args.sizes.split(",")):
            res["runs"].append(bench(pkg, ctx, kind, dtype, n, args.reps, args.warmup))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    try:
        res["lobpcg"] = bench_lobpcg(pkg, ctx, 4096, 10, 3)
    except Exception as e:                                     # the solve figures above are kept whatever the eigensolver run does
        res["lobpcg"] = {"error": f"{type(e).__name__}: {e}"}
    print(json.dumps(res["lobpcg"]), file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT), "runs": len(res["runs"])}))


if __name__ == "__main__":
    main()
