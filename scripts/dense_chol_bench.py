#!/usr/bin/env python
"""Measurements behind DESIGN.md section 24: writes ONE JSON object (profiles/dense_chol_bench.json).

First the bits: the factor and one solve at a small n against tests/dense_ref/dense_chol_ref.c (same_bits), all four types.  Then, for
Float64 and ComplexF64 and n = 1024, 4096, 8192 (a Hermitian matrix with uniform entries and a dominant real diagonal), medians of --reps
after --warmup, timed between two HIP events on the context's stream unless said otherwise:

  factor   one cholesky_(A) on a fresh copy (the copy is outside the window) and -- Float64 -- one lu_(A) of the same binary on the same
           matrix.  With --families DIR the split by kernel family is added from the kernel statistics of a profiler run of
           `--only-factor` (see below): diagonal block, panel rows, trailing update, and the trailing update's multiply-subtract rate
           against the unfused vector rate of the chip (the spec peak / 4; a complex multiply-subtract counts as four real ones).
  ldiv     one ldiv_(y, F, x), split into its forward and backward half when --families has the kernel statistics, against the LU's ldiv_
           (Float64), against one y = A x of the same matrix, and against the route it replaces: download, scipy.linalg.cho_solve on the
           host, upload (wall clock).

`--only-factor N DTYPE REPS` runs REPS factorisations and REPS solves and exits; under `rocprofv3 --kernel-trace --stats -d DIR -o
chol_DTYPE_N --output-format csv -- python scripts/dense_chol_bench.py --only-factor N DTYPE REPS` it leaves DIR/chol_DTYPE_N_kernel_stats.csv.

Usage: python scripts/dense_chol_bench.py [--reps 5] [--warmup 1] [--sizes 1024,4096,8192] [--families DIR] [--out profiles/dense_chol_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import __graft_entry__ as graft  # noqa: E402
from dense_lu_bench import SPEC_TFLOPS, stats, timed, upload, wall  # noqa: E402

FAMILIES = {"k_chol_diag": "diagonal_block", "k_chol_panel": "panel_rows", "k_chol_trail": "trailing_update", "k_chol_fwd": "solve_forward",
            "k_chol_bwd": "solve_backward"}
REPS_TRACED = 2
DTYPES = (np.float64, np.complex128)


def matrix(n, dtype):
    """Hermitian, uniform(-1, 1) components off the diagonal, a real diagonal of 2 n: strictly diagonally dominant, so positive definite"""
    rng = np.random.default_rng(n)
    G = rng.uniform(-1.0, 1.0, (n, n))
    if np.dtype(dtype).kind == "c":
        G = G + 1j * rng.uniform(-1.0, 1.0, (n, n))
    A = np.tril(G, -1)
    A = A + A.conj().T + 2.0 * n * np.eye(n)
    return np.asfortranarray(A.astype(dtype))


def check_bits(pkg, ctx, ref):
    import dense_chol_host as ch
    out = {}
    for dtype in ch.DTYPES:
        n = 323
        A, b = ch.hpd(n, dtype), ch.vector(n, dtype)
        want, info = ref.factor(A)
        F = pkg.cholesky(upload(pkg, ctx, A))
        ok = info == 0 and F.info == 0 and ch.same_bits(F.factors.to_numpy(), want) and \
            ch.same_bits(F.solve(pkg.HipVector.from_numpy(b, ctx)).to_numpy(), ref.solve(want, b))
        if not ok:
            raise SystemExit(f"dense Cholesky differs from the checker at n = {n}, {np.dtype(dtype)}: nothing is measured")
        out[np.dtype(dtype).name] = {"n": n, "bit_identical_to_checker": True}
    return out


def trailing_pairs(n, W):
    """multiply-subtracts of the trailing updates of one factorisation: the lower triangle of every trailing block, diagonal included"""
    return sum((n - k1) * (n - k1 + 1) // 2 * W for k1 in range(W, n, W))


def family_split(directory, dtype, n, W):
    found = glob.glob(os.path.join(directory, "**", f"chol_{dtype}_{n}_kernel_stats.csv"), recursive=True)
    if not found:
        return None
    split = {v: 0.0 for v in FAMILIES.values()}
    calls = {v: 0 for v in FAMILIES.values()}
    with open(found[0]) as f:
        rows = csv.DictReader(f)
        col = {what: next(c for c in rows.fieldnames if what in c.lower()) for what in ("name", "calls", "total")}    # Name, Calls, TotalDurationNs
        assert "ns" in col["total"].lower(), col
        for row in rows:
            for key, fam in FAMILIES.items():
                if key in row[col["name"]]:
                    split[fam] += float(row[col["total"]]) / 1e3 / REPS_TRACED
                    calls[fam] += int(row[col["calls"]])
    out = {k + "_us": round(v, 1) for k, v in split.items()}
    out["factor_kernel_sum_us"] = round(split["diagonal_block"] + split["panel_rows"] + split["trailing_update"], 1)
    out["launches_traced_per_factorisation"] = (calls["diagonal_block"] + calls["panel_rows"] + calls["trailing_update"]) // REPS_TRACED
    out["launches_traced_per_solve"] = (calls["solve_forward"] + calls["solve_backward"]) // REPS_TRACED
    if split["trailing_update"] > 0:
        real_pairs = trailing_pairs(n, W) * (4 if dtype.startswith("complex") else 1)
        rate = real_pairs / (split["trailing_update"] * 1e-6)
        yard = SPEC_TFLOPS["float64"] * 1e12 / 4
        out["trailing_real_multiply_subtracts_per_s"] = float(f"{rate:.4g}")
        out["unfused_vector_rate_per_s"] = yard
        out["trailing_share_of_unfused_vector_rate"] = round(rate / yard, 4)
    return out


def bench(pkg, ctx, n, dtype, reps, warmup, families):
    import scipy.linalg
    name = np.dtype(dtype).name
    A = matrix(n, dtype)
    M = upload(pkg, ctx, A)
    work = pkg.HipMatrix(n, n, dtype, ctx)
    holder = {}

    def fresh():
        work.buf.copyto_(M.buf)

    def factor(make):
        def run():
            holder["F"] = None                               # the previous handle goes first: it refers to `work`
            holder["F"] = make(work)
        return run
    res = {"n": n, "dtype": name}
    if name == "float64":
        res["lu_factor"] = stats(timed(ctx, factor(pkg.lu_), reps, warmup, before=fresh))
    res["factor"] = stats(timed(ctx, factor(pkg.cholesky_), reps, warmup, before=fresh))
    F = holder["F"]
    plan = F.plan()
    res["plan"] = plan
    if "lu_factor" in res:
        res["factor"]["ratio_to_lu"] = round(res["factor"]["median_us"] / res["lu_factor"]["median_us"], 3)
    if families:
        split = family_split(families, name, n, plan["W"])
        if split:
            res["factor"]["families"] = split
    rng = np.random.default_rng(1)
    b = rng.standard_normal(n).astype(dtype)
    x, y = pkg.HipVector.from_numpy(b, ctx), pkg.HipVector(n, dtype, ctx).fill_(0)
    res["ldiv"] = stats(timed(ctx, lambda: F.ldiv_(y, x), 4 * reps, warmup))
    res["ldiv"]["us_per_launch"] = round(res["ldiv"]["median_us"] / plan["launches_solve"], 2)
    res["mul"] = stats(timed(ctx, lambda: pkg.mul_(y, M, x), 4 * reps, warmup))
    res["ldiv"]["ratio_to_mul"] = round(res["ldiv"]["median_us"] / res["mul"]["median_us"], 1)
    if name == "float64":
        G = pkg.lu(M)
        res["lu_ldiv"] = stats(timed(ctx, lambda: G.ldiv_(y, x), 4 * reps, warmup))
        res["ldiv"]["ratio_to_lu_ldiv"] = round(res["ldiv"]["median_us"] / res["lu_ldiv"]["median_us"], 2)
        del G
    host = scipy.linalg.cho_factor(A, lower=True)

    def host_route():
        v = scipy.linalg.cho_solve(host, x.to_numpy())
        y.copyto_(pkg.HipVector.from_numpy(v.astype(dtype), ctx))
    res["host_route"] = stats(wall(ctx, host_route, reps, warmup))
    res["ldiv"]["ratio_to_host_route"] = round(res["ldiv"]["median_us"] / res["host_route"]["median_us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--families", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_chol_bench.json"))
    ap.add_argument("--only-factor", nargs=3, metavar=("N", "DTYPE", "REPS"), default=None)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    if args.only_factor:
        n, dtype, reps = int(args.only_factor[0]), np.dtype(args.only_factor[1]), int(args.only_factor[2])
        M = upload(pkg, ctx, matrix(n, dtype))
        x = pkg.HipVector(n, dtype, ctx).fill_(1)
        for _ in range(reps):
            pkg.cholesky(M).ldiv_(pkg.HipVector(n, dtype, ctx).fill_(0), x)
        ctx.synchronize()
        return
    import dense_chol_host as ch
    ref = ch.build(tempfile.mkdtemp())
    res = {"device": ctx.info()["arch"], "reps": args.reps, "warmup": args.warmup, "spec_vector_TFLOPS": SPEC_TFLOPS, "checked_first": check_bits(pkg, ctx, ref),
           "runs": []}
    for dtype in DTYPES:
        for n in (int(v) for v in args.sizes.split(",")):
            res["runs"].append(bench(pkg, ctx, n, dtype, args.reps, args.warmup, args.families))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": os.path.relpath(args.out, ROOT), "runs": len(res["runs"])}))


if __name__ == "__main__":
    main()
