#!/usr/bin/env python
"""Measurements behind DESIGN.md section 27: writes ONE JSON object (profiles/dense_qr_bench.json).

First the bits: factors, tau, one solve and the thin Q at a small shape against tests/dense_ref/dense_qr_ref.c, both types, both forms of
the apply kernel.  Then medians of --reps after --warmup, timed between two HIP events on the context's stream unless said otherwise:

  square   Float64, n = 1024, 4096, 8192 (standard normal entries): one qr_(A) on a fresh copy (the copy is outside the window) against one
           lu_(A) of the same library on the same matrix, and against the host route qr_ replaces: download, numpy.linalg.qr (mode "raw":
           LAPACK's geqrf, factors and tau), upload (wall clock).  One F.solve(b) against the LU's ldiv_ and against download +
           numpy.linalg.lstsq + upload.  With --families DIR the split of qr_ by kernel family (k_qr_panel, k_qr_apply) is added from the
           kernel statistics of a profiler run of `--only-factor`.
  tall     Float64, m = 2^20 with n = 8 and n = 32: qr_ and one solve against the same host routes.  Rows are not split across workgroups,
           so these shapes run on at most n compute units.

`--only-factor M N REPS` runs REPS factorisations and exits; under `rocprofv3 --kernel-trace --stats -d DIR -o qr_M_N --output-format csv --
python scripts/dense_qr_bench.py --only-factor M N REPS` it leaves DIR/qr_M_N_kernel_stats.csv.

Usage: python scripts/dense_qr_bench.py [--reps 5] [--warmup 1] [--sizes 1024,4096,8192] [--tall 8,32] [--families DIR] [--lstsq-max 4096] [--out profiles/dense_qr_bench.json]
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

FAMILIES = {"k_qr_panel": "panel", "k_qr_apply": "trailing_update"}
REPS_TRACED = 2
TALL_ROWS = 1 << 20


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
    m, n = A.shape
    M = pkg.HipMatrix(m, n, A.dtype, ctx)
    padded = A if M.ld == m else np.asfortranarray(np.vstack([A, np.zeros((M.ld - m, n), A.dtype)]))
    M.buf.copy_from_host(padded.ravel(order="F"))
    return M


def matrix(m, n, dtype):
    return np.asfortranarray(np.random.default_rng(m + n).standard_normal((m, n)).astype(dtype))


def check_bits(pkg, ctx, ref):
    import dense_qr_host as qh
    out = {}
    for dtype in (np.float64, np.float32):
        m, n = 323, 70
        A, b = qh.random(m, n, dtype), qh.vector(m, dtype)
        QR, tau, z = ref.factor(A)
        for rows in (0, m - 1):
            F = pkg.qr(upload(pkg, ctx, A), resident_rows=rows)
            ok = z == 0 and F.info()["resident"] == (rows == 0) and qh.same_bits(F.factors.to_numpy(), QR) and qh.same_bits(F.tau, tau) and \
                qh.same_bits(F.solve(pkg.HipVector.from_numpy(b, ctx)).to_numpy(), ref.solve(QR, tau, b)) and qh.same_bits(F.Q().to_numpy(), ref.thin_q(QR, tau))
            if not ok:
                raise SystemExit(f"dense QR differs from the checker at {m} x {n}, {np.dtype(dtype)}, resident_rows = {rows}: nothing is measured")
        out[np.dtype(dtype).name] = {"m": m, "n": n, "bit_identical_to_checker": True, "forms": ["resident", "streaming"]}
    return out


def family_split(directory, m, n):
    found = glob.glob(os.path.join(directory, "**", f"qr_{m}_{n}_kernel_stats.csv"), recursive=True)
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
    return out


def bench(pkg, ctx, m, n, dtype, reps, warmup, families, with_lu, lstsq_max):
    name = np.dtype(dtype).name
    A = matrix(m, n, dtype)
    M = upload(pkg, ctx, A)
    work = pkg.HipMatrix(m, n, dtype, ctx)
    holder = {}

    def fresh():
        holder["F"] = None                                   # the previous handle goes first: it refers to `work`
        work.buf.copyto_(M.buf)

    def factor_qr():
        holder["F"] = pkg.qr_(work)

    def factor_lu():
        holder["F"] = pkg.lu_(work)
    res = {"m": m, "n": n, "dtype": name, "qr": stats(timed(ctx, factor_qr, reps, warmup, before=fresh))}
    F = holder["F"]
    res["info"] = F.info()
    if families:
        split = family_split(families, m, n)
        if split:
            res["qr"]["families"] = split
    b = np.random.default_rng(1).standard_normal(m).astype(dtype)
    db, x = pkg.HipVector.from_numpy(b, ctx), pkg.HipVector(n, dtype, ctx).fill_(0)
    res["solve"] = stats(timed(ctx, lambda: F.ldiv_(x, db), 2 * reps, warmup))

    def download():                                          # one copy of the whole buffer
        return M.buf.to_numpy().reshape(n, M.ld).T[:m]

    def host_qr():
        f, tau = np.linalg.qr(download(), mode="raw")
        work.buf.copy_from_host(np.asfortranarray(np.vstack([f.T, np.zeros((work.ld - m, n), dtype)])).ravel(order="F"))
    res["host_qr_route"] = stats(wall(ctx, host_qr, max(reps // 2, 2), 0))
    res["qr"]["ratio_to_host_route"] = round(res["qr"]["median_us"] / res["host_qr_route"]["median_us"], 3)

    def host_lstsq():
        v = np.linalg.lstsq(download(), db.to_numpy(), rcond=None)[0]
        x.copyto_(pkg.HipVector.from_numpy(v.astype(dtype), ctx))
    if n <= lstsq_max:                                       # numpy's lstsq is an SVD: minutes per call on a large square matrix
        res["host_lstsq_route"] = stats(wall(ctx, host_lstsq, 2, 0))
        res["solve"]["ratio_to_host_route"] = round(res["solve"]["median_us"] / res["host_lstsq_route"]["median_us"], 4)
    else:
        res["host_lstsq_route"] = f"not run: n > --lstsq-max = {lstsq_max}"
    if with_lu:
        res["lu"] = stats(timed(ctx, factor_lu, reps, warmup, before=fresh))
        L = holder["F"]
        y = pkg.HipVector(n, dtype, ctx).fill_(0)
        res["lu_ldiv"] = stats(timed(ctx, lambda: L.ldiv_(y, db), 2 * reps, warmup))
        res["qr"]["ratio_to_lu"] = round(res["qr"]["median_us"] / res["lu"]["median_us"], 2)
        res["solve"]["ratio_to_lu_ldiv"] = round(res["solve"]["median_us"] / res["lu_ldiv"]["median_us"], 2)
    holder["F"] = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--tall", default="8,32")
    ap.add_argument("--families", default=None)
    ap.add_argument("--lstsq-max", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_qr_bench.json"))
    ap.add_argument("--only-factor", nargs=3, metavar=("M", "N", "REPS"), default=None)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    if args.only_factor:
        m, n, reps = (int(v) for v in args.only_factor)
        M = upload(pkg, ctx, matrix(m, n, np.float64))
        for _ in range(reps):
            pkg.qr(M)
        ctx.synchronize()
        return
    import dense_qr_host as qh
    ref = qh.build(tempfile.mkdtemp())
    res = {"device": ctx.info()["arch"], "reps": args.reps, "warmup": args.warmup, "checked_first": check_bits(pkg, ctx, ref), "square": [], "tall": []}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    for n in (int(v) for v in args.sizes.split(",") if v):
        res["square"].append(bench(pkg, ctx, n, n, np.float64, args.reps, args.warmup, args.families, True, args.lstsq_max))
        print(json.dumps(res["square"][-1]), file=sys.stderr, flush=True)
        save()
    for n in (int(v) for v in args.tall.split(",") if v):
        res["tall"].append(bench(pkg, ctx, TALL_ROWS, n, np.float64, args.reps, args.warmup, args.families, False, args.lstsq_max))
        print(json.dumps(res["tall"][-1]), file=sys.stderr, flush=True)
        save()
    print(json.dumps({"written": os.path.relpath(args.out, ROOT), "square": len(res["square"]), "tall": len(res["tall"])}))


if __name__ == "__main__":
    main()
