#!/usr/bin/env python
"""Measurements behind DESIGN.md section 17: prints ONE JSON object.

On the 128^3 Laplacian pattern (n = 2,097,152 rows, 14,581,760 entries) with ComplexF64 values (the Laplacian plus a Hermitian imaginary
part on the same pattern):

  spmv_c64        mik_spmv on the complex operator (k_spmv_complex)
  spmv_f64_csr    the yardstick: the real Float64 mik_spmv on the same pattern pinned to its CSR arrays (set_layout("csr"), k_spmv_rowgather)
  dot_c64         mik_dot, one complex scalar back on the host per call
  mgs_c64_k30     mik_orthogonalize(ModifiedGramSchmidt) against k = 30 basis columns, h and nrm back on the host
  cg_step_c64     one step of the generic cg iterable (xpby, SpMV, dot, two axpy, norm: two host waits)

The two SpMV figures are microseconds per call between two HIP events around `--inner` back-to-back calls (mik_time_spmv), the two
operators alternating inside every repetition; the other three are a host clock around calls that each end in the host wait for their
scalar.  Every window lasts 10 ms or more.  Median / minimum / maximum of --reps windows after --warmup.  `bytes` is the SURVEY section 8d count nnz (s + 4) + (n + 1) 4 +
2 n s with s = sizeof(element); `TBps` = bytes / median time; `per_byte_ratio` = the complex SpMV's rate over the real row-gather
kernel's (1.0: as close to the memory system per byte moved).

Usage: python scripts/complex_bench.py [--N 128] [--reps 9] [--warmup 2] [--inner 400] > profiles/complex_bench.json
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

HBM_PEAK = 8.0e12        # bytes / s, the MI355X specification


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stats(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "windows": len(us)}


def host_windows(ctx, fn, inner, reps, warmup, setup=None):
    out = []
    for it in range(warmup + reps):
        if setup is not None:
            setup()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.synchronize()
        if it >= warmup:
            out.append((time.perf_counter() - t0) * 1e6 / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=400)
    args = ap.parse_args()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(args.N, 3)
    nnz = int(nzval.size)
    rows = rowval - 1
    cols = np.repeat(np.arange(n), np.diff(colptr))
    cval = nzval.astype(np.complex128)
    cval[rows == cols] += 0.01                     # keeps the Hermitian operator positive definite for the cg step
    cval[rows < cols] += 0.1j
    cval[rows > cols] -= 0.1j
    log(f"uploading {n} x {n}, {nnz} entries")
    Ar = pkg.HipCSR(n, n, colptr, rowval, nzval, index_base=1, ctx=ctx).set_layout("csr")
    Ac = pkg.HipCSR(n, n, colptr, rowval, cval, index_base=1, ctx=ctx)
    rng = np.random.default_rng(0)
    xr = pkg.HipVector.from_numpy(rng.standard_normal(n), ctx)
    yr = xr.similar()
    xc = pkg.HipVector.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n), ctx)
    yc = xc.similar()
    res = {"N": args.N, "n": n, "nnz": nnz, "info": {k: ctx.info()[k] for k in ("arch", "compute_units", "xcds")},
           "kernels": {"spmv_c64": Ac.spmv_kernel(), "spmv_f64_csr": Ar.spmv_kernel()}}
    assert res["kernels"]["spmv_f64_csr"] == "k_spmv_rowgather", res["kernels"]
    # the two products agree with the host at this size before anything is timed
    import scipy.sparse as sp
    M = sp.csc_matrix((cval, rows, colptr - 1), shape=(n, n))
    err = np.max(np.abs(pkg.mul_(yc, Ac, xc).to_numpy() - M @ xc.to_numpy()))
    assert err < 1e-12 * 14, err
    t = {"spmv_c64": [], "spmv_f64_csr": []}
    for it in range(args.warmup + args.reps):
        for name, A, x, y in (("spmv_c64", Ac, xc, yc), ("spmv_f64_csr", Ar, xr, yr)):
            us = A.time_spmv(x, y, reps=args.inner) * 1e3
            if it >= args.warmup:
                t[name].append(us)
    for name, A in (("spmv_c64", Ac), ("spmv_f64_csr", Ar)):
        s = stats(t[name])
        s["bytes"] = A.spmv_algorithmic_bytes()
        s["TBps"] = s["bytes"] / s["median_us"] / 1e6
        s["share_of_hbm_peak"] = s["TBps"] * 1e12 / HBM_PEAK
        res[name] = s
    res["per_byte_ratio"] = res["spmv_c64"]["TBps"] / res["spmv_f64_csr"]["TBps"]
    log("spmv done", res["per_byte_ratio"])
    res["dot_c64"] = stats(host_windows(ctx, lambda: pkg.dot(xc, yc), args.inner, args.reps, args.warmup))
    res["dot_c64"]["bytes"] = 2 * n * 16
    k = 30
    V = pkg.HipMatrix(n, k, np.complex128, ctx)
    for j in range(k):
        V.col(j).copy_from_host((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2 * n))
    w0 = xc.copy()
    w, h = xc.similar(), np.zeros(k, np.complex128)

    def mgs():
        w.copyto_(w0)
        pkg.orthogonalize_and_normalize_(V, k, w, h)
    res["mgs_c64_k30"] = stats(host_windows(ctx, mgs, 20, args.reps, args.warmup))
    res["mgs_c64_k30"]["bytes"] = (k + 2 * k + 2 + 2) * n * 16          # k columns, w read and written per pass, the scale, the copy
    del V
    b = pkg.HipVector.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n), ctx)
    state = {}

    def fresh():                                      # every window: the first 60 steps of a solve from x = 0 (it has not converged by then)
        state["it"], state["i"] = pkg.cg_iterator_(b.zero(), Ac, b, reltol=1e-30, maxiter=10 ** 6, initially_zero=True), 0

    def step():
        _res, state["i"] = state["it"].iterate(state["i"])
    res["cg_step_c64"] = stats(host_windows(ctx, step, 60, args.reps, args.warmup, setup=fresh))
    res["cg_step_c64"]["bytes"] = Ac.spmv_algorithmic_bytes() + (3 + 2 + 3 + 3 + 1) * n * 16
    for name in ("dot_c64", "mgs_c64_k30", "cg_step_c64"):
        res[name]["TBps"] = res[name]["bytes"] / res[name]["median_us"] / 1e6
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
