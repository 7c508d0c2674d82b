#!/usr/bin/env python
"""Measurements behind DESIGN.md section 12: prints ONE JSON object.

  rotate   mik_basis_rotate against the same product composed the only way the library could do it before (l calls of mik_gemv_n into
           zeroed columns), fp64 / fp32, n = 2^20 / 2^24, (k, l) = (12, 6) / (40, 20): microseconds (HIP events on the context's stream,
           median of --reps after --warmup), the fraction of the 6.29 TB/s copy ceiling that the algorithmic traffic (k + l) n sizeof(T)
           reaches, and the same for the composed form with its l (k + 2) n sizeof(T) bytes;
  reorth   mik_svdl_reorth against the chain of calls that defines it (mik_nrm2, mik_gemv_t, mik_gemv_n, mik_nrm2, mik_scal), same table
           (one Gram-Schmidt pass; k basis vectors);
  svdl     one full svdl on the large case of tests/test_gpu_svdl.py: wall time per restart and its split into SpMV, re-orthogonalisation,
           rotation and host SVD (each bracketed by a stream synchronisation, so the parts are upper bounds).

Usage: python scripts/svdl_bench.py [--reps 20] [--warmup 3] [--small] > profiles/svdl_bench.json
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

COPY_CEILING = 6.29e12      # bytes / s, the copy ceiling BASELINE.md quotes
_vp = C.c_void_p


def timed(ctx, fn, before, reps, warmup):
    """median microseconds of fn() between two HIP events on the context's stream; before() runs outside the bracket"""
    import torch
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    out = []
    try:
        with torch.cuda.stream(stream):
            for it in range(warmup + reps):
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
    return statistics.median(out)


def bench_rotate(pkg, ctx, dt, n, k, l, reps, warmup):
    rng = np.random.default_rng(0)
    es = np.dtype(dt).itemsize
    V, Y = pkg.HipMatrix(n, k, dt, ctx), pkg.HipMatrix(n, l, dt, ctx)
    col = rng.standard_normal(n).astype(dt)
    for j in range(k):
        V.col(j).copy_from_host(np.roll(col, j))
    F = np.asfortranarray(rng.standard_normal((k, l)).astype(dt))
    code = pkg._lib.dtype_code(dt)
    L = pkg.lib()

    def new():
        pkg._lib.check(L.mik_basis_rotate(ctx.handle, code, n, k, l, _vp(V.buf.ptr), V.ld, F.ctypes.data_as(_vp), k, _vp(Y.buf.ptr), Y.ld),
                       "mik_basis_rotate", ctx.handle)

    def old():
        for j in range(l):
            pkg.gemv_n_(Y.col(j), V, k, F[:, j], 1.0)

    t_new = timed(ctx, new, lambda: None, reps, warmup)
    t_old = timed(ctx, old, lambda: Y.buf.fill_(0), reps, warmup)
    b_new, b_old = (k + l) * n * es, l * (k + 2) * n * es
    return {"dtype": np.dtype(dt).name, "n": n, "k": k, "l": l, "rotate_us": round(t_new, 1), "rotate_fraction_of_copy_ceiling": round(b_new / (t_new * 1e-6) / COPY_CEILING, 3),
            "composed_us": round(t_old, 1), "composed_fraction_of_copy_ceiling": round(b_old / (t_old * 1e-6) / COPY_CEILING, 3),
            "gain": round(t_old / t_new, 2), "byte_ratio": round(b_old / b_new, 2)}


def bench_reorth(pkg, ctx, dt, n, k, reps, warmup):
    rng = np.random.default_rng(1)
    es = np.dtype(dt).itemsize
    T = np.dtype(dt).type
    Q = pkg.HipMatrix(n, k, dt, ctx)
    col = rng.standard_normal(n).astype(dt)
    for j in range(k):
        Q.col(j).copy_from_host(np.roll(col, 7 * j) / np.linalg.norm(col))      # not orthonormal: timing only, one pass either way
    q0 = pkg.HipVector.from_numpy(rng.standard_normal(n).astype(dt), ctx)
    q = q0.similar()
    code = pkg._lib.dtype_code(dt)
    L = pkg.lib()
    alpha, beta, passes = np.zeros(1, dt), np.zeros(1, dt), C.c_int(0)         # alpha = 0: never a second pass

    def new():
        pkg._lib.check(L.mik_svdl_reorth(ctx.handle, code, n, k, _vp(Q.buf.ptr), Q.ld, _vp(q.ptr), alpha.ctypes.data_as(_vp), beta.ctypes.data_as(_vp),
                                         C.byref(passes)), "mik_svdl_reorth", ctx.handle)

    def old():
        pkg.norm(q)
        pkg.gemv_n_(q, Q, k, pkg.gemv_t_(Q, k, q), -1)
        nw = pkg.norm(q)
        q.scal_(T(1) / nw)

    t_new = timed(ctx, new, lambda: q.copyto_(q0), reps, warmup)
    t_old = timed(ctx, old, lambda: q.copyto_(q0), reps, warmup)
    b_new, b_old = (2 * k + 5) * n * es, (2 * k + 7) * n * es
    return {"dtype": np.dtype(dt).name, "n": n, "k": k, "reorth_us": round(t_new, 1), "reorth_fraction_of_copy_ceiling": round(b_new / (t_new * 1e-6) / COPY_CEILING, 3),
            "chain_us": round(t_old, 1), "chain_fraction_of_copy_ceiling": round(b_old / (t_old * 1e-6) / COPY_CEILING, 3), "gain": round(t_old / t_new, 2)}


def bench_svdl(pkg, ctx, n):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_svdl_host import big_case
    import importlib
    mod = importlib.import_module(pkg.__name__ + ".svdl")
    A, d, kw = big_case(n)
    Ad = pkg.extras.with_adjoint_from_scipy(A)
    parts = {"spmv": 0.0, "reorth": 0.0, "rotate": 0.0, "host_svd": 0.0}

    def bracket(name, fn):
        def run(*a, **k):
            ctx.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            ctx.synchronize()
            parts[name] += time.perf_counter() - t
            return out
        return run

    ops = mod.DeviceOps(Ad)
    ops.mul, ops.mul_adj = bracket("spmv", ops.mul), bracket("spmv", ops.mul_adj)
    ops.reorth, ops.rotate = bracket("reorth", ops.reorth), bracket("rotate", ops.rotate)
    real_svd = mod._Bsvd
    mod._Bsvd = bracket("host_svd", real_svd)
    try:
        pkg.svdl(Ad, ops=mod.DeviceOps(Ad), **kw)                      # warm-up: kernels loaded, workspace grown
        for key in parts:
            parts[key] = 0.0
        ctx.synchronize()
        t = time.perf_counter()
        s, L, h = pkg.svdl(Ad, log=True, ops=ops, **kw)
        ctx.synchronize()
        wall = time.perf_counter() - t
    finally:
        mod._Bsvd = real_svd
    out = {"m": A.shape[0], "n": n, "nsv": kw["nsv"], "k": 2 * kw["nsv"], "restarts": h.iters, "converged": bool(h.isconverged), "mvps": h.mvps, "mtvps": h.mtvps,
           "wall_ms_per_restart": round(wall * 1e3 / h.iters, 3), "error": float(np.linalg.norm(s - d[:6]))}
    out.update({f"{key}_ms_per_restart": round(v * 1e3 / h.iters, 3) for key, v in parts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="n = 2^16 only (a quick check of the script)")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    sizes = [2 ** 16] if args.small else [2 ** 20, 2 ** 24]
    res = {"device": ctx.info()["arch"], "copy_ceiling_TBps": COPY_CEILING / 1e12, "reps": args.reps, "rotate": [], "reorth": []}
    for dt in (np.float64, np.float32):
        for n in sizes:
            for (k, l) in ((12, 6), (40, 20)):
                res["rotate"].append(bench_rotate(pkg, ctx, dt, n, k, l, args.reps, args.warmup))
                res["reorth"].append(bench_reorth(pkg, ctx, dt, n, k, args.reps, args.warmup))
    res["svdl"] = bench_svdl(pkg, ctx, sizes[0] if args.small else 2 ** 20)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
