#!/usr/bin/env python
"""Measurements behind DESIGN.md section 13: prints ONE JSON object.

  spmm     mik_spmm against b calls of mik_spmv on the 3-D Laplacian (CSR layout), b = 4 / 8 / 16: microseconds (HIP events on the context's
           stream, median of --reps after --warmup), the fraction of the 6.29 TB/s copy ceiling the algorithmic traffic reaches -- the
           operator once per block of 8 columns plus b vectors in and out, against b times the operator plus the same vectors;
  update   mik_block_update against its composition (three mik_basis_rotate into temporaries and two additions, per block triple);
  gram     mik_block_gram against q calls of mik_gemv_t;
  lobpcg   one full lobpcg for the 8 smallest pairs of the 3-D Laplacian with the Jacobi preconditioner: wall time per iteration and its
           split by sweep (each bracketed by a stream synchronisation, so the parts are upper bounds).

Usage: python scripts/lobpcg_bench.py [--reps 20] [--warmup 3] [--small] > profiles/lobpcg_bench.json
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import __graft_entry__ as graft  # noqa: E402
from svdl_bench import COPY_CEILING, timed  # noqa: E402

_vp = C.c_void_p


def frac(nbytes, us):
    return round(nbytes / (us * 1e-6) / COPY_CEILING, 3)


def filled(pkg, ctx, n, k, dt, seed):
    M = pkg.HipMatrix(n, k, dt, ctx)
    col = np.random.default_rng(seed).standard_normal(n).astype(dt)
    for j in range(k):
        M.col(j).copy_from_host(np.roll(col, 3 * j))
    return M


def bench_spmm(pkg, ctx, dt, N, reps, warmup):
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, 3, dtype=dt)
    A = pkg.HipCSR(n, n, cp, rv, nz, index_base=1, ctx=ctx).set_layout("csr")
    es = np.dtype(dt).itemsize
    op_bytes = A.nnz * (es + 4) + (n + 1) * 4
    out = []
    L = pkg.lib()
    for b in (4, 8, 16):
        X, Y = filled(pkg, ctx, n, b, dt, b), pkg.HipMatrix(n, b, dt, ctx)

        def new():
            pkg._lib.check(L.mik_spmm(ctx.handle, A.handle, b, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld), "mik_spmm", ctx.handle)

        def old():
            for j in range(b):
                pkg.mul_(Y.col(j), A, X.col(j))

        t_new, t_old = timed(ctx, new, lambda: None, reps, warmup), timed(ctx, old, lambda: None, reps, warmup)
        b_new, b_old = -(-b // 8) * op_bytes + 2 * b * n * es, b * op_bytes + 2 * b * n * es
        out.append({"dtype": np.dtype(dt).name, "N": N, "b": b, "spmm_us": round(t_new, 1), "spmm_fraction_of_copy_ceiling": frac(b_new, t_new),
                    "spmv_loop_us": round(t_old, 1), "spmv_loop_fraction_of_copy_ceiling": frac(b_old, t_old), "gain": round(t_old / t_new, 2),
                    "byte_ratio": round(b_old / b_new, 2)})
    return out


def bench_update(pkg, ctx, dt, n, s, reps, warmup):
    es = np.dtype(dt).itemsize
    X, R, P = filled(pkg, ctx, n, s, dt, 1), filled(pkg, ctx, n, s, dt, 2), filled(pkg, ctx, n, s, dt, 3)
    Xo, Po, T1 = (pkg.HipMatrix(n, s, dt, ctx) for _ in range(3))
    V = np.asfortranarray(np.random.default_rng(4).standard_normal((3 * s, s)).astype(dt))
    Vx, Vr, Vp = (np.asfortranarray(V[i * s:(i + 1) * s]) for i in range(3))
    code = pkg._lib.dtype_code(dt)
    L = pkg.lib()
    one = np.ones(1, dt)

    def new():
        pkg._lib.check(L.mik_block_update(ctx.handle, code, n, s, s, s, _vp(X.buf.ptr), X.ld, _vp(R.buf.ptr), R.ld, _vp(P.buf.ptr), P.ld,
                                          V.ctypes.data_as(_vp), 3 * s, _vp(Xo.buf.ptr), Xo.ld, _vp(Po.buf.ptr), Po.ld), "mik_block_update", ctx.handle)

    def rot(W, F, Y):
        pkg._lib.check(L.mik_basis_rotate(ctx.handle, code, n, s, s, _vp(W.buf.ptr), W.ld, F.ctypes.data_as(_vp), s, _vp(Y.buf.ptr), Y.ld),
                       "mik_basis_rotate", ctx.handle)

    def add(Y, W):                                             # Y .+= W, the whole padded block as one vector
        pkg._lib.check(L.mik_axpy(ctx.handle, code, Y.ld * s, one.ctypes.data_as(_vp), _vp(W.buf.ptr), _vp(Y.buf.ptr)), "mik_axpy", ctx.handle)

    def old():
        rot(R, Vr, Po)
        rot(P, Vp, T1)
        add(Po, T1)
        rot(X, Vx, Xo)
        add(Xo, Po)

    t_new, t_old = timed(ctx, new, lambda: None, reps, warmup), timed(ctx, old, lambda: None, reps, warmup)
    b_new, b_old = 5 * s * n * es, 12 * s * n * es              # 3 reads + 2 writes; 3 rotations (2 each) + 2 additions (3 each)
    return {"dtype": np.dtype(dt).name, "n": n, "sx_b1_b2": [s, s, s], "update_us": round(t_new, 1), "update_fraction_of_copy_ceiling": frac(b_new, t_new),
            "composed_us": round(t_old, 1), "composed_fraction_of_copy_ceiling": frac(b_old, t_old), "gain": round(t_old / t_new, 2),
            "byte_ratio": round(b_old / b_new, 2)}


def bench_gram(pkg, ctx, dt, n, s, reps, warmup):
    es = np.dtype(dt).itemsize
    X, Y = filled(pkg, ctx, n, s, dt, 5), filled(pkg, ctx, n, s, dt, 6)
    G = np.zeros((s, s), dt, order="F")
    code = pkg._lib.dtype_code(dt)
    L = pkg.lib()

    def new():
        pkg._lib.check(L.mik_block_gram(ctx.handle, code, n, s, s, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld, G.ctypes.data_as(_vp), s),
                       "mik_block_gram", ctx.handle)

    def old():
        for j in range(s):
            pkg.gemv_t_(X, s, Y.col(j))

    t_new, t_old = timed(ctx, new, lambda: None, reps, warmup), timed(ctx, old, lambda: None, reps, warmup)
    b_min, b_new, b_old = 2 * s * n * es, 2 * s * (s // 4) * n * es, s * (s + 1) * n * es
    return {"dtype": np.dtype(dt).name, "n": n, "p_q": [s, s], "gram_us": round(t_new, 1), "gram_fraction_of_copy_ceiling_min_bytes": frac(b_min, t_new),
            "gram_fraction_of_copy_ceiling_issued_bytes": frac(b_new, t_new), "gemv_t_loop_us": round(t_old, 1),
            "gemv_t_loop_fraction_of_copy_ceiling": frac(b_old, t_old), "gain": round(t_old / t_new, 2), "byte_ratio_min": round(b_old / b_min, 2)}


def bench_lobpcg(pkg, ctx, dt, N, maxiter):
    mod = importlib.import_module(pkg.__name__ + ".lobpcg")
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, 3, dtype=dt)
    A = pkg.HipCSR(n, n, cp, rv, nz, index_base=1, ctx=ctx)
    P = pkg.JacobiPrec(pkg.HipVector(n, dt, ctx).fill_(6))
    X0 = np.random.default_rng(7).random((n, 8)).astype(dt)
    parts = {k: 0.0 for k in ("spmm", "gram", "rdiv", "update", "residuals", "gather_cols", "precond", "host_rayleigh_ritz")}

    def bracket(name, fn):
        def run(*a, **k):
            ctx.synchronize()
            t = time.perf_counter()
            out = fn(*a, **k)
            ctx.synchronize()
            parts[name] += time.perf_counter() - t
            return out
        return run

    ops = mod.DeviceOps(A)
    for name in ("spmm", "gram", "rdiv", "update", "residuals", "gather_cols", "precond"):
        setattr(ops, name, bracket(name, getattr(ops, name)))
    pkg.lobpcg(A, False, X0, P=P, maxiter=3)                   # warm-up: kernels loaded, workspace grown
    it = mod.LOBPCGIterator(A, None, False, X0, None, P, None, ops=ops)
    sub = it._sub_problem

    def sub_timed(bs1, bs2):                                   # its X'AX in iteration 1 is counted under gram as well
        t = time.perf_counter()
        sub(bs1, bs2)
        parts["host_rayleigh_ritz"] += time.perf_counter() - t

    it._sub_problem = sub_timed
    ctx.synchronize()
    t = time.perf_counter()
    r = mod.lobpcg_(it, maxiter=maxiter, not_zeros=True)
    ctx.synchronize()
    wall = time.perf_counter() - t
    iters = min(r.iterations, maxiter)
    out = {"dtype": np.dtype(dt).name, "N": N, "n": n, "block": 8, "iterations": int(iters), "converged": bool(r.converged), "tolerance": float(r.tolerance),
           "max_residual": float(np.max(r.residual_norms)), "lambda": [float(v) for v in r.lam], "wall_ms_per_iteration": round(wall * 1e3 / iters, 3)}
    out.update({f"{k}_ms_per_iteration": round(v * 1e3 / iters, 3) for k, v in parts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=60)
    ap.add_argument("--small", action="store_true", help="32^3 and n = 2^16 only (a quick check of the script)")
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    grids, sizes = ([32], [2 ** 16]) if args.small else ([128, 256], [2 ** 20, 2 ** 24])
    res = {"device": ctx.info()["arch"], "copy_ceiling_TBps": COPY_CEILING / 1e12, "reps": args.reps, "spmm": [], "update": [], "gram": [], "lobpcg": []}
    for dt in (np.float64, np.float32):
        for N in grids:
            res["spmm"] += bench_spmm(pkg, ctx, dt, N, args.reps, args.warmup)
        for n in sizes:
            for s in (8, 16):
                res["update"].append(bench_update(pkg, ctx, dt, n, s, args.reps, args.warmup))
                res["gram"].append(bench_gram(pkg, ctx, dt, n, s, args.reps, args.warmup))
        res["lobpcg"].append(bench_lobpcg(pkg, ctx, dt, grids[0], args.maxiter))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
