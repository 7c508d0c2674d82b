#!/usr/bin/env python
"""Measurements behind DESIGN.md section 20 (lobpcg for ComplexF64 / ComplexF32): writes ONE JSON object.

  spmm     complex mik_spmm at b = 4 / 8 / 16 against b calls of mik_spmv on the same operator (what the library could do before the complex
           block entries): the 128^3 Laplacian pattern with complex values;
  gram     mik_block_gram against p * q calls of mik_dot at n = 2^20, 8 and 16 columns a side;
  update   mik_block_update (sx = b1 = b2 = s) and
  rdiv     mik_block_rdiv at n = 2^20, s = 8 / 16 / 32: against the real instances on the same bytes (a real block of 2 n rows of the component
           type) and against the bytes they move / the copy ceiling (rdiv re-reads the finished columns once per later panel of 8 columns;
           update re-reads X, R and P once per panel of output columns: `bytes_issued`; `bytes_min` is one read and one write of every block);
  lobpcg   one full complex lobpcg, the 8 smallest pairs of H = D L D^H on the 64^3 Laplacian, split by sweep (each part bracketed by a stream
           synchronisation, so the parts are upper bounds).

Microseconds are medians of --reps windows between two HIP events on the context's stream after --warmup; gram ends in a host wait and is
timed the same way (the events bracket it).

Usage: python scripts/complex_lobpcg_bench.py [--reps 20] [--warmup 3] [--small] [--parts spmm,gram,...] [--out profiles/complex_lobpcg_bench.json]
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
RDIV_PW = 8                                   # CBlk<R>::RDIV_PW of csrc/mik_lobpcg_complex.h
SPMM_CB = 4                                   # MIK_CSPMM_CB
UPD_LB = {16: 8, 8: 16}                       # CBlk<R>::UPD_LB by element size


def frac(nbytes, us):
    return round(nbytes / (us * 1e-6) / COPY_CEILING, 3)


def real_of(T):
    return np.float64 if np.dtype(T) == np.complex128 else np.float32


def filled(pkg, ctx, n, k, dt, seed):
    M = pkg.HipMatrix(n, k, dt, ctx)
    rng = np.random.default_rng(seed)
    col = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        col = col + 1j * rng.standard_normal(n)
    col = (col / np.sqrt(n)).astype(dt)
    for j in range(k):
        M.col(j).copy_from_host(np.roll(col, 3 * j))
    return M


def complex_laplacian(pkg, ctx, N, T):
    """the N^3 Laplacian pattern with a Hermitian imaginary part on the same pattern"""
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3)
    rows = rowval - 1
    cols = np.repeat(np.arange(n), np.diff(colptr))
    cval = nzval.astype(np.complex128)
    cval[rows < cols] += 0.1j
    cval[rows > cols] -= 0.1j
    return n, pkg.HipCSR(n, n, colptr, rowval, cval.astype(T), index_base=1, ctx=ctx)


def bench_spmm(pkg, ctx, T, N, reps, warmup):
    n, A = complex_laplacian(pkg, ctx, N, T)
    es = np.dtype(T).itemsize
    cb = SPMM_CB
    op_bytes = A.nnz * (es + 4) + (n + 1) * 4
    L = pkg.lib()
    out = []
    for b in (4, 8, 16):
        X, Y = filled(pkg, ctx, n, b, T, b), pkg.HipMatrix(n, b, T, ctx)

        def new():
            pkg._lib.check(L.mik_spmm(ctx.handle, A.handle, b, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld), "mik_spmm", ctx.handle)

        def old():
            for j in range(b):
                pkg.mul_(Y.col(j), A, X.col(j))

        t_new, t_old = timed(ctx, new, lambda: None, reps, warmup), timed(ctx, old, lambda: None, reps, warmup)
        b_new, b_old = -(-b // cb) * op_bytes + 2 * b * n * es, b * op_bytes + 2 * b * n * es
        out.append({"dtype": np.dtype(T).name, "N": N, "b": b, "column_block": cb, "spmm_us": round(t_new, 1), "spmm_fraction_of_copy_ceiling": frac(b_new, t_new),
                    "spmv_loop_us": round(t_old, 1), "spmv_loop_fraction_of_copy_ceiling": frac(b_old, t_old), "gain": round(t_old / t_new, 2),
                    "byte_ratio": round(b_old / b_new, 2)})
    return out


def bench_gram(pkg, ctx, T, n, s, reps, warmup):
    es = np.dtype(T).itemsize
    X, Y = filled(pkg, ctx, n, s, T, 5), filled(pkg, ctx, n, s, T, 6)
    G = np.zeros((s, s), T, order="F")
    code = pkg._lib.dtype_code(T)
    L = pkg.lib()

    def new():
        pkg._lib.check(L.mik_block_gram(ctx.handle, code, n, s, s, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld, G.ctypes.data_as(_vp), s),
                       "mik_block_gram", ctx.handle)

    def old():
        for j in range(s):
            for i in range(s):
                pkg.dot(X.col(i), Y.col(j))

    t_new, t_old = timed(ctx, new, lambda: None, reps, warmup), timed(ctx, old, lambda: None, max(3, reps // 4), 1)
    b_min, b_new, b_old = 2 * s * n * es, 2 * s * (s // 4) * n * es, 2 * s * s * n * es
    return {"dtype": np.dtype(T).name, "n": n, "p_q": [s, s], "gram_us": round(t_new, 1), "gram_fraction_of_copy_ceiling_min_bytes": frac(b_min, t_new),
            "gram_fraction_of_copy_ceiling_issued_bytes": frac(b_new, t_new), "dot_loop_us": round(t_old, 1),
            "dot_loop_fraction_of_copy_ceiling": frac(b_old, t_old), "gain": round(t_old / t_new, 2)}


def bench_update(pkg, ctx, T, n, s, reps, warmup):
    L = pkg.lib()
    out = {"dtype": np.dtype(T).name, "n": n, "sx_b1_b2": [s, s, s]}
    for tag, dt, rows in (("complex", T, n), ("real_same_bytes", real_of(T), 2 * n)):
        es = np.dtype(dt).itemsize
        X, R, P = filled(pkg, ctx, rows, s, dt, 1), filled(pkg, ctx, rows, s, dt, 2), filled(pkg, ctx, rows, s, dt, 3)
        Xo, Po = pkg.HipMatrix(rows, s, dt, ctx), pkg.HipMatrix(rows, s, dt, ctx)
        V = np.asfortranarray(filled_host(4, (3 * s, s), dt))
        code = pkg._lib.dtype_code(dt)

        def run():
            pkg._lib.check(L.mik_block_update(ctx.handle, code, rows, s, s, s, _vp(X.buf.ptr), X.ld, _vp(R.buf.ptr), R.ld, _vp(P.buf.ptr), P.ld,
                                              V.ctypes.data_as(_vp), 3 * s, _vp(Xo.buf.ptr), Xo.ld, _vp(Po.buf.ptr), Po.ld), "mik_block_update", ctx.handle)

        t = timed(ctx, run, lambda: None, reps, warmup)
        b_min = 5 * s * rows * es
        out[f"{tag}_us"] = round(t, 1)
        out[f"{tag}_fraction_of_copy_ceiling_min_bytes"] = frac(b_min, t)
        if tag == "complex":
            panels = -(-s // (UPD_LB[es] if s > 8 else max(s, 4)))
            out["panels"] = panels
            out["complex_fraction_of_copy_ceiling_issued_bytes"] = frac((3 * panels + 2) * s * rows * es, t)
        del X, R, P, Xo, Po
    out["complex_over_real"] = round(out["complex_us"] / out["real_same_bytes_us"], 2)
    return out


def filled_host(seed, shape, dt):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    if np.dtype(dt).kind == "c":
        a = a + 1j * rng.standard_normal(shape)
    return (a / np.sqrt(shape[0])).astype(dt)


def bench_rdiv(pkg, ctx, T, n, s, reps, warmup):
    L = pkg.lib()
    out = {"dtype": np.dtype(T).name, "n": n, "s": s}
    for tag, dt, rows in (("complex", T, n), ("real_same_bytes", real_of(T), 2 * n)):
        es = np.dtype(dt).itemsize
        X0, X = filled(pkg, ctx, rows, s, dt, 7), pkg.HipMatrix(rows, s, dt, ctx)
        R = np.triu(filled_host(8, (s, s), dt), 1)
        R = np.asfortranarray(R + np.diag(1 + np.arange(s) / s).astype(dt))
        code = pkg._lib.dtype_code(dt)

        def restore():                                               # outside the bracket: X is overwritten by every call
            X.buf.copyto_(X0.buf)

        def run():
            pkg._lib.check(L.mik_block_rdiv(ctx.handle, code, rows, s, R.ctypes.data_as(_vp), s, _vp(X.buf.ptr), X.ld), "mik_block_rdiv", ctx.handle)

        t = timed(ctx, run, restore, reps, warmup)
        out[f"{tag}_us"] = round(t, 1)
        out[f"{tag}_fraction_of_copy_ceiling_min_bytes"] = frac(2 * s * rows * es, t)
        if tag == "complex":
            panels = -(-s // RDIV_PW)
            reread = RDIV_PW * panels * (panels - 1) // 2              # finished columns re-read before the later panels
            out["panels"] = panels
            out["complex_fraction_of_copy_ceiling_issued_bytes"] = frac((2 * s + reread) * rows * es, t)
        del X0, X
    out["complex_over_real"] = round(out["complex_us"] / out["real_same_bytes_us"], 2)
    return out


def bench_lobpcg(pkg, ctx, T, N, maxiter):
    mod = importlib.import_module(pkg.__name__ + ".lobpcg")
    import scipy.sparse as sp
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, 3, index_base=0)
    Lr = sp.coo_matrix(sp.csc_matrix((nz, rv, cp), shape=(n, n)))
    d = np.exp(2j * np.pi * np.random.default_rng(1).random(n))
    H = sp.csr_matrix(((d[Lr.row] * np.conj(d[Lr.col]) * Lr.data).astype(T), (Lr.row, Lr.col)), shape=(n, n))
    H = ((H + H.conj().T) * 0.5).astype(T).tocsr()                      # exactly Hermitian
    H.sort_indices()
    A = pkg.HipCSR(n, n, H.indptr.astype(np.int64), H.indices.astype(np.int64), H.data, index_base=0, is_csc=False, ctx=ctx)
    rng = np.random.default_rng(7)
    X0 = (rng.random((n, 8)) + 1j * rng.random((n, 8))).astype(T)
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
    pkg.lobpcg(A, False, X0, maxiter=3)                        # warm-up: kernels loaded, workspace grown
    it = mod.LOBPCGIterator(A, None, False, X0, None, None, None, ops=ops)
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
    out = {"dtype": np.dtype(T).name, "N": N, "n": n, "block": 8, "preconditioner": None, "iterations": int(iters), "converged": bool(r.converged),
           "tolerance": float(r.tolerance), "max_residual": float(np.max(r.residual_norms)), "lambda": [float(v.real) for v in r.lam],
           "wall_ms_per_iteration": round(wall * 1e3 / iters, 3)}
    out.update({f"{k}_ms_per_iteration": round(v * 1e3 / iters, 3) for k, v in parts.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=60)
    ap.add_argument("--small", action="store_true", help="32^3 and n = 2^16 only (a quick check of the script)")
    ap.add_argument("--parts", default="spmm,gram,update,rdiv,lobpcg", help="comma-separated sections to measure")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_lobpcg_bench.json"))
    args = ap.parse_args()
    if not os.path.exists(os.path.join(graft.PKG_DIR, "libmik.so")):
        graft.build()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    N_spmm, N_lob, n = (32, 16, 2 ** 16) if args.small else (128, 64, 2 ** 20)
    res = {"device": ctx.info()["arch"], "copy_ceiling_TBps": COPY_CEILING / 1e12, "reps": args.reps, "spmm": [], "gram": [], "update": [], "rdiv": [],
           "lobpcg": []}
    parts = set(args.parts.split(","))
    for T in (np.complex128, np.complex64):
        if "spmm" in parts:
            res["spmm"] += bench_spmm(pkg, ctx, T, N_spmm, args.reps, args.warmup)
        for s in (8, 16):
            if "gram" in parts:
                res["gram"].append(bench_gram(pkg, ctx, T, n, s, args.reps, args.warmup))
        for s in (8, 16, 32):
            if "update" in parts:
                res["update"].append(bench_update(pkg, ctx, T, n, s, args.reps, args.warmup))
            if "rdiv" in parts:
                res["rdiv"].append(bench_rdiv(pkg, ctx, T, n, s, args.reps, args.warmup))
        if "lobpcg" in parts:
            res["lobpcg"].append(bench_lobpcg(pkg, ctx, T, N_lob, args.maxiter))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
