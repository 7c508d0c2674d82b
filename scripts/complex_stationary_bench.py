#!/usr/bin/env python
"""Measurements behind DESIGN.md section 21 (the stationary methods on ComplexF64 / ComplexF32 CSR operators): writes ONE JSON object.

Operator: H = D L D^H, L the N^3 Laplacian (N = 128: 2 097 152 rows, 382 levels either way) and D a unit-modulus diagonal, in ComplexF64 and
ComplexF32; the real kernels run on L itself in Float64 / Float32.

  methods   microseconds per iteration of jacobi / gauss_seidel / sor / ssor (one _step() of the iterable, omega = 1.2), complex and real;
  sweeps    one forward substitution, plain and relaxed with a Float64 and a Float32 omega, in microseconds and per level; mik_diag_ldiv alone
            (one complex division a row) with its fraction of the copy ceiling on 3 n elements (x, d, y);
  checker   the C checker of tests/complex_ref/complex_stationary_ref.c on one core, seconds per iteration;
  parity    every device result (--check-iters iterations of each method, both substitutions, ldiv) against the checker, bit for bit.

Microseconds are medians of --reps windows between two HIP events on the context's stream after --warmup.

Usage: python scripts/complex_stationary_bench.py [--N 128] [--reps 20] [--warmup 3] [--check-iters 2] [--out profiles/complex_stationary_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from svdl_bench import COPY_CEILING, timed  # noqa: E402
import complex_stationary_host as ch  # noqa: E402
import stationary_host as sh  # noqa: E402

OMEGA = 1.2


def operators(pkg, N, T, seed=5):
    """(complex CMat H = D L D^H in T, real sh.Mat L in real(T)), both 0-based CSC"""
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3, index_base=0)
    cols = np.repeat(np.arange(n), np.diff(colptr))
    d = np.exp(2j * np.pi * np.random.default_rng(seed).random(n))
    val = d[rowval] * np.conj(d[cols]) * nzval
    val[rowval == cols] = nzval[rowval == cols]                           # |d_i|^2 = 1: the diagonal is L's
    val = val.astype(T)
    H = ch.CMat(sp.csc_matrix((val, rowval, colptr), shape=(n, n)), T)
    Lr = sh.Mat(sp.csc_matrix((nzval.astype(ch.real_of(T)), rowval, colptr), shape=(n, n)), ch.real_of(T))
    assert H.nz.size == Lr.nz.size == nzval.size
    return H, Lr


def device(pkg, ctx, M):
    return pkg.HipCSR(M.n, M.n, M.cp, M.rv, M.nz, index_base=0, ctx=ctx)


def vectors(M, seed, count):
    rng = np.random.default_rng(seed)
    if M.dtype.kind == "c":
        return [ch.cnormal(rng, M.dtype, M.n) for _ in range(count)]
    return [rng.standard_normal(M.n).astype(M.dtype) for _ in range(count)]


def bench_methods(pkg, ctx, M, A, reps, warmup):
    b, x0 = vectors(M, 1, 2)
    V = lambda a: pkg.HipVector.from_numpy(a, ctx)
    out = {}
    for name, make in (("jacobi", lambda: pkg.jacobi_iterable(V(x0), A, V(b), maxiter=1 << 30)),
                       ("gauss_seidel", lambda: pkg.gauss_seidel_iterable(V(x0), A, V(b), maxiter=1 << 30)),
                       ("sor", lambda: pkg.sor_iterable(V(x0), A, V(b), OMEGA, maxiter=1 << 30)),
                       ("ssor", lambda: pkg.ssor_iterable(V(x0), A, V(b), OMEGA, maxiter=1 << 30))):
        it = make()
        out[name + "_us_per_iteration"] = round(timed(ctx, it._step, lambda: None, reps, warmup), 1)
    return out


def bench_sweeps(pkg, ctx, M, A, reps, warmup):
    S = pkg.StationaryOperator(A)
    info = S.info()
    x, y = vectors(M, 2, 2)
    xd, yd, keep = pkg.HipVector.from_numpy(x, ctx), pkg.HipVector.from_numpy(y, ctx), pkg.HipVector.from_numpy(x, ctx)
    es = M.dtype.itemsize
    out = {"levels_forward": info["levels_forward"], "launches_forward": info["launches_forward"], "analysis_ms": round(info["analysis_ms"], 1)}
    restore = lambda: xd.copyto_(keep)                                       # every window starts from the same x
    for tag, omega in (("plain", None), ("relaxed_omega_float64", 1.2), ("relaxed_omega_float32", np.float32(1.2))):
        t = timed(ctx, (lambda: S.forward_sub_(xd)) if omega is None else (lambda: S.forward_sub_(xd, omega, yd)), restore, reps, warmup)
        out["forward_" + tag + "_us"] = round(t, 1)
        out["forward_" + tag + "_us_per_level"] = round(t / info["levels_forward"], 3)
    t = timed(ctx, lambda: S.diag_ldiv_(yd, xd), restore, reps, warmup)
    out["diag_ldiv_us"] = round(t, 1)
    out["diag_ldiv_fraction_of_copy_ceiling"] = round(3 * M.n * es / (t * 1e-6) / COPY_CEILING, 3)
    return out


def bench_checker(cref, M, iters=1):
    b, x0 = vectors(M, 1, 2)
    out = {}
    for name, run in (("jacobi", lambda: cref.jacobi(M, b, x0, iters)), ("gauss_seidel", lambda: cref.gauss_seidel(M, b, x0, iters)),
                      ("sor", lambda: cref.sor(M, b, x0, OMEGA, iters)), ("ssor", lambda: cref.ssor(M, b, x0, OMEGA, iters))):
        t0 = time.perf_counter()
        run()
        out[name + "_s_per_iteration"] = round((time.perf_counter() - t0) / iters, 3)
    return out


def parity(pkg, ctx, cref, M, A, k):
    """device against checker, bit for bit; raises on the first difference"""
    b, x0, y = vectors(M, 3, 3)
    V = lambda a: pkg.HipVector.from_numpy(a, ctx)
    checked = []

    def same(name, got, want):
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), f"{M.dtype.name} {name}: the device differs from the checker"
        checked.append(name)

    same("jacobi", pkg.jacobi_(V(x0), A, V(b), maxiter=k).to_numpy(), cref.jacobi(M, b, x0, k)[0])
    same("gauss_seidel", pkg.gauss_seidel_(V(x0), A, V(b), maxiter=k).to_numpy(), cref.gauss_seidel(M, b, x0, k)[0])
    for omega, tag in ((1.2, "float64"), (np.float32(1.2), "float32"), (1, "int")):
        same("sor_omega_" + tag, pkg.sor_(V(x0), A, V(b), omega, maxiter=k).to_numpy(), cref.sor(M, b, x0, omega, k)[1])
        same("ssor_omega_" + tag, pkg.ssor_(V(x0), A, V(b), omega, maxiter=k).to_numpy(), cref.ssor(M, b, x0, omega, k)[0])
    S = pkg.StationaryOperator(A)
    assert cref.diag(M) == 0
    same("diag_ldiv", S.diag_ldiv_(V(y), V(x0)).to_numpy(), cref.ldiv(M, x0))
    for upper in (False, True):
        sub = S.backward_sub_ if upper else S.forward_sub_
        same("backward_sub" if upper else "forward_sub", sub(V(x0)).to_numpy(), cref.sub(M, upper, x0))
    return checked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check-iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complex_stationary_bench.json"))
    args = ap.parse_args()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    with tempfile.TemporaryDirectory() as tmp:
        cref, rref = ch.build(tmp), sh.build(tmp)
        res = {"N": args.N, "omega": OMEGA, "reps": args.reps, "warmup": args.warmup, "copy_ceiling_bytes_per_s": COPY_CEILING, "types": {}}
        for T in ch.CTYPES:
            H, Lr = operators(pkg, args.N, T)
            A, Ar = device(pkg, ctx, H), device(pkg, ctx, Lr)
            entry = {"n": H.n, "nnz": int(H.nz.size)}
            print(f"{np.dtype(T).name}: n = {H.n}, parity", file=sys.stderr, flush=True)
            entry["parity_bit_for_bit"] = parity(pkg, ctx, cref, H, A, args.check_iters)
            print(f"{np.dtype(T).name}: timing", file=sys.stderr, flush=True)
            entry["complex"] = {**bench_methods(pkg, ctx, H, A, args.reps, args.warmup), **bench_sweeps(pkg, ctx, H, A, args.reps, args.warmup)}
            entry["real_on_L"] = {**bench_methods(pkg, ctx, Lr, Ar, args.reps, args.warmup), **bench_sweeps(pkg, ctx, Lr, Ar, args.reps, args.warmup)}
            entry["complex_over_real"] = {k: round(entry["complex"][k] / entry["real_on_L"][k], 2) for k in entry["complex"]
                                          if k.endswith(("_us", "_us_per_iteration")) and entry["real_on_L"][k] > 0}
            print(f"{np.dtype(T).name}: checker", file=sys.stderr, flush=True)
            entry["checker_one_core"] = bench_checker(cref, H)
            entry["real_checker_one_core"] = {"jacobi_s_per_iteration": round(_time(lambda: rref.jacobi(Lr, *vectors(Lr, 1, 2), 1)), 3)}
            res["types"][np.dtype(T).name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def _time(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
