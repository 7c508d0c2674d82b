#!/usr/bin/env python
"""Measurements behind DESIGN.md section 19: prints ONE JSON object.

Vectors of n = N^3 = 2,097,152 ComplexF64 (and ComplexF32) elements; the operator of the solver steps is the 128^3 Laplacian pattern with
a Hermitian imaginary part on the same pattern (section 17's).  For every new sweep, in the same run:

  <sweep>          the fused entry
  <sweep>_chain    the chain of L1 calls it replaces (same bits)
  <sweep>_real     the real entry of the same shape on the same bytes (the 2 n interleaved reals; a dot where the sweep has a dot)

  axpy_dot_rdot / _cdot / _cnorm   mik_axpy_dot: real alpha + dot, complex alpha + dot, complex alpha + norm       (host wait each)
  minres_update_c                  mik_minres_update with five complex scalars, iteration >= 3                     (no host wait)
  mr_update_l2 / _l4               mik_bicgstab_mr_update                                                          (host wait)
  gram_k3 / _k5                    mik_gram against k (k + 1) / 2 mik_dot calls                                    (host wait)
  gemv_t_k5                        mik_gemv_t against 5 mik_dot calls                                              (host wait)
  <solver>_step_fused / _unfused   one iteration of minres, chebyshev and bicgstabl(l = 2) on the CSR operator

Entries that end in a host wait are timed with a host clock around `inner` calls; entries without one with two HIP events on the
context's stream around `inner` back-to-back calls.  Every window lasts 12 ms or more (`inner` comes from a first window of 20 calls); median / minimum / maximum of --reps windows after
--warmup.  The three variants of a sweep alternate inside every repetition.  `faster_than_chain` says whether the fused median beats the
chain's by more than the spread (max - min) of either's windows.

Usage: python scripts/complex_solvers_bench.py [--N 128] [--reps 9] [--warmup 2] > profiles/complex_solvers_bench.json
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


def stats(us):
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "windows": len(us)}


class Timer:
    def __init__(self, ctx):
        import torch
        self.torch, self.ctx = torch, ctx
        self.stream = torch.cuda.Stream()
        ctx.set_stream(self.stream.cuda_stream)

    def host(self, fn, inner):
        self.ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        self.ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6 / inner

    def events(self, fn, inner):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        self.ctx.synchronize()
        e0.record(self.stream)
        for _ in range(inner):
            fn()
        e1.record(self.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner

    def close(self):
        self.ctx.synchronize()
        self.ctx.set_stream(None)


WINDOW_US = 12e3         # every window lasts this long or longer


def compare(timer, variants, reps, warmup, waits=True):
    """variants: {name: fn}; they alternate inside every repetition.  `inner` of a variant: from a first window of 20 calls."""
    clock = timer.host if waits else timer.events
    inner = {k: max(20, int(WINDOW_US / clock(fn, 20)) + 1) for k, fn in variants.items()}
    t = {k: [] for k in variants}
    for it in range(warmup + reps):
        for name, fn in variants.items():
            us = clock(fn, inner[name])
            if it >= warmup:
                t[name].append(us)
    out = {k: dict(stats(v), inner=inner[k]) for k, v in t.items()}
    names = list(variants)
    if len(names) > 1:
        f, c = out[names[0]], out[names[1]]
        spread = max(f["max_us"] - f["min_us"], c["max_us"] - c["min_us"])
        out["fused_over_chain"] = f["median_us"] / c["median_us"]
        out["faster_than_chain"] = bool(c["median_us"] - f["median_us"] > spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    pkg = graft.load_package()
    ctx = pkg.default_context()
    timer = Timer(ctx)
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(args.N, 3)
    rows = rowval - 1
    cols = np.repeat(np.arange(n), np.diff(colptr))
    cval = nzval.astype(np.complex128)
    cval[rows == cols] += 1.0
    cval[rows < cols] += 0.1j
    cval[rows > cols] -= 0.1j
    res = {"N": args.N, "n": n, "nnz": int(nzval.size), "info": {k: ctx.info()[k] for k in ("arch", "compute_units", "xcds")}}
    rng = np.random.default_rng(0)
    kw = dict(reps=args.reps, warmup=args.warmup)
    for T in (np.complex128, np.complex64):
        tag = "c64" if T == np.complex128 else "c32"
        RT = np.float64 if T == np.complex128 else np.float32
        log(tag)
        vec = lambda: pkg.HipVector.from_numpy(((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2 * n)).astype(T), ctx)
        rv = lambda v: pkg.HipVector.wrap(v.ptr, 2 * v.n, RT, ctx, owner=v)
        x, y, z, v1, v2, v3 = (vec() for _ in range(6))
        r = {}
        a_r, a_c = RT(1e-3), T(1e-3 - 2e-3j)
        r["axpy_dot_rdot"] = compare(timer, {"fused": lambda: pkg.axpy_dot_(a_r, x, y, z), "chain": lambda: (y.axpy_(a_r, x), pkg.dot(z, y)),
                                             "real": lambda: pkg.axpy_dot_(a_r, rv(x), rv(y), rv(z))}, **kw)
        r["axpy_dot_cdot"] = compare(timer, {"fused": lambda: pkg.axpy_dot_(a_c, x, y, z), "chain": lambda: (y.axpy_(a_c, x), pkg.dot(z, y)),
                                             "real": lambda: pkg.axpy_dot_(a_r, rv(x), rv(y), rv(z))}, **kw)
        r["axpy_dot_cnorm"] = compare(timer, {"fused": lambda: pkg.axpy_dot_(a_c, x, y, None), "chain": lambda: (y.axpy_(a_c, x), pkg.norm(y)),
                                              "real": lambda: pkg.axpy_dot_(a_r, rv(x), rv(y), None)}, **kw)
        sc_c = [T(1 + 1e-4j), T(-1e-3 + 1e-3j), T(1e-3j), T(1 - 1e-4j), T(1e-3 + 1e-3j)]
        sc_r = [RT(1), RT(-1e-3), RT(1e-3), RT(1), RT(1e-3)]

        def chain_minres():
            v1.scal_(sc_c[0]); v3.copyto_(v2); v3.axpy_(sc_c[1], y); v3.axpy_(sc_c[2], z); v3.scal_(sc_c[3]); x.axpy_(sc_c[4], v3)
        r["minres_update_c"] = compare(timer, {"fused": lambda: pkg.minres_update_(x, v1, v2, y, z, v3, *sc_c, hints=3), "chain": chain_minres,
                                               "real": lambda: pkg.minres_update_(rv(x), rv(v1), rv(v2), rv(y), rv(z), rv(v3), *sc_r, hints=3)},
                                       waits=False, **kw)
        for l in (2, 4):
            us, rs = pkg.HipMatrix(n, l + 1, T, ctx), pkg.HipMatrix(n, l + 1, T, ctx)
            usr, rsr = pkg.HipMatrix(2 * n, l + 1, RT, ctx), pkg.HipMatrix(2 * n, l + 1, RT, ctx)
            for j in range(l + 1):
                us.col(j).copyto_(vec()); rs.col(j).copyto_(vec())
                usr.col(j).copyto_(rv(us.col(j))); rsr.col(j).copyto_(rv(rs.col(j)))
            g = (np.full(l, 1e-3) * (1 + 1j)).astype(T)

            def chain_mr():
                pkg.gemv_n_(us.col(0), us, l, g, -1.0, col0=1); pkg.gemv_n_(x, rs, l, g, 1.0, col0=0); pkg.gemv_n_(rs.col(0), rs, l, g, -1.0, col0=1)
                pkg.norm(rs.col(0))
            r[f"mr_update_l{l}"] = compare(timer, {"fused": lambda: pkg.bicgstab_mr_update_(us, rs, x, l, g), "chain": chain_mr,
                                                    "real": lambda: pkg.bicgstab_mr_update_(usr, rsr, rv(x), l, g.real.astype(RT))},
                                           **kw)
            for k in (l + 1,):
                r[f"gram_k{k}"] = compare(timer, {"fused": lambda: pkg.gram_(rs, k),
                                                  "chain": lambda: [pkg.dot(rs.col(a), rs.col(b)) for a in range(k) for b in range(a, k)],
                                                  "real": lambda: pkg.gram_(rsr, k)}, **kw)
            if l == 4:
                r["gemv_t_k5"] = compare(timer, {"fused": lambda: pkg.gemv_t_(rs, 5, x), "chain": lambda: [pkg.dot(rs.col(a), x) for a in range(5)],
                                                 "real": lambda: pkg.gemv_t_(rsr, 5, rv(x))}, **kw)
            del us, rs, usr, rsr
        # one iteration of each solver on the CSR operator, fused and unfused
        A = pkg.HipCSR(n, n, colptr, rowval, cval.astype(T), index_base=1, ctx=ctx)
        b = vec()
        state = {}
        makers = {
            "minres": lambda f: pkg.minres_iterable_(b.zero(), A, b, initially_zero=True, reltol=1e-30, maxiter=10 ** 6, fused=f),
            "chebyshev": lambda f: pkg.chebyshev_iterable_(b.zero(), A, b, 0.9, 13.1, initially_zero=True, reltol=1e-30, maxiter=10 ** 6, fused=f),
            "bicgstabl2": lambda f: pkg.bicgstabl_iterator_(b.zero(), A, b, 2, initial_zero=True, reltol=1e-30, max_mv_products=10 ** 9, fused=f),
        }
        for name, make in makers.items():
            steps = 80 if name != "bicgstabl2" else 8                     # a window: the first steps of a fresh solve, 10 ms or more

            def runner(f):
                def go():
                    it = make(f)
                    i = it.start()
                    timer.ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        _res, i = it.iterate(i)
                    timer.ctx.synchronize()
                    state["us"] = (time.perf_counter() - t0) * 1e6 / steps
                return go
            t = {"fused": [], "unfused": []}
            for itn in range(args.warmup + args.reps):
                for key, f in (("fused", True), ("unfused", False)):
                    runner(f)()
                    if itn >= args.warmup:
                        t[key].append(state["us"])
            s = {k: stats(v) for k, v in t.items()}
            s["fused_over_unfused"] = s["fused"]["median_us"] / s["unfused"]["median_us"]
            r[f"{name}_step"] = s
        res[tag] = r
        del A
    timer.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
