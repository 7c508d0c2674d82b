#!/usr/bin/env python
"""Measurements behind DESIGN.md section 22: prints ONE JSON object.

Vectors of n = N^3 = 2,097,152 ComplexF64 (and ComplexF32) elements; the operator of the solver steps is the 128^3 Laplacian pattern with
a Hermitian imaginary part on the same pattern (section 21's), uploaded with its adjoint.  Every device result is first compared bit for
bit with the chain of L1 calls it replaces (the run stops at a difference); then, in the same run and alternating inside every repetition:

  <sweep>          the fused entry (mik_axpy2_dot with and without the dot, mik_scal2, mik_qmr_update; complex scalars)
  <sweep>_chain    the chain of L1 calls it replaces (same bits)
  <sweep>_real     the real entry of the same shape on the same bytes (the 2 n interleaved reals)

  qmr_step_fused / _unfused        one QMR iteration on the CSR operator and its adjoint
  idrs8_cycle_fused / _unfused     one IDR(8) cycle (s + 1 = 9 steps), composed from the complex entries / one L1 call per statement

The clocks, the windows (12 ms or more), `inner`, the repetitions and `faster_than_chain` are those of scripts/complex_solvers_bench.py.

Usage: python scripts/complex_extras_bench.py [--N 128] [--reps 9] [--warmup 2] > profiles/complex_extras_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402
from complex_solvers_bench import Timer, compare, log, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    pkg = graft.load_package()
    ex = pkg.extras
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
        a, b, c, d = T(1e-3 - 2e-3j), T(-1e-3 + 1e-3j), T(1 - 1e-4j), T(1e-3 + 1e-3j)
        ar, br, cr, dr = RT(1e-3), RT(-1e-3), RT(1), RT(1e-3)

        def chain_a2(with_dot):
            y.axpy_(a, v1); y.axpy_(b, v2)
            return pkg.dot(z, y) if with_dot else None

        def chain_qmr():
            v3.copyto_(v1); v3.axpy_(a, y); v3.axpy_(b, z); v3.scal_(c); x.axpy_(d, v3)

        # bits first: the fused entries against their chains on copies of the same data
        keep = {k: v.to_numpy() for k, v in (("x", x), ("y", y), ("z", z))}
        got = ex._axpy2_dot(y, a, v1, b, v2, z)
        yf = y.to_numpy(); y.copy_from_host(keep["y"])
        assert got == chain_a2(True) and np.array_equal(yf, y.to_numpy()), "mik_axpy2_dot differs from its chain"
        y.copy_from_host(keep["y"])
        ex._qmr_update(v1, a, y, b, z, c, d, x, v3)
        xf, pf = x.to_numpy(), v3.to_numpy(); x.copy_from_host(keep["x"])
        chain_qmr()
        assert np.array_equal(xf, x.to_numpy()) and np.array_equal(pf, v3.to_numpy()), "mik_qmr_update differs from its chain"
        x.copy_from_host(keep["x"])
        ex._scal2(c, y, T(1) / c, z)
        yf, zf = y.to_numpy(), z.to_numpy(); y.copy_from_host(keep["y"]); z.copy_from_host(keep["z"])
        y.scal_(c); z.scal_(T(1) / c)
        assert np.array_equal(yf, y.to_numpy()) and np.array_equal(zf, z.to_numpy()), "mik_scal2 differs from its chain"
        y.copy_from_host(keep["y"]); z.copy_from_host(keep["z"])

        L, h = pkg.lib(), ctx.handle
        p = lambda v: pkg.api._vp(v.ptr)
        sp_ = lambda dt, val: pkg.api._scalar(dt, val)
        r = {}
        (ka, pa), (kb, pb) = sp_(RT, ar), sp_(RT, br)
        out = np.zeros(2, RT)
        po = out.ctypes.data_as(pkg.api._vp)
        real_a2 = lambda zz: L.mik_axpy2_dot(h, pkg._lib.dtype_code(RT), 2 * n, pa, p(v1), pb, p(v2), p(y), p(zz) if zz is not None else None, po)
        r["axpy2_dot"] = compare(timer, {"fused": lambda: ex._axpy2_dot(y, a, v1, b, v2, z), "chain": lambda: chain_a2(True), "real": lambda: real_a2(z)}, **kw)
        r["axpy2_nodot"] = compare(timer, {"fused": lambda: ex._axpy2_dot(y, a, v1, b, v2, None), "chain": lambda: chain_a2(False),
                                           "real": lambda: real_a2(None)}, waits=False, **kw)
        ci = T(1) / c
        (kc, pc), (kd, pd) = sp_(RT, cr), sp_(RT, cr)
        r["scal2"] = compare(timer, {"fused": lambda: ex._scal2(c, y, ci, z), "chain": lambda: (y.scal_(c), z.scal_(ci)),
                                     "real": lambda: L.mik_scal2(h, pkg._lib.dtype_code(RT), 2 * n, pc, p(y), pd, p(z))}, waits=False, **kw)
        sr = [sp_(RT, s) for s in (ar, br, cr, dr)]
        r["qmr_update"] = compare(timer, {"fused": lambda: ex._qmr_update(v1, a, y, b, z, c, d, x, v3), "chain": chain_qmr,
                                          "real": lambda: L.mik_qmr_update(h, pkg._lib.dtype_code(RT), 2 * n, p(v1), sr[0][1], p(y), sr[1][1], p(z), sr[2][1],
                                                                           sr[3][1], p(x), p(v3))}, waits=False, **kw)
        # one QMR iteration and one IDR(8) cycle on the CSR operator, fused and unfused
        A = ex.with_adjoint(n, n, colptr, rowval, cval.astype(T), index_base=1, ctx=ctx)
        bb = vec()
        P = ((rng.random((n, 8)) + 1j * rng.random((n, 8)))).astype(T)
        PM = pkg.HipMatrix.from_numpy(P, ctx)
        state = {}

        def qmr_run(f, steps=30):
            it = ex.qmr_iterable_(bb.zero(), A, bb, reltol=1e-30, maxiter=10 ** 6, initially_zero=True, fused=f)
            i = 1
            timer.ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                _res, i = it.iterate(i)
            timer.ctx.synchronize()
            state["us"] = (time.perf_counter() - t0) * 1e6 / steps
            return it.x

        def idrs_run(f, cycles=3):
            it = ex.idrs_iterable_(None, bb.zero(), A, bb, 8, None, 0.0, 1e-30, 10 ** 6, P=PM, fused=f)
            st = (1, 1)
            timer.ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(9 * cycles):
                _res, st = it.iterate(st)
            timer.ctx.synchronize()
            state["us"] = (time.perf_counter() - t0) * 1e6 / cycles
            return it.X
        for name, run in (("qmr_step", qmr_run), ("idrs8_cycle", idrs_run)):
            assert np.array_equal(run(True).to_numpy(), run(False).to_numpy()), f"{name}: fused and unfused differ"
            t = {"fused": [], "unfused": []}
            for itn in range(args.warmup + args.reps):
                for key, f in (("fused", True), ("unfused", False)):
                    run(f)
                    if itn >= args.warmup:
                        t[key].append(state["us"])
            s = {k: stats(v) for k, v in t.items()}
            s["fused_over_unfused"] = s["fused"]["median_us"] / s["unfused"]["median_us"]
            r[name] = s
        res[tag] = r
        del A, PM
    timer.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
