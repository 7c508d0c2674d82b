"""Jacobi / Gauss-Seidel / SOR / SSOR per iteration on the 128^3 and 256^3 Laplacians (fp64), against the one-core C restatement
of src/stationary_sparse.jl (tests/stationary_ref/stationary_ref.c, gcc -O2 -ffp-contract=off).  Prints one JSON line.

    python scripts/stationary_bench.py            # SIZES=128,256 ITERS=5 by default

Per size: microseconds per iteration of each method on the device (host wall clock around ITERS iterations, synchronised: launch
costs included), levels / launches per triangular sweep and microseconds per level of one forward sweep, the analysis time of
mik_stationary_create, the C restatement's time per iteration on one core, and Jacobi's row-parallel pass (mul!(-1, O, x, 1, next))
next to mik_spmv on the same operator with set_layout("csr").  Every device result is checked against the C restatement bit for bit.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import stationary_host as sh

pkg = g.load_package()
SIZES = [int(s) for s in os.environ.get("SIZES", "128,256").split(",")]
ITERS = int(os.environ.get("ITERS", 5))
ref = sh.build(tempfile.mkdtemp(prefix="stationary_ref_"))
ctx = pkg.default_context()


def wall(fn, reps):
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def c_time(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e6, out


line = {"metric": "stationary_us_per_iteration", "dtype": "float64", "iters": ITERS, "sizes": {}}
for N in SIZES:
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, 3)
    M = sh.Mat.from_csc(n, cp, rv, nz)
    A = pkg.HipCSR(n, n, cp, rv, nz)
    del cp, rv
    S = pkg.StationaryOperator(A)
    info = S.info()
    b = pkg.fixtures.hashed_rhs(n)
    bd = pkg.HipVector.from_numpy(b)
    x = pkg.HipVector(n).fill_(0)
    w = x.similar()
    its = {"jacobi": pkg.JacobiIterable(S, x, w, bd, 1), "gauss_seidel": pkg.GaussSeidelIterable(S, x, bd, 1),
           "sor": pkg.SORIterable(S, 1.5, x, w, bd, 1), "ssor": pkg.SSORIterable(S, 1.5, x, w, bd, 1)}
    res = {"n": n, "levels": [info["levels_forward"], info["levels_backward"]], "launches": [info["launches_forward"], info["launches_backward"]],
           "analysis_ms": round(info["analysis_ms"], 1), "stationary_bytes": info["bytes"], "device_us": {}, "c_one_core_us": {}, "bit_exact": {}}
    cfun = {"jacobi": lambda x0: ref.jacobi(M, b, x0, 1)[0], "gauss_seidel": lambda x0: ref.gauss_seidel(M, b, x0, 1)[0],
            "sor": lambda x0: ref.sor(M, b, x0, 1.5, 1)[1], "ssor": lambda x0: ref.ssor(M, b, x0, 1.5, 1)[0]}
    for name, it in its.items():
        x.fill_(0)
        w.fill_(0)
        it.x = x
        if hasattr(it, "next"):
            it.next = w
        it.iterate(1)                                                  # one iteration from 0: the bits checked below
        got = it.x.to_numpy()
        tc, want = c_time(lambda: cfun[name](np.zeros(n)))
        res["bit_exact"][name] = bool(np.array_equal(got, want))
        res["c_one_core_us"][name] = round(tc, 1)
        res["device_us"][name] = round(wall(lambda: it.iterate(1), ITERS), 1)
    fwd = wall(lambda: S.forward_sub_(x), ITERS)
    res["forward_sweep_us"] = round(fwd, 1)
    res["us_per_level"] = round(fwd / max(info["levels_forward"], 1), 2)
    res["gs_speedup_vs_c"] = round(res["c_one_core_us"]["gauss_seidel"] / res["device_us"]["gauss_seidel"], 1)
    # Jacobi's row-parallel pass next to the SpMV on the plain CSR arrays of the same operator
    res["offdiag_mul_us"] = round(wall(lambda: S.offdiag_mul_(-1, x, 1, w), 20), 1)
    A.set_layout("csr")
    y = x.similar()
    res["spmv_csr_us"] = round(A.time_spmv(x, y, reps=20) * 1e3, 1)
    res["spmv_csr_kernel"] = A.spmv_kernel()
    line["sizes"][str(N)] = res
    del its, S, A, M, x, w, y, bd
print(json.dumps(line))
