"""Reductions and fused sweeps beyond 1024 segments: every reduction-bearing entry of the C ABI, bit for bit against the oracle's TREE
mode, at the sizes where the code that evaluates the tree of include/mik.h changes form.  GPU box only (-m gpu).

The ladder (tests/ladder.py) is computed per dtype from what the context reports -- SEG = 256 * W * L from mik_reduce_shape, cap =
sweep_grid_cap from mik_ctx_info, level-2 width 1024 -- as n = (m - 1) * SEG + SEG / 2 + 3 (a partial last segment that is no multiple
of W) for

    m1024 / m1025                          both sides of the consumer-side / separate finaliser switch
    batch8_minus1 / batch8_plus500         entry to the 8-deep load batch of level2_sum; +500: threads of one wave on different trip counts
    cap_plus1 / two_cap_plus37             the grid-stride loop of the sweep runs 2 / 3 times, the last pass ragged
    batch32_minus524 / batch32_plus517     entry to the 32-deep load batch, again split inside a wave
    control_16k                            m = 16 * 1024, n = m * SEG: the round case the 128^3 / 256^3 solves already cover

test_the_ladder_as_the_context_reports_it prints m, n and the regime of every rung for both dtypes.

Which entry runs which rungs, and why:

    full ladder      mik_dot, mik_nrm2 (also on a vector whose plain sum of squares underflows: the rescaled second pass), and one
                     sweep per launch helper of csrc/mik_kernels.h:
                       launch_map        mik_axpy_dot (all three forms)
                       launch_map2       the fused PCG tail (OpPcgUpdateR: |r|^2 and dot(c, r) in one sweep), two cg! steps with a diagonal Pl
                     and the dot fused into the SpMV (one partial per 256-row block, mik_spmv_dot_shape: the ladder in THAT segment size)
                     through cg! on a 1-D Laplacian, on the CSR arrays and in the operator's default layout.
    m <= 1024 only   launch_map_with (k_map_with: mik_bicgstab_step, mik_minres_step) and launch_map_pro (k_map_pro: the launch-lean
                     Modified Gram-Schmidt chain) finalise their producer's reduction inside the consumer and are only chosen up to 1024
                     segments, so on a 256-CU part their grid-stride loop never runs twice.  They run m = 1024 / 1025 (both sides of the
                     choice) and, planned for an 8-CU machine (development knob MIK_KNOB_MACHINE: cap = 256), m = cap + 1 and
                     2 * cap + 37 -- the same two cap rules, on the shape where they bite.
    three rungs      (m1025, cap_plus1, batch32_plus517) mik_axpy2_nrm2 (with and without hints), mik_xpby_nrm2, mik_lsqr_update,
                     mik_lsmr_update, mik_axpy2_dot -- more operators on launch_map, whose ladder mik_axpy_dot walks in full -- and the
                     entries with launch code of their own: mik_gemv_t, mik_gram, mik_bicgstab_mr_update, mik_orthogonalize (MGS, CGS,
                     DGKS), mik_svdl_reorth.  Tail loop, ragged grid and the deepest batch, where a slip in their own grid sizing,
                     workspace or 64-bit indexing would show.

Next to every bit comparison of dot / nrm2 the derived bound of tests/test_oracle_cross.py (ladder.dot_bound: gamma_{D+1} * sum |x_i y_i|,
D = W*L + 6 + 3 + ceil(m/1024) + 6 + 15) is asserted for the DEVICE result against a sum that shares no code with the oracle.

A case is skipped only when the device reports less free memory than it needs; on an MI355X (288 GB) none does.  The largest vector
has 33.6 M fp64 / 67 M fp32 elements (268 MB): device vectors are allocated per case and freed before the next."""
import ctypes as C
import gc
import time

import numpy as np
import pytest

from conftest import KN
from ladder import RUNGS, THREE, depth, dot_bound, exact_dot, ladder, nrm_bound

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
_vp = C.c_void_p
_BASE = {}
_TOP = {}


@pytest.fixture(autouse=True)
def _free_device_memory_between_cases():
    yield
    gc.collect()


def rungs_of(ctx, dtype):
    W, L = ctx.reduce_shape(dtype)
    lad = ladder(W, L, ctx.info()["sweep_grid_cap"])
    _TOP[np.dtype(dtype).type] = max(n for _, n, _ in lad.values()) + 4096
    return W, L, lad


def need(nbytes):
    """skip only when the device reports less free memory than the case needs (never on an MI355X)"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"the device reports {free} B of free memory, this case needs {nbytes} B")


def base(dtype, j, n, off=0):
    """vector j (0..4) of the fixed pseudo-random pool, n elements from element `off` on: generated once per dtype at the ladder's top size
    (rungs_of has been called: every test starts with it)"""
    dtype = np.dtype(dtype).type
    if dtype not in _BASE:
        rng = np.random.default_rng(77)
        _BASE[dtype] = [rng.standard_normal(_TOP[dtype], dtype=dtype) for _ in range(5)]
    v = _BASE[dtype][j]
    assert off + n <= v.size
    return v[off:off + n]


def dev(pkg, a):
    return pkg.HipVector.from_numpy(a)


def scal(dtype, v):
    a = np.array([v], dtype)
    return a, a.ctypes.data_as(_vp)


# ==============================================================================================
# the ladder itself
# ==============================================================================================
def test_the_ladder_as_the_context_reports_it(ctx):
    cap = ctx.info()["sweep_grid_cap"]
    assert cap == 32 * ctx.info()["compute_units"]
    for dtype in DTYPES:
        W, L, lad = rungs_of(ctx, dtype)
        print(f"\n{np.dtype(dtype).name}: W = {W}, L = {L}, SEG = {256 * W * L}, sweep_grid_cap = {cap}")
        for name in RUNGS:
            m, n, what = lad[name]
            print(f"  {name:18s} m = {m:6d}  n = {n:9d}  D = {depth(W, L, m)}  {what}")
        assert lad["m1024"][0] == 1024 and lad["m1025"][0] == 1025 and lad["cap_plus1"][0] == cap + 1 and lad["two_cap_plus37"][0] == 2 * cap + 37
        assert all(n % (256 * W * L) % W != 0 for name, (m, n, _) in lad.items() if name != "control_16k")


# ==============================================================================================
# mik_dot / mik_nrm2                                                          (launch_map, full ladder)
# ==============================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", RUNGS)
def test_dot_nrm2_on_the_ladder(pkg, orc, ctx, rung, dtype):
    W, L, lad = rungs_of(ctx, dtype)
    m, n, what = lad[rung]
    need(3 * n * np.dtype(dtype).itemsize)
    x, y = base(dtype, 0, n), base(dtype, 1, n)
    dx, dy = dev(pkg, x), dev(pkg, y)
    ld = np.longdouble
    d = pkg.dot(dx, dy)
    want = orc.dot(x, y, "tree", W, L)
    s, a, err = exact_dot(x, y)
    print(f"{np.dtype(dtype).name} {rung}: m={m} n={n} [{what}] dot {d!r} oracle {want!r}  |dot - exact| = {float(abs(ld(d) - s)):.3e} bound {float(dot_bound(W, L, m, dtype, a, err)):.3e}")
    assert d == dtype(want)
    assert abs(ld(d) - s) <= dot_bound(W, L, m, dtype, a, err)
    nr = pkg.norm(dx)
    s2, a2, err2 = exact_dot(x, x)
    assert nr == dtype(orc.nrm2(x, "tree", W, L))
    assert abs(ld(nr) - np.sqrt(s2)) <= nrm_bound(W, L, m, dtype, s2, err2)
    # the rescaled second pass (OpScaledSq): the plain sum of squares of x * 2^-k underflows to 0; the scaling is by a power of two on
    # both sides, so the exact norm is 2^-k times the one above
    k = 700 if dtype == np.float64 else 80
    xs = np.ldexp(x, -k)
    assert xs.dtype == x.dtype and np.array_equal(np.ldexp(xs, k), x)           # exact: nothing became denormal
    assert float(np.sum(xs[:4096] * xs[:4096])) == 0.0                          # ... but every square underflows
    dx.copy_from_host(xs)
    ns = pkg.norm(dx)
    assert ns == dtype(orc.nrm2(xs, "tree", W, L)) and ns > 0
    assert abs(ld(ns) * ld(2) ** k - np.sqrt(s2)) <= nrm_bound(W, L, m, dtype, s2, err2)


# ==============================================================================================
# mik_axpy_dot, all three forms                                               (launch_map, full ladder)
# ==============================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", RUNGS)
def test_axpy_dot_on_the_ladder(pkg, orc, ctx, rung, dtype):
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(4 * n * np.dtype(dtype).itemsize)
    x, y, z = base(dtype, 0, n), base(dtype, 1, n), base(dtype, 2, n)
    alpha = dtype(-0.7321)
    dx, dy, dz = dev(pkg, x), dev(pkg, y), dev(pkg, z)
    got = pkg.axpy_dot_(alpha, dx, dy, dz)
    y1 = y + alpha * x
    assert np.array_equal(dy.to_numpy(), y1) and got == dtype(orc.dot(z, y1, "tree", W, L))
    got = pkg.axpy_dot_(alpha, None, dy, dz)                                    # no update, just the projection
    assert np.array_equal(dy.to_numpy(), y1) and got == dtype(orc.dot(z, y1, "tree", W, L))
    got = pkg.axpy_dot_(alpha, dz, dy, None, hints=1)                           # update + norm, x streamed
    y2 = y1 + alpha * z
    assert np.array_equal(dy.to_numpy(), y2) and got == dtype(orc.nrm2(y2, "tree", W, L))


# ==============================================================================================
# the other launch_map sweeps                                                 (three rungs)
# ==============================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", THREE)
def test_fused_sweeps_of_the_widened_solvers_on_three_rungs(pkg, orc, ctx, rung, dtype):
    """element-wise results against the one-rounded-operation numpy expression, reductions against the tree oracle"""
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(6 * n * np.dtype(dtype).itemsize)
    lib = pkg.lib()
    code = pkg._lib.dtype_code(dtype)
    alpha = dtype(-0.7321)
    u, xs, c, r = (base(dtype, j, n) for j in range(4))
    # x += a u; r -= a c; norm(r)                                                               mik_axpy2_nrm2
    for hints in (0, 7):
        du, dxs, dc, dr = dev(pkg, u), dev(pkg, xs), dev(pkg, c), dev(pkg, r)
        got = pkg.axpy2_nrm2_(alpha, du, dxs, dc, dr, hints=hints)
        r1 = r - alpha * c
        assert np.array_equal(dxs.to_numpy(), xs + alpha * u) and np.array_equal(dr.to_numpy(), r1), hints
        assert got == dtype(orc.nrm2(r1, "tree", W, L)), hints
        del du, dxs, dc, dr
    # y = x + beta y; norm(y)                                                                   mik_xpby_nrm2
    beta = dtype(0.4173)
    du, dy = dev(pkg, u), dev(pkg, xs)
    got = pkg.extras.xpby_nrm2_(du, beta, dy)
    y1 = u + beta * xs
    assert np.array_equal(dy.to_numpy(), y1) and got == dtype(orc.nrm2(y1, "tree", W, L))
    # y += a x1 (+ b x2); dot(y, z)                                                             mik_axpy2_dot
    dy.copy_from_host(xs)
    dc, dr = dev(pkg, c), dev(pkg, r)
    got = pkg.extras._axpy2_dot(dy, alpha, du, beta, dc, dr)
    y2 = (xs + alpha * u) + beta * c
    assert np.array_equal(dy.to_numpy(), y2) and got == dtype(orc.dot(y2, r, "tree", W, L))
    dy.copy_from_host(xs)
    got = pkg.extras._axpy2_dot(dy, alpha, du, beta, None, dr)
    y3 = xs + alpha * u
    assert np.array_equal(dy.to_numpy(), y3) and got == dtype(orc.dot(y3, r, "tree", W, L))
    del du, dy, dc, dr
    # LSQR tail: x += t1 w; w = t2 w + v; norm(w / rho)                                         mik_lsqr_update
    t1, t2, irho = dtype(0.37), dtype(-0.81), dtype(1 / 1.7)
    x0, w0, v0 = xs, u, c
    dx, dw, dv = dev(pkg, x0), dev(pkg, w0), dev(pkg, v0)
    out = np.zeros(1, dtype)
    assert lib.mik_lsqr_update(ctx.handle, code, n, scal(dtype, t1)[1], scal(dtype, t2)[1], scal(dtype, irho)[1], _vp(dx.ptr), _vp(dw.ptr), _vp(dv.ptr),
                               out.ctypes.data_as(_vp)) == 0
    w1 = t2 * w0 + v0
    assert np.array_equal(dx.to_numpy(), x0 + t1 * w0) and np.array_equal(dw.to_numpy(), w1)
    assert out[0] == dtype(orc.nrm2(w1 * irho, "tree", W, L))
    del dx, dw, dv
    # LSMR: hbar = hbar c1 + h; x += c2 hbar; h = h c3 + v; norm(x)                             mik_lsmr_update
    c1, c2, c3 = dtype(-0.29), dtype(0.66), dtype(1.21)
    hb0, h0, x0, v0 = u, xs, c, r
    dhb, dh, dx, dv = dev(pkg, hb0), dev(pkg, h0), dev(pkg, x0), dev(pkg, v0)
    assert lib.mik_lsmr_update(ctx.handle, code, n, scal(dtype, c1)[1], scal(dtype, c2)[1], scal(dtype, c3)[1], _vp(dhb.ptr), _vp(dh.ptr), _vp(dx.ptr),
                               _vp(dv.ptr), out.ctypes.data_as(_vp)) == 0
    hb1 = hb0 * c1 + h0
    x1 = x0 + c2 * hb1
    assert np.array_equal(dhb.to_numpy(), hb1) and np.array_equal(dx.to_numpy(), x1) and np.array_equal(dh.to_numpy(), h0 * c3 + v0)
    assert out[0] == dtype(orc.nrm2(x1, "tree", W, L))


# ==============================================================================================
# entries with launch code of their own                                       (three rungs)
# ==============================================================================================
def basis(dtype, n, k=3):
    """k nearly orthonormal columns: pool vectors 1.. scaled by 1 / sqrt(n) (one rounded multiplication)"""
    V = np.empty((n, k), dtype, order="F")
    s = dtype(1 / np.sqrt(n))
    for j in range(k):
        V[:, j] = base(dtype, 1 + j, n) * s
    return V


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", THREE)
def test_gemv_t_gram_and_the_bicgstab_mr_update_on_three_rungs(pkg, orc, ctx, rung, dtype):
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(9 * n * np.dtype(dtype).itemsize)
    V = basis(dtype, n)
    w = base(dtype, 0, n)
    dV, dw = pkg.HipMatrix.from_numpy(V), dev(pkg, w)
    cols = [np.ascontiguousarray(V[:, j]) for j in range(3)]
    h = pkg.gemv_t_(dV, 3, dw)
    assert np.array_equal(h, np.array([orc.dot(cols[j], w, "tree", W, L) for j in range(3)], dtype))
    M = pkg.gram_(dV, 3)
    want = np.array([[orc.dot(cols[r], cols[c], "tree", W, L) for c in range(3)] for r in range(3)], dtype)
    assert np.array_equal(M, want) and np.array_equal(M, M.T)
    for r in range(3):
        for c in range(r, 3):
            assert M[r, c] == pkg.dot(dV.col(r), dV.col(c))                     # include/mik.h: entry (r, c) equals mik_dot of the columns
    del dw
    # l = 2: us[:, 0] -= us[:, 1:3] g; x += rs[:, 0:2] g; rs[:, 0] -= rs[:, 1:3] g; norm(rs[:, 0])     (the statements of src/bicgstabl.jl:127-132
    # as the oracle's gemv_n writes them: y += (alpha * g_j) * col_j, column by column)
    g = np.array([0.61, -0.27], dtype)
    US = np.asfortranarray(np.stack([base(dtype, 0, n), base(dtype, 3, n), base(dtype, 4, n)], axis=1))
    x0 = base(dtype, 2, n, 64)
    dUS, dx = pkg.HipMatrix.from_numpy(US), dev(pkg, x0)
    out = np.zeros(1, dtype)
    assert pkg.lib().mik_bicgstab_mr_update(ctx.handle, pkg._lib.dtype_code(dtype), n, 2, _vp(dUS.col(0).ptr), dUS.ld, _vp(dV.col(0).ptr), dV.ld,
                                            _vp(dx.ptr), g.ctypes.data_as(_vp), out.ctypes.data_as(_vp)) == 0
    rs0 = orc.gemv_n(V[:, 1:3], g, cols[0], -1.0)
    assert np.array_equal(dUS.col(0).to_numpy(), orc.gemv_n(US[:, 1:3], g, US[:, 0], -1.0))
    assert np.array_equal(dx.to_numpy(), orc.gemv_n(V[:, 0:2], g, x0, 1.0))
    assert np.array_equal(dV.col(0).to_numpy(), rs0)
    assert out[0] == dtype(orc.nrm2(rs0, "tree", W, L))
    assert np.array_equal(dV.col(1).to_numpy(), cols[1]) and np.array_equal(dUS.col(2).to_numpy(), US[:, 2])     # the other columns are only read


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["mgs", "cgs", "dgks"])
@pytest.mark.parametrize("rung", THREE)
def test_orthogonalize_on_three_rungs(pkg, orc, ctx, rung, method, dtype):
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(6 * n * np.dtype(dtype).itemsize)
    V = basis(dtype, n)
    w0 = base(dtype, 0, n)
    if method == "dgks":                                                        # almost inside the span: the re-orthogonalisation loop runs
        w0 = ((V[:, 0] * dtype(0.8) + V[:, 1] * dtype(-0.5)) + V[:, 2] * dtype(0.3)) + dtype(1e-3 / np.sqrt(n)) * w0
    Mth = {"mgs": pkg.ModifiedGramSchmidt(), "cgs": pkg.ClassicalGramSchmidt(), "dgks": pkg.DGKS()}[method]
    dV, dw = pkg.HipMatrix.from_numpy(V), dev(pkg, w0)
    h = np.zeros(3, dtype)
    nrm = pkg.orthogonalize_and_normalize_(dV, 3, dw, h, Mth)
    wo, ho, no = orc.orthogonalize(V, w0, method=method, mode="tree", W=W, L=L)
    assert nrm == no and np.array_equal(h, ho) and np.array_equal(dw.to_numpy(), wo)
    if method == "dgks":
        wc, hc, nc = orc.orthogonalize(V, w0, method="cgs", mode="tree", W=W, L=L)
        assert not np.array_equal(hc, ho) or nc != no                           # the loop really ran


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", THREE)
def test_svdl_reorth_against_its_composed_calls_on_three_rungs(pkg, orc, ctx, rung, dtype):
    from test_gpu_svdl import chain, reorth
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(6 * n * np.dtype(dtype).itemsize)
    V = basis(dtype, n)
    dQ = pkg.HipMatrix.from_numpy(V, ctx)
    alpha = dtype(1 / np.sqrt(2))
    generic = base(dtype, 0, n)
    dependent = ((V[:, 0] * dtype(0.8) + V[:, 1] * dtype(-0.5)) + V[:, 2] * dtype(0.3)) + dtype(1e-6 / np.sqrt(n)) * generic
    for name, qh, want_passes in (("generic", generic, 1), ("dependent", dependent, 2)):
        q1, q2 = dev(pkg, qh), dev(pkg, qh)
        b1, p1 = chain(pkg, dQ, 3, q1, alpha)
        b2, p2 = reorth(pkg, ctx, dQ, 3, q2, alpha)
        assert p1 == p2 == want_passes, (name, p1, p2)
        assert b1 == b2 and np.array_equal(q1.to_numpy(), q2.to_numpy()), name
        if name == "generic":                                                   # the chain's own first norm against the oracle
            assert pkg.norm(dev(pkg, qh)) == dtype(orc.nrm2(qh, "tree", W, L))


# ==============================================================================================
# launch_map2: the fused PCG tail                                             (full ladder)
# ==============================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", RUNGS)
def test_pcg_two_reductions_in_one_sweep_on_the_ladder(pkg, orc, ctx, rung, dtype):
    """cg! with a diagonal Pl forms |r|^2 and dot(c, r) in ONE sweep (OpPcgUpdateR through k_map2).  The operator is a diagonal matrix, so that
    the ladder's n costs n stored entries: two steps, history and x against the oracle."""
    W, L, lad = rungs_of(ctx, dtype)
    m, n, _ = lad[rung]
    need(12 * n * 8)
    a = np.abs(base(dtype, 0, n)) + dtype(1)
    d = np.abs(base(dtype, 1, n)) + dtype(1)
    b = base(dtype, 2, n)
    ptr, idx = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64)
    dA = pkg.HipCSR(n, n, ptr, idx, a, index_base=0)
    x, ch = pkg.cg(dA, dev(pkg, b), Pl=pkg.JacobiPrec(dev(pkg, d)), maxiter=2, reltol=0.0, log=True)
    xo, ho = orc.cg(orc.CSC(n, ptr, idx, a, 0), b, maxiter=2, reltol=0.0, jacobi_diag=d, mode="tree", shape=ctx.cg_shape(dtype))
    assert ch.iters == ho["iters"] == 2
    assert np.array_equal(ch["resnorm"], np.asarray(ho["resnorm"], dtype=np.float64)) and np.array_equal(x.to_numpy(), xo)


# ==============================================================================================
# launch_map_with / launch_map_pro: consumer-side finalisers, m <= 1024
# ==============================================================================================
SMALL_MACHINE = 8 | (1 << 16)           # compute units | XCDs << 16: sweep_grid_cap = 256, so that 256 < m <= 1024 takes several grid-stride passes


def lean_sizes(ctx, dtype):
    """[(plan, m, n)]: m = 1024 / 1025 as the machine is, m = cap + 1 and 2 * cap + 37 planned for 8 compute units"""
    W, L, _ = rungs_of(ctx, dtype)
    SEG = 256 * W * L
    r = SEG // 2 + 3
    out = [(0, mm, (mm - 1) * SEG + r) for mm in (1024, 1025)]
    ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
    try:
        cap = ctx.info()["sweep_grid_cap"]
    finally:
        ctx.set_tuning(KN.MACHINE, 0)
    assert cap == 256
    for mm in (cap + 1, 2 * cap + 37):
        assert cap < mm <= 1024
        out.append((SMALL_MACHINE, mm, (mm - 1) * SEG + r))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_modified_gram_schmidt_lean_chain_at_the_switch_and_on_a_ragged_grid(pkg, orc, ctx, dtype):
    """k_map_pro: every pass finalises the previous pass's reduction itself up to 1024 segments; 1025 takes the general chain"""
    W, L = ctx.reduce_shape(dtype)
    for plan, m, n in lean_sizes(ctx, dtype):
        V = basis(dtype, n)
        w0 = base(dtype, 0, n)
        ctx.set_tuning(KN.MACHINE, plan)
        try:
            dV, dw = pkg.HipMatrix.from_numpy(V), dev(pkg, w0)
            h = np.zeros(3, dtype)
            nrm = pkg.orthogonalize_and_normalize_(dV, 3, dw, h, pkg.ModifiedGramSchmidt())
        finally:
            ctx.set_tuning(KN.MACHINE, 0)
        wo, ho, no = orc.orthogonalize(V, w0, method="mgs", mode="tree", W=W, L=L)
        assert nrm == no and np.array_equal(h, ho) and np.array_equal(dw.to_numpy(), wo), (plan, m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("solver", ["bicgstab2", "minres"])
def test_whole_iteration_calls_at_the_switch_and_on_a_ragged_grid(pkg, orc, ctx, solver, dtype):
    """k_map_with: the sweeps of mik_bicgstab_step / mik_minres_step finalise their producers' reductions themselves up to 1024 segments
    (mik_bicgstab_step whatever the operator's kernel; mik_minres_step where the projection has at most 1024 partials), 1025 takes the
    separate finalisers.  1-D Laplacian of the ladder's n rows, a few iterations against the oracle with the shapes the handles report."""
    for plan, m, n in lean_sizes(ctx, dtype):
        A = orc.laplace(n, 1).astype(dtype)
        b = orc.hashed_rhs(n).astype(dtype)
        ctx.set_tuning(KN.MACHINE, plan)
        try:
            dA = pkg.HipCSR(n, n, A.colptr, A.rowval, A.nzval, index_base=A.index_base)
            x = dev(pkg, np.zeros(n, dtype))
            if solver == "bicgstab2":
                sh = (orc.hashed_rhs(n) + 0.5).astype(dtype)
                it = pkg.bicgstabl_iterator_(x, dA, dev(pkg, b), 2, max_mv_products=12, reltol=0.0, initial_zero=True, r_shadow=dev(pkg, sh))
                shape = it.dot_shape()
                hist = np.array(list(it))
            else:
                it = pkg.minres_iterable_(x, dA, dev(pkg, b), initially_zero=True, maxiter=5, reltol=0.0)
                shape = it.proj_shape()
                hist = np.array(list(it))
            xs = x.to_numpy()
        finally:
            ctx.set_tuning(KN.MACHINE, 0)
        if solver == "bicgstab2":
            xo, ho = orc.bicgstabl(A, b, 2, None, r_shadow=sh, max_mv_products=12, reltol=0.0, mode="tree", shape=ctx.reduce_shape(dtype), dot_shape=shape)
            assert hist.size == 3
        else:
            xo, ho = orc.minres(A, b, maxiter=5, reltol=0.0, mode="tree", shape=ctx.reduce_shape(dtype), proj_shape=shape)
            assert hist.size == 5
        assert np.array_equal(hist, ho["resnorm"], equal_nan=True) and np.array_equal(xs, xo, equal_nan=True), (plan, m)


# ==============================================================================================
# the dot fused into the SpMV                                                 (full ladder, in ITS segment size)
# ==============================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rung", RUNGS)
def test_spmv_fused_dot_on_the_ladder(pkg, orc, ctx, rung, dtype):
    """dot(u, c) leaves the SpMV launch as one partial per 256 * Ld rows (mik_spmv_dot_shape); cg! divides by it (alpha, src/cg.jl:55), so two
    steps of history and x carry its bits.  1-D Laplacian of n = (m - 1) * 256 * Ld + r rows, on the CSR arrays and in the default layout."""
    Wd, Ld = ctx.spmv_dot_shape()
    m, n, _ = ladder(Wd, Ld, ctx.info()["sweep_grid_cap"])[rung]
    A = orc.laplace(n, 1).astype(dtype)
    b = orc.hashed_rhs(n).astype(dtype)
    dA = pkg.HipCSR(n, n, A.colptr, A.rowval, A.nzval, index_base=A.index_base)
    xo, ho = orc.cg(A, b, maxiter=2, reltol=0.0, mode="tree", shape=ctx.cg_shape(dtype))
    for layout in ("csr", "auto"):
        dA.set_layout(layout)
        x, ch = pkg.cg(dA, dev(pkg, b), maxiter=2, reltol=0.0, log=True)
        assert ch.iters == 2 and np.array_equal(ch["resnorm"], np.asarray(ho["resnorm"], dtype=np.float64)), (layout, dA.spmv_kernel())
        assert np.array_equal(x.to_numpy(), xo), (layout, dA.spmv_kernel())


# ==============================================================================================
# the solvers the README quotes at 256^3, at 256^3 -- and on 211^3 rows
# ==============================================================================================
_OPERATOR = {}


def operator(pkg, orc, N):
    """(oracle CSC, device operator, b) of the N^3 Laplacian; one size is kept at a time"""
    if _OPERATOR.get("N") != N:
        _OPERATOR.clear()
        gc.collect()
        n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3)
        _OPERATOR.update(N=N, A=orc.CSC(n, colptr, rowval, nzval, 1), dA=pkg.HipCSR(n, n, colptr, rowval, nzval), b=pkg.fixtures.hashed_rhs(n))
    return _OPERATOR["A"], _OPERATOR["dA"], _OPERATOR["b"]


@pytest.mark.parametrize("N", [256, 211])
@pytest.mark.parametrize("solver", ["pcg_jacobi", "chebyshev", "minres", "bicgstab2"])
def test_solvers_of_the_readme_at_full_size(pkg, orc, ctx, solver, N):
    """PCG (Jacobi), Chebyshev, MINRES and BiCGStab(2) on the 256^3 Laplacian (16.8 M rows, the size README quotes them at) and on 211^3 =
    9,393,931 rows (odd; 9,174 fp64 segments: past the grid cap, ragged in both tree shapes), fp64, hashed_rhs: history and x bit-identical to the
    oracle run with the dot shapes the handle reports, in the operator's default layout and on its CSR arrays.

    Iterations: 4 (BiCGStab(2): 2 outer iterations = 8 products).  The count is bounded by the oracle, which runs on one core of the host:
    measured at 256^3 next to an MI355X (EPYC 9575F), PCG 1.0 s, Chebyshev 0.7 s, MINRES 0.9 s, BiCGStab(2) 2.1 s, once per solver where
    both layouts report the same shapes (at 211^3 MINRES and BiCGStab(2) report two: 0.55 s and 1.2 s each), the device part 0.1 s or less;
    generating and uploading the operator, once per size, takes most of the 2.2 - 3.8 s of a case.  On an 8-core build host the same oracle
    runs take 3.5 / 2.6 / 3.2 / 6.8 s."""
    A, dA, b = operator(pkg, orc, N)
    n = A.n
    need(12 * n * 8 + 2 * A.nnz * 12)
    shape = ctx.reduce_shape(np.float64)
    cache = {}
    try:
        for layout in ("auto", "csr"):
            dA.set_layout(layout)
            x = dev(pkg, np.zeros(n))
            db = dev(pkg, b)
            t0 = time.perf_counter()
            if solver == "pcg_jacobi":
                d = 6 + 0.1 * np.arange(n) / n
                it = pkg.cg_iterator_(x, dA, db, pkg.JacobiPrec(dev(pkg, d)), reltol=0.0, initially_zero=True, maxiter=4)
                key = ctx.cg_shape(np.float64)
                ref = lambda: orc.cg(A, b, maxiter=4, reltol=0.0, jacobi_diag=d, mode="tree", shape=key)
            elif solver == "chebyshev":
                it = pkg.chebyshev_iterable_(x, dA, db, 4.5e-4, 12.0, reltol=0.0, initially_zero=True, maxiter=4)
                key = shape
                ref = lambda: orc.chebyshev(A, b, 4.5e-4, 12.0, maxiter=4, reltol=0.0, mode="tree", shape=shape)
            elif solver == "minres":
                it = pkg.minres_iterable_(x, dA, db, reltol=0.0, initially_zero=True, maxiter=4)
                key = it.proj_shape()
                ref = lambda: orc.minres(A, b, maxiter=4, reltol=0.0, mode="tree", shape=shape, proj_shape=key)
            else:
                sh = pkg.fixtures.hashed_rhs(n) + 0.5
                it = pkg.bicgstabl_iterator_(x, dA, db, 2, reltol=0.0, max_mv_products=8, initial_zero=True, r_shadow=dev(pkg, sh))
                key = it.dot_shape()
                ref = lambda: orc.bicgstabl(A, b, 2, None, r_shadow=sh, max_mv_products=8, reltol=0.0, mode="tree", shape=shape, dot_shape=key)
            hist = np.array(list(it))
            t1 = time.perf_counter()
            if key not in cache:
                cache[key] = ref()
            xo, ho = cache[key]
            print(f"{solver} {N}^3 {layout} ({dA.spmv_kernel()}): device {t1 - t0:.2f} s, oracle {time.perf_counter() - t1:.2f} s, shape {key}")
            assert hist.size == (2 if solver == "bicgstab2" else 4) == len(ho["resnorm"])
            assert np.array_equal(hist, ho["resnorm"]), (layout, hist, ho["resnorm"])
            assert np.array_equal(x.to_numpy(), xo), layout
    finally:
        dA.set_layout("auto")
