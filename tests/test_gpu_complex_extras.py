"""Complex qmr, IDR(s) and the power method on the device.  The three QMR sweeps are compared bit for bit with the C
restatement (tests/complex_ref/complex_extras_ref.c), with the chain of L1 calls each replaces and, in their real-scalar forms, with the
real entry on the same memory; the adjoint of a complex `with_adjoint` operator with the checker's column loop; the solvers run the
complex test sets of test/qmr.jl, test/idrs.jl and test/simple_eigensolvers.jl and must agree bit for bit -- x, every residual, the
counts -- with the numpy double of tests/complex_extras_host.py running the same Python."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_extras_host as ce
import complex_host as ch
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_extras_host import eref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)
from complex_solvers_host import sref  # noqa: F401  (fixture)
from conftest import KN
from test_gpu_complex_solvers import SMALL_MACHINE, Block, real_view, rnd, seg, size_of

pytestmark = pytest.mark.gpu

CT = [np.complex128, np.complex64]
SIZES = ["1", "S-1", "S", "S+1", "5S+3"]
_vp = C.c_void_p
INVALID = 1


def _sc(dtype, v):
    a = np.asarray([v], dtype)
    return a, a.ctypes.data_as(_vp)


def _ptr(v):
    return _vp(v.ptr if v is not None else None)


def axpy2_dot(pkg, y, a, x1, b, x2, z, real=False):
    """mik_axpy2_dot -> (status, out); real: both scalars are reals of the component type and MIK_SCALAR_REAL is set"""
    st = ch.real_of(y.dtype) if real else y.dtype
    (ka, pa), (kb, pb) = _sc(st, a), _sc(st, 0 if b is None else b)
    out = np.full(1, np.nan, y.dtype)
    code = y.code | (pkg._lib.MIK_SCALAR_REAL if real else 0)
    rc = pkg.lib().mik_axpy2_dot(y.ctx.handle, code, y.n, pa, _ptr(x1), pb if b is not None else None, _ptr(x2), _ptr(y), _ptr(z), out.ctypes.data_as(_vp))
    return rc, out[0]


def qmr_update(pkg, v, h1, pc, h0, pp, inv, g, x, po, real=False):
    st = ch.real_of(x.dtype) if real else x.dtype
    sc = [_sc(st, 0 if s is None else s) for s in (h1, h0, inv, g)]
    code = x.code | (pkg._lib.MIK_SCALAR_REAL if real else 0)
    return pkg.lib().mik_qmr_update(x.ctx.handle, code, x.n, _ptr(v), sc[0][1], _ptr(pc), sc[1][1], _ptr(pp), sc[2][1], sc[3][1], _ptr(x), _ptr(po))


def scal2(pkg, a, x, b, y, real=False):
    st = ch.real_of(x.dtype) if real else x.dtype
    (ka, pa), (kb, pb) = _sc(st, a), _sc(st, b)
    return pkg.lib().mik_scal2(x.ctx.handle, x.code | (pkg._lib.MIK_SCALAR_REAL if real else 0), x.n, pa, _ptr(x), pb, _ptr(y))


# ---------------------------------------------------------------------------------------------
# the three entries
# ---------------------------------------------------------------------------------------------
def check_entries(pkg, ctx, eref, T, n, offset=0, offset_only=None, dot=True, others=True):
    """every form of the three entries at n elements.  offset: the byte offset of the operands (8: the element-wise variant);
    offset_only: only that operand is offset (each alignment term of the 16-byte test alone)"""
    shape, rt = ctx.reduce_shape(T), ch.real_of(T).type
    rng = np.random.default_rng(n + 17)
    hs = {k: rnd(rng, T, n) for k in ("x1", "x2", "y", "z", "v", "pc", "pp", "x")}
    a, b, h1, h0, inv, g = T(0.5 - 1.25j), T(-0.75 + 0.5j), T(0.25 + 0.5j), T(-1.5 - 0.25j), T(0.5 + 0.5j), T(1.25 - 0.75j)

    def V(name):
        off = offset if offset_only in (None, name) else 0
        return Block(pkg, ctx, [hs[name]], None, off).col(0)
    x1, x2, z = V("x1"), V("x2"), V("z")
    if dot:
        for with_x2 in (True, False):
            for with_z in (True, False):
                y, want = V("y"), hs["y"].copy()
                rc, got = axpy2_dot(pkg, y, a, x1, b if with_x2 else None, x2 if with_x2 else None, z if with_z else None)
                exp = eref.axpy2_dot(want, a, hs["x1"], b, hs["x2"] if with_x2 else None, hs["z"] if with_z else None, shape)
                assert rc == 0 and np.array_equal(y.to_numpy(), want), (with_x2, with_z)
                assert (got == exp) if with_z else np.isnan(got), (with_x2, with_z)      # z NULL: out untouched
                y2 = V("y").axpy_(a, x1)                                     # the chain of L1 calls it replaces
                if with_x2:
                    y2.axpy_(b, x2)
                assert np.array_equal(y2.to_numpy(), want) and (not with_z or got == pkg.dot(z, y2))
        # real scalars: with z the complex kernel's real form; without z the real entry over 2 n, also called on the same memory
        ar, br = rt(-0.75), rt(1.5)
        y, want = V("y"), hs["y"].copy()
        rc, got = axpy2_dot(pkg, y, ar, x1, br, x2, z, real=True)
        assert rc == 0 and got == eref.axpy2_dot(want, ar, hs["x1"], br, hs["x2"], hs["z"], shape) and np.array_equal(y.to_numpy(), want)
        y2, y3 = V("y"), V("y")
        assert axpy2_dot(pkg, y2, ar, x1, br, x2, None, real=True)[0] == 0 and np.array_equal(y2.to_numpy(), want)
        assert axpy2_dot(pkg, real_view(pkg, y3), ar, real_view(pkg, x1), br, real_view(pkg, x2), None)[0] == 0 and np.array_equal(y3.to_numpy(), want)
        assert pkg.dot(z, y2) == got
    if not others:
        return
    # scal2
    xa, xb, wa, wb = V("x1"), V("x2"), hs["x1"].copy(), hs["x2"].copy()
    assert scal2(pkg, inv, xa, g, xb) == 0
    eref.scal2(inv, wa, g, wb)
    assert np.array_equal(xa.to_numpy(), wa) and np.array_equal(xb.to_numpy(), wb)
    assert np.array_equal(V("x1").scal_(inv).to_numpy(), wa) and np.array_equal(V("x2").scal_(g).to_numpy(), wb)      # the chain
    xa, xb, xc, xd = V("x1"), V("x2"), V("x1"), V("x2")                      # real scalars: the real entry over 2 n
    assert scal2(pkg, rt(0.5), xa, rt(-3), xb, real=True) == 0 and scal2(pkg, rt(0.5), real_view(pkg, xc), rt(-3), real_view(pkg, xd)) == 0
    assert np.array_equal(xa.to_numpy(), xc.to_numpy()) and np.array_equal(xb.to_numpy(), xd.to_numpy())
    assert np.array_equal(xa.to_numpy(), V("x1").scal_(rt(0.5)).to_numpy())
    # qmr_update: iterations 1, 2, >= 3; p_out its own vector and p_prev's storage
    v, pc = V("v"), V("pc")
    for cur, prev in ((False, False), (True, False), (True, True)):
        for alias in ((False, True) if prev else (False,)):
            pp, x = V("pp"), V("x")
            po = pp if alias else Block(pkg, ctx, [np.zeros(n, T)], None, offset if offset_only is None else 0).col(0)
            assert qmr_update(pkg, v, h1, pc if cur else None, h0, pp if prev else None, inv, g, x, po) == 0
            wx, wp = hs["x"].copy(), np.zeros(n, T)
            eref.qmr_update(hs["v"], h1, hs["pc"] if cur else None, h0, hs["pp"] if prev else None, inv, g, wx, wp)
            assert np.array_equal(x.to_numpy(), wx) and np.array_equal(po.to_numpy(), wp), (cur, prev, alias)
            t, x2_ = V("v"), V("x")                                          # the chain: src/qmr.jl:196-202
            if cur:
                t.axpy_(h1, pc)
            if prev:
                t.axpy_(h0, V("pp"))
            t.scal_(inv)
            x2_.axpy_(g, t)
            assert np.array_equal(t.to_numpy(), wp) and np.array_equal(x2_.to_numpy(), wx)
    sr = [rt(0.5), rt(-0.25), rt(2), rt(-1.5)]                               # four real scalars: the real entry over 2 n
    xa, pa, xb, pb = V("x"), V("pp"), V("x"), V("pp")
    assert qmr_update(pkg, v, sr[0], pc, sr[1], pa, sr[2], sr[3], xa, pa, real=True) == 0
    assert qmr_update(pkg, real_view(pkg, v), sr[0], real_view(pkg, pc), sr[1], real_view(pkg, pb), sr[2], sr[3], real_view(pkg, xb), real_view(pkg, pb)) == 0
    assert np.array_equal(xa.to_numpy(), xb.to_numpy()) and np.array_equal(pa.to_numpy(), pb.to_numpy())


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", SIZES)
def test_the_three_entries(pkg, ctx, eref, T, which):
    check_entries(pkg, ctx, eref, T, size_of(ctx, T, which))


@pytest.mark.parametrize("T", CT)
def test_axpy2_dot_past_1024_segments(pkg, ctx, eref, T):
    check_entries(pkg, ctx, eref, T, size_of(ctx, T, "1024S+1"), others=False)


@pytest.mark.parametrize("T", CT)
def test_second_pass_of_the_grid_stride_loops(pkg, ctx, eref, T):
    n = size_of(ctx, T, "2 passes")
    ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
    try:
        assert ctx.info()["sweep_grid_cap"] == 256 < (n + seg(ctx, T) - 1) // seg(ctx, T) <= 512      # two passes, the second ragged
        check_entries(pkg, ctx, eref, T, n)
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


@pytest.mark.parametrize("only", [None, "y", "z", "x2", "pp", "x"])
@pytest.mark.parametrize("T", CT)
def test_elementwise_variants(pkg, ctx, eref, T, only):
    """operands at an 8-byte offset (all of them, then one alone): the element-wise variant, the same bits as the checker's"""
    check_entries(pkg, ctx, eref, T, size_of(ctx, T, "S+1"), offset=8, offset_only=only)


@pytest.mark.parametrize("T", CT)
def test_refusals_of_the_three_entries(pkg, ctx, T):
    """the INVALID cases, as for the real codes: null scalars, null vectors, forbidden aliasing; nothing is written"""
    n = 100
    rng = np.random.default_rng(5)
    hs = [rnd(rng, T, n) for _ in range(5)]
    v, pc, pp, x, po = (pkg.HipVector.from_numpy(h, ctx) for h in hs)
    L, code = pkg.lib(), pkg._lib.dtype_code(T)
    one, p = np.ones(2, T), _ptr
    s = one.ctypes.data_as(_vp)
    out = np.zeros(1, T).ctypes.data_as(_vp)
    for c in (code, code | pkg._lib.MIK_SCALAR_REAL):
        assert L.mik_axpy2_dot(ctx.handle, c, n, None, p(v), s, p(pc), p(x), None, out) == INVALID                    # a NULL
        assert L.mik_axpy2_dot(ctx.handle, c, n, s, p(v), None, p(pc), p(x), None, out) == INVALID                    # x2 without b
        assert L.mik_axpy2_dot(ctx.handle, c, n, s, p(v), s, p(pc), p(x), p(pp), None) == INVALID                     # z without out
        assert L.mik_axpy2_dot(ctx.handle, c, n, s, None, s, None, p(x), None, out) == INVALID                        # x1 NULL
        assert L.mik_scal2(ctx.handle, c, n, None, p(x), s, p(po)) == INVALID and L.mik_scal2(ctx.handle, c, n, s, p(x), None, p(po)) == INVALID
        assert L.mik_scal2(ctx.handle, c, n, s, None, s, p(po)) == INVALID
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), s, p(pp), None, s, p(x), p(po)) == INVALID          # inv NULL
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), s, p(pp), s, None, p(x), p(po)) == INVALID          # g NULL
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), None, p(pc), s, p(pp), s, s, p(x), p(po)) == INVALID          # p_curr without neg_h1
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), None, p(pp), s, s, p(x), p(po)) == INVALID          # p_prev without neg_h0
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), s, p(pp), s, s, p(x), p(v)) == INVALID              # p_out is v
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), s, p(pp), s, s, p(x), p(pc)) == INVALID             # p_out is p_curr
        assert L.mik_qmr_update(ctx.handle, c, n, p(v), s, p(pc), s, p(pp), s, s, None, p(po)) == INVALID
    for d, h in zip((v, pc, pp, x, po), hs):
        assert np.array_equal(d.to_numpy(), h)
    empty = pkg.HipVector(0, T, ctx)                                         # n = 0: nothing to do, dot = 0
    rc, got = axpy2_dot(pkg, empty, T(1), empty, None, None, empty)
    assert rc == 0 and got == 0


# ---------------------------------------------------------------------------------------------
# adjoint(A) of a complex operator
# ---------------------------------------------------------------------------------------------
def _adjoint_cases(T):
    rng = np.random.default_rng(61)
    rt = ch.real_of(T)

    def sprand(m, n, density):
        M = sp.random(m, n, density, random_state=rng, format="csc", dtype=rt) + 1j * sp.random(m, n, density, random_state=rng, format="csc", dtype=rt)
        return sp.csc_matrix(M.astype(T))
    gaps = sprand(300, 700, 0.02).tolil()                                     # adjoint: 700 rows in three row blocks, some of them empty
    gaps[:, 250:270] = 0
    gaps[:, 699] = 0
    long_col = sprand(900, 40, 0.05).tolil()                                  # one column of A with 600 entries: a row of the adjoint past MIK_LONG_ROW = 256
    long_col[:600, 7] = (rnd(rng, T, 600) + T(2)).reshape(-1, 1)
    return dict(gaps=sp.csc_matrix(gaps), rectangular=sprand(130, 61, 0.1), long_row=sp.csc_matrix(long_col))


@pytest.mark.parametrize("idx", [np.int64, np.int32])
@pytest.mark.parametrize("case", ["gaps", "rectangular", "long_row"])
@pytest.mark.parametrize("T", CT)
def test_adjoint_of_a_complex_operator(pkg, ctx, eref, ref, T, case, idx):
    M = _adjoint_cases(T)[case]
    M.eliminate_zeros()
    M.sort_indices()
    m, n = M.shape
    A = pkg.extras.with_adjoint(m, n, M.indptr.astype(idx), M.indices.astype(idx), M.data, index_base=0, ctx=ctx)
    assert A.adj.adj is A and pkg.extras.adjoint(A) is A.adj and (A.adj.n_rows, A.adj.n_cols) == (n, m)
    xh = rnd(np.random.default_rng(62), T, m)
    y = pkg.mul_(pkg.HipVector(n, T, ctx), A.adj, pkg.HipVector.from_numpy(xh, ctx)).to_numpy()
    want = eref.adj_mul(M, xh)                                               # the reference's loop over the columns of A
    lens = np.diff(M.indptr)
    short = lens <= 256
    assert np.array_equal(y[short], want[short])
    if case == "long_row":
        # a row past MIK_LONG_ROW is summed in the wave shape of the SpMV, not serially: held to the SpMV checker on
        # the arrays the adjoint operator holds, and to the serial loop within the rounding of a sum of 600 terms
        assert not short.all()
        up = ref.spmv(M.indptr.astype(np.int32), M.indices.astype(np.int32), np.conj(M.data), xh, n)
        assert np.array_equal(y, up)
        eps = np.finfo(ch.real_of(T)).eps
        assert np.all(np.abs(y[~short] - want[~short]) <= 600 * eps * np.abs(np.conj(M.toarray()[:, ~short]).T) @ np.abs(xh))
    else:
        assert short.all()
    # and A itself is untouched by the conjugation
    xn = rnd(np.random.default_rng(63), T, n)
    Mr = sp.csr_matrix(M)
    Mr.sort_indices()
    ya = pkg.mul_(pkg.HipVector(m, T, ctx), A, pkg.HipVector.from_numpy(xn, ctx)).to_numpy()
    assert np.array_equal(ya, ref.spmv(Mr.indptr.astype(np.int32), Mr.indices.astype(np.int32), Mr.data, xn, m))


# ---------------------------------------------------------------------------------------------
# the solvers: the complex test sets, device against the double running the same Python
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def device(pkg, ctx):
    return ce.DeviceBackend(pkg, ctx)


def on_host(pkg, ref, dref, sref, eref, run):
    """run(backend) on the numpy double, extras.py routed to it for the duration"""
    with pytest.MonkeyPatch.context() as mp:
        be = ce.HostBackend(pkg, ref, dref, sref)
        ce.patch(mp, pkg, be, eref)
        return run(be)


@pytest.mark.parametrize("kind,idx", [("csr", np.int64), ("csr", np.int32), ("dense", np.int64), ("linop", np.int64)])
@pytest.mark.parametrize("T", CT)
def test_qmr_sets(pkg, device, ref, dref, sref, eref, T, kind, idx):
    host = on_host(pkg, ref, dref, sref, eref, lambda be: (ce.qmr_sets(be, T, kind), ce.termination(be, T, "qmr", kind)))
    for fused in (True, False):
        dev = ce.qmr_sets(device, T, kind, fused=fused, idx=idx), ce.termination(device, T, "qmr", kind, fused=fused)
        ce.check_qmr_sets(dev[0], T)
        ce.check_termination(dev[1])
        ce.same(dev[0], host[0])
        ce.same(dev[1], host[1])


@pytest.mark.parametrize("kind,idx", [("csr", np.int64), ("csr", np.int32), ("dense", np.int64), ("linop", np.int64)])
@pytest.mark.parametrize("T", CT)
def test_idrs_sets(pkg, device, ref, dref, sref, eref, T, kind, idx):
    """without and with smoothing (test/idrs.jl:20-32), sparse (:35-43), termination (:82-106)"""
    host = on_host(pkg, ref, dref, sref, eref, lambda be: (ce.idrs_sets(be, T, kind), ce.termination(be, T, "idrs", kind)))
    for fused in (True, False):
        dev = ce.idrs_sets(device, T, kind, fused=fused, idx=idx), ce.termination(device, T, "idrs", kind, fused=fused)
        ce.check_idrs_sets(dev[0], T)
        ce.check_termination(dev[1])
        ce.same(dev[0], host[0])
        ce.same(dev[1], host[1])


def test_idrs_with_a_preconditioner(pkg, device, ref, dref, sref, eref):
    """test/idrs.jl:45-62 (ComplexF64, n = 1000, Int32 indices on the device)"""
    T = np.complex128
    host = on_host(pkg, ref, dref, sref, eref, lambda be: ce.idrs_prec_sets(be, T))
    dev = ce.idrs_prec_sets(device, T, idx=np.int32)
    ce.check_idrs_prec_sets(dev, T)
    ce.same(dev, host)


@pytest.mark.parametrize("T", CT)
def test_complex_idrs_has_no_fused_handle(pkg, device, T):
    inp = ce.idrs_inputs(T)
    it = pkg.extras.idrs_iterable_(None, device.vector(np.zeros(inp["n"], T)), device.operator(inp["S"]), device.vector(inp["bs"]), ce.S, None, 0.0,
                                   inp["reltol"], 10, P=inp["P"], fused=True)
    assert it._step is None and it._compose
    assert it.iterate() is not None and it._step is None
    with pytest.raises(TypeError, match="JacobiPrec is not offered for complex element types"):
        pkg.extras.idrs(device.operator(inp["S"]), device.vector(inp["bs"]), Pl=pkg.JacobiPrec(device.vector(np.ones(inp["n"], T))), P=inp["P"])


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("T", CT)
def test_power_method_sets(pkg, device, ref, dref, sref, eref, T, kind):
    host = on_host(pkg, ref, dref, sref, eref, lambda be: ce.powm_sets(be, T, kind))
    dev = ce.powm_sets(device, T, kind)
    ce.check_powm_sets(dev, T)
    ce.same(dev, host)
