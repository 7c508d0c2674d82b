"""Complex dense operators on the device: y = A x and y = A' x on a ComplexF64 / ComplexF32 column-major matrix.

Every comparison is np.array_equal: the contract fixes every bit.  References: the C restatement of the two orders
(tests/complex_ref/complex_dense_ref.c); for n <= C also mik_spmv of the fully stored complex CSR; for the adjoint also mik_dot of every
column on the device.  Rc = rows per workgroup (mik_dense_mul_shape_for), S = 256 W L (mik_reduce_shape), U = 8 columns in flight
(MIK_CDM_U).  Every y is a view between guard elements that must stay untouched, and every launch-shape case first asserts its
mik_dev_dense_plan (include/mik_dev.h: computed by the helper the launch itself uses).  The solvers run the complex Matrix{T} test sets of
test/cg.jl:27-47,99-121 and test/gmres.jl:16-36,76-98 on a HipMatrix and must agree bit for bit with the numpy double."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import complex_dense_host as cdh
import complex_host as ch
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)
from conftest import KN

pytestmark = pytest.mark.gpu

CT = [np.complex128, np.complex64]
_vp = C.c_void_p
U = 8                               # MIK_CDM_U
TCOLS = 32                          # MIK_CDM_TCOLS
STREAM_BYTES = 192.0e6              # MIK_DM_STREAM_BYTES
SMALL_MACHINE = 8 | (1 << 16)       # 8 compute units, 1 XCD: 4 * CUs = 32 workgroups over (gx, gy), mik_max_grid = 256
NOTIMPL = 5


def rnd(T, *shape, seed=0):
    rng = np.random.default_rng(seed)
    rt = ch.real_of(T)
    a = rng.standard_normal(shape[::-1]).astype(rt) + 1j * rng.standard_normal(shape[::-1]).astype(rt)
    return a.astype(T).T                                              # column-major


def shapes(pkg, ctx, T):
    """(C, Rc, (W, L), S)"""
    c, r = cdh.mul_shape(pkg, T)
    w, l = ctx.reduce_shape(T)
    assert w == 16 // np.dtype(T).itemsize and r % 256 == 0
    return c, r, (w, l), 256 * w * l


@contextlib.contextmanager
def machine(ctx, value):
    ctx.set_tuning(KN.MACHINE, value)
    try:
        yield
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


class Dev:
    """A complex matrix in a raw device buffer with its own mik_dense handle: leading dimension lda (elements), its first element
    `byte_off` bytes into the allocation.  The padding rows are NaN: they must never be read."""

    def __init__(self, pkg, ctx, A, lda=None, byte_off=0):
        T = A.dtype
        self.pkg, self.ctx, self.m, self.n, self.T = pkg, ctx, A.shape[0], A.shape[1], T
        self.lda = int(self.m if lda is None else lda)
        store = np.full((self.lda, max(self.n, 1)), np.nan + 1j * np.nan, T, order="F")
        store[:self.m, :self.n] = A
        self.buf = pkg.HipVector(store.size + 1, T, ctx)
        self.ptr = self.buf.ptr + byte_off
        pkg.HipVector.wrap(self.ptr, store.size, T, ctx, owner=self.buf).copy_from_host(store.reshape(-1, order="F"))
        self.h = self.create(self.n)

    def create(self, n):
        h = _vp()
        assert self.pkg.lib().mik_dense_create(self.ctx.handle, self.pkg._lib.dtype_code(self.T), self.m, n, _vp(self.ptr), self.lda, C.byref(h)) == 0
        return h

    def col(self, j):
        return self.pkg.HipVector.wrap(self.ptr + j * self.lda * np.dtype(self.T).itemsize, self.m, self.T, self.ctx, owner=self.buf)

    def close(self):
        self.pkg.lib().mik_dense_destroy(self.h)


class Out:
    """a result vector as a view `byte_off` bytes past 64 guard elements, 64 more behind it; every real of the guards is 7, so that a shifted
    view leaves the same pattern; `read` returns the view's elements after checking that the guards are still there"""

    def __init__(self, pkg, ctx, n, T, byte_off=0):
        self.n, self.T, self.off = int(n), T, byte_off
        self.buf = pkg.HipVector(64 + self.n + 65, T, ctx).fill_(T(7 + 7j))
        self.y = pkg.HipVector.wrap(self.buf.ptr + 64 * np.dtype(T).itemsize + byte_off, self.n, T, ctx, owner=self.buf)
        assert (self.y.ptr % 16 != 0) == bool(byte_off)

    def read(self):
        rt = ch.real_of(self.T)
        a = self.buf.to_numpy().view(rt)
        lo = (64 * np.dtype(self.T).itemsize + self.off) // rt.itemsize
        hi = lo + 2 * self.n
        assert np.all(a[:lo] == 7) and np.all(a[hi:] == 7)
        out = a[lo:hi].copy().view(self.T)
        self.buf.fill_(self.T(7 + 7j))
        return out


def matrix(pkg, ctx, A):
    """a HipMatrix in one copy: the padding rows of the leading dimension are zero, as HipMatrix leaves them"""
    M = pkg.HipMatrix(A.shape[0], A.shape[1], A.dtype, ctx)
    store = np.zeros((M.ld, A.shape[1]), A.dtype, order="F")
    store[:A.shape[0]] = A
    M.buf.copy_from_host(store.reshape(-1, order="F"))
    return M


def V(pkg, ctx, a, byte_off=0):
    a = np.ascontiguousarray(a)
    if not byte_off:
        return pkg.HipVector.from_numpy(a, ctx)
    buf = pkg.HipVector(a.size + 1, a.dtype, ctx)
    v = pkg.HipVector.wrap(buf.ptr + byte_off, a.size, a.dtype, ctx, owner=buf).copy_from_host(a)
    assert v.ptr % 16 != 0
    return v


def plan(pkg, h, adjoint, x, y):
    vec, streamed = C.c_int(-1), C.c_int(-1)
    gx, gy, cols, nseg = (C.c_int64(-1) for _ in range(4))
    assert pkg.lib().mik_dev_dense_plan(h, int(adjoint), _vp(x.ptr), _vp(y.ptr), C.byref(vec), C.byref(streamed), C.byref(gx), C.byref(gy),
                                        C.byref(cols), C.byref(nseg)) == 0
    return {"vec": vec.value, "streamed": streamed.value, "gx": gx.value, "gy": gy.value, "cols": cols.value, "nseg": nseg.value}


def expect(p, **want):
    assert {k: p[k] for k in want} == want, (p, want)


def mul(pkg, h, adjoint, x, out):
    assert pkg.lib().mik_dense_mul(h, int(adjoint), _vp(x.ptr), _vp(out.y.ptr)) == 0
    return out.read()


def same_bits(a, b):
    rt = ch.real_of(a.dtype)
    a, b = np.ascontiguousarray(a).view(rt), np.ascontiguousarray(b).view(rt)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def full_csr(pkg, ctx, A):
    m, n = A.shape
    return pkg.HipCSR(m, n, (np.arange(m + 1) * n).astype(np.int64), np.tile(np.arange(n), m).astype(np.int64), np.ascontiguousarray(A).reshape(-1),
                      index_base=0, is_csc=False, ctx=ctx)


def device_dots(pkg, col, n, xd):
    return np.array([pkg.dot(col(j), xd) for j in range(n)], xd.dtype)


# ---- creation and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_create_accepts_the_complex_codes_and_the_block_entries_refuse_them(pkg, ctx, T):
    M = pkg.HipMatrix(5, 5, T, ctx)
    h = _vp()
    L = pkg.lib()
    assert L.mik_dense_create(ctx.handle, pkg._lib.dtype_code(T), 5, 5, _vp(M.buf.ptr), M.ld, C.byref(h)) == 0 and h      # MIK_OK
    name ="ComplexF64" if T == np.complex128 else "ComplexF32"
    try:
        assert L.mik_dense_block_reserve(h) == NOTIMPL and name in L.mik_last_error(ctx.handle).decode()
        X = pkg.HipMatrix(5, 2, T, ctx)
        assert L.mik_dense_mm(h, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld) == NOTIMPL and name in L.mik_last_error(ctx.handle).decode()
        assert L.mik_dense_create(ctx.handle, pkg._lib.dtype_code(T), 5, 5, _vp(M.buf.ptr), 4, C.byref(_vp())) == 3      # lda < m: MIK_ERR_MISMATCH, as for the real codes
    finally:
        L.mik_dense_destroy(h)
    with pytest.raises(TypeError, match=str(np.dtype(T))):
        M.mm_(X, X)
    with pytest.raises(TypeError, match=str(np.dtype(T))):
        M.reserve_block_()
    with pytest.raises(TypeError, match=str(np.dtype(T))):
        pkg.lobpcg(M, False, 1, dense=True)
    assert M.adj.adj is M and pkg.extras.adjoint(M) is M.adj


# ---- N form -------------------------------------------------------------------------------------------------------------------------
def n_table(C_, Rc):
    """a covering table of m in {1, Rc - 1, Rc, Rc + 1, 2 Rc + 1} x n in {1, U - 1, U, U + 1, C - 1, C, C + 1, 5 C + 3}: every m and every n
    at least once, the row-block edges against one chunk, one chunk + 1 and several chunks"""
    return [(1, 1), (1, 5 * C_ + 3), (Rc - 1, U - 1), (Rc - 1, C_ + 1), (Rc, U), (Rc, C_), (Rc, 5 * C_ + 3), (Rc + 1, U + 1), (Rc + 1, C_ - 1),
            (Rc + 1, C_ + 1), (2 * Rc + 1, 1), (2 * Rc + 1, C_), (2 * Rc + 1, 5 * C_ + 3)]


@pytest.mark.parametrize("T", CT)
def test_n_form_against_the_checker_and_the_full_csr(pkg, ctx, dref, T):
    C_, Rc, _, _ = shapes(pkg, ctx, T)
    for m, n in n_table(C_, Rc):
        A, x = rnd(T, m, n, seed=m + n), rnd(T, n, seed=7)
        M, xd, out = matrix(pkg, ctx, A), V(pkg, ctx, x), Out(pkg, ctx, m, T)
        expect(plan(pkg, M.dense, 0, xd, out.y), vec=1, streamed=0, gx=-(-m // Rc), cols=-(-n // C_), nseg=0)
        got = mul(pkg, M.dense, 0, xd, out)
        assert np.array_equal(got, dref.mul_n(A, x, C_)), (m, n)
        if n <= C_:
            assert np.array_equal(got, (full_csr(pkg, ctx, A) @ xd).to_numpy()), (m, n)
        assert np.array_equal((M @ xd).to_numpy(), got)
    # empty dimensions: nothing is launched, the empty sum is (+0, +0)
    M = pkg.HipMatrix(4, 0, T, ctx)
    assert same_bits((M @ pkg.HipVector(0, T, ctx)).to_numpy(), np.zeros(4, T))


# ---- T form -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_t_form_against_the_checker_and_mik_dot(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    for m, n in ((1, 1), (1, 33), (S - 1, 2), (S, 3), (S + 1, 4), (S + 1, 5), (5 * S + 3, 33), (1024 * S + 3, 2)):
        A, x = rnd(T, m, n, seed=m % 1000 + n), rnd(T, m, seed=9)
        M, xd, out = matrix(pkg, ctx, A), V(pkg, ctx, x), Out(pkg, ctx, n, T)
        expect(plan(pkg, M.dense, 1, xd, out.y), vec=1, streamed=0, nseg=-(-m // S), cols=-(-n // TCOLS))
        got = mul(pkg, M.dense, 1, xd, out)
        assert np.array_equal(got, dref.mul_t(A, x, shape)), (m, n)
        assert np.array_equal(got, device_dots(pkg, M.col, n, xd)), (m, n)
        assert np.array_equal((M.adj @ xd).to_numpy(), got)
    M = pkg.HipMatrix(0, 3, T, ctx)
    assert same_bits((M.adj @ pkg.HipVector(0, T, ctx)).to_numpy(), np.zeros(3, T))


# ---- the scalar-load variant: each alignment term on its own ------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_each_alignment_term_alone_takes_the_scalar_variant_with_the_same_bits(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    for adjoint, m, n in ((0, Rc + 1, C_ - 1), (0, Rc + 1, 2 * C_ + 1), (1, S + 1, 5)):
        A = rnd(T, m, n, seed=40 + n)
        x = rnd(T, m if adjoint else n, seed=41)
        want = dref.mul_t(A, x, shape) if adjoint else dref.mul_n(A, x, C_)
        lda_even = m + m % 2
        cases = [("aligned", dict(lda=lda_even), 0, 0, 1), ("base + 8", dict(lda=lda_even, byte_off=8), 0, 0, 0)]
        if T == np.complex64:
            cases.append(("lda odd", dict(lda=lda_even + 1), 0, 0, 0))
        if adjoint:
            cases.append(("x + 8", dict(lda=lda_even), 8, 0, 0))
            cases.append(("y + 8", dict(lda=lda_even), 0, 8, 1))                       # the finaliser writes y: it never matters
        else:
            cases.append(("x + 8", dict(lda=lda_even), 8, 0, 1))                       # x comes by scalar loads: it never matters
            cases.append(("y + 8", dict(lda=lda_even), 0, 8, 0 if n <= C_ else 1))     # only a y the product kernel writes itself
        for name, kw, xoff, yoff, vec in cases:
            D = Dev(pkg, ctx, A, **kw)
            xd, out = V(pkg, ctx, x, xoff), Out(pkg, ctx, n if adjoint else m, T, yoff)
            expect(plan(pkg, D.h, adjoint, xd, out.y), vec=vec)
            got = mul(pkg, D.h, adjoint, xd, out)
            assert np.array_equal(got, want), (name, adjoint, m, n)
            if adjoint:
                assert np.array_equal(got, device_dots(pkg, D.col, n, xd)), name
            D.close()


# ---- combine batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_combine_batches_on_a_three_row_matrix(pkg, ctx, dref, T):
    C_, Rc, _, _ = shapes(pkg, ctx, T)
    for nc in (2, 9, 10, 33, 42):                                     # the tail alone, the 8-batch, 8 + tail, the 32-batch, 32 + 8 + tail
        n = nc * C_ - 5
        A, x = rnd(T, 3, n, seed=nc), rnd(T, n, seed=nc + 1)
        M, xd, out = matrix(pkg, ctx, A), V(pkg, ctx, x), Out(pkg, ctx, 3, T)
        expect(plan(pkg, M.dense, 0, xd, out.y), vec=1, gx=1, gy=nc, cols=nc)
        assert np.array_equal(mul(pkg, M.dense, 0, xd, out), dref.mul_n(A, x, C_)), nc


# ---- grid-stride loops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_n_form_chunk_loop_takes_two_and_three_ragged_passes_in_both_variants(pkg, ctx, dref, T):
    C_, Rc, _, _ = shapes(pkg, ctx, T)
    for m, n, gx, gy, nc, passes in ((65, 33 * C_ + 3, 1, 32, 34, 2), (Rc + 1, 32 * C_ + 1, 2, 16, 33, 3)):
        A, x = rnd(T, m, n, seed=nc), rnd(T, n, seed=3)
        want = dref.mul_n(A, x, C_)
        xd = V(pkg, ctx, x)
        for vec, kw in ((1, dict(lda=m + m % 2)), (0, dict(lda=m + m % 2, byte_off=8))):
            D, out = Dev(pkg, ctx, A, **kw), Out(pkg, ctx, m, T)
            with machine(ctx, SMALL_MACHINE):
                p = plan(pkg, D.h, 0, xd, out.y)
                expect(p, vec=vec, streamed=0, gx=gx, gy=gy, cols=nc)
                assert -(-nc // gy) == passes and nc % gy != 0
                small = mul(pkg, D.h, 0, xd, out)
            expect(plan(pkg, D.h, 0, xd, out.y), vec=vec, gx=gx, cols=nc)
            as_queried = mul(pkg, D.h, 0, xd, out)
            assert np.array_equal(small, want) and np.array_equal(as_queried, want), (m, n, vec)
            D.close()


@pytest.mark.parametrize("T", CT)
def test_t_form_column_batch_loop_and_segment_loop_take_a_second_pass(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    # (m, n, gx, gy, batches, segments): 34 batches over 32 workgroups; 293 segments over mik_max_grid = 256 workgroups
    for m, n, gx, gy, batches, nseg in ((S - 1, 33 * TCOLS + 5, 1, 32, 34, 1), (292 * S + 3, 5, 256, 1, 1, 293)):
        A, x = rnd(T, m, n, seed=n), rnd(T, m, seed=5)
        want = dref.mul_t(A, x, shape)
        D, xd, out = Dev(pkg, ctx, A, lda=m + m % 2), V(pkg, ctx, x), Out(pkg, ctx, n, T)
        with machine(ctx, SMALL_MACHINE):
            expect(plan(pkg, D.h, 1, xd, out.y), vec=1, streamed=0, gx=gx, gy=gy, cols=batches, nseg=nseg)
            assert -(-batches // gy) * -(-nseg // gx) == 2
            small = mul(pkg, D.h, 1, xd, out)
        expect(plan(pkg, D.h, 1, xd, out.y), vec=1, cols=batches, nseg=nseg)
        as_queried = mul(pkg, D.h, 1, xd, out)
        assert np.array_equal(small, want) and np.array_equal(as_queried, want), (m, n)
        D.close()


# ---- streamed kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_streamed_kernels_on_both_sides_of_their_threshold(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    es = np.dtype(T).itemsize
    m = 2 * Rc + 1
    n = int(STREAM_BYTES // (m * es)) + 1
    assert m * n * es > STREAM_BYTES >= m * (n - 1) * es
    A, xn, xt = rnd(T, m, n, seed=30), rnd(T, n, seed=31), rnd(T, m, seed=32)
    D = Dev(pkg, ctx, A, lda=m + m % 2)
    less = D.create(n - 1)                                           # a second handle over the same buffer: one column fewer
    xnd, xtd = V(pkg, ctx, xn), V(pkg, ctx, xt)
    want_t = dref.mul_t(A, xt, shape)
    try:
        for h, k, streamed in ((D.h, n, 1), (less, n - 1, 0)):
            out = Out(pkg, ctx, m, T)
            xk = xnd.view(0, k)
            expect(plan(pkg, h, 0, xk, out.y), vec=1, streamed=streamed, gx=3, cols=-(-k // C_))
            assert np.array_equal(mul(pkg, h, 0, xk, out), dref.mul_n(A[:, :k], xn[:k], C_)), (k, "N")
            out = Out(pkg, ctx, k, T)
            expect(plan(pkg, h, 1, xtd, out.y), vec=1, streamed=streamed, nseg=-(-m // S), cols=-(-k // TCOLS))
            assert np.array_equal(mul(pkg, h, 1, xtd, out), want_t[:k]), (k, "T")
    finally:
        pkg.lib().mik_dense_destroy(less)
        D.close()


# ---- special values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_special_values_and_nan_padding_rows_under_16_byte_loads(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    for adjoint, m, n in ((0, Rc - 1, 2 * C_ + 1), (0, Rc + 1, C_), (1, S - 1, 37), (1, S + 1, 37)):
        A = np.array(rnd(T, m, n, seed=70 + n), order="F")
        k = m if adjoint else n
        x = (np.abs(rnd(T, k, seed=71).real) + 1j * np.abs(rnd(T, k, seed=72).imag)).astype(T)
        if adjoint:
            A[:, 3] = T(complex(-0.0, -0.0))                           # a column of -0.0 parts
            A[7 % m, 20], x[7 % m] = T(complex(np.inf, 0.0)), T(0)     # Inf * 0 = NaN in both components of column 20 only
            nan_at = [20]
        else:
            A[3 % m, :] = T(complex(-0.0, -0.0))                       # a row of -0.0 parts
            A[0, 5], x[5] = T(complex(np.inf, 0.0)), T(0)              # ... of row 0 only
            nan_at = [0]
        want = dref.mul_t(A, x, shape) if adjoint else dref.mul_n(A, x, C_)
        assert np.array_equal(np.flatnonzero(np.isnan(want.real) & np.isnan(want.imag)), nan_at) and np.isnan(want).sum() == 1
        lda = -(-(m + 1) // 64) * 64                                   # an aligned base, NaN rows behind row m
        for byte_off, vec in ((0, 1), (8, 0)):
            D, xd, out = Dev(pkg, ctx, A, lda=lda, byte_off=byte_off), V(pkg, ctx, x), Out(pkg, ctx, n if adjoint else m, T)
            expect(plan(pkg, D.h, adjoint, xd, out.y), vec=vec)
            got = mul(pkg, D.h, adjoint, xd, out)
            assert same_bits(got, want), (adjoint, m, n, byte_off)
            if adjoint:
                assert same_bits(got, device_dots(pkg, D.col, n, xd))
            D.close()


# ---- interleaving ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
def test_one_handle_alternates_between_the_directions_and_leaves_a_real_handle_alone(pkg, ctx, dref, T):
    C_, Rc, shape, S = shapes(pkg, ctx, T)
    rt = ch.real_of(T)
    Ar = np.asfortranarray(np.random.default_rng(1).standard_normal((300, 200)).astype(rt))
    Mr, xr = pkg.HipMatrix.from_numpy(Ar, ctx), pkg.HipVector.from_numpy(np.random.default_rng(2).standard_normal(200).astype(rt), ctx)
    before = (Mr @ xr).to_numpy()
    m, n = S + 1, 2 * C_ + 1
    A, xn, xt = rnd(T, m, n, seed=80), rnd(T, n, seed=81), rnd(T, m, seed=82)
    M, xnd, xtd = matrix(pkg, ctx, A), V(pkg, ctx, xn), V(pkg, ctx, xt)
    outs = {0: Out(pkg, ctx, m, T), 1: Out(pkg, ctx, n, T)}
    expect(plan(pkg, M.dense, 0, xnd, outs[0].y), cols=3)            # chunk partials in the workspace ...
    expect(plan(pkg, M.dense, 1, xtd, outs[1].y), nseg=2)            # ... and the segment sums of both segments
    want = {0: dref.mul_n(A, xn, C_), 1: dref.mul_t(A, xt, shape)}
    for turn, adjoint in enumerate((0, 1, 0, 1)):
        assert np.array_equal(mul(pkg, M.dense, adjoint, xtd if adjoint else xnd, outs[adjoint]), want[adjoint]), turn
    assert np.array_equal((Mr @ xr).to_numpy(), before)


# ---- solvers --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backends(pkg, ctx, ref, dref):
    return cdh.DenseDeviceBackend(pkg, ctx), cdh.DenseHostBackend(pkg, ref, dref)


@pytest.mark.parametrize("T", CT)
def test_cg_complex_full_system(backends, T):
    dev, host = (ch.cg_full(be, T) for be in backends)
    ch.check_cg_full(dev)
    ch.same(dev, host)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_termination_criterion(backends, T, solver):
    dev, host = (ch.termination(be, T, solver) for be in backends)
    ch.check_termination(dev)
    ch.same(dev, host)


@pytest.mark.parametrize("T", CT)
def test_gmres_complex_sets(backends, T):
    dev, host = (ch.gmres_sets(be, T, False) for be in backends)
    ch.check_gmres_sets(dev)
    ch.same(dev, host)


@pytest.mark.parametrize("T", CT)
def test_one_system_beyond_a_chunk_through_cg_and_gmres(pkg, backends, T):
    n = 197
    A, b, reltol = cdh.beyond_a_chunk(T, 1, n)
    res = []
    for be in backends:
        Ad, bd = be.operator(A), be.vector(b)
        x1, h1 = pkg.cg_(be.vector(np.zeros(n, T)), Ad, bd, initially_zero=True, reltol=reltol, maxiter=n, log=True, ops=be.ops)
        x2, h2 = pkg.gmres_(be.vector(np.zeros(n, T)), Ad, bd, initially_zero=True, restart=5, reltol=reltol, maxiter=n, log=True, ops=be.ops)
        res.append(dict(x1=x1.to_numpy(), h1=ch._hist(h1), x2=x2.to_numpy(), h2=ch._hist(h2)))
    dev, host = res
    ch.same(dev, host)
    Ad, bd = A.astype(np.complex128), b.astype(np.complex128)
    assert dev["h1"]["conv"] and np.linalg.norm(Ad @ dev["x1"] - bd) / np.linalg.norm(bd) <= reltol
    assert dev["h2"]["conv"] and np.all(np.diff(dev["h2"]["res"]) <= 0.0)
    # the public entries without `ops` (fused=True is ignored for a complex operator), and the refusals a complex CSR operator has
    M, bv = backends[0].operator(A), backends[0].vector(b)
    x3, h3 = pkg.cg(M, bv, reltol=reltol, maxiter=n, log=True)
    assert np.array_equal(x3.to_numpy(), dev["x1"]) and np.array_equal(np.array(h3["resnorm"]), dev["h1"]["res"])
    x4, h4 = pkg.gmres(M, bv, restart=5, reltol=reltol, maxiter=n, log=True)
    assert np.array_equal(x4.to_numpy(), dev["x2"]) and h4.mvps == dev["h2"]["mvps"]
    with pytest.raises(TypeError, match="JacobiPrec.*complex"):
        pkg.cg(M, bv, Pl=pkg.JacobiPrec(bv))
