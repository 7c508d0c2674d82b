"""Complex bicgstabl, minres and chebyshev on the device.  Every entry of the layer they stand on is compared bit for
bit with the C restatement (tests/complex_ref/complex_solvers_ref.c), every fused entry with the chain of L1 calls it replaces, every
forwarded form with the real entry on the same memory; the solvers run the complex test sets of test/bicgstabl.jl:13-70,
test/minres.jl:32-96 and test/chebyshev.jl:26-94 and must agree bit for bit -- x, every residual, the counts -- with the numpy double of
tests/complex_solvers_host.py running the same Python."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_host as ch
import complex_solvers_host as cs
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)
from complex_solvers_host import sref  # noqa: F401  (fixture)
from conftest import KN

pytestmark = pytest.mark.gpu

CT = [np.complex128, np.complex64]
SIZES = ["1", "S-1", "S", "S+1", "5S+3", "1024S+1"]
SMALL_MACHINE = 8 | (1 << 16)           # compute units | XCDs << 16: sweep_grid_cap = 256
_vp = C.c_void_p


def seg(ctx, T):
    w, l = ctx.reduce_shape(T)
    assert w == 16 // np.dtype(T).itemsize
    return 256 * w * l


def size_of(ctx, T, which):
    S = seg(ctx, T)
    return {"1": 1, "S-1": S - 1, "S": S, "S+1": S + 1, "5S+3": 5 * S + 3, "1024S+1": 1024 * S + 1, "2 passes": 257 * S + 3}[which]


def rnd(rng, T, n):
    rt = ch.real_of(T)
    return (rng.standard_normal(n).astype(rt) + 1j * rng.standard_normal(n).astype(rt)).astype(T)


def real_view(pkg, v):
    """the same device memory as a vector of 2 n reals"""
    return pkg.HipVector.wrap(v.ptr, 2 * v.n, ch.real_of(v.dtype), v.ctx, owner=v)


class Block:
    """k columns of n elements in one device buffer with a chosen leading dimension and byte offset, and the host copy with the same ld:
    what a `HipMatrix` is to the entries (buf, ld, n, cols, col), without its alignment"""

    def __init__(self, pkg, ctx, cols_h, ld=None, offset_bytes=0):
        T = cols_h[0].dtype
        self.n, self.cols, self.dtype, self.ctx = len(cols_h[0]), len(cols_h), np.dtype(T), ctx
        self.ld = (self.n + 63) // 64 * 64 if ld is None else ld
        assert offset_bytes in (0, 8) and self.ld >= self.n
        self.raw = pkg.HipVector(self.ld * self.cols + 2, T, ctx)
        self.buf = pkg.HipVector.wrap(self.raw.ptr + offset_bytes, self.ld * self.cols, T, ctx, owner=self.raw)
        assert self.buf.ptr % 16 == offset_bytes
        self.store = np.zeros(self.ld * self.cols, T)
        for j, c in enumerate(cols_h):
            self.store[j * self.ld: j * self.ld + self.n] = c
        self.buf.copy_from_host(self.store)

    def col(self, j):
        return self.buf.view(j * self.ld, self.n)

    def host_col(self, j):
        return self.store[j * self.ld: j * self.ld + self.n]

    def download(self):
        return self.buf.to_numpy()


def columns(rng, T, n, k):
    """k columns; past the fifth they are the first five scaled by powers of two (cheap at a million rows)"""
    base = [rnd(rng, T, n) / ch.real_of(T).type(np.sqrt(2 * n)) for _ in range(min(k, 5))]
    return [base[j % 5] * ch.real_of(T).type(2.0 ** (j // 5)) for j in range(k)]


# ---------------------------------------------------------------------------------------------
# gemv_t and gram
# ---------------------------------------------------------------------------------------------
def check_gemv_t_and_gram(pkg, ctx, sref, T, n, ld=None, offset=0, ks=(1, 2, 5, 31)):
    shape = ctx.reduce_shape(T)
    rng = np.random.default_rng(n + 7)
    V = Block(pkg, ctx, columns(rng, T, n, max(ks)), ld, offset)
    wh = rnd(rng, T, n)
    w = pkg.HipVector.from_numpy(wh, ctx)
    for k in ks:
        h = pkg.gemv_t_(V, k, w)
        assert h.dtype == np.dtype(T) and np.array_equal(h, sref.gemv_t(V.store, V.ld, k, wh, shape)), k
        if k <= 2:                                                       # h[j] has the bits of the complex mik_dot
            assert all(h[j] == pkg.dot(V.col(j), w) for j in range(k))
    for k in range(1, min(5, max(ks)) + 1):
        M = pkg.gram_(V, k)
        assert np.array_equal(M, sref.gram(V.store, V.ld, n, k, shape)), k
        assert not np.signbit(M.diagonal().imag).any() and np.array_equal(M.real, M.real.T) and np.array_equal(M.imag, -M.imag.T)
        if k == 5:                                                       # every entry equals mik_dot of its pair (as numbers: the sign of a zero aside)
            for r in range(k):
                for c in range(k):
                    assert M[r, c] == pkg.dot(V.col(r), V.col(c)), (r, c)
        # a view that starts at the second column: col0
        if k == 2 and V.cols >= 3:
            assert np.array_equal(pkg.gram_(V, 2, col0=1), sref.gram(V.store[V.ld:], V.ld, n, 2, shape))


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", SIZES)
def test_gemv_t_and_gram(pkg, ctx, sref, T, which):
    check_gemv_t_and_gram(pkg, ctx, sref, T, size_of(ctx, T, which))


# ---------------------------------------------------------------------------------------------
# axpy_dot: four forms, x NULL
# ---------------------------------------------------------------------------------------------
def check_axpy_dot(pkg, ctx, sref, T, n, offset=0):
    shape, rt = ctx.reduce_shape(T), ch.real_of(T).type
    rng = np.random.default_rng(n + 11)
    xh, yh, zh = rnd(rng, T, n), rnd(rng, T, n), rnd(rng, T, n)

    def V(a):
        b = Block(pkg, ctx, [a], None, offset)
        return b.col(0)
    x, z = V(xh), V(zh)
    for alpha in (rt(-0.75), T(0.5 - 1.25j)):
        for with_z in (True, False):
            y, want = V(yh), yh.copy()
            got = pkg.axpy_dot_(alpha, x, y, z if with_z else None, hints=1)
            exp = sref.axpy_dot(alpha, xh, want, zh if with_z else None, shape)
            assert got.dtype == (np.dtype(T) if with_z else ch.real_of(T)) and got == exp, (alpha, with_z)
            assert np.array_equal(y.to_numpy(), want)
            # the chain of L1 calls it replaces
            y2 = V(yh).axpy_(alpha, x)
            assert np.array_equal(y2.to_numpy(), want) and got == (pkg.dot(z, y2) if with_z else pkg.norm(y2))
            if not with_z and not np.iscomplexobj(alpha):                 # forwarded: the real entry over the 2 n interleaved reals
                y3 = V(yh)
                assert pkg.axpy_dot_(alpha, real_view(pkg, x), real_view(pkg, y3), None) == got and np.array_equal(y3.to_numpy(), want)
    y = V(yh)                                                            # x NULL: no update
    assert pkg.axpy_dot_(T(1j), None, y, z) == sref.axpy_dot(T(0), None, yh.copy(), zh, shape) == pkg.dot(z, y)
    assert pkg.axpy_dot_(rt(2), None, y, None) == pkg.norm(y) == sref.axpy_dot(rt(0), None, yh.copy(), None, shape)
    assert np.array_equal(y.to_numpy(), yh)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", SIZES)
def test_axpy_dot_forms(pkg, ctx, sref, T, which):
    check_axpy_dot(pkg, ctx, sref, T, size_of(ctx, T, which))


# ---------------------------------------------------------------------------------------------
# minres_update: both forms, the NULL patterns of iterations 1, 2 and >= 3
# ---------------------------------------------------------------------------------------------
def check_minres_update(pkg, ctx, sref, T, n, offset=0):
    rt = ch.real_of(T).type
    rng = np.random.default_rng(n + 13)
    hs = [rnd(rng, T, n) for _ in range(5)]                              # v_next, v_curr, w_curr, w_prev, x
    V = lambda a: Block(pkg, ctx, [a], None, offset).col(0)
    for sc in ([rt(0.5), rt(-1.25), rt(0.75), rt(2.5), rt(-0.3)], [T(0.5 + 0j), T(-1.25 + 0.5j), T(0.75j), T(2.5 - 1j), T(-0.3 + 0.2j)]):
        for pat in (1, 2, 3):
            vn, vc, wc, wp, xx = (V(a) for a in hs)
            wn = V(np.full(n, np.nan, T))
            wcur, wprev = (wc if pat >= 2 else None), (wp if pat >= 3 else None)
            pkg.minres_update_(xx, vn, vc, wcur, wprev, wn, *sc, hints=3)
            h = [a.copy() for a in hs]
            hwn = np.full(n, np.nan, T)
            sref.minres_update(h[4], h[0], h[1], h[2] if pat >= 2 else None, h[3] if pat >= 3 else None, hwn, sc)
            got = [vn.to_numpy(), wn.to_numpy(), xx.to_numpy()]
            assert np.array_equal(got[0], h[0]) and np.array_equal(got[1], hwn) and np.array_equal(got[2], h[4]), (pat, sc[1])
            assert np.array_equal(vc.to_numpy(), hs[1]) and np.array_equal(wc.to_numpy(), hs[2]) and np.array_equal(wp.to_numpy(), hs[3])
            # the chain of L1 calls it replaces (src/minres.jl:115, :138-144)
            vn2, vc2, wc2, wp2, xx2 = (V(a) for a in hs)
            wn2 = V(np.zeros(n, T))
            vn2.scal_(sc[0])
            wn2.copyto_(vc2)
            if pat >= 2:
                wn2.axpy_(sc[1], wc2)
            if pat >= 3:
                wn2.axpy_(sc[2], wp2)
            wn2.scal_(sc[3])
            xx2.axpy_(sc[4], wn2)
            assert np.array_equal(vn2.to_numpy(), got[0]) and np.array_equal(wn2.to_numpy(), got[1]) and np.array_equal(xx2.to_numpy(), got[2])
            if not np.iscomplexobj(sc[0]):                               # forwarded: the real entry over the 2 n interleaved reals
                vn3, vc3, wc3, wp3, xx3 = (V(a) for a in hs)
                wn3 = V(np.zeros(n, T))
                rv = lambda v: None if v is None else real_view(pkg, v)
                pkg.minres_update_(rv(xx3), rv(vn3), rv(vc3), rv(wc3 if pat >= 2 else None), rv(wp3 if pat >= 3 else None), rv(wn3), *sc)
                assert np.array_equal(vn3.to_numpy(), got[0]) and np.array_equal(wn3.to_numpy(), got[1]) and np.array_equal(xx3.to_numpy(), got[2])


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", SIZES)
def test_minres_update_forms(pkg, ctx, sref, T, which):
    check_minres_update(pkg, ctx, sref, T, size_of(ctx, T, which))


# ---------------------------------------------------------------------------------------------
# the BiCGStab minimal-residual update: l = 1, 2, 4 and 8 (the largest the entry accepts)
# ---------------------------------------------------------------------------------------------
def check_mr_update(pkg, ctx, sref, T, n, ld=None, offset=0, ls=(1, 2, 4, 8), scale=None):
    shape = ctx.reduce_shape(T)
    rng = np.random.default_rng(n + 17)
    lmax = max(ls)
    ucols, rcols, xh = columns(rng, T, n, lmax + 1), columns(rng, T, n, lmax + 1)[::-1], rnd(rng, T, n)
    if scale is not None:
        rcols = [(c * scale).astype(T) for c in rcols]
    for l in ls:
        gamma = rnd(rng, T, l)
        us, rs = Block(pkg, ctx, ucols[:l + 1], ld, offset), Block(pkg, ctx, rcols[:l + 1], ld, offset)
        x = Block(pkg, ctx, [xh], None, offset).col(0)
        got = pkg.bicgstab_mr_update_(us, rs, x, l, gamma)
        hu, hr, hx = us.store.copy(), rs.store.copy(), xh.copy()
        want = sref.mr_update(hu, us.ld, hr, rs.ld, hx, l, gamma, shape)
        assert got.dtype == ch.real_of(T) and got == want and (scale is None or got > 0), l
        assert np.array_equal(us.download(), hu) and np.array_equal(rs.download(), hr) and np.array_equal(x.to_numpy(), hx), l
        # the chain it replaces: three mul!(y, V, c, alpha, 1) and a norm (src/bicgstabl.jl:127-129, :132)
        us2, rs2 = Block(pkg, ctx, ucols[:l + 1], ld, offset), Block(pkg, ctx, rcols[:l + 1], ld, offset)
        x2 = Block(pkg, ctx, [xh], None, offset).col(0)
        pkg.gemv_n_(us2.col(0), us2, l, gamma, -1.0, col0=1)
        pkg.gemv_n_(x2, rs2, l, gamma, 1.0, col0=0)
        pkg.gemv_n_(rs2.col(0), rs2, l, gamma, -1.0, col0=1)
        assert np.array_equal(us2.download(), hu) and np.array_equal(rs2.download(), hr) and np.array_equal(x2.to_numpy(), hx), l
        assert pkg.norm(rs2.col(0)) == got


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", SIZES)
def test_bicgstab_mr_update(pkg, ctx, sref, T, which):
    n = size_of(ctx, T, which)
    check_mr_update(pkg, ctx, sref, T, n, ls=(1, 2, 4, 8) if n < 10 ** 5 else (2, 8))


def test_mr_update_bounds(pkg, ctx):
    """l = 9 is refused (MIK_ERR_INVALID): 8 is the largest l the entry accepts, for complex as for real"""
    T = np.complex128
    us = pkg.HipMatrix(8, 10, T, ctx)
    with pytest.raises(pkg.MikError) as e:
        pkg.bicgstab_mr_update_(us, us, us.col(0), 9, np.ones(9, T))
    assert e.value.code == 1


# ---------------------------------------------------------------------------------------------
# the two Chebyshev sweeps: forwarded with the flag, refused without it
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", ["S+1", "5S+3"])
def test_chebyshev_sweeps_and_refusals(pkg, ctx, sref, T, which):
    n, shape, rt = size_of(ctx, T, which), ctx.reduce_shape(T), ch.real_of(T).type
    rng = np.random.default_rng(n + 19)
    uh, xh, chh, rh = (rnd(rng, T, n) for _ in range(4))
    V = lambda a: pkg.HipVector.from_numpy(a, ctx)
    u, x, c, r = V(uh), V(xh), V(chh), V(rh)
    got = pkg.axpy2_nrm2_(rt(0.37), u, x, c, r, hints=7)
    hx, hr = xh.copy(), rh.copy()
    assert got.dtype == ch.real_of(T) and got == sref.axpy2_nrm2(0.37, uh, hx, chh, hr, shape)
    assert np.array_equal(x.to_numpy(), hx) and np.array_equal(r.to_numpy(), hr)
    x2, r2 = V(xh), V(rh)                                                # the real entry on the same memory
    assert pkg.axpy2_nrm2_(rt(0.37), real_view(pkg, u), real_view(pkg, x2), real_view(pkg, c), real_view(pkg, r2)) == got
    assert np.array_equal(x2.to_numpy(), hx) and np.array_equal(r2.to_numpy(), hr)
    x3, r3 = V(xh), V(rh)                                                # the chain: src/chebyshev.jl:51, :52, :54
    x3.axpy_(rt(0.37), u); r3.axpy_(rt(-0.37), c)
    assert np.array_equal(x3.to_numpy(), hx) and np.array_equal(r3.to_numpy(), hr) and pkg.norm(r3) == got
    for first in (True, False):
        d, d2, want = V(uh), V(uh), uh.copy()
        pkg.cheb_direction_(d, r, rt(0.21), first)
        sref.cheb_direction(want, hr, 0.21, first)
        pkg.cheb_direction_(real_view(pkg, d2), real_view(pkg, r), rt(0.21), first)
        assert np.array_equal(d.to_numpy(), want) and np.array_equal(d2.to_numpy(), want)
        d3 = V(uh).copyto_(r)                                            # the chain: u .= c; u .+= beta .* c
        if not first:
            d3.axpy_(rt(0.21), r)
        assert np.array_equal(d3.to_numpy(), want)
    # refusals: a complex code without the flag (INVALID), a diagonal preconditioner (NOTIMPL)
    code, one = pkg._lib.dtype_code(T), np.ones(2, ch.real_of(T))
    p = lambda v: _vp(v.ptr)
    out = np.zeros(2, ch.real_of(T))
    L = pkg.lib()
    assert L.mik_axpy2_nrm2(ctx.handle, code, n, one.ctypes.data_as(_vp), p(u), p(x), p(c), p(r), out.ctypes.data_as(_vp), 0) == 1
    assert L.mik_cheb_direction(ctx.handle, code, n, p(r), None, one.ctypes.data_as(_vp), 0, p(u)) == 1
    assert L.mik_cheb_direction(ctx.handle, code | pkg._lib.MIK_SCALAR_REAL, n, p(r), p(c), one.ctypes.data_as(_vp), 0, p(u)) == 5
    assert np.array_equal(x.to_numpy(), hx) and np.array_equal(u.to_numpy(), uh)


# ---------------------------------------------------------------------------------------------
# the element-wise variants, each alignment term alone; a norm outside the safe range; two passes of the grid-stride loops; specials
# ---------------------------------------------------------------------------------------------
def check_mgs_and_gemv_n(pkg, ctx, ref, T, n, ld=None, offset=0, ks=(0, 1, 3)):
    """Modified Gram-Schmidt and y += alpha V c on a basis with a chosen leading dimension and byte offset.  k = 0 is the norm-only pass,
    k = 3 runs a first, a middle and a last pass."""
    shape = ctx.reduce_shape(T)
    rng = np.random.default_rng(n + 31)
    V = Block(pkg, ctx, columns(rng, T, n, max(ks)), ld, offset)
    wh, c, alpha = rnd(rng, T, n), rnd(rng, T, max(ks)), T(0.5 - 0.75j)
    vec = lambda: Block(pkg, ctx, [wh], None, offset).col(0)
    for k in ks:
        w, h, want = vec(), np.zeros(max(k, 1), T), wh.copy()
        nrm = pkg.orthogonalize_and_normalize_(V, k, w, h)
        hh, hn = ref.mgs(V.store, V.ld, k, want, shape)
        assert nrm.dtype == ch.real_of(T) and nrm == hn and np.array_equal(h[:k], hh) and np.array_equal(w.to_numpy(), want), k
        if k == 0:                                                       # the sum of squares alone: the bits of norm(w)
            assert nrm == pkg.norm(vec())
        y, want = vec(), wh.copy()
        pkg.gemv_n_(y, V, k, c, alpha)
        ref.gemv_n(V.store, V.ld, k, c, alpha, want)
        assert np.array_equal(y.to_numpy(), want), k


# (an odd leading dimension breaks 16-byte alignment at ComplexF32 only: a ComplexF64 element is 16 bytes)
@pytest.mark.parametrize("T,term", [(np.complex128, "base+8"), (np.complex128, "ld>n"), (np.complex64, "base+8"), (np.complex64, "ld>n"),
                                    (np.complex64, "odd ld")])
def test_elementwise_variants(pkg, ctx, ref, sref, T, term):
    n = size_of(ctx, T, "S+1")
    if term == "base+8":
        check_gemv_t_and_gram(pkg, ctx, sref, T, n, offset=8, ks=(1, 5))
        check_mr_update(pkg, ctx, sref, T, n, offset=8, ls=(2,))
        check_axpy_dot(pkg, ctx, sref, T, n, offset=8)
        check_minres_update(pkg, ctx, sref, T, n, offset=8)
        check_mgs_and_gemv_n(pkg, ctx, ref, T, n, offset=8)
    else:
        ld = n + 64 + (n % 2) + (term == "odd ld")                        # even and past n; one more: odd
        assert ld > n and (ld % 2 == 1) == (term == "odd ld")
        check_gemv_t_and_gram(pkg, ctx, sref, T, n, ld=ld, ks=(1, 5))
        check_mr_update(pkg, ctx, sref, T, n, ld=ld, ls=(2,))
        check_mgs_and_gemv_n(pkg, ctx, ref, T, n, ld=ld)


@pytest.mark.parametrize("T", CT)
def test_norm_outside_the_safe_range(pkg, ctx, sref, T):
    """a vector scaled by 1e-200 (1e-30 at ComplexF32): every square underflows, the scaled second pass runs"""
    n, shape, rt = size_of(ctx, T, "S+1"), ctx.reduce_shape(T), ch.real_of(T).type
    tiny = rt(1e-200 if T == np.complex128 else 1e-30)
    rng = np.random.default_rng(23)
    xh, yh = (rnd(rng, T, n) * tiny).astype(T), (rnd(rng, T, n) * tiny).astype(T)
    x, y = pkg.HipVector.from_numpy(xh, ctx), pkg.HipVector.from_numpy(yh, ctx)
    want = yh.copy()
    got = pkg.axpy_dot_(T(0.5 - 1j), x, y, None)
    assert got == sref.axpy_dot(T(0.5 - 1j), xh, want, None, shape) and got > 0 and np.array_equal(y.to_numpy(), want) and got == pkg.norm(y)
    check_mr_update(pkg, ctx, sref, T, n, ls=(2,), scale=tiny)


@pytest.mark.parametrize("T", CT)
def test_second_pass_of_the_grid_stride_loops(pkg, ctx, sref, T):
    n = size_of(ctx, T, "2 passes")
    ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
    try:
        assert ctx.info()["sweep_grid_cap"] == 256 < (n + seg(ctx, T) - 1) // seg(ctx, T) <= 512      # two passes, the second ragged
        check_gemv_t_and_gram(pkg, ctx, sref, T, n, ks=(2, 5))
        check_axpy_dot(pkg, ctx, sref, T, n)
        check_minres_update(pkg, ctx, sref, T, n)
        check_mr_update(pkg, ctx, sref, T, n, ls=(2,))
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


@pytest.mark.parametrize("T", CT)
def test_signed_zeros_and_nan_from_inf_times_zero(pkg, ctx, sref, T):
    n, shape = 37, ctx.reduce_shape(T)
    rng = np.random.default_rng(29)
    xh, yh, zh = rnd(rng, T, n), rnd(rng, T, n), rnd(rng, T, n)
    xh[3], yh[3] = T(complex(-0.0, 0.0)), T(complex(-0.0, -0.0))
    xh[5], yh[5] = T(complex(np.inf, 0.0)), T(complex(1.0, -0.0))       # (a + b i) (inf + 0 i): b * inf and a * 0 ... NaN in both components
    xh[9] = T(complex(0.0, -0.0))
    alpha = T(complex(0.0, 0.0))
    x, y, z = (pkg.HipVector.from_numpy(a, ctx) for a in (xh, yh, zh))
    want = yh.copy()
    got = pkg.axpy_dot_(alpha, x, y, z)
    exp = sref.axpy_dot(alpha, xh, want, zh, shape)
    out = y.to_numpy()
    assert np.isnan(out[5].real) and np.isnan(out[5].imag) and np.isnan(got.real) and np.isnan(got.imag)
    assert np.array_equal(out.view(ch.real_of(T)), want.view(ch.real_of(T)), equal_nan=True)
    ok = ~np.isnan(want.view(ch.real_of(T)))                             # (the sign of a NaN is not part of the contract)
    assert np.array_equal(np.signbit(out.view(ch.real_of(T)))[ok], np.signbit(want.view(ch.real_of(T)))[ok])
    assert np.isnan(exp.real) and np.isnan(exp.imag)
    # the same through the complex minres_update and the MR update
    hs = [xh, yh, zh, rnd(rng, T, n), rnd(rng, T, n)]
    V = lambda a: pkg.HipVector.from_numpy(a, ctx)
    vn, vc, wc, wp, xx = (V(a) for a in hs)
    wn = V(np.zeros(n, T))
    sc = [T(complex(-0.0, 0.0)), T(1j), T(complex(0.0, -0.0)), T(1 - 1j), T(-1.0)]
    pkg.minres_update_(xx, vn, vc, wc, wp, wn, *sc)
    h = [a.copy() for a in hs]
    hwn = np.zeros(n, T)
    sref.minres_update(h[4], h[0], h[1], h[2], h[3], hwn, sc)
    rv = lambda a: a.view(ch.real_of(T))
    for dev, host in ((vn, h[0]), (wn, hwn), (xx, h[4])):
        d = dev.to_numpy()
        ok = ~np.isnan(rv(host))
        assert np.array_equal(rv(d), rv(host), equal_nan=True) and np.array_equal(np.signbit(rv(d))[ok], np.signbit(rv(host))[ok])


# ---------------------------------------------------------------------------------------------
# solvers: the reference's complex test sets, device against the numpy double, CSR and dense, fused and unfused
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backends(pkg, ctx, ref, dref, sref):
    return cs.DeviceBackend(pkg, ctx), cs.DeviceBackend(pkg, ctx, dense=True), cs.HostBackend(pkg, ref, dref, sref)


def run_sets(backends, scenario, *args):
    dev, dense, host = backends
    fused = scenario(dev, *args, True)
    cs.same(fused, scenario(host, *args, True))                          # x, every residual, counts, isconverged: the numpy double's
    cs.same(fused, scenario(dev, *args, False))                          # fused = unfused
    cs.same(fused, scenario(dense, *args, True))                         # n <= 64: the dense operator sums a row in the CSR order
    return fused


@pytest.mark.parametrize("T", CT)
def test_bicgstabl_complex_sets(backends, T):
    cs.check_bicgstabl_sets(run_sets(backends, cs.bicgstabl_sets, T))


@pytest.mark.parametrize("T", CT)
def test_minres_complex_sets(backends, T):
    cs.check_minres_sets(run_sets(backends, cs.minres_sets, T), T)


@pytest.mark.parametrize("T", CT)
def test_chebyshev_complex_sets(backends, T):
    cs.check_cheb_sets(run_sets(backends, cs.cheb_sets, T), T)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["bicgstabl", "minres", "chebyshev"])
def test_termination_criterion(backends, T, solver):
    cs.check_termination(run_sets(backends, cs.termination, T, solver), solver)


def hermitian_laplacian(pkg, T, n):
    """the leading n x n block of the 3-D Laplacian fixture, its diagonal shifted by 1, plus i K with K real and skew-symmetric on the same
    pattern: Hermitian, strictly diagonally dominant, so positive definite (DESIGN.md section 17's)"""
    N = int(np.ceil(n ** (1 / 3)))
    while N ** 3 < n:
        N += 1
    m, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3)
    L = sp.csc_matrix((nzval, rowval - 1, colptr - 1), shape=(m, m)).tocsr()[:n, :n].tocoo()
    val = L.data.astype(np.complex128)
    val[L.row == L.col] += 1.0
    val[L.row < L.col] += 0.1j
    val[L.row > L.col] -= 0.1j
    return sp.csr_matrix((val.astype(T), (L.row, L.col)), shape=(n, n))


@pytest.mark.parametrize("T", CT)
def test_hermitian_laplacian_three_solvers(pkg, ctx, backends, T):
    n = size_of(ctx, T, "S+1")
    M = hermitian_laplacian(pkg, T, n)
    assert abs(M - M.conj().T).max() == 0
    b = rnd(np.random.default_rng(2), T, n)
    offdiag = abs(M - sp.diags(M.diagonal())).sum(axis=1).max()          # Gershgorin on the host: the diagonal is 7
    lmin, lmax = 7.0 - offdiag, 7.0 + offdiag
    assert lmin > 0
    res = []
    for be in (backends[0], backends[2]):
        A, bv = be.operator(M), be.vector(b)
        zeros = lambda: be.vector(np.zeros(n, T))
        x1, h1 = pkg.minres_(zeros(), A, bv, initially_zero=True, maxiter=80, log=True, ops=be.ops)
        x2, h2 = pkg.chebyshev_(zeros(), A, bv, lmin, lmax, initially_zero=True, maxiter=30, log=True, ops=be.ops)
        x3, h3 = pkg.bicgstabl_(zeros(), A, bv, 2, initial_zero=True, max_mv_products=200, log=True, ops=be.ops)
        res.append(dict(x1=x1.to_numpy(), h1=cs._hist(h1), x2=x2.to_numpy(), h2=cs._hist(h2), x3=x3.to_numpy(), h3=cs._hist(h3)))
    dev, host = res
    cs.same(dev, host)
    Md, bd = M.astype(np.complex128), b.astype(np.complex128)
    reltol, eps = np.sqrt(np.finfo(ch.real_of(T)).eps), np.finfo(ch.real_of(T)).eps
    # The recurrence of src/chebyshev.jl:43-45 as written in v0.9.4 (u = c + beta c) does not contract on an interval as wide as Gershgorin's
    # here (lmax / lmin = 13.4; the complex128 numpy restatement grows by 1.3 a step): 30 steps are compared bit for bit, not held to a tolerance.
    assert dev["h2"]["iters"] == 30 and np.isfinite(dev["h2"]["res"]).all() and not dev["h2"]["conv"]
    for k in ("1", "3"):
        # the stopping test is on the recurrence residual; the true one differs by the rounding of the steps taken: at most
        # eps ||A|| ||x|| per step and product (||A||_inf < 14, two products per bicgstabl step and l = 2 of them per iteration)
        steps = dev["h" + k]["mvps"]
        gap = steps * eps * 14 * np.linalg.norm(dev["x" + k]) / np.linalg.norm(bd)
        assert dev["h" + k]["conv"] and np.linalg.norm(Md @ dev["x" + k] - bd) / np.linalg.norm(bd) <= reltol + gap, k
    # the public entries without `ops` (zerox, the default r_shadow), a LinearOperator callback, and the adjoint of a dense matrix
    A, bv = backends[0].operator(M), backends[0].vector(b)
    x, h = pkg.minres(A, bv, maxiter=80, log=True)
    assert np.array_equal(x.to_numpy(), dev["x1"]) and np.array_equal(np.array(h["resnorm"]), dev["h1"]["res"])
    op = pkg.LinearOperator(n, T, lambda y, v: pkg.mul_(y, A, v), ctx)
    x, h = pkg.chebyshev(op, bv, lmin, lmax, maxiter=30, log=True)
    assert np.array_equal(x.to_numpy(), dev["x2"]) and np.array_equal(np.array(h["resnorm"]), dev["h2"]["res"])
    x, h = pkg.bicgstabl(A, bv, 2, max_mv_products=200, log=True)        # the default r_shadow: re and im from the hashed vector
    assert h.isconverged and np.linalg.norm(Md @ x.to_numpy() - bd) / np.linalg.norm(bd) <= 10 * reltol
    it = pkg.bicgstabl_iterator_(bv.zero(), A, bv, 2, initial_zero=True)
    sh = it.r_shadow.to_numpy()
    assert np.array_equal(sh.real, (pkg.fixtures.hashed_rhs(n) + 0.5).astype(ch.real_of(T)))
    assert np.array_equal(sh.imag, (pkg.fixtures.hashed_rhs(2 * n, start=n) + 0.5).astype(ch.real_of(T)))
    small = 48                                                           # the adjoint of a dense operator: A' = A for a Hermitian matrix, as numbers
    Ms = hermitian_laplacian(pkg, T, small).toarray()
    D = pkg.HipMatrix.from_numpy(Ms, ctx)
    bs = pkg.HipVector.from_numpy(b[:small].copy(), ctx)
    xa, ha = pkg.minres(D.adj, bs, log=True)
    assert ha.isconverged and np.linalg.norm(Ms.astype(np.complex128) @ xa.to_numpy() - b[:small]) / np.linalg.norm(b[:small]) <= 10 * reltol


def test_refusals(pkg, ctx):
    """the two whole-iteration handles on a complex CSR (NOTIMPL), JacobiPrec, and the iterables never create the handles"""
    T = np.complex128
    n = 600
    M = hermitian_laplacian(pkg, T, n)
    A = ch.DeviceBackend(pkg, ctx).operator(M)
    b = pkg.HipVector.from_numpy(rnd(np.random.default_rng(4), T, n), ctx)
    x = b.zero()
    v = [x.similar() for _ in range(6)]
    h = _vp()
    L = pkg.lib()
    p = lambda q: _vp(q.ptr)
    assert L.mik_minres_create(ctx.handle, A.handle, p(x), p(v[0]), p(v[1]), p(v[2]), p(v[3]), p(v[4]), p(v[5]), 1.0, 0, C.byref(h)) == 5
    rs = pkg.HipMatrix(n, 3, T, ctx)
    assert L.mik_bicgstab_create(ctx.handle, A.handle, 2, p(x), p(rs.col(0)), rs.ld, p(rs.col(0)), rs.ld, p(b), None, C.byref(h)) == 5
    for it in (pkg.minres_iterable_(b.zero(), A, b), pkg.bicgstabl_iterator_(b.zero(), A, b, 2)):
        assert it._step is None
    for call in (lambda: pkg.bicgstabl(A, b, Pl=pkg.JacobiPrec(b)), lambda: pkg.chebyshev(A, b, 1.0, 13.0, Pl=pkg.JacobiPrec(b))):
        with pytest.raises(TypeError, match="JacobiPrec.*complex"):
            call()


def test_real_path_is_untouched_by_complex_solves(pkg, ctx):
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(12, 3)
    A = pkg.HipCSR(n, n, colptr, rowval, nzval, index_base=1, ctx=ctx)
    b = pkg.HipVector.from_numpy(pkg.fixtures.hashed_rhs(n), ctx)

    def real_run():
        x1, h1 = pkg.minres(A, b, maxiter=10, log=True)
        x2, h2 = pkg.bicgstabl(A, b, 2, max_mv_products=20, log=True)
        return np.array(h1["resnorm"]), x1.to_numpy(), np.array(h2["resnorm"]), x2.to_numpy()
    before = real_run()
    T = np.complex128
    M = hermitian_laplacian(pkg, T, 600)
    Ac = ch.DeviceBackend(pkg, ctx).operator(M)
    bc = pkg.HipVector.from_numpy(rnd(np.random.default_rng(4), T, 600), ctx)
    _x, hm = pkg.minres(Ac, bc, log=True)
    _x, hb = pkg.bicgstabl(Ac, bc, 2, log=True)
    _x, hc = pkg.chebyshev(Ac, bc, 0.9, 13.1, maxiter=20, log=True)
    assert hm.isconverged and hb.isconverged and hc.iters == 20
    after = real_run()
    assert len(before[0]) == 10 and all(np.array_equal(p, q) for p, q in zip(before, after))
