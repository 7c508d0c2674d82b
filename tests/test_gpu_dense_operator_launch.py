"""The dense operator past one grid pass, one combine batch and the cache: the loops, batches and variants of csrc/mik_dense_mul.h that
the shapes of tests/test_gpu_dense_operator.py do not reach.

    k_dense_n_combine      the 8-deep and the 32-deep batch of partials and the tail, in every combination
    k_dense_n              the chunk loop c += gridDim.y takes 2, 3 and 4 passes, the last ragged, in the 16-byte and in the scalar variant
    k_dense_t              the column-batch loop and the segment loop take a second (third) pass, ragged
    streamed variants      k_dense_n<T, true, true, C> and k_dense_t<T, true, true>, on both sides of their threshold with one matrix
    alignment              each term of the 16-byte variant's condition on its own; NaN padding rows under 16-byte loads
    one handle             N, T, N, T through the workspace both directions share
    special values         -0.0 and Inf * 0 in the T form

Every case first asserts on the launch plan (mik_dev_dense_plan, include/mik_dev.h -- computed by the helper the launch itself uses) that
it reaches the path it is meant for; the grid-stride cases plan for a machine of 8 compute units (MIK_KNOB_MACHINE: 4 * CUs = 32
workgroups, mik_max_grid = 256) and are repeated on the machine as queried: results never depend on the plan.  Shapes come from
mik_dense_mul_shape and mik_reduce_shape; the tables of expected grids live in tests/dense_operator_host.py, where
tests/test_dense_operator_launch_host.py holds them to the restated launch arithmetic without a GPU.

References.  N form: the C restatement of the chunked order (tests/dense_ref/dense_mul_ref.c), bit for bit, and
|y - A x| <= (C + nc) eps (|A| |x|) against a product in float64 (Float32 data) / np.longdouble (Float64 data): a term passes through at
most 1 + (C - 1) + (nc - 1) roundings of eps / 2, so the factor leaves a margin of 2.  T form: the oracle's tree dot of every column and
mik_dot on the device (machine as queried), bit for bit, and ladder.dot_bound for the segment count of the case.  Every y is a view
into a longer buffer filled with 7 whose elements on both sides must stay 7."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import dense_operator_host as dh
from conftest import KN
from dense_operator_host import Out, Raw, V, ref, shape  # noqa: F401  (ref, shape: fixtures)

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
DTYPES = [np.float64, np.float32]


@contextlib.contextmanager
def machine(ctx, value):
    ctx.set_tuning(KN.MACHINE, value)
    try:
        yield
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


def mul(pkg, handle, adjoint, x, out):
    """mik_dense_mul into the view of `out`; the result, with the guard elements checked"""
    assert pkg.lib().mik_dense_mul(handle, int(adjoint), _vp(x.ptr), _vp(out.y.ptr)) == 0
    return out.read()


def expect(p, **want):
    assert {k: p[k] for k in want} == want, (p, want)


def segment(ctx, dtype):
    W, L = ctx.reduce_shape(dtype)
    return W, L, 256 * W * L


def device_dots(pkg, col, n, xd):
    """mik_dot of every column with x, on the machine as queried"""
    return np.array([pkg.dot(col(j), xd) for j in range(n)], xd.dtype)


VARIANTS = ("HipMatrix", "Raw")


def variants(pkg, ctx, A, lda, which=VARIANTS):
    """(name, vec, handle, column view, keep-alive) of a HipMatrix (16-byte variant) and of the same matrix with leading dimension lda, one
    element into its allocation (scalar variant)"""
    if "HipMatrix" in which:
        M = dh.matrix(pkg, ctx, A)
        yield "HipMatrix", 1, M.dense, M.col, M
        del M
    if "Raw" in which:
        raw = Raw(pkg, ctx, A, lda, off=1)
        assert raw.rc == 0
        yield "Raw", 0, raw.h, raw.col, raw
        raw.close()


# ---- a: the batches of k_dense_n_combine ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_takes_its_batch_of_8_its_batch_of_32_and_the_tail(pkg, ctx, ref, shape, dtype):
    C_, R = shape
    m = 65
    assert [dh.combine_trips(nc) for nc in dh.COMBINE_NC] == list(dh.COMBINE_TRIPS)
    for nc in dh.COMBINE_NC:
        n = nc * C_ - 5                                               # the last chunk is ragged
        A, x = dh.normal(m, n, dtype, seed=nc), dh.vec(n, dtype, seed=nc)
        want = ref.chunked(A, x, C_)
        M, xd, out = dh.matrix(pkg, ctx, A), V(pkg, ctx, x), Out(pkg, ctx, m, dtype)
        p = dh.plan(pkg, M.dense, 0, xd, out.y)
        expect(p, vec=1, streamed=0, gx=1, gy=nc, cols=nc)           # one pass over the chunks: the combine kernel is what differs
        got = mul(pkg, M.dense, 0, xd, out)
        assert np.array_equal(got, want), nc
        assert dh.within_n_bound(got, A, x, C_), nc


# ---- b: the chunk loop of k_dense_n --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(3))
def test_n_form_chunk_loop_takes_several_passes_in_both_variants(pkg, ctx, ref, shape, case, dtype):
    C_, R = shape
    m, n, gx, gy, nc, passes = dh.CHUNK_STRIDE(C_, R)[case]
    A, x = dh.normal(m, n, dtype, seed=10 + case), dh.vec(n, dtype, seed=10 + case)
    want = ref.chunked(A, x, C_)
    xd = V(pkg, ctx, x)
    for name, vec, h, _, keep in variants(pkg, ctx, A, m + 1):
        out = Out(pkg, ctx, m, dtype)
        with machine(ctx, dh.SMALL_MACHINE):
            p = dh.plan(pkg, h, 0, xd, out.y)
            expect(p, vec=vec, streamed=0, gx=gx, gy=gy, cols=nc, nseg=0)
            assert -(-p["cols"] // p["gy"]) == passes >= 2 and (p["cols"] % p["gy"] != 0 or p["gy"] == 1)      # several passes, the last ragged
            small = mul(pkg, h, 0, xd, out)
        p = dh.plan(pkg, h, 0, xd, out.y)
        expect(p, vec=vec, streamed=0, gx=gx, cols=nc)
        as_queried = mul(pkg, h, 0, xd, out)
        assert np.array_equal(small, want), (name, m, n)
        assert np.array_equal(as_queried, want), (name, m, n)
    assert dh.within_n_bound(small, A, x, C_)


# ---- c, d: the two loops of k_dense_t ------------------------------------------------------------------------------------------------
def _t_strided(pkg, orc, ctx, dtype, m, n, which, seed, **plan_small):
    W, L, S = segment(ctx, dtype)
    A, x = dh.normal(m, n, dtype, seed=seed), dh.vec(m, dtype, seed=seed)
    want = dh.tree_cols(orc, A, x, W, L)
    xd = V(pkg, ctx, x)
    assert m % 2 == 1
    for name, vec, h, col, keep in variants(pkg, ctx, A, m + 2, which):      # an odd leading dimension
        out = Out(pkg, ctx, n, dtype)
        with machine(ctx, dh.SMALL_MACHINE):
            p = dh.plan(pkg, h, 1, xd, out.y)
            expect(p, vec=vec, streamed=0, **plan_small)
            assert p["cols"] == -(-n // dh.TCOLS) and p["nseg"] == -(-m // S)
            small = mul(pkg, h, 1, xd, out)
        p = dh.plan(pkg, h, 1, xd, out.y)
        expect(p, vec=vec, streamed=0, cols=plan_small["cols"], nseg=plan_small["nseg"])
        as_queried = mul(pkg, h, 1, xd, out)
        assert np.array_equal(small, want), (name, m, n)
        assert np.array_equal(as_queried, want), (name, m, n)
        assert np.array_equal(small, device_dots(pkg, col, n, xd)), (name, m, n)
    assert dh.within_t_bound(small, A, x, W, L)


@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_column_batch_loop_takes_a_second_pass(pkg, orc, ctx, dtype):
    W, L, S = segment(ctx, dtype)
    (m0, n0, gx0, gy0, b0, p0), (m1, n1, gx1, gy1, b1, p1) = dh.BATCH_STRIDE(S)
    assert p0 == -(-b0 // gy0) == 2 and b0 % gy0 != 0 and n0 % dh.TCOLS == 5          # the last batch runs k = 4, then k = 1
    _t_strided(pkg, orc, ctx, dtype, m0, n0, ("HipMatrix",), 20, gx=gx0, gy=gy0, cols=b0, nseg=1)
    assert p1 == -(-b1 // gy1) == 3 and b1 % gy1 != 0
    _t_strided(pkg, orc, ctx, dtype, m1, n1, VARIANTS, 21, gx=gx1, gy=gy1, cols=b1, nseg=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_segment_loop_takes_a_second_pass(pkg, orc, ctx, dtype):
    W, L, S = segment(ctx, dtype)
    (m, n, gx, gy, batches, nseg, passes), = dh.SEGMENT_STRIDE(S)
    assert passes == -(-nseg // gx) == 2 and nseg % gx != 0 and batches == 2 and gy == 1    # ragged; one workgroup walks both column batches
    _t_strided(pkg, orc, ctx, dtype, m, n, ("HipMatrix",), 22, gx=gx, gy=gy, cols=batches, nseg=nseg)


# ---- e: the streamed variants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_variants_on_both_sides_of_their_threshold(pkg, orc, ctx, ref, shape, dtype):
    """one matrix of just over 192e6 bytes, uploaded once (lda = m rounded up to 64, NaN padding rows): its handle takes the streamed
    kernels in both directions, a second handle over the same buffer with one column fewer the cached ones"""
    C_, R = shape
    W, L, S = segment(ctx, dtype)
    m, n = dh.streamed_shape(R, np.dtype(dtype).itemsize)
    A, xn, xt = dh.normal(m, n, dtype, seed=30), dh.vec(n, dtype, seed=30), dh.vec(m, dtype, seed=31)
    big = Raw(pkg, ctx, A, -(-m // 64) * 64, off=0)
    assert big.rc == 0
    less = big.narrower(n - 1)
    assert less.rc == 0
    xnd, xtd = V(pkg, ctx, xn), V(pkg, ctx, xt)
    want_t = dh.tree_cols(orc, A, xt, W, L)
    dots = device_dots(pkg, big.col, n, xtd)
    assert np.array_equal(dots, want_t)
    for op, k, streamed in ((big, n, 1), (less, n - 1, 0)):
        out = Out(pkg, ctx, m, dtype)
        xk = xnd.view(0, k)
        expect(dh.plan(pkg, op.h, 0, xk, out.y), vec=1, streamed=streamed, gx=-(-m // R), cols=-(-k // C_))
        got = mul(pkg, op.h, 0, xk, out)
        assert np.array_equal(got, ref.chunked(A[:, :k], xn[:k], C_)), (k, "N")
        assert dh.within_n_bound(got, A[:, :k], xn[:k], C_), (k, "N")
        out = Out(pkg, ctx, k, dtype)
        expect(dh.plan(pkg, op.h, 1, xtd, out.y), vec=1, streamed=streamed, nseg=-(-m // S), cols=-(-k // dh.TCOLS))
        got = mul(pkg, op.h, 1, xtd, out)
        assert np.array_equal(got, want_t[:k]) and np.array_equal(got, dots[:k]), (k, "T")
        assert dh.within_t_bound(got, A[:, :k], xt, W, L), (k, "T")
    less.close()
    big.close()


# ---- f: alignment --------------------------------------------------------------------------------------------------------------------
def _create(pkg, ctx, dtype, m, n, ptr, lda):
    h = _vp()
    assert pkg.lib().mik_dense_create(ctx.handle, pkg._lib.dtype_code(dtype), m, n, _vp(ptr), lda, C.byref(h)) == 0
    return h


@pytest.mark.parametrize("dtype", DTYPES)
def test_n_form_an_unaligned_y_leaves_the_16_byte_variant_only_when_the_product_kernel_stores_into_it(pkg, ctx, ref, shape, dtype):
    C_, R = shape
    for m in (65, R + 1):
        n = 2 * C_ + 1
        A, x = dh.normal(m, n, dtype, seed=40 + m), dh.vec(n, dtype, seed=40 + m)
        M = dh.matrix(pkg, ctx, A)
        assert M.buf.ptr % 16 == 0 and M.ld % 4 == 0
        one = _create(pkg, ctx, dtype, m, C_, M.buf.ptr, M.ld)          # the first chunk alone: k_dense_n stores into y itself
        try:
            for h, k, vec_when_y_is_odd in ((one, C_, 0), (M.dense, n, 1)):      # n = 2C + 1: the partials go to the workspace, the combine kernel stores
                want = ref.chunked(A[:, :k], x[:k], C_)
                for x_odd in (False, True):
                    xd = dh.at_odd_offset(pkg, ctx, x[:k]) if x_odd else V(pkg, ctx, x[:k])
                    for y_odd in (False, True):
                        out = Out(pkg, ctx, m, dtype, odd=y_odd)
                        expect(dh.plan(pkg, h, 0, xd, out.y), vec=vec_when_y_is_odd if y_odd else 1, cols=-(-k // C_))     # x never matters
                        assert np.array_equal(mul(pkg, h, 0, xd, out), want), (m, k, x_odd, y_odd)
        finally:
            pkg.lib().mik_dense_destroy(one)


@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_an_unaligned_x_takes_the_scalar_variant(pkg, orc, ctx, dtype):
    W, L, S = segment(ctx, dtype)
    m, n = S + 1, 5
    A, x = dh.normal(m, n, dtype, seed=50), dh.vec(m, dtype, seed=50)
    want = dh.tree_cols(orc, A, x, W, L)
    M = dh.matrix(pkg, ctx, A)
    for x_odd in (False, True):
        xd = dh.at_odd_offset(pkg, ctx, x) if x_odd else V(pkg, ctx, x)
        for y_odd in (False, True):                                     # y is written by the finaliser: it never matters
            out = Out(pkg, ctx, n, dtype, odd=y_odd)
            expect(dh.plan(pkg, M.dense, 1, xd, out.y), vec=0 if x_odd else 1, nseg=2, cols=1)
            got = mul(pkg, M.dense, 1, xd, out)
            assert np.array_equal(got, want), (x_odd, y_odd)
            assert np.array_equal(got, device_dots(pkg, M.col, n, xd)), (x_odd, y_odd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_aligned_base_with_a_leading_dimension_of_half_vectors(pkg, orc, ctx, ref, shape, dtype):
    """lda = 2 (mod 4) from an aligned base: every other column of Float32 starts 8 bytes off a 16-byte boundary -- the scalar variant; for
    Float64 every column is aligned and the 16-byte variant stays"""
    C_, R = shape
    W, L, S = segment(ctx, dtype)
    vec = 0 if dtype == np.float32 else 1
    assert (W == 4) == (dtype == np.float32)
    for adjoint, m, n in ((0, R + 1, 2 * C_ + 1), (1, S + 1, 5)):
        lda = m + (2 - m) % 4
        assert lda % 4 == 2 and m <= lda < m + 4
        A = dh.normal(m, n, dtype, seed=60 + adjoint)
        x = dh.vec(m if adjoint else n, dtype, seed=60)
        raw = Raw(pkg, ctx, A, lda, off=0)
        assert raw.rc == 0 and raw.buf.ptr % 16 == 0
        xd, out = V(pkg, ctx, x), Out(pkg, ctx, n if adjoint else m, dtype)
        expect(dh.plan(pkg, raw.h, adjoint, xd, out.y), vec=vec)
        got = mul(pkg, raw.h, adjoint, xd, out)
        if adjoint:
            assert np.array_equal(got, dh.tree_cols(orc, A, x, W, L)) and np.array_equal(got, device_dots(pkg, raw.col, n, xd))
        else:
            assert np.array_equal(got, ref.chunked(A, x, C_))
        raw.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16_byte_loads_never_reach_into_nan_padding_rows(pkg, orc, ctx, ref, shape, dtype):
    """HipMatrix pads its leading dimension with zeros, which a load that strays past row m would add unnoticed: here the padding is NaN
    and the 16-byte variant runs -- an aligned base, lda = m rounded up to 64"""
    C_, R = shape
    W, L, S = segment(ctx, dtype)
    for adjoint, m, n in ((0, R - 1, 2 * C_ + 1), (0, R + 1, 2 * C_ + 1), (1, S - 1, 37), (1, S + 1, 37)):
        lda = -(-m // 64) * 64
        assert lda > m
        A = dh.normal(m, n, dtype, seed=70 + m % 7)
        x = dh.vec(m if adjoint else n, dtype, seed=70)
        raw = Raw(pkg, ctx, A, lda, off=0)
        assert raw.rc == 0 and np.isnan(raw.buf.view(m, lda - m).to_numpy()).all()
        xd, out = V(pkg, ctx, x), Out(pkg, ctx, n if adjoint else m, dtype)
        expect(dh.plan(pkg, raw.h, adjoint, xd, out.y), vec=1)
        got = mul(pkg, raw.h, adjoint, xd, out)
        if adjoint:
            assert np.array_equal(got, dh.tree_cols(orc, A, x, W, L)) and np.array_equal(got, device_dots(pkg, raw.col, n, xd)), m
        else:
            assert np.array_equal(got, ref.chunked(A, x, C_)), m
        raw.close()


# ---- g: one handle, one workspace, two directions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_handle_alternates_between_the_directions(pkg, orc, ctx, ref, shape, dtype):
    C_, R = shape
    W, L, S = segment(ctx, dtype)
    m, n = S + 1, 2 * C_ + 1
    A, xn, xt = dh.normal(m, n, dtype, seed=80), dh.vec(n, dtype, seed=80), dh.vec(m, dtype, seed=81)
    M, xnd, xtd = dh.matrix(pkg, ctx, A), V(pkg, ctx, xn), V(pkg, ctx, xt)
    outs = {0: Out(pkg, ctx, m, dtype), 1: Out(pkg, ctx, n, dtype)}
    expect(dh.plan(pkg, M.dense, 0, xnd, outs[0].y), cols=3)          # chunk partials in the workspace ...
    expect(dh.plan(pkg, M.dense, 1, xtd, outs[1].y), nseg=2)          # ... and the segment sums of both segments
    want = {0: ref.chunked(A, xn, C_), 1: dh.tree_cols(orc, A, xt, W, L)}
    first = {}
    for turn, adjoint in enumerate((0, 1, 0, 1)):
        got = mul(pkg, M.dense, adjoint, xtd if adjoint else xnd, outs[adjoint])
        assert np.array_equal(got, first.setdefault(adjoint, got)), turn
        assert np.array_equal(got, want[adjoint]), turn


# ---- h: special values in the T form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_special_values(pkg, orc, ctx, dtype):
    W, L, S = segment(ctx, dtype)
    m, n = S + 1, 37
    A, x = np.array(dh.normal(m, n, dtype, seed=90), order="F"), np.abs(dh.vec(m, dtype, seed=90))
    A[:, 3] = -0.0                                                     # every product of column 3 is -0.0
    A[7, 20], x[7] = np.inf, 0                                         # Inf * 0 = NaN in column 20 only; the other columns add +-0 there
    want = dh.tree_cols(orc, A, x, W, L)
    assert np.array_equal(np.flatnonzero(np.isnan(want)), [20]) and want[3] == 0
    xd = V(pkg, ctx, x)
    for name, vec, h, col, keep in variants(pkg, ctx, A, m + 2):
        out = Out(pkg, ctx, n, dtype)
        expect(dh.plan(pkg, h, 1, xd, out.y), vec=vec, nseg=2, cols=2)
        got = mul(pkg, h, 1, xd, out)
        dots = device_dots(pkg, col, n, xd)
        assert np.array_equal(np.isnan(got), np.isnan(dots)) and np.array_equal(np.flatnonzero(np.isnan(got)), [20]), name
        assert got[3] == 0 and np.array_equal(np.signbit(got[3]), np.signbit(dots[3])), name      # the sign of the zero is mik_dot's
        ok = ~np.isnan(dots)
        assert np.array_equal(got[ok], dots[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(dots[ok])), name
        assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok])), name
