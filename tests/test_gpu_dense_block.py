"""The block product of a dense device matrix, Y[:, j] = A X[:, j] (mik_dense_mm, csrc/mik_dense_mul.h k_dense_nb), and lobpcg on
``HipMatrix`` operators.

The contract is one of bits: column j of Y equals mik_dense_mul on that column, which equals the chunked order restated in C
(tests/dense_ref/dense_mul_ref.c) -- whatever b, the group width, the placement of A, X and Y, the launch shape, and whether a narrow last
group runs through the block kernel or, as the library chooses below its threshold, through the vector kernels.  Every comparison is
np.array_equal; the data (tests/lobpcg_gpu_util.wide, tests/dense_operator_host.rect) moves bits under an FMA or another association.
Each case runs with the handle's threshold as the library has it and with the block kernel forced at every width
(mik_dev_dense_block_min_width), and asserts the plan (mik_dev_dense_block_plan, computed by the helper the launch runs) before the bits.
The solver tests hold ``lobpcg(..., dense=True)`` on ``HipMatrix`` operators to the numpy double (tests/lobpcg_double.py with the dense operator of
tests/lobpcg_dense_double.py) bit for bit."""
import contextlib
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as sp

import dense_block_host as bh
import dense_operator_host as dh
from conftest import KN
from dense_operator_host import Raw, ref, shape  # noqa: F401  (ref, shape: fixtures)
from lobpcg_dense_double import DenseOperator, separated, sym
from lobpcg_double import HostJacobi, NumpyOps, operator
from lobpcg_gpu_util import Blk, same_trace, wide

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
DTYPES = [np.float64, np.float32]
FILL = 7.0


@pytest.fixture(scope="session")
def gw(pkg):
    return bh.block_shape(pkg)


@contextlib.contextmanager
def machine(ctx, value):
    ctx.set_tuning(KN.MACHINE, value)
    try:
        yield
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


def expect(p, **want):
    assert {k: p[k] for k in want} == want, (p, want)


class Case:
    """one matrix with its right-hand sides: the host reference of every column (the chunked order in C) computed once"""

    def __init__(self, ref, C_, A, X):
        self.A, self.X, self.m, self.n = A, X, A.shape[0], A.shape[1]
        self.want = np.stack([ref.chunked(A, X[:, j], C_) for j in range(X.shape[1])], axis=1) if X.shape[1] else np.zeros((self.m, 0), A.dtype)


def vector_columns(pkg, ctx, handle, case, b):
    """mik_dense_mul of the first b columns on the device"""
    Xd = Blk(pkg, ctx, case.X[:, :b], False)
    y = pkg.HipVector(case.m, case.A.dtype, ctx)
    out = []
    for j in range(b):
        assert pkg.lib().mik_dense_mul(handle, 0, _vp(Xd.col(j).ptr), _vp(y.ptr)) == 0
        out.append(y.to_numpy())
    return np.stack(out, axis=1)


def block(pkg, ctx, handle, case, b, offset, forced, **plan):
    """Y of mik_dense_mm for the first b columns (X and Y aligned, or one element into their buffers with an odd leading dimension), after the
    plan was held to `plan`; Y's padding must keep its fill"""
    Xd = Blk(pkg, ctx, case.X[:, :b], offset)
    Yd = Blk(pkg, ctx, np.full((case.m, b), FILL, case.A.dtype), offset, fill=FILL)
    bh.min_width(pkg, handle, 1 if forced else 0)
    try:
        p = bh.plan(pkg, handle, b, Xd, Yd)
        expect(p, **plan)
        assert bh.mm(pkg, handle, b, Xd, Yd) == 0, pkg.lib().mik_last_error(ctx.handle)
    finally:
        bh.min_width(pkg, handle, 0)
    pad = Yd.padding()
    assert np.array_equal(pad, np.full(pad.size, FILL, pad.dtype))
    return Yd.get(), p


def operands(pkg, ctx, A, which=("HipMatrix", "Raw")):
    """(name, 16-byte matrix, handle, keep-alive): a HipMatrix, and the same matrix one element into its buffer with an odd leading dimension"""
    if "HipMatrix" in which:
        M = dh.matrix(pkg, ctx, A)
        yield "HipMatrix", 1, M.dense, M
        del M
    if "Raw" in which:
        m = A.shape[0]
        raw = Raw(pkg, ctx, A, m + 1 + m % 2, off=1)
        assert raw.rc == 0 and raw.lda % 2 == 1
        yield "Raw", 0, raw.h, raw
        raw.close()


# ---- a, b: bits and placement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(5))
def test_every_column_has_the_bits_of_the_vector_product_at_every_width_and_placement(pkg, ctx, ref, shape, gw, case, dtype):
    C_, R = shape
    m, n = bh.bit_shapes(C_, R)[case]
    rng = np.random.default_rng(100 + case)
    cs = Case(ref, C_, dh.rect(m, n, dtype, seed=case), wide(rng, (n, bh.B_MAX), dtype, span=12))
    if n <= C_:
        serial = np.stack([ref.serial(cs.A, cs.X[:, j]) for j in range(bh.B_MAX)], axis=1)
        assert np.array_equal(cs.want, serial)                           # one chunk: Julia's own order
    for name, a16, h, keep in operands(pkg, ctx, cs.A):
        vec_cols = vector_columns(pkg, ctx, h, cs, bh.B_MAX)
        assert np.array_equal(vec_cols, cs.want), name
        for offset in (False, True):
            vec = int(bool(a16 and (n > C_ or not offset)))              # one chunk: the product kernel stores into Y itself
            for b in bh.widths(gw):
                for forced in (True, False):
                    model = bh.model_nb(m, n, b, C_, R, gw, 0, 1 if forced else bh.GW_MIN)
                    got, p = block(pkg, ctx, h, cs, b, offset, forced, vec=vec, streamed=0, chunks=dh._ceil(n, C_), gx=dh._ceil(m, R),
                                   groups=model["groups"], last_w=model["last_w"], vector_cols=model["vector_cols"])
                    assert np.array_equal(got, vec_cols[:, :b]), (name, offset, b, forced)
                    assert np.array_equal(np.signbit(got), np.signbit(cs.want[:, :b])), (name, offset, b, forced)


# ---- c: every loop takes a second pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(3))
def test_chunk_loop_takes_several_passes_in_two_groups(pkg, ctx, ref, shape, gw, case, dtype):
    C_, R = shape
    m, n, gx, gy, nc, passes = dh.CHUNK_STRIDE(C_, R)[case]
    b = gw + 1
    cs = Case(ref, C_, dh.normal(m, n, dtype, seed=10 + case), wide(np.random.default_rng(110 + case), (n, b), dtype, span=12))
    for name, a16, h, keep in operands(pkg, ctx, cs.A):
        with machine(ctx, dh.SMALL_MACHINE):
            small, p = block(pkg, ctx, h, cs, b, False, True, vec=a16, streamed=0, gx=gx, gy=gy, chunks=nc, groups=2, last_w=1, vector_cols=0)
            assert dh._ceil(p["chunks"], p["gy"]) == passes >= 2
        as_queried, _ = block(pkg, ctx, h, cs, b, True, False, vec=a16, gx=gx, chunks=nc, groups=1, last_w=gw, vector_cols=1)
        assert np.array_equal(small, cs.want), (name, m, n)
        assert np.array_equal(as_queried, cs.want), (name, m, n)
        assert np.array_equal(vector_columns(pkg, ctx, h, cs, b), cs.want), (name, m, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_combine_takes_its_batches_and_its_tail_for_three_columns(pkg, ctx, ref, shape, gw, dtype):
    C_, R = shape
    m, b = 65, 3
    assert [dh.combine_trips(nc) for nc in dh.COMBINE_NC] == list(dh.COMBINE_TRIPS)
    for nc in dh.COMBINE_NC:
        n = nc * C_ - 5
        cs = Case(ref, C_, dh.normal(m, n, dtype, seed=nc), wide(np.random.default_rng(120 + nc), (n, b), dtype, span=12))
        M = dh.matrix(pkg, ctx, cs.A)
        for offset in (False, True):
            got, _ = block(pkg, ctx, M.dense, cs, b, offset, False, vec=1, streamed=0, gx=1, gy=nc, chunks=nc, groups=1, last_w=3, vector_cols=0)
            assert np.array_equal(got, cs.want), (nc, offset)


@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_variant_on_both_sides_of_its_threshold(pkg, ctx, ref, shape, gw, dtype):
    C_, R = shape
    m, n = dh.streamed_shape(R, np.dtype(dtype).itemsize)
    b = gw + 1
    A = dh.normal(m, n, dtype, seed=30)
    X = wide(np.random.default_rng(130), (n, b), dtype, span=12)
    big = Raw(pkg, ctx, A, dh._ceil(m, 64) * 64, off=0)
    assert big.rc == 0
    less = big.narrower(n - 1)
    assert less.rc == 0
    for op, k, streamed in ((big, n, 1), (less, n - 1, 0)):
        cs = Case(ref, C_, A[:, :k], X[:k, :0])                          # no host reference yet: each costs a copy of the matrix
        cs.X = X[:k]
        got, _ = block(pkg, ctx, op.h, cs, b, False, True, vec=1, streamed=streamed, gx=dh._ceil(m, R), chunks=dh._ceil(k, C_), groups=2, last_w=1)
        assert np.array_equal(got, vector_columns(pkg, ctx, op.h, cs, b)), k
        for j in (gw - 1, gw):                                           # the last column of the full group, the column of the second group
            assert np.array_equal(got[:, j], ref.chunked(cs.A, cs.X[:, j], C_)), (k, j)
    less.close()
    big.close()


# ---- d: refusals and empties ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_blocks(pkg, ctx, shape):
    C_, R = shape
    OK, INVALID, MISMATCH, NOTIMPL = 0, 1, 3, 5                         # include/mik.h
    L = pkg.lib()
    m, n = 70, C_ + 3
    A = dh.rect(m, n, np.float64)
    M = dh.matrix(pkg, ctx, A)
    h = M.dense
    X = Blk(pkg, ctx, np.ones((n, 33)), False)
    Y = Blk(pkg, ctx, np.full((m, 33), FILL), False, fill=FILL)

    def untouched():
        flat = Y.buf.to_numpy()
        return np.array_equal(flat, np.full(flat.size, FILL))

    mm = lambda b, xp, ldx, yp, ldy: L.mik_dense_mm(h, b, _vp(xp), ldx, _vp(yp), ldy)
    assert mm(33, X.ptr, X.ld, Y.ptr, Y.ld) == NOTIMPL
    assert mm(-1, X.ptr, X.ld, Y.ptr, Y.ld) == INVALID
    assert mm(2, X.ptr, n - 1, Y.ptr, Y.ld) == MISMATCH
    assert mm(2, X.ptr, X.ld, Y.ptr, m - 1) == MISMATCH
    assert mm(2, None, X.ld, Y.ptr, Y.ld) == INVALID and mm(2, X.ptr, X.ld, None, Y.ld) == INVALID
    assert mm(2, Y.ptr + 8, Y.ld, Y.ptr, Y.ld) == INVALID                # Y overlaps X
    assert mm(2, X.ptr, X.ld, M.buf.ptr + 8 * (M.ld + 3), M.ld) == INVALID        # Y overlaps A
    assert L.mik_dense_mm(None, 2, _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld) == INVALID
    assert mm(0, X.ptr, X.ld, Y.ptr, Y.ld) == OK and mm(0, None, 0, None, 0) == OK
    assert untouched() and np.array_equal(M.to_numpy(), A)               # nothing was launched
    # m = 0: nothing to write; n = 0: the empty sum, +0.0 in every column
    for dtype in DTYPES:
        e = _vp()
        assert L.mik_dense_create(ctx.handle, pkg._lib.dtype_code(dtype), 0, 5, None, 1, C.byref(e)) == 0
        assert L.mik_dense_mm(e, 3, _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld) == OK and untouched()
        L.mik_dense_destroy(e)
        Z = Blk(pkg, ctx, np.full((m, 9), -1.0, dtype), True, fill=FILL)
        assert L.mik_dense_create(ctx.handle, pkg._lib.dtype_code(dtype), m, 0, None, m, C.byref(e)) == 0
        assert L.mik_dense_mm(e, 9, None, 1, _vp(Z.ptr), Z.ld) == OK
        z, pad = Z.get(), Z.padding()
        assert np.array_equal(z, np.zeros((m, 9), dtype)) and not np.signbit(z).any() and np.array_equal(pad, np.full(pad.size, FILL, dtype))
        p = bh.plan(pkg, e, 9, Z, Z)
        expect(p, groups=0, vector_cols=0, gx=0, gy=0, chunks=0)
        L.mik_dense_destroy(e)


# ---- e: the two workspaces -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_vector_products_around_a_block_product_keep_their_bits(pkg, ctx, ref, shape, gw, dtype):
    C_, R = shape
    m, n, b = R + 1, 3 * C_ + 5, gw + 2
    cs = Case(ref, C_, dh.rect(m, n, dtype, seed=7), wide(np.random.default_rng(140), (n, b), dtype, span=12))
    M = dh.matrix(pkg, ctx, cs.A)
    L = pkg.lib()
    Xd, Yd = Blk(pkg, ctx, cs.X, False), Blk(pkg, ctx, np.full((m, b), FILL, dtype), False, fill=FILL)
    assert bh.plan(pkg, M.dense, b, Xd, Yd)["workspace_bytes"] == 0
    assert L.mik_dense_block_reserve(M.dense) == 0
    bytes_ = bh.plan(pkg, M.dense, b, Xd, Yd)["workspace_bytes"]
    assert bytes_ == gw * dh._ceil(n, C_) * dh._ceil(m, R) * R * np.dtype(dtype).itemsize
    assert L.mik_dense_block_reserve(M.dense) == 0 and bh.plan(pkg, M.dense, b, Xd, Yd)["workspace_bytes"] == bytes_      # idempotent
    y0, y1 = pkg.HipVector(m, dtype, ctx), pkg.HipVector(m, dtype, ctx)
    # all three are enqueued before anything is read back: the vector product's partials are in flight when the block product starts
    assert L.mik_dense_mul(M.dense, 0, _vp(Xd.col(b - 1).ptr), _vp(y0.ptr)) == 0
    assert bh.mm(pkg, M.dense, b, Xd, Yd) == 0
    assert L.mik_dense_mul(M.dense, 0, _vp(Xd.col(0).ptr), _vp(y1.ptr)) == 0
    assert np.array_equal(y0.to_numpy(), cs.want[:, b - 1]) and np.array_equal(y1.to_numpy(), cs.want[:, 0])
    assert np.array_equal(Yd.get(), cs.want)
    # one chunk: nothing to reserve
    S = dh.matrix(pkg, ctx, cs.A[:, :C_])
    assert L.mik_dense_block_reserve(S.dense) == 0 and bh.plan(pkg, S.dense, b, Xd, Yd)["workspace_bytes"] == 0


# ---- f: HipMatrix.mm_ ------------------------------------------------------------------------------------------------------------------------
def test_mm_method_of_hipmatrix(pkg, ctx, ref, shape):
    C_, R = shape
    m, n, b = 33, C_ + 9, 5
    cs = Case(ref, C_, dh.rect(m, n, np.float64, seed=8), wide(np.random.default_rng(150), (n, b), np.float64, span=12))
    A, X, Y = pkg.HipMatrix.from_numpy(cs.A, ctx), pkg.HipMatrix.from_numpy(cs.X, ctx), pkg.HipMatrix(m, b, np.float64, ctx)
    assert A.mm_(Y, X) is Y and np.array_equal(Y.to_numpy(), cs.want)
    Y2 = pkg.HipMatrix(m, b, np.float64, ctx)
    A.mm_(Y2, X, 2)
    assert np.array_equal(Y2.to_numpy()[:, :2], cs.want[:, :2]) and not Y2.to_numpy()[:, 2:].any()
    with pytest.raises(ValueError, match="DimensionMismatch"):
        A.mm_(X, X)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        A.mm_(Y, X, b + 1)


# ---- g: lobpcg on HipMatrix operators ----------------------------------------------------------------------------------------------------------
def max_err(A, B, X, lam):
    BX = X if B is None else B @ X
    Rm = A @ X - BX * lam[None, :]
    return np.max(np.sqrt(np.sum(Rm * Rm, axis=0)))


def both(pkg, orc, ref, ctx, C_, A, B, largest, rest, jacobi, b_csr=False, **kw):
    """(device run on HipMatrix operators -- B as a HipCSR when b_csr --, run on the numpy double) of one lobpcg call"""
    dt, n = A.dtype, A.shape[0]
    Ad = pkg.HipMatrix.from_numpy(A, ctx)
    Bd = None if B is None else (pkg.HipCSR.from_scipy(sp.csc_matrix(B), ctx) if b_csr else pkg.HipMatrix.from_numpy(B, ctx))
    Bh = None if B is None else (operator(orc, sp.csc_matrix(B)) if b_csr else DenseOperator(ref, B, C_))
    d = np.diag(A).astype(dt)
    dev = (Ad, largest) if B is None else (Ad, Bd, largest)
    dbl = (DenseOperator(ref, A, C_), largest) if B is None else (DenseOperator(ref, A, C_), Bh, largest)
    rd = pkg.lobpcg(*dev, *rest, P=pkg.JacobiPrec(pkg.HipVector.from_numpy(d, ctx)) if jacobi else None, log=True, rng=np.random.default_rng(5),
                    dense=True, **kw)
    rh = pkg.lobpcg(*dbl, *rest, P=HostJacobi(d) if jacobi else None, log=True, rng=np.random.default_rng(5), ops=NumpyOps(orc, n, dt), **kw)
    return rd, rh


def same_result(rd, rh):
    same_trace(rd.trace, rh.trace)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms) and rd.iterations == rh.iterations
    assert np.array_equal(rd.X.to_numpy()[:, :len(rd.lam)], rh.X.to_numpy()[:, :len(rh.lam)])


def tol_of(pkg, dt):
    return import_module(pkg.__name__ + ".lobpcg").default_tolerance(dt)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("generalized", [False, True])
def test_lobpcg_reference_cases_on_device_matrices_equal_the_double(pkg, orc, ctx, ref, shape, dtype, generalized):
    """test/lobpcg.jl:34-71 (n = 10) on HipMatrix operators: the trace of the double bit for bit, and the reference's residual checks"""
    C_, R = shape
    n = 10
    A, B = sym(n, dtype, 31), (sym(n, dtype, 32) if generalized else None)
    b = np.random.default_rng(33).random((n, 1)).astype(dtype)
    tol = tol_of(pkg, dtype)
    for largest in (True, False):
        for jacobi in (False, True):
            rd, rh = both(pkg, orc, ref, ctx, C_, A, B, largest, (b,), jacobi, tol=tol, maxiter=200)
            same_result(rd, rh)
            X = rd.X.to_numpy()
            assert rd.converged
            if generalized:
                assert max_err(A, B, X, rd.lam) <= tol                   # :63
            else:
                assert np.linalg.norm(A @ X - X * rd.lam[None, :]) <= tol        # :44
            r2 = pkg.lobpcg(*((pkg.HipMatrix.from_numpy(A, ctx),) + (() if B is None else (pkg.HipMatrix.from_numpy(B, ctx),))), largest, X,
                            tol=10 * tol, log=True, dense=True)
            assert len(r2.trace) == 1                                    # :46-48, :65-67


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("generalized", [False, True])
def test_lobpcg_above_one_chunk_with_a_block_of_4_equals_the_double(pkg, orc, ctx, ref, shape, dtype, generalized):
    C_, R = shape
    n = 3 * C_ + 5
    A, B = separated(n, dtype, 34), (sym(n, dtype, 36, shift=40) if generalized else None)
    X0 = np.random.default_rng(35).random((n, 4)).astype(dtype)
    for largest in (True, False):
        for jacobi in (False, True):
            if jacobi:                                                   # a diagonal a Jacobi preconditioner can divide by
                Aj = A + np.diag(np.full(n, 50, dtype))
            rd, rh = both(pkg, orc, ref, ctx, C_, Aj if jacobi else A, B, largest, (X0,), jacobi, tol=tol_of(pkg, dtype), maxiter=25)
            same_result(rd, rh)
            assert rd.iterations >= 2


def test_lobpcg_dense_a_with_sparse_b_and_the_batched_driver(pkg, orc, ctx, ref, shape):
    C_, R = shape
    n, dt = 3 * C_ + 5, np.float64
    A = separated(n, dt, 37)
    Bs = sp.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).toarray().astype(dt)
    X0 = np.random.default_rng(38).random((n, 4)).astype(dt)
    rd, rh = both(pkg, orc, ref, ctx, C_, A, Bs, False, (X0,), False, b_csr=True, tol=tol_of(pkg, dt), maxiter=25)
    same_result(rd, rh)
    # lobpcg(A, largest, X0, nev): 4 pairs in batches of 2, the second deflated against the first
    rd, rh = both(pkg, orc, ref, ctx, C_, A, None, True, (X0[:, :2], 4), False, tol=tol_of(pkg, dt), maxiter=60)
    assert len(rd.lam) == 4 and np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms)
    assert np.array_equal(rd.iterations, rh.iterations) and np.array_equal(rd.converged, rh.converged)
    for ta, tb in zip(rd.trace, rh.trace):
        same_trace(ta, tb)
    assert np.array_equal(rd.X.to_numpy()[:, :4], rh.X.to_numpy()[:, :4])
    assert np.all(rd.converged) and max_err(A, None, rd.X.to_numpy()[:, :4], rd.lam) <= tol_of(pkg, dt)


def test_lobpcg_refuses_what_is_not_a_device_operator(pkg, ctx):
    A = pkg.HipMatrix.from_numpy(sym(10, np.float64, 31), ctx)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.lobpcg(pkg.HipMatrix(10, 9, np.float64, ctx), True, 1, dense=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.lobpcg(A, pkg.HipMatrix.from_numpy(sym(10, np.float32, 32), ctx), True, 1, dense=True)
    with pytest.raises(TypeError, match="callbacks are not supported"):
        pkg.lobpcg(A, lambda y, x: y, True, 1, dense=True)
    with pytest.raises(TypeError, match="HipCSR.*dense=True"):          # the dense route is asked for: without the keyword a HipMatrix is refused as before
        pkg.lobpcg(A, True, 1)
    with pytest.raises(TypeError, match="HipCSR.*dense=True"):
        pkg.LOBPCGIterator(A, None, True, np.ones((10, 1)))


# ---- h: nothing is allocated inside the loop ---------------------------------------------------------------------------------------------------
def test_no_device_allocation_inside_the_iteration_loop_with_dense_operators(pkg, ctx, shape, gw, monkeypatch):
    C_, R = shape
    n = 3 * C_ + 5
    A, B = pkg.HipMatrix.from_numpy(separated(n, np.float64, 39) + 50 * np.eye(n), ctx), pkg.HipMatrix.from_numpy(sym(n, np.float64, 40, shift=40), ctx)
    P = pkg.JacobiPrec(pkg.HipVector.from_numpy(A.to_numpy().diagonal().copy(), ctx))
    Cm = np.random.default_rng(9).random((n, 2))
    L = pkg.lib()
    real = L.mik_malloc
    count = [0]

    def counting(*args):
        count[0] += 1
        return real(*args)

    monkeypatch.setattr(L, "mik_malloc", counting)
    it = pkg.LOBPCGIterator(A, B, False, np.random.default_rng(10).random((n, 4)), None, P, Cm, dense=True)
    X = it.XBlocks
    held = lambda: [bh.plan(pkg, M.dense, 4, X.block, X.A_block)["workspace_bytes"] for M in (A, B)]
    before = held()
    assert before == [gw * dh._ceil(n, C_) * R * 8] * 2                  # reserved when the iterator was built
    seen = []
    step = it.step

    def watched(tol, log):
        seen.append(count[0])
        return step(tol, log)

    it.step = watched
    pkg.lobpcg_(it, maxiter=12, not_zeros=True)
    seen.append(count[0])
    monkeypatch.undo()
    assert count[0] > 0 and len(seen) > 5
    assert len(set(seen)) == 1, seen
    assert held() == before
