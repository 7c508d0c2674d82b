"""The dense operator on the device: mul!(y, A::Matrix, x) against the C restatement of its chunked order (tests/dense_ref/dense_mul_ref.c)
and against the sparse product of the fully stored matrix, mul!(y, adjoint(A), x) against mik_dot column by column, special values,
refusals, and the solvers on a HipMatrix -- through the library's own callback, with no Python frame per product.  Every comparison of
device results is np.array_equal.

The adjoint product is the fixed tree of mik_dot, the sparse adjoint product a serial row sum: on a general matrix the two differ in the
last bits whatever the size.  The solvers that use the adjoint are therefore compared bit for bit with the sparse route only where every
sum is exact (the Diagonal case of test/svdl.jl:20, inside one chunk); lsqr / lsmr / qmr run beyond one chunk (C = 64) and are held to the
residual bounds of tests/test_lsqr_lsmr.py and tests/test_qmr.py."""
import ctypes as C

import numpy as np
import pytest

import dense_operator_host as dh
from dense_operator_host import Raw, V, ref, shape  # noqa: F401  (ref, shape: fixtures)
from test_svdl_host import diag_case

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
DTYPES = [np.float64, np.float32]


def full_csc(A):
    """every entry of the m x n matrix stored: (colptr, rowval, nzval), 0-based"""
    m, n = A.shape
    return np.arange(0, m * n + 1, m, dtype=np.int64), np.tile(np.arange(m, dtype=np.int64), n), np.ascontiguousarray(A.T).reshape(-1).copy()


def full_csr_operator(pkg, ctx, A, adjoint=False):
    cp, rv, nz = full_csc(A)
    if adjoint:
        return pkg.extras.with_adjoint(A.shape[0], A.shape[1], cp, rv, nz, index_base=0, ctx=ctx)
    return pkg.HipCSR(A.shape[0], A.shape[1], cp, rv, nz, index_base=0, ctx=ctx)


def n_cases(C_, R):
    """every m with two n, every n with two m, both rectangular directions"""
    return [(1, 1), (1, 5 * C_ + 3), (63, C_ - 1), (63, 2 * C_ + 1), (64, C_), (64, 2 * C_), (65, C_ + 1), (65, 1), (R - 1, C_ - 1), (R - 1, 5 * C_ + 3),
            (R, C_), (R, 2 * C_ + 1), (R + 1, C_ + 1), (R + 1, 2 * C_), (2 * R + 1, 1), (2 * R + 1, 5 * C_ + 3)]


# ---- the N form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_n_form_equals_the_restatement_whatever_the_leading_dimension_and_alignment(pkg, ctx, ref, shape, dtype):
    C_, R = shape
    cases = n_cases(C_, R)
    for want, axis in ((set([1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1]), 0), (set([1, C_ - 1, C_, C_ + 1, 2 * C_, 2 * C_ + 1, 5 * C_ + 3]), 1)):
        for v in want:
            assert sum(1 for c in cases if c[axis] == v) >= 2, (axis, v)
    for m, n in cases:
        A, x = dh.rect(m, n, dtype, seed=1), dh.vec(n, dtype, seed=1)
        want = ref.chunked(A, x, C_)
        M, xd = pkg.HipMatrix.from_numpy(A, ctx), V(pkg, ctx, x)
        assert M.ld % 64 == 0 and M.ld >= m
        y = pkg.HipVector(m, dtype, ctx).fill_(7)
        assert pkg.mul_(y, M, xd) is y
        assert np.array_equal(y.to_numpy(), want), (m, n, "padded ld")
        assert np.array_equal((M @ xd).to_numpy(), want), (m, n, "A * x")
        raw = Raw(pkg, ctx, A, m + 1)                              # unaligned columns: the scalar-load variant
        assert raw.rc == 0
        ybuf = pkg.HipVector(m + 1, dtype, ctx).fill_(7)
        for yv in (y.fill_(7), ybuf.view(1, m)):                   # ... into an aligned and into an unaligned y
            assert raw.mul(0, xd, yv) == 0
            assert np.array_equal(yv.to_numpy(), want), (m, n, "lda = m + 1")
        raw.close()
        if n <= min(C_, 256):                                      # inside one chunk: also the sparse product of the fully stored matrix
            ys = pkg.HipVector(m, dtype, ctx)
            pkg.mul_(ys, full_csr_operator(pkg, ctx, A), xd)
            assert np.array_equal(ys.to_numpy(), want), (m, n, "mik_spmv")


# ---- the T form -----------------------------------------------------------------------------------------------------------------
def _t_case(pkg, ctx, dtype, m, n, raw_lda=None):
    A, x = dh.rect(m, n, dtype, seed=2), dh.vec(m, dtype, seed=2)
    xd = V(pkg, ctx, x)
    y = pkg.HipVector(n, dtype, ctx).fill_(7)
    if raw_lda is None:
        M = pkg.HipMatrix.from_numpy(A, ctx)
        assert pkg.mul_(y, M.adj, xd) is y
        want = np.array([pkg.dot(M.col(j), xd) for j in range(n)], dtype)
    else:
        raw = Raw(pkg, ctx, A, raw_lda)
        assert raw.rc == 0 and raw.mul(1, xd, y) == 0
        want = np.array([pkg.dot(raw.col(j), xd) for j in range(n)], dtype)
        raw.close()
    got = y.to_numpy()
    assert np.array_equal(got, want), (m, n, raw_lda)
    # ... and it is the product: a term passes through at most 40 roundings of the two-level tree at these sizes
    A64, x64 = A.T.astype(np.float64), x.astype(np.float64)
    assert np.all(np.abs(got - A64 @ x64) <= 40 * np.finfo(dtype).eps * (np.abs(A64) @ np.abs(x64)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_equals_mik_dot_of_every_column(pkg, ctx, dtype):
    W, L = ctx.reduce_shape(dtype)
    S = 256 * W * L
    ms, ns = (1, S - 1, S, S + 1, 2 * S + 5), (1, 3, 4, 5, 33)
    for i, m in enumerate(ms):                                   # every m with two n, every n with two m
        for n in (ns[i], ns[(i + 2) % 5]):
            _t_case(pkg, ctx, dtype, m, n)
    _t_case(pkg, ctx, dtype, S + 1, 5, raw_lda=S + 2)           # an unaligned leading dimension: the scalar-load variant
    _t_case(pkg, ctx, dtype, 2 * S + 5, 4, raw_lda=2 * S + 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_t_form_past_1024_segments_takes_the_second_tree_level(pkg, ctx, dtype):
    W, L = ctx.reduce_shape(dtype)
    _t_case(pkg, ctx, dtype, 1024 * 256 * W * L + 3, 2)


# ---- special values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(pkg, ctx, ref, shape, dtype):
    C_, R = shape
    m, n = 70, 2 * C_ + 9
    A, x = dh.rect(m, n, dtype, seed=3), np.abs(dh.vec(n, dtype, seed=3))
    A[5, :] = -0.0                                                 # every product of row 5 is -0.0: the sums start from +0
    M, y = pkg.HipMatrix.from_numpy(A, ctx), pkg.HipVector(m, dtype, ctx)
    got = pkg.mul_(y, M, V(pkg, ctx, x)).to_numpy()
    assert got[5] == 0 and not np.signbit(got[5]) and np.array_equal(got, ref.chunked(A, x, C_))
    A = dh.rect(m, n, dtype, seed=4)
    A[[3, 40], C_ + 2] = 0
    x = dh.vec(n, dtype, seed=4)
    x[C_ + 2] = np.inf                                             # Inf * 0 = NaN in rows 3 and 40, +-Inf elsewhere
    want = ref.chunked(A, x, C_)
    got = pkg.mul_(y, pkg.HipMatrix.from_numpy(A, ctx), V(pkg, ctx, x)).to_numpy()
    assert np.array_equal(np.flatnonzero(np.isnan(want)), [3, 40]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    raw = Raw(pkg, ctx, np.zeros((5, 0), dtype), 5, off=0)        # n = 0: the empty sum
    assert raw.rc == 0
    y5 = pkg.HipVector(5, dtype, ctx).fill_(7)
    assert raw.mul(0, pkg.HipVector(1, dtype, ctx), y5) == 0
    got = y5.to_numpy()
    assert np.array_equal(got, np.zeros(5, dtype)) and not np.signbit(got).any()
    raw.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx):
    A = dh.rect(40, 40, np.float64)
    M = pkg.HipMatrix.from_numpy(A, ctx)
    x = V(pkg, ctx, dh.vec(40, np.float64))
    with pytest.raises(pkg.MikError) as e:
        pkg.mul_(x, M, x)                                          # x and y overlap
    assert e.value.code == 1
    with pytest.raises(pkg.MikError) as e:
        pkg.mul_(M.col(3), M, x)                                   # y overlaps A
    assert e.value.code == 1
    h = _vp()
    assert pkg.lib().mik_dense_create(ctx.handle, 0, 40, 40, _vp(M.buf.ptr), 39, C.byref(h)) == 3 and not h      # lda < m: MIK_ERR_MISMATCH
    assert pkg.lib().mik_dense_create(ctx.handle, 0, 40, 40, None, 40, C.byref(h)) == 1 and not h                # a NULL matrix: MIK_ERR_INVALID
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.mul_(pkg.HipVector(40, np.float64, ctx), M, V(pkg, ctx, dh.vec(40, np.float32)))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.mul_(pkg.HipVector(40, np.float64, ctx), M.adj, V(pkg, ctx, dh.vec(39, np.float64)))
    with pytest.raises(TypeError, match="HipCSR"):
        pkg.lobpcg(M, False, 2)                                    # lobpcg needs a block product: still refused
    W = pkg.HipMatrix.from_numpy(dh.rect(40, 50, np.float64), ctx)  # a rectangular matrix never reaches the library's callback
    for Aop, k in ((W, 40), (W.adj, 50)):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            pkg.cg(Aop, V(pkg, ctx, dh.vec(k, np.float64)))
        with pytest.raises(ValueError, match="DimensionMismatch"):
            pkg.gmres(Aop, V(pkg, ctx, dh.vec(k, np.float64)))


# ---- solvers inside one chunk: one arithmetic with the sparse route ---------------------------------------------------------------
def _small_sizes(C_):
    return (48, 200) if C_ >= 256 else (min(48, C_ - 8), C_ - 1)


def _same(a, b):
    (xa, ha), (xb, hb) = a, b
    return ha.iters == hb.iters and ha.isconverged == hb.isconverged and np.array_equal(ha["resnorm"], hb["resnorm"]) and np.array_equal(xa.to_numpy(), xb.to_numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_and_gmres_inside_one_chunk_equal_the_sparse_route_and_the_oracle(pkg, orc, ctx, shape, dtype):
    C_, _ = shape
    W, L = ctx.reduce_shape(dtype)
    for n in _small_sizes(C_):
        assert n <= min(C_, 256)
        b = dh.vec(n, dtype, seed=n)
        bd = V(pkg, ctx, b)
        A = dh.spd(n, dtype)
        M, S = pkg.HipMatrix.from_numpy(A, ctx), full_csr_operator(pkg, ctx, A)
        Sf = pkg.LinearOperator(n, dtype, lambda y, v, S=S: pkg.mul_(y, S, v), ctx)
        dense = pkg.cg(M, bd, log=True, maxiter=4 * n)
        assert dense[1].isconverged and _same(dense, pkg.cg(Sf, bd, log=True, maxiter=4 * n)), n
        xo, ho = orc.cg(orc.CSC.from_dense(A), b, maxiter=4 * n, mode="tree", shape=(W, L, W, L))
        assert np.array_equal(dense[1]["resnorm"], ho["resnorm"]) and np.array_equal(dense[0].to_numpy(), xo), n
        A = dh.shifted(n, dtype)
        M, S = pkg.HipMatrix.from_numpy(A, ctx), full_csr_operator(pkg, ctx, A)
        Sf = pkg.LinearOperator(n, dtype, lambda y, v, S=S: pkg.mul_(y, S, v), ctx)
        dense = pkg.gmres(M, bd, log=True)
        assert dense[1].isconverged and _same(dense, pkg.gmres(Sf, bd, log=True)), n


# ---- solvers over several chunks: the native callback and the Python path are one arithmetic ----------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_solvers_over_several_chunks(pkg, ctx, shape, dtype):
    C_, _ = shape
    n = 2 * C_ + 17
    reltol = float(np.sqrt(np.finfo(dtype).eps))
    b = dh.vec(n, dtype, seed=9)
    bd = V(pkg, ctx, b)
    R = np.random.default_rng(n).random((n, n))
    spd = np.asfortranarray((R.T @ R / n + np.eye(n)).astype(dtype))
    B = dh.shifted(n, dtype)
    sym = np.asfortranarray(B + B.T)
    rspd = np.asfortranarray((B.astype(np.float64).T @ B.astype(np.float64)).astype(dtype))      # randSPD of test/chebyshev.jl:8-11
    ev = np.linalg.eigvalsh(rspd.astype(np.float64))                                              # approx_eigenvalue_bounds, :13-18
    lmin, lmax = float(ev[0] - (ev[-1] - ev[0]) / 100), float(ev[-1] + (ev[-1] - ev[0]) / 100)
    runs = (("cg", spd, lambda A: pkg.cg(A, bd, log=True, maxiter=4 * n)),
            ("gmres", B, lambda A: pkg.gmres(A, bd, log=True)),
            ("bicgstabl", B, lambda A: pkg.bicgstabl(A, bd, 2, log=True)),
            ("minres", sym, lambda A: pkg.minres(A, bd, log=True)),
            ("chebyshev", rspd, lambda A: pkg.chebyshev(A, bd, lmin, lmax, log=True, maxiter=10 * n)))
    for name, A, run in runs:
        assert np.count_nonzero(A) == A.size
        M = pkg.HipMatrix.from_numpy(A, ctx)
        Mf = pkg.LinearOperator(n, dtype, lambda y, v, M=M: pkg.mul_(y, M, v), ctx)
        dense = run(M)
        assert _same(dense, run(Mf)), name
        x = dense[0].to_numpy().astype(np.float64)
        res = np.linalg.norm(b.astype(np.float64) - A.astype(np.float64) @ x)
        print(f"   {name} {np.dtype(dtype).name} n = {n}: {dense[1].iters} iterations, |b - A x| = {res:.3e}, bound {reltol * np.linalg.norm(b.astype(np.float64)):.3e}")
        assert dense[1].isconverged, name
        assert res <= reltol * np.linalg.norm(b.astype(np.float64)), name


# ---- rectangular and adjoint solvers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lsqr_lsmr_on_a_rectangular_matrix_and_qmr(pkg, ctx, shape, dtype):
    """300 x 120 and 120 x 120 lie beyond one chunk (and the sparse adjoint sums serially where the dense one is the tree of mik_dot), so
    the runs are held to residual bounds.  lsqr / lsmr: a consistent system with |A|_F = 1 and |x| < 7; both stop when their residual
    estimate is at most btol |b| + atol |A| |x| (src/lsqr.jl test1, src/lsmr.jl test1; the estimate of |A| grows towards |A|_F and never
    passes it), to which the true residual adds rounding of at most iters * eps * (|b| + |A|_F |x|).  Float64 with the tolerances of
    tests/test_lsqr_lsmr.py (1e-6 / 1e-7) also stays inside that test's bound of 1e-4; Float32 runs with sqrt(eps) and sqrt(eps) / 10.
    qmr: test/qmr.jl:15-23, |A x - b| / |b| <= 10 sqrt(eps(T)) after qmr(A, b), and for Float64 the 1e-3 of tests/test_qmr.py."""
    C_, _ = shape
    m, n = 300, 120
    assert max(m, n) > min(C_, 256)
    eps = float(np.finfo(dtype).eps)
    A = dh.rect(m, n, np.float64, seed=6)
    A = np.asfortranarray((A / np.linalg.norm(A)).astype(dtype))
    A64 = A.astype(np.float64)
    xt = np.arange(n, 0, -1, dtype=np.float64) / n
    b = (A64 @ xt).astype(dtype)
    b64 = b.astype(np.float64)
    assert np.count_nonzero(A) == A.size
    M, bd = pkg.HipMatrix.from_numpy(A, ctx), V(pkg, ctx, b)
    assert pkg.extras.adjoint(M) is M.adj and (M.adj.size(1), M.adj.size(2)) == (n, m)
    tol = 1e-6 if dtype == np.float64 else float(np.sqrt(eps))
    for name, fn, t in (("lsqr", pkg.extras.lsqr, tol), ("lsmr", pkg.extras.lsmr, tol / 10)):
        x, h = fn(M, bd, atol=t, btol=t, conlim=1e10, maxiter=10 * n, log=True)
        x64 = x.to_numpy().astype(np.float64)
        res = np.linalg.norm(b64 - A64 @ x64)
        scale = np.linalg.norm(b64) + np.linalg.norm(A64) * np.linalg.norm(x64)
        bound = (t + h.iters * eps) * scale
        print(f"   {name} {np.dtype(dtype).name}: {h.iters} iterations, |b - A x| = {res:.3e}, bound {bound:.3e}")
        assert h.mvps > 0 and h.mtvps > 0 and h.iters < 10 * n and res <= bound, name
        if dtype == np.float64:
            assert bound < 1e-4 and res <= 1e-4, name
    B = dh.shifted(n, dtype)
    c = dh.vec(n, dtype, seed=8)
    x, h = pkg.extras.qmr(pkg.HipMatrix.from_numpy(B, ctx), V(pkg, ctx, c), log=True)
    res = np.linalg.norm(B.astype(np.float64) @ x.to_numpy().astype(np.float64) - c.astype(np.float64)) / np.linalg.norm(c.astype(np.float64))
    print(f"   qmr {np.dtype(dtype).name}: {h.iters} iterations, |A x - b| / |b| = {res:.3e}, bound {10 * np.sqrt(eps):.3e}")
    assert h.isconverged and res <= 10 * np.sqrt(eps)
    if dtype == np.float64:
        assert res <= 1e-3


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_other_solvers_accept_a_matrix(pkg, ctx, shape, dtype):
    """idrs and the power method take the path they take for any non-CSR operator: the same bits as on a LinearOperator over mul_"""
    C_, _ = shape
    n = 2 * C_ + 17
    B = dh.shifted(n, dtype)
    M = pkg.HipMatrix.from_numpy(B, ctx)
    Mf = pkg.LinearOperator(n, dtype, lambda y, v: pkg.mul_(y, M, v), ctx)
    b = V(pkg, ctx, dh.vec(n, dtype, seed=10))
    P = np.random.default_rng(5).random((n, 4)).astype(dtype)
    assert _same(pkg.extras.idrs(M, b, s=4, P=P, log=True), pkg.extras.idrs(Mf, b, s=4, P=P, log=True))
    x0 = dh.vec(n, dtype, seed=11)
    lam, x, h = pkg.extras.powm_(M, V(pkg, ctx, x0), maxiter=20, log=True)
    lam2, x2, h2 = pkg.extras.powm_(Mf, V(pkg, ctx, x0), maxiter=20, log=True)
    assert lam == lam2 and np.array_equal(x.to_numpy(), x2.to_numpy()) and np.array_equal(h["resnorm"], h2["resnorm"])
    # invpowm_: B has the action of inv(A - sigma I) (src/simple.jl:185) -- here that inverse as a dense matrix
    sigma = float(n)
    inv = np.asfortranarray(np.linalg.inv(B.astype(np.float64) - sigma * np.eye(n)).astype(dtype))
    Mi = pkg.HipMatrix.from_numpy(inv, ctx)
    Mif = pkg.LinearOperator(n, dtype, lambda y, v: pkg.mul_(y, Mi, v), ctx)
    lam, x, h = pkg.extras.invpowm_(Mi, V(pkg, ctx, x0), shift=sigma, maxiter=20, log=True)
    lam2, x2, h2 = pkg.extras.invpowm_(Mif, V(pkg, ctx, x0), shift=sigma, maxiter=20, log=True)
    assert lam == lam2 and np.isfinite(lam) and np.array_equal(x.to_numpy(), x2.to_numpy()) and np.array_equal(h["resnorm"], h2["resnorm"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_svdl_on_the_diagonal_matrix_equals_the_sparse_route(pkg, ctx, shape, dtype):
    """test/svdl.jl:20, Matrix(Diagonal(1:n)): n = 30 lies inside one chunk and every sum has one non-zero term, so the dense operator and
    the fully stored sparse one (with its adjoint) give the same bits"""
    C_, _ = shape
    S, kw = diag_case(dtype)
    A = np.asfortranarray(S.toarray().astype(dtype))
    assert max(A.shape) <= min(C_, 256)
    sd, Ld, hd = pkg.svdl(pkg.HipMatrix.from_numpy(A, ctx), log=True, **kw)
    ss, Ls, hs = pkg.svdl(full_csr_operator(pkg, ctx, A, adjoint=True), log=True, **kw)
    assert hd.isconverged and hd.iters == hs.iters and np.array_equal(sd, ss)
    assert all(np.array_equal(a, b) for a, b in zip(hd["ritz"], hs["ritz"])) and np.array_equal(np.array(hd["betas"]), np.array(hs["betas"]))
    assert np.linalg.norm(sd - np.arange(30, 25, -1.0)) < 5 ** 2 * 1e-5
    with pytest.raises(TypeError):
        pkg.svdl(object())


# ---- the C ABI with no Python in the loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_through_the_c_abi_with_the_librarys_own_callback(pkg, ctx, shape, dtype):
    C_, _ = shape
    L = pkg.lib()
    n = 2 * C_ + 17
    R = np.random.default_rng(n).random((n, n))
    A = np.asfortranarray((R.T @ R / n + np.eye(n)).astype(dtype))
    b = dh.vec(n, dtype, seed=12)
    M, bd = pkg.HipMatrix.from_numpy(A, ctx), V(pkg, ctx, b)
    reltol = float(np.sqrt(np.finfo(dtype).eps))
    xw, hw = pkg.cg(M, bd, log=True, maxiter=4 * n)
    op = pkg._lib.MikOperator(pkg._lib.dtype_code(dtype), n, None, C.cast(L.mik_dense_mul_fn, pkg._lib.MUL_FN), M.dense)
    x, u, r, c = (pkg.HipVector(n, dtype, ctx).fill_(0) for _ in range(4))
    h = _vp()
    assert L.mik_cg_create_op(ctx.handle, C.byref(op), None, _vp(x.ptr), _vp(bd.ptr), _vp(u.ptr), _vp(r.ptr), _vp(c.ptr), 0.0, reltol, 4 * n, 1, C.byref(h)) == 0
    res = np.zeros(4 * n)
    steps = C.c_int64()
    assert L.mik_cg_iterate_many(h, 0, 4 * n, res.ctypes.data_as(C.POINTER(C.c_double)), C.byref(steps)) == 0
    assert L.mik_cg_destroy(h) == 0
    assert steps.value == hw.iters and np.array_equal(res[:steps.value], hw["resnorm"][-steps.value:]) and np.array_equal(x.to_numpy(), xw.to_numpy())
