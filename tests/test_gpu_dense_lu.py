"""lu(A) / lu_(A) on a dense device matrix and ldiv_ (iterativesolvers.jl_amd/dense_lu.py over the mik_dense_lu_* entries), bit for bit
against tests/dense_ref/dense_lu_ref.c -- the contract's unblocked loops restated in C.  Every comparison of device values with the
checker's is dense_lu_host.same_bits (NaN positions, and the bits everywhere else: -0.0 is not +0.0); comparisons with a fixture's
construction are np.array_equal.  Every shape comes from mik_dense_lu_info.  Non-finite data, poisoned padding, other leading dimensions
and ties in later columns are in test_gpu_dense_lu_edges.py.  The reference's own statements with lu(A) as Pl / Pr carry the reference's own bounds."""
import ctypes as C

import numpy as np
import pytest

import dense_lu_host as lh

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lh.build(tmp_path_factory.mktemp("dense_lu_ref_gpu"))


@pytest.fixture(scope="module")
def shape(pkg, ctx):
    """(W, R, T, one-launch row limit): panel width, rows per workgroup of the pivot search, the larger tile edge of the trailing update"""
    info = pkg.lu(pkg.HipMatrix.from_numpy(np.ones((1, 1)))).info()
    assert info["W"] >= 2 and info["R"] >= 2 and info["tile_rows"] >= 2 and info["tile_cols"] >= 2 and info["launches_solve"] == 3
    return info["W"], info["R"], max(info["tile_rows"], info["tile_cols"]), info["one_launch_rows"]


def plan_launches(n, W):
    """the launches of one factorisation, restated: per panel one search of its first column, a pick per column, an update per column
    that has rows below it, the interchanges outside the panel when there are columns outside it, and -- with columns to the right --
    the strip solve and the trailing update"""
    total = 0
    for k0 in range(0, n, W):
        k1 = min(k0 + W, n)
        w = k1 - k0
        total += 1 + w + (w if k1 < n else w - 1) + (1 if n > w else 0) + (2 if k1 < n else 0)
    return total


def sizes(shape):
    W, R, T, one = shape
    s = {1, 2, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3, R - 1, R, R + 1, 2 * R + W + 1, T - 1, T, T + 1, 1025}
    if one:
        s |= {one - 1, one, one + 1}
    return sorted(s)


_CASES = {}


def case(pkg, ref, n, dtype):
    """(A, the checker's factors and ipiv, the device factorisation of a copy of A) -- computed once per size and type"""
    key = (n, np.dtype(dtype).name)
    if key not in _CASES:
        A = lh.random(n, dtype)
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0 and np.isfinite(LU).all()
        M = pkg.HipMatrix.from_numpy(A)
        assert M.ld != n or n % 64 == 0
        _CASES[key] = (A, LU, ipiv, M, pkg.lu(M))
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_factors_and_pivots_bit_for_bit(pkg, ctx, ref, shape, dtype):
    W = shape[0]
    for n in sizes(shape):
        A, LU, ipiv, M, F = case(pkg, ref, n, dtype)
        info = F.info()
        assert info["launches_factor"] == plan_launches(n, W) and info["launches_solve"] == 1 + 2 * -(-n // W), n
        assert F.n == n and F.dtype == np.dtype(dtype) and F.ipiv.dtype == np.int64
        assert np.array_equal(F.ipiv, ipiv), (n, np.flatnonzero(F.ipiv != ipiv)[:4])
        got = F.factors.to_numpy()
        assert lh.same_bits(got, LU), f"factors differ, n = {n}, {np.dtype(dtype)}, first at {lh.first_difference(got, LU)}"
        assert F.factors is not M and np.array_equal(M.to_numpy(), A)                  # lu(A) leaves A untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_ldiv_bit_for_bit(pkg, ctx, ref, shape, dtype):
    for n in sizes(shape):
        A, LU, ipiv, M, F = case(pkg, ref, n, dtype)
        b = lh.vector(n, dtype)
        want = ref.solve(LU, ipiv, b)
        assert np.isfinite(want).all()
        x, y = pkg.HipVector.from_numpy(b), pkg.HipVector(n, dtype).fill_(0)
        assert F.ldiv_(y, x) is y
        assert lh.same_bits(y.to_numpy(), want), (n, lh.first_difference(y.to_numpy(), want))
        assert np.array_equal(x.to_numpy(), b)                                         # x is untouched in the two-argument form
        assert F.ldiv_(x) is x and lh.same_bits(x.to_numpy(), want)                    # ldiv!(F, x)
        s = F.solve(pkg.HipVector.from_numpy(b))
        assert s is not y and lh.same_bits(s.to_numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_fixture_on_the_device(pkg, ctx, dtype):
    """equality, not a tolerance: the interchanges are the permutation, the factors are L and U, the solve returns x"""
    n = 130
    A, L, U, rows, x, b = lh.exact(n, dtype)
    F = pkg.lu(pkg.HipMatrix.from_numpy(A))
    assert np.array_equal(lh.permutation_of(F.ipiv), rows)
    LU = F.factors.to_numpy()
    assert np.array_equal(np.tril(LU, -1) + np.eye(n, dtype=dtype), L) and np.array_equal(np.triu(LU), U)
    assert np.array_equal(F.solve(pkg.HipVector.from_numpy(b)).to_numpy(), x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pivot_rules(pkg, ctx, ref, shape, dtype):
    W, R, T, _ = shape
    n = 3 * R + 7
    rows = (R - 1, R, 2 * R + 3, 3 * R + 6)                       # four different workgroups of the search; the first must win
    A = lh.ties(n, dtype, rows)
    LU, ipiv, _ = ref.factor(A)
    F = pkg.lu(pkg.HipMatrix.from_numpy(A))
    assert ipiv[0] == rows[0] + 1 == F.ipiv[0] and np.array_equal(F.ipiv, ipiv) and lh.same_bits(F.factors.to_numpy(), LU)
    rows = (2 * R + 3, 3 * R + 6)                                 # ... also when no candidate sits in the first workgroups
    F = pkg.lu(pkg.HipMatrix.from_numpy(lh.ties(n, dtype, rows)))
    assert F.ipiv[0] == rows[0] + 1
    n = 2 * R + 1                                                 # every pivot in the last row of the last workgroup
    A = lh.last_row(n, dtype)
    LU, ipiv, _ = ref.factor(A)
    F = pkg.lu(pkg.HipMatrix.from_numpy(A))
    assert (ipiv == n).all() and np.array_equal(F.ipiv, ipiv) and lh.same_bits(F.factors.to_numpy(), LU)
    n = 2 * W + 1
    F = pkg.lu(pkg.HipMatrix.from_numpy(lh.dominant(n, dtype)))
    assert np.array_equal(F.ipiv, np.arange(1, n + 1))            # identity pivots


def test_in_place_views_and_overlap(pkg, ctx, ref, shape):
    W, R, T, _ = shape
    n = 2 * R + W + 1
    for dtype in DTYPES:
        A, LU, ipiv, _, _ = case(pkg, ref, n, dtype)
        M = pkg.HipMatrix.from_numpy(A)
        F = pkg.lu_(M)
        assert F.factors is M and lh.same_bits(M.to_numpy(), LU)                       # lu!(A): in place
        b = lh.vector(n, dtype)
        want = ref.solve(LU, ipiv, b)
        big = pkg.HipVector(3 * n + 40, dtype).fill_(7)
        y, x = big.view(3, n), big.view(n + 9, n)
        x.copy_from_host(b)
        F.ldiv_(y, x)
        h = big.to_numpy()
        assert lh.same_bits(h[3:3 + n], want) and np.array_equal(h[n + 9:2 * n + 9], b)
        untouched = np.ones(3 * n + 40, bool)
        untouched[3:3 + n] = untouched[n + 9:2 * n + 9] = False
        assert (h[untouched] == 7).all()                                               # nothing was stored outside y
        F.ldiv_(x)                                                                     # in place at a non-zero offset
        h = big.to_numpy()
        assert lh.same_bits(h[n + 9:2 * n + 9], want) and (h[untouched] == 7).all()
        with pytest.raises(pkg.MikError) as ei:
            F.ldiv_(big.view(0, n), big.view(5, n))                                    # a partial overlap
        assert ei.value.code == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_singular_exception_with_the_one_based_index(pkg, ctx, dtype):
    n = 300
    for zero in (0.0, -0.0):
        for k in (0, n // 2, n - 1):
            A = lh.zero_column(n, dtype, k, zero)
            if k < n - 1:
                A[:, n - 1] = zero                                                     # a later zero column is not the one reported
            for factor in (pkg.lu, pkg.lu_):
                with pytest.raises(np.linalg.LinAlgError) as ei:
                    factor(pkg.HipMatrix.from_numpy(A))
                assert isinstance(ei.value, pkg.SingularException) and ei.value.col == k + 1 and f"SingularException({k + 1})" in str(ei.value)


def test_refusals(pkg, ctx):
    L, lib = pkg.lib(), pkg._lib
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.lu(pkg.HipMatrix(6, 4))
    for dtype in (np.complex128, np.complex64):
        for factor in (pkg.lu, pkg.lu_):
            with pytest.raises(TypeError, match=np.dtype(dtype).name):
                factor(pkg.HipMatrix(4, 4, dtype))
    A = pkg.HipMatrix.from_numpy(lh.dominant(10, np.float64))
    h, col = C.c_void_p(), C.c_int64()
    for n, ld in ((10, 9), (0, 64), (-1, 64)):
        assert L.mik_dense_lu_create(ctx.handle, C.c_void_p(A.buf.ptr), n, ld, lib.MIK_F64, C.byref(col), C.byref(h)) == 3
    for code, name in ((lib.MIK_C64, "ComplexF64"), (lib.MIK_C32, "ComplexF32")):      # through the C entry: named, not implemented
        assert L.mik_dense_lu_create(ctx.handle, C.c_void_p(A.buf.ptr), 10, A.ld, code, C.byref(col), C.byref(h)) == 5
        assert name in L.mik_last_error(ctx.handle).decode()
    assert np.array_equal(A.to_numpy(), lh.dominant(10, np.float64))                   # a refused call has not touched the matrix
    F = pkg.lu(A)
    v = pkg.HipVector(10).fill_(1)
    for bad in (pkg.HipVector(11).fill_(1), pkg.HipVector(10, np.float32).fill_(1)):
        for call in (lambda: F.ldiv_(v, bad), lambda: F.ldiv_(bad, v), lambda: F.ldiv_(bad), lambda: F.solve(bad)):
            with pytest.raises(ValueError, match="DimensionMismatch"):
                call()
    b = pkg.HipVector(10).fill_(1)
    with pytest.raises(ValueError, match="DimensionMismatch"):                         # the callback never sees a length: checked where it is bound
        pkg.gmres(pkg.HipMatrix.from_numpy(lh.dominant(12, np.float64)), pkg.HipVector(12).fill_(1), Pl=F)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.cg(pkg.HipMatrix.from_numpy(lh.dominant(10, np.float32)), pkg.HipVector(10, np.float32).fill_(1), Pl=F)
    Ac = pkg.HipMatrix.from_numpy(lh.dominant(10, np.float64).astype(np.complex128))
    with pytest.raises(ValueError, match="DimensionMismatch"):                         # a complex solve given a real factorisation
        pkg.gmres(Ac, pkg.HipVector(10, np.complex128).fill_(1), Pl=F)
    assert np.isfinite(F.solve(b).to_numpy()).all()


# ---- as a preconditioner: the reference's statements with the reference's bounds -------------------------------------------------------
def _csr(pkg, orc, A):
    S = orc.CSC.from_dense(A)
    return pkg.HipCSR(S.n, S.n, S.colptr, S.rowval, S.nzval, index_base=S.index_base)


def _orders(shape):
    return (10, 2 * shape[0] + 1)                                                      # the reference's n, and a solve that crosses panels


@pytest.mark.parametrize("dtype", DTYPES)
def test_gmres_exact_left_and_right_preconditioner(pkg, orc, ctx, shape, dtype):
    """test/gmres.jl:28-35 on the matrix as a HipMatrix and as a full HipCSR"""
    reltol = float(np.sqrt(np.finfo(dtype).eps))
    for n in _orders(shape):
        rng = np.random.default_rng(1234321 + n)
        A = (rng.random((n, n)) + np.eye(n)).astype(dtype)
        b = rng.random(n).astype(dtype)
        A64 = A.astype(np.float64)
        F = pkg.lu(pkg.HipMatrix.from_numpy(A))
        db = pkg.HipVector.from_numpy(b)
        for op in (pkg.HipMatrix.from_numpy(A), _csr(pkg, orc, A)):
            x, h = pkg.gmres(op, db, Pl=F, maxiter=1, restart=1, reltol=reltol, log=True)
            assert h.isconverged, (n, type(op).__name__)
            r = F.solve(pkg.HipVector.from_numpy((A64 @ x.to_numpy() - b).astype(dtype))).to_numpy()        # F \ (A x - b)
            assert np.linalg.norm(r.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)) <= reltol, (n, type(op).__name__)
            x, h = pkg.gmres(op, db, Pl=pkg.Identity(), Pr=F, maxiter=1, restart=1, reltol=reltol, log=True)
            assert h.isconverged, (n, type(op).__name__)
            assert np.linalg.norm(A64 @ x.to_numpy() - b) / np.linalg.norm(b.astype(np.float64)) <= reltol, (n, type(op).__name__)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_with_the_factorisation_as_pl_converges_immediately(pkg, ctx, shape, dtype):
    """test/cg.jl:44-47 (a factorisation of A as Pl): niters <= 2, nprods <= 2"""
    for n in _orders(shape):
        rng = np.random.default_rng(1234321 + n)
        M = rng.random((n, n))
        A = (M.T @ M + np.eye(n)).astype(dtype)
        b = rng.random(n).astype(dtype)
        dA = pkg.HipMatrix.from_numpy(A)
        x, ch = pkg.cg(dA, pkg.HipVector.from_numpy(b), Pl=pkg.lu(dA), log=True)
        assert pkg.niters(ch) <= 2 and pkg.nprods(ch) <= 2, (n, pkg.niters(ch), pkg.nprods(ch))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [2, 4])
def test_bicgstabl_with_the_lu_of_a_nearby_matrix(pkg, ctx, ref, shape, dtype, l):
    """test/bicgstabl.jl:40-42.  The reference skips Float32 on Linux because its generator gives a SingularException there; here Float32
    runs with numpy's default_rng(123 + n), for which the checker completes the factorisation (asserted)."""
    reltol = float(np.sqrt(np.finfo(dtype).eps))
    for n in _orders(shape):
        rng = np.random.default_rng(123 + n)
        A = (rng.random((n, n)) + 15 * np.eye(n)).astype(dtype)
        b = (A @ np.ones(n, dtype)).astype(dtype)
        near = (A + rng.random((n, n)).astype(dtype)).astype(dtype)
        assert ref.factor(np.asfortranarray(near))[2] == 0
        F = pkg.lu(pkg.HipMatrix.from_numpy(near))
        # a real solve takes any ldiv_ preconditioner on its statement-by-statement branch, which `ops` selects
        x3, his3 = pkg.bicgstabl(pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b), l, Pl=F, max_mv_products=100, log=True, reltol=reltol,
                                 ops=pkg.DeviceKrylovOps)
        A64 = A.astype(np.float64)
        assert np.linalg.norm(A64 @ x3.to_numpy() - b) / np.linalg.norm(b.astype(np.float64)) <= reltol, (n, l)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inverse_iteration_with_ldiv_as_the_operator(pkg, ctx, dtype):
    """test/simple_eigensolvers.jl:33-48: F = lu(A - sigma I), Fmap = LinearMap((y, x) -> ldiv!(y, F, x)), invpowm(Fmap; shift = sigma)"""
    n = 10
    rng = np.random.default_rng(1234321)
    A = (rng.random((n, n)) + np.eye(n)).astype(dtype)
    A = (A.T @ A).astype(dtype)
    A64 = A.astype(np.float64)
    lams = np.linalg.eigvalsh(A64)
    tol = n ** 2 * np.linalg.cond(A64) * np.finfo(dtype).eps
    idx = n // 2                                                                       # 1-based in the reference
    sigma = dtype(0.75 * lams[idx - 1] + 0.25 * lams[idx])
    F = pkg.lu(pkg.HipMatrix.from_numpy((A - sigma * np.eye(n, dtype=dtype)).astype(dtype)))
    Fmap = pkg.LinearOperator(n, dtype, F.ldiv_)
    x0 = pkg.HipVector.from_numpy(rng.random(n).astype(dtype))
    lam, x, history = pkg.extras.invpowm_(Fmap, x0, shift=sigma, tol=tol, maxiter=10 * n, log=True)
    assert isinstance(history, pkg.ConvergenceHistory)
    xh = x.to_numpy().astype(np.float64)
    assert np.linalg.norm(A64 @ xh - float(lam) * xh) <= tol
    assert abs(float(lam) - lams[idx - 1]) <= np.sqrt(np.finfo(dtype).eps) * max(abs(float(lam)), abs(lams[idx - 1]))      # isapprox


# ---- the library callback is the Python route ---------------------------------------------------------------------------------------------
class PlainLdiv:
    """a preconditioner that is NOT a DenseLU for the library: only ldiv_(y, x), like any user type"""

    def __init__(self, F):
        self.F = F
        self.calls = 0

    def ldiv_(self, y, x=None):
        self.calls += 1
        return self.F.ldiv_(y, x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_solvers_reach_the_factorisation_without_a_python_frame(pkg, ctx, shape, dtype, monkeypatch):
    n = 2 * shape[0] + 1
    rng = np.random.default_rng(99)
    A = (rng.random((n, n)) + np.eye(n)).astype(dtype)
    b = rng.random(n).astype(dtype)
    F = pkg.lu(pkg.HipMatrix.from_numpy((A + 0.3 * rng.random((n, n))).astype(dtype)))           # nearby: several iterations
    calls = {"n": 0}
    inner = pkg.DenseLU.ldiv_

    def counted(self, y, x=None):
        calls["n"] += 1
        return inner(self, y, x)
    dA, db = pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b)
    M = rng.random((n, n))
    S = (M.T @ M / n + np.eye(n)).astype(dtype)
    G = pkg.lu(pkg.HipMatrix.from_numpy((S + 0.05 * np.diag(rng.random(n))).astype(dtype)))
    dS = pkg.HipMatrix.from_numpy(S)
    plain_f, plain_g = PlainLdiv(F), PlainLdiv(G)
    x1, h1 = pkg.gmres(dA, db, Pl=plain_f, restart=8, maxiter=24, log=True)
    y1, g1 = pkg.cg(dS, db, Pl=plain_g, maxiter=12, log=True)
    assert plain_f.calls > 1 and plain_g.calls > 1 and h1.iters > 1 and g1.iters > 1
    monkeypatch.setattr(pkg.DenseLU, "ldiv_", counted)
    x0, h0 = pkg.gmres(dA, db, Pl=F, restart=8, maxiter=24, log=True)
    y0, g0 = pkg.cg(dS, db, Pl=G, maxiter=12, log=True)
    assert calls["n"] == 0                                                             # no Python frame per ldiv!
    assert np.array_equal(h0["resnorm"], h1["resnorm"]) and np.array_equal(x0.to_numpy(), x1.to_numpy()) and h0.mvps == h1.mvps
    assert np.array_equal(g0["resnorm"], g1["resnorm"]) and np.array_equal(y0.to_numpy(), y1.to_numpy()) and g0.mvps == g1.mvps
