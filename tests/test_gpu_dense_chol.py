"""cholesky(A) / cholesky_(A) on a dense device matrix and ldiv_ (iterativesolvers.jl_amd/dense_chol.py over the mik_dense_chol_* entries)
in Float64, Float32, ComplexF64 and ComplexF32, bit for bit against tests/dense_ref/dense_chol_ref.c -- the contract's unblocked loops
restated in C.  Every comparison of device values with the checker's is dense_chol_host.same_bits (NaN positions, and the bits everywhere
else: -0.0 is not +0.0); comparisons with a fixture's construction are np.array_equal.  Every shape comes from mik_dense_chol_info
(F.plan()).  Every width of a last panel, extreme magnitudes, poisoned unread parts, any ld and non-finite right-hand sides are in
test_gpu_dense_chol_edges.py.  The reference's own statements with cholesky(A) as Pl carry the reference's own bounds."""
import ctypes as C

import numpy as np
import pytest

import dense_chol_host as ch

pytestmark = pytest.mark.gpu

DTYPES = ch.DTYPES


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("dense_chol_ref_gpu"))


@pytest.fixture(scope="module")
def shapes(pkg, ctx):
    """per element type (W, R, T): panel width, rows per workgroup of the panel kernel, the larger tile edge of the trailing update"""
    out = {}
    for dtype in DTYPES:
        p = pkg.cholesky(pkg.HipMatrix.from_numpy(np.ones((1, 1), dtype))).plan()
        assert p["W"] >= 2 and p["R"] >= 2 and p["tile_rows"] >= 2 and p["tile_cols"] >= 2
        assert p["launches_factor"] == 1 and p["launches_solve"] == 2 and p["info"] == 0
        out[np.dtype(dtype).name] = (p["W"], p["R"], max(p["tile_rows"], p["tile_cols"]))
    return out


def shape_of(shapes, dtype):
    return shapes[np.dtype(dtype).name]


def sizes(shape):
    W, R, T = shape
    return sorted({1, 2, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3, R - 1, R, R + 1, 2 * R + W + 1, T - 1, T, T + 1})


_CASES = {}


def case(pkg, ref, n, dtype):
    """(A, the checker's array, the device matrix holding A, the device factorisation of a copy of A) -- computed once per size and type"""
    key = (n, np.dtype(dtype).name)
    if key not in _CASES:
        A = ch.hpd(n, dtype)
        out, info = ref.factor(A)
        assert info == 0 and np.isfinite(out).all()
        M = pkg.HipMatrix.from_numpy(A)
        _CASES[key] = (A, out, M, pkg.cholesky(M))
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_bit_for_bit(pkg, ctx, ref, shapes, dtype):
    W = shape_of(shapes, dtype)[0]
    for n in sizes(shape_of(shapes, dtype)):
        A, out, M, F = case(pkg, ref, n, dtype)
        p = F.plan()
        assert p["launches_factor"] == ch.plan_launches(n, W) and p["launches_solve"] == 2 * -(-n // W), n
        assert F.n == n and F.dtype == np.dtype(dtype) and F.uplo == "L" and F.info == 0 and p["info"] == 0 and F.issuccess()
        got = F.factors.to_numpy()
        assert ch.same_bits(got, out), f"factor differs, n = {n}, {np.dtype(dtype)}, first at {ch.first_difference(got, out)}"
        iu = np.triu_indices(n, 1)
        assert ch.same_bits(got[iu], A[iu])                                            # the strict upper triangle: the input's bits
        assert F.factors is not M and np.array_equal(M.to_numpy(), A)                  # cholesky(A) leaves A untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_ldiv_bit_for_bit(pkg, ctx, ref, shapes, dtype):
    for n in sizes(shape_of(shapes, dtype)):
        A, out, M, F = case(pkg, ref, n, dtype)
        b = ch.vector(n, dtype)
        want = ref.solve(out, b)
        assert np.isfinite(want).all()
        x, y = pkg.HipVector.from_numpy(b), pkg.HipVector(n, dtype).fill_(0)
        assert F.ldiv_(y, x) is y
        assert ch.same_bits(y.to_numpy(), want), (n, ch.first_difference(y.to_numpy(), want))
        assert np.array_equal(x.to_numpy(), b)                                         # x is untouched in the two-argument form
        assert F.ldiv_(x) is x and ch.same_bits(x.to_numpy(), want)                    # ldiv!(F, x)
        s = F.solve(pkg.HipVector.from_numpy(b))
        assert s is not y and ch.same_bits(s.to_numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_fixture_on_the_device(pkg, ctx, dtype):
    """equality, not a tolerance: the factor is L, the solve returns x"""
    n = 130
    A, L, x, b = ch.exact(n, dtype)
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
    assert np.array_equal(ch.lower(F.factors.to_numpy()), L)
    assert np.array_equal(F.solve(pkg.HipVector.from_numpy(b)).to_numpy(), x)


def test_in_place_views_and_overlap(pkg, ctx, ref, shapes):
    for dtype in DTYPES:
        W, R, T = shape_of(shapes, dtype)
        n = 2 * R + W + 1
        A, out, _, _ = case(pkg, ref, n, dtype)
        M = pkg.HipMatrix.from_numpy(A)
        F = pkg.cholesky_(M)
        assert F.factors is M and ch.same_bits(M.to_numpy(), out)                      # cholesky!(A): in place
        b = ch.vector(n, dtype)
        want = ref.solve(out, b)
        big = pkg.HipVector(3 * n + 40, dtype).fill_(7)
        y, x = big.view(3, n), big.view(n + 9, n)
        x.copy_from_host(b)
        F.ldiv_(y, x)
        h = big.to_numpy()
        assert ch.same_bits(h[3:3 + n], want) and np.array_equal(h[n + 9:2 * n + 9], b)
        untouched = np.ones(3 * n + 40, bool)
        untouched[3:3 + n] = untouched[n + 9:2 * n + 9] = False
        assert (h[untouched] == 7).all()                                               # nothing was stored outside y
        F.ldiv_(x)                                                                     # in place at a non-zero offset
        h = big.to_numpy()
        assert ch.same_bits(h[n + 9:2 * n + 9], want) and (h[untouched] == 7).all()
        with pytest.raises(pkg.MikError) as ei:
            F.ldiv_(big.view(0, n), big.view(5, n))                                    # a partial overlap
        assert ei.value.code == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ch.FAILURES)
def test_posdef_exception_with_the_one_based_index(pkg, ctx, ref, shapes, dtype, kind):
    L, lib = pkg.lib(), pkg._lib
    n, W = 130, shape_of(shapes, dtype)[0]
    for k in ch.failure_columns(n, W):
        A, out, info = ch.failing_case(ref, n, dtype, k, kind)
        M = pkg.HipMatrix.from_numpy(A)
        for factor in (pkg.cholesky, pkg.cholesky_):
            with pytest.raises(np.linalg.LinAlgError) as ei:
                factor(pkg.HipMatrix.from_numpy(A))
            assert isinstance(ei.value, pkg.PosDefException) and ei.value.k == info and f"PosDefException({info})" in str(ei.value), (k, kind)
        with pytest.raises(pkg.PosDefException):
            pkg.cholesky(M)
        assert ch.same_bits(M.to_numpy(), A)                                           # after a failed cholesky(A), A is untouched
        F = pkg.cholesky(M, check=False)                                               # no exception
        assert F.info == info and F.plan()["info"] == info and not F.issuccess()
        got = F.factors.to_numpy()
        assert ch.same_bits(ch.lower(got)[:, :k], ch.lower(out)[:, :k])                # the columns before the failure are complete
        v = pkg.HipVector(n, dtype).fill_(1)
        with pytest.raises(pkg.MikError) as ei:
            F.ldiv_(v)
        assert ei.value.code == 1
        assert L.mik_dense_chol_solve(F.handle, C.c_void_p(v.ptr), C.c_void_p(v.ptr)) == 1         # the C entry refuses it too
        h, col = C.c_void_p(), C.c_int64()
        D = pkg.HipMatrix.from_numpy(A)
        assert L.mik_dense_chol_create(ctx.handle, C.c_void_p(D.buf.ptr), n, D.ld, lib.dtype_code(np.dtype(dtype)), 1, C.byref(col), C.byref(h)) == 8
        assert col.value == info and not h.value and f"PosDefException({info})" in L.mik_last_error(ctx.handle).decode()


def test_refusals(pkg, ctx, ref):
    L, lib = pkg.lib(), pkg._lib
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.cholesky(pkg.HipMatrix(6, 4))
    with pytest.raises(TypeError):
        pkg.cholesky(np.eye(3))
    A0 = ch.hpd(10, np.float64)
    A = pkg.HipMatrix.from_numpy(A0)
    h, col = C.c_void_p(), C.c_int64()
    for n, ld in ((10, 9), (0, 64), (-1, 64)):
        assert L.mik_dense_chol_create(ctx.handle, C.c_void_p(A.buf.ptr), n, ld, lib.MIK_F64, 1, C.byref(col), C.byref(h)) == 3
    assert L.mik_dense_chol_create(ctx.handle, C.c_void_p(A.buf.ptr), 2 ** 31 - 64, 2 ** 31, lib.MIK_F64, 1, C.byref(col), C.byref(h)) == 5
    assert np.array_equal(A.to_numpy(), A0)                                            # a refused call has not touched the matrix
    F = pkg.cholesky(A)
    v = pkg.HipVector(10).fill_(1)
    for bad in (pkg.HipVector(11).fill_(1), pkg.HipVector(10, np.float32).fill_(1), pkg.HipVector(10, np.complex128).fill_(1)):
        for call in (lambda: F.ldiv_(v, bad), lambda: F.ldiv_(bad, v), lambda: F.ldiv_(bad), lambda: F.solve(bad)):
            with pytest.raises(ValueError, match="DimensionMismatch"):
                call()
    # as Pl: the callback never sees a length or a type, so they are checked where it is bound
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.cg(pkg.HipMatrix.from_numpy(ch.hpd(12, np.float64)), pkg.HipVector(12).fill_(1), Pl=F)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.gmres(pkg.HipMatrix.from_numpy(ch.hpd(10, np.float32)), pkg.HipVector(10, np.float32).fill_(1), Pl=F)
    with pytest.raises(ValueError, match="DimensionMismatch"):                         # a complex solve given a real factorisation
        pkg.cg(pkg.HipMatrix.from_numpy(ch.hpd(10, np.complex128)), pkg.HipVector(10, np.complex128).fill_(1), Pl=F)
    assert np.isfinite(F.solve(v).to_numpy()).all()


# ---- what is read and what is not ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_upper_triangle_and_padding_rows(pkg, ctx, ref, shapes, dtype):
    """The strict upper triangle and the rows [n, ld) of every column are NaN: the factor and the solve are those of the clean matrix, so
    neither region is read; and not one bit of either is written."""
    W, R, T = shape_of(shapes, dtype)
    n = 2 * R + W + 1
    A, out, _, _ = case(pkg, ref, n, dtype)
    P = ch.poisoned(A)
    M = pkg.HipMatrix(n, n, dtype)
    assert M.ld > n
    nan = np.dtype(dtype).type(np.nan * (1 + 1j) if ch.is_complex(dtype) else np.nan)
    host = np.full((M.ld, n), nan, dtype, order="F")
    host[:n, :] = P
    M.buf.copy_from_host(host.ravel(order="F"))
    F = pkg.cholesky_(M)
    back = M.buf.to_numpy().reshape((M.ld, n), order="F")
    assert F.info == 0
    assert ch.same_bits(ch.lower(back[:n, :]), ch.lower(out)), ch.first_difference(ch.lower(back[:n, :]), ch.lower(out))
    iu = np.triu_indices(n, 1)
    assert np.array_equal(_bits(back[:n, :][iu]), _bits(host[:n, :][iu])) and np.array_equal(_bits(back[n:, :]), _bits(host[n:, :]))
    b = ch.vector(n, dtype)
    assert ch.same_bits(F.solve(pkg.HipVector.from_numpy(b)).to_numpy(), ref.solve(out, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_entries_follow_the_checker(pkg, ctx, ref, shapes, dtype):
    """An Inf on the diagonal is a positive pivot (its column becomes 0 or NaN as the divisions say); a NaN below the diagonal reaches the
    pivot of its row and fails that column.  The kernels index nothing through a value, so both simply run."""
    W, R, T = shape_of(shapes, dtype)
    n = 2 * W + 1
    A = ch.hpd(n, dtype)
    A[W + 3, W + 3] = np.inf
    out, info = ref.factor(A)
    assert info == 0 and not np.isfinite(ch.lower(out)).all()
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
    got = F.factors.to_numpy()
    assert F.info == 0 and ch.same_bits(ch.lower(got), ch.lower(out)), ch.first_difference(ch.lower(got), ch.lower(out))
    b = ch.vector(n, dtype)
    assert ch.same_bits(F.solve(pkg.HipVector.from_numpy(b)).to_numpy(), ref.solve(out, b))
    A = ch.hpd(n, dtype)
    A[W + 5, 2] = np.nan
    out, info = ref.factor(A)
    assert info == W + 6
    with pytest.raises(pkg.PosDefException) as ei:
        pkg.cholesky(pkg.HipMatrix.from_numpy(A))
    assert ei.value.k == info
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A), check=False)
    got = F.factors.to_numpy()
    assert F.info == info and ch.same_bits(ch.lower(got)[:, :info - 1], ch.lower(out)[:, :info - 1])


# ---- as a preconditioner: the reference's statements with the reference's bounds -------------------------------------------------------
def _uniform(rng, shape, dtype):
    v = rng.random(shape)
    return (v + 1j * rng.random(shape) if ch.is_complex(dtype) else v).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cg_with_cholesky_as_pl_converges_immediately(pkg, ctx, shapes, dtype, monkeypatch):
    """test/cg.jl:44-47: F = cholesky(A, Val(false)); cg(A, b; Pl=F): niters <= 2, nprods <= 2.  The real types reach the factorisation
    through the library's own callback (no Python frame per ldiv!), the complex types through the generic iterable's ldiv_."""
    calls = {"n": 0}
    inner = pkg.DenseCholesky.ldiv_

    def counted(self, y, x=None):
        calls["n"] += 1
        return inner(self, y, x)
    monkeypatch.setattr(pkg.DenseCholesky, "ldiv_", counted)
    for n in (10, 2 * shape_of(shapes, dtype)[0] + 1):
        rng = np.random.default_rng(1234321 + n)
        M = _uniform(rng, (n, n), dtype)
        A = (M.conj().T @ M + np.eye(n)).astype(dtype)
        b = _uniform(rng, n, dtype)
        dA = pkg.HipMatrix.from_numpy(A)
        calls["n"] = 0
        x, h = pkg.cg(dA, pkg.HipVector.from_numpy(b), Pl=pkg.cholesky(dA), log=True)
        assert pkg.niters(h) <= 2 and pkg.nprods(h) <= 2, (n, pkg.niters(h), pkg.nprods(h))
        assert (calls["n"] > 0) == ch.is_complex(dtype), (n, calls["n"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_chebyshev_with_cholesky_as_pl(pkg, ctx, dtype):
    """test/chebyshev.jl:59-66: B_fact = cholesky!(B, Val(false)); bounds from the eigenvalues of B \\ A; converged, and
    norm(A x - b) / norm(b) <= sqrt(eps(real(T)))"""
    n = 10
    rng = np.random.default_rng(1234321)
    wide = np.complex128 if ch.is_complex(dtype) else np.float64

    def rand_spd():
        G = (_uniform(rng, (n, n), dtype) + n * np.eye(n)).astype(dtype)
        return (G.conj().T @ G).astype(dtype)
    A, b, B = rand_spd(), _uniform(rng, n, dtype), rand_spd()
    reltol = float(np.sqrt(np.finfo(ch.real_of(dtype)).eps))
    ev = np.linalg.eigvals(np.linalg.solve(B.astype(wide), A.astype(wide))).real        # approx_eigenvalue_bounds(B_fact \ A), :13-18
    d = (ev.max() - ev.min()) / 100
    dB = pkg.HipMatrix.from_numpy(B)
    F = pkg.cholesky_(dB)
    assert F.factors is dB and F.issuccess()
    # a real solve takes any ldiv_ preconditioner on its statement-by-statement branch, which `ops` selects; a complex one is always there
    x, h = pkg.chebyshev(pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b), ev.min() - d, ev.max() + d, Pl=F, reltol=reltol, maxiter=10 * n, log=True,
                         ops=pkg.DeviceKrylovOps)
    assert h.isconverged
    assert np.linalg.norm(A.astype(wide) @ x.to_numpy().astype(wide) - b.astype(wide)) / np.linalg.norm(b.astype(wide)) <= reltol
