"""lu(A) / lu_(A) / ldiv_ where test_gpu_dense_lu.py's standard-normal matrices never go: NaN and Inf in the searched column and in the
right-hand side, the sign of zero, poisoned padding rows, leading dimensions that are no multiple of 64, pivot ties in the columns the
fused search and a later panel's search see, subnormal and near-overflow magnitudes.  Every comparison with the checker
(tests/dense_ref/dense_lu_ref.c) is dense_lu_host.same_bits: no tolerance anywhere.  Every fixture comes from a dense_lu_host.*_case
function, which first asserts on the checker what the fixture exists for, at the W and R mik_dense_lu_info reports."""
import ctypes as C

import numpy as np
import pytest

import dense_lu_host as lh

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lh.build(tmp_path_factory.mktemp("dense_lu_ref_gpu_edges"))


@pytest.fixture(scope="module")
def shape(pkg, ctx):
    """(W, R): panel width, rows per workgroup of the pivot search"""
    info = pkg.lu(pkg.HipMatrix.from_numpy(np.ones((1, 1)))).info()
    assert info["W"] >= 4 and info["R"] >= 64 and info["R"] % 2 == 0
    return info["W"], info["R"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def poisons(dtype):
    return (np.nan, np.inf, np.finfo(dtype).max)


def agree(pkg, ref, A, LU, ipiv, tag, column=None, row=None):
    """lu of a copy of A: the pivot of `column` is `row` (1-based; asserted outright, ahead of the rest), and the pivots, the factors and
    the solve of one finite b are the checker's.  Returns the factorisation."""
    n, dtype = A.shape[0], A.dtype
    F = pkg.lu(pkg.HipMatrix.from_numpy(A))
    if column is not None:
        assert F.ipiv[column] == row, f"{tag}: the loop takes row {row} as the pivot of column {column + 1}, the device row {F.ipiv[column]} (1-based)"
    assert np.array_equal(F.ipiv, ipiv), (tag, "ipiv differs first at", np.flatnonzero(F.ipiv != ipiv)[:4].tolist())
    got = F.factors.to_numpy()
    assert lh.same_bits(got, LU), (tag, "factors differ first at", lh.first_difference(got, LU))
    b = lh.vector(n, dtype)
    y = F.solve(pkg.HipVector.from_numpy(b)).to_numpy()
    want = ref.solve(LU, ipiv, b)
    assert lh.same_bits(y, want), (tag, "solution differs first at", lh.first_difference(y, want))
    return F


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("column", range(4))
def test_a_nan_hides_no_candidate_and_wins_only_in_the_first_row(pkg, ctx, ref, shape, dtype, column):
    """The loop skips a NaN below the first searched row and keeps one in the first row.  Columns 0, 1, W - 1, W: the stand-alone search,
    the fused search, the last column of a panel, the stand-alone search of a later panel."""
    W, R = shape
    c = lh.lead_columns(W)[column]
    for nan_off, max_off in lh.nan_hidden_offsets(R):
        A, LU, ipiv = lh.nan_hidden_case(ref, dtype, c, R, nan_off, max_off)
        agree(pkg, ref, A, LU, ipiv, f"NaN at +{nan_off}, 5.0 at +{max_off}", c, c + max_off + 1)
    for whole_column in (False, True):
        A, LU, ipiv = lh.nan_pivot_case(ref, dtype, c, R, whole_column)
        agree(pkg, ref, A, LU, ipiv, "NaN column" if whole_column else "NaN above 5.0 and -7.0", c, c + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_of_both_signs_in_one_column(pkg, ctx, ref, shape, dtype):
    A, LU, ipiv = lh.inf_pair_case(ref, dtype, shape[1])
    agree(pkg, ref, A, LU, ipiv, "+Inf in row 5, -Inf in row R + 3", 0, 6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_zero_column_with_a_nan_in_it(pkg, ctx, ref, shape, dtype, zero):
    """best == 0 with a NaN elsewhere in the column is SingularException(k + 1); a NaN in the first searched row is not"""
    W, R = shape
    for k in (0, 1, W):
        n = k + R + 7
        for nan_off in (0, 1, R, R + 2):
            A, LU, ipiv, singular = lh.zero_nan_case(ref, dtype, k, n, nan_off, zero)
            if singular:
                with pytest.raises(np.linalg.LinAlgError) as ei:
                    pkg.lu(pkg.HipMatrix.from_numpy(A))
                assert isinstance(ei.value, pkg.SingularException) and ei.value.col == k + 1, (k, nan_off, zero)
            else:
                F = pkg.lu(pkg.HipMatrix.from_numpy(A))                                 # no exception
                got = F.factors.to_numpy()
                assert np.array_equal(F.ipiv, ipiv) and lh.same_bits(got, LU), (k, zero, lh.first_difference(got, LU))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("column", range(4))
def test_pivot_ties_after_column_zero(pkg, ctx, ref, shape, dtype, column):
    """the first of four equal magnitudes in four workgroups, in the fused search (columns 1, W - 1, W + 1) and in a later panel's own (W)"""
    W, R = shape
    c = (1, W - 1, W, W + 1)[column]
    A, LU, ipiv, rows = lh.late_ties_case(ref, dtype, c, R)
    agree(pkg, ref, A, LU, ipiv, "ties", c, rows[0] + 1)
    A, LU, ipiv, rows = lh.late_ties_case(ref, dtype, c, R, drop=2)                     # ... also with no candidate in the first workgroups
    assert pkg.lu(pkg.HipMatrix.from_numpy(A)).ipiv[c] == rows[0] + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_subnormal_and_near_overflow_magnitudes(pkg, ctx, ref, shape, dtype):
    for which in (0, 1):
        A, LU, ipiv = lh.scaled_case(ref, dtype, shape[0], which)
        agree(pkg, ref, A, LU, ipiv, ("scale", lh.scales(dtype)[which]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_right_hand_side_on_finite_factors(pkg, ctx, ref, shape, dtype):
    """+Inf, NaN and -0.0 in b.  The exact fixture's L holds exact zeros, so 0 * Inf arises -- in the checker and on the device alike.  An
    Inf or a NaN anywhere in b makes the whole solution NaN once the backward chain has met it, so one more b carries its Inf where only
    the last row of the forward chain sees it, and a b of -0.0 alone gives a solution of zeros of both signs."""
    W = shape[0]
    for name, A in (("exact", lh.exact(130, dtype)[0]), ("random", lh.random(2 * W + 1, dtype))):
        n = A.shape[0]
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0 and np.isfinite(LU).all()
        F = agree(pkg, ref, A, LU, ipiv, name)
        rhs = {key: lh.vector(n, dtype) for key in ("inf", "nan", "some -0.0")}
        rhs["inf"][n // 3] = np.inf
        rhs["nan"][2 * n // 3] = np.nan
        rhs["some -0.0"][::3] = -0.0
        rhs["all -0.0"] = np.full(n, -0.0, dtype)
        rhs["inf last"] = lh.vector(n, dtype)                                           # reaches only the last row of the forward chain,
        rhs["inf last"][lh.permutation_of(ipiv)[n - 1]] = np.inf                        # so the backward one starts from a signed Inf
        for key, b in rhs.items():
            want = ref.solve(LU, ipiv, b)
            if key == "inf last":
                assert np.isinf(want[n - 1]) and np.isnan(want).any()                   # Inf - Inf, and on the exact fixture 0 * Inf
            if key == "all -0.0":
                assert (want == 0).all() and np.signbit(want).any() and not np.signbit(want).all()
            x, y = pkg.HipVector.from_numpy(b), pkg.HipVector(n, dtype).fill_(7)
            assert F.ldiv_(y, x) is y
            got = y.to_numpy()
            assert lh.same_bits(got, want), (name, key, lh.first_difference(got, want))
            assert lh.same_bits(x.to_numpy(), b)                                        # x is untouched in the two-argument form
            assert lh.same_bits(F.ldiv_(x).to_numpy(), want), (name, key, "ldiv_(x)")
            assert lh.same_bits(F.solve(pkg.HipVector.from_numpy(b)).to_numpy(), want), (name, key, "solve")


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_padding_rows_of_a_hipmatrix(pkg, ctx, ref, shape, dtype):
    """HipMatrix zero-fills the rows [n, ld) of every column, so a lane that read past row n would go unseen: fill them with NaN, +Inf and
    the largest finite value instead.  Nothing of them may reach the factors, and none may be written."""
    W, R = shape
    for n in (R + 1, 2 * R + W + 1):
        A = lh.random(n, dtype)
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0
        for poison in poisons(dtype):
            M = pkg.HipMatrix(n, n, dtype)
            assert M.ld > n
            host = np.full((M.ld, n), poison, dtype, order="F")
            host[:n, :] = A
            M.buf.copy_from_host(host.ravel(order="F"))
            F = pkg.lu_(M)
            back = M.buf.to_numpy().reshape((M.ld, n), order="F")
            assert np.array_equal(F.ipiv, ipiv), (n, poison, np.flatnonzero(F.ipiv != ipiv)[:4].tolist())
            assert lh.same_bits(back[:n, :], LU), (n, poison, lh.first_difference(back[:n, :], LU))
            assert np.array_equal(bits(back[n:, :]), bits(host[n:, :])), (n, poison)


@pytest.mark.parametrize("dtype", DTYPES)
def test_leading_dimensions_through_the_c_entry(pkg, ctx, ref, shape, dtype):
    """The C entry takes any ld >= n: ld = n (odd: column starts aligned to the element only), n + 1, 2 n + 3.  The padding rows and 64
    elements before and after the matrix are poisoned; the vectors sit at odd element offsets between poisoned elements."""
    L, lib = pkg.lib(), pkg._lib
    n = shape[0] + 1
    A, b = lh.random(n, dtype), lh.vector(n, dtype)
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0
    want = ref.solve(LU, ipiv, b)
    xo, yo = 3, (n + 9) | 1
    for ld in (n, n + 1, 2 * n + 3):
        for poison in poisons(dtype):
            host = np.full(64 + ld * n + 64, poison, dtype)
            mat = host[64:64 + ld * n].reshape((ld, n), order="F")                       # a view
            mat[:n, :] = A
            inside = np.zeros(host.size, bool)
            inside[64:64 + ld * n].reshape((ld, n), order="F")[:n, :] = True
            assert np.shares_memory(mat, host) and inside.sum() == n * n
            vhost = np.full(2 * n + 40, poison, dtype)
            vhost[xo:xo + n] = b
            big, vecs = pkg.HipVector.from_numpy(host), pkg.HipVector.from_numpy(vhost)
            x, y = vecs.view(xo, n), vecs.view(yo, n)
            h, col = C.c_void_p(), C.c_int64()
            assert L.mik_dense_lu_create(ctx.handle, C.c_void_p(big.view(64, ld * n).ptr), n, ld, lib.dtype_code(dtype), C.byref(col), C.byref(h)) == 0
            try:
                got_ipiv = np.zeros(n, np.int64)
                assert col.value == 0 and L.mik_dense_lu_ipiv(h, got_ipiv.ctypes.data_as(C.POINTER(C.c_int64))) == 0
                assert L.mik_dense_lu_solve(h, C.c_void_p(y.ptr), C.c_void_p(x.ptr)) == 0
                back, vback = big.to_numpy(), vecs.to_numpy()
            finally:
                assert L.mik_dense_lu_destroy(h) == 0
            tag = (ld, poison)
            assert np.array_equal(got_ipiv, ipiv), tag
            got = back[64:64 + ld * n].reshape((ld, n), order="F")[:n, :]
            assert lh.same_bits(got, LU), (tag, lh.first_difference(got, LU))
            assert np.array_equal(bits(back)[~inside], bits(host)[~inside]), tag        # padding, before and after: not one bit written
            assert lh.same_bits(vback[yo:yo + n], want), (tag, lh.first_difference(vback[yo:yo + n], want))
            vhost[yo:yo + n] = vback[yo:yo + n]
            assert np.array_equal(bits(vback), bits(vhost)), tag                        # x and every poisoned element around both vectors
