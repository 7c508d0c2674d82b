"""The checker of the dense LU tests (tests/dense_ref/dense_lu_ref.c, the bit contract restated as unblocked loops) against what needs no
device: the library's host loop mik_lu_solve, the exactly representable fixture, the pivot-rule fixtures, a blocked numpy plan, and the
conditions of the non-finite, tied and scaled fixtures of the device tests.  Comparisons on finite data are np.array_equal; where a NaN
or the sign of a zero matters they are dense_lu_host.same_bits."""
import numpy as np
import pytest

import dense_lu_host as lh

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lh.build(tmp_path_factory.mktemp("dense_lu_ref"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_equals_the_host_loop_of_the_library(pkg, ref, dtype):
    """mik_lu_solve (csrc/mik_krylov.hip, lu_solve<T>) is the loop the contract names: same factors, same x"""
    for n in (1, 2, 3, 10, 65, 130):
        A, b = lh.random(n, dtype), lh.vector(n, dtype)
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0
        Ah, bh = A.copy(order="F"), b.copy()
        pkg.lu_solve_(Ah, bh)
        assert np.array_equal(Ah, LU), (n, dtype)
        assert np.array_equal(bh, ref.solve(LU, ipiv, b)), (n, dtype)
        assert np.isfinite(bh).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_is_independent_of_the_leading_dimension(ref, dtype):
    A = lh.random(70, dtype)
    a, b = ref.factor(A), ref.factor(A, ld=128)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_on_the_exact_fixture(ref, dtype):
    """the anchor that shares no code with anything: the interchanges are the permutation, the factors are L and U, the solve returns x"""
    for n in (1, 2, 7, 24, 65, 130):
        A, L, U, rows, x, b = lh.exact(n, dtype)
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0
        assert np.array_equal(lh.permutation_of(ipiv), rows), n
        assert np.array_equal(np.tril(LU, -1) + np.eye(n, dtype=dtype), L) and np.array_equal(np.triu(LU), U), n
        assert np.array_equal(ref.solve(LU, ipiv, b), x), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_pivot_rules(ref, dtype):
    n = 600
    rows = (17, 300, 301, 599)
    _, ipiv, singular = ref.factor(lh.ties(n, dtype, rows))
    assert singular == 0 and ipiv[0] == rows[0] + 1                         # the first of the equal magnitudes
    for n in (2, 65, 513):
        _, ipiv, singular = ref.factor(lh.last_row(n, dtype))
        assert singular == 0 and (ipiv == n).all(), n
    for n in (1, 2, 65, 300):
        _, ipiv, singular = ref.factor(lh.dominant(n, dtype))
        assert singular == 0 and np.array_equal(ipiv, np.arange(1, n + 1)), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_reports_the_first_zero_pivot_column(ref, dtype):
    n = 40
    for zero in (0.0, -0.0):
        for k in (0, n // 2, n - 1):
            A = lh.zero_column(n, dtype, k, zero)
            if k < n - 1:
                A[:, n - 1] = zero                                          # a later zero column is not the one reported
            assert ref.factor(A)[2] == k + 1, (k, zero)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W", [1, 4, 8])
def test_a_blocked_plan_has_the_bits_of_the_unblocked_loop(ref, dtype, W):
    """panels of W columns, interchanges outside the panel, strip solve, trailing update: k stays ascending per element.  Finite data
    only, and not to be extended to NaN: blocked() finds its pivot with np.argmax, which returns the first NaN and is not the loop."""
    for n in (1, 2, 7, 8, 9, 30):
        A = lh.random(n, dtype)
        LU, ipiv, _ = ref.factor(A)
        Lb, pb = lh.blocked(A, W)
        assert Lb.dtype == dtype and np.array_equal(pb, ipiv) and np.array_equal(Lb, LU), (n, W)


# ---- the non-finite, tied and scaled fixtures: the conditions each exists for, on the checker ------------------------------------------
# The device tests call the same *_case functions at the shapes mik_dense_lu_info reports; no device is open here, so these run at the
# shapes the kernels are written for today.  The conditions themselves hold at any W and R.
W, R = 64, 256


def test_same_bits():
    for dtype in DTYPES:
        a = np.array([1.0, -0.0, 0.0, np.nan, np.inf, -np.inf], dtype)
        assert lh.same_bits(a, a.copy()) and lh.first_difference(a, a.copy()) == []
        b = a.copy()
        b[3] = -np.nan                                                      # the sign and the payload of a NaN are not compared
        b.view(np.uint64 if dtype == np.float64 else np.uint32)[3] |= 1
        assert np.isnan(b[3]) and lh.same_bits(a, b)
        for i, v in ((1, 0.0), (2, -0.0), (3, 1.0), (0, np.nan), (4, -np.inf), (0, np.nextafter(dtype(1), dtype(2)))):
            b = a.copy()
            b[i] = v
            assert not lh.same_bits(a, b) and lh.first_difference(a, b) == [[i]], (i, v)
        assert np.array_equal(a[:3], np.array([1.0, 0.0, -0.0], dtype))      # what np.array_equal does not see
        assert not lh.same_bits(a, a[:5]) and not lh.same_bits(a, a.astype(np.float32 if dtype == np.float64 else np.float64))
    assert not lh.same_bits(np.arange(3), np.arange(3))                     # floating point only


@pytest.mark.parametrize("dtype", DTYPES)
def test_lead_keeps_the_trailing_block(ref, dtype):
    for c in (1, W - 1, W + 1):
        n = c + 9
        A = lh.lead(n, dtype, c)
        LU, ipiv, singular = ref.factor(A)
        assert singular == 0 and np.array_equal(ipiv[:c], np.arange(1, c + 1))
        assert lh.same_bits(LU[:c, :], A[:c, :]) and (LU[c:, :c] == 0).all()              # steps 0 .. c - 1 changed nothing
        assert lh.same_bits(LU[c:, c:], ref.factor(np.asfortranarray(A[c:, c:]))[0])      # column c was searched as the fixture left it


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", lh.lead_columns(W))
def test_nan_fixtures(ref, dtype, c):
    for nan_off, max_off in lh.nan_hidden_offsets(R):
        A, LU, ipiv = lh.nan_hidden_case(ref, dtype, c, R, nan_off, max_off)
        assert np.isfinite(LU).all(axis=1).sum() == c + nan_off
    assert sum(nan_off >= 100 for nan_off, _ in lh.nan_hidden_offsets(R)) >= 2             # the comparison is not mostly NaN
    for whole_column in (False, True):
        lh.nan_pivot_case(ref, dtype, c, R, whole_column)


@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_fixture(ref, dtype):
    lh.inf_pair_case(ref, dtype, R)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_column_with_a_nan(ref, dtype):
    for zero in (0.0, -0.0):
        for k in (0, 1, W):
            for nan_off in (0, 1, R, R + 2):
                lh.zero_nan_case(ref, dtype, k, k + R + 7, nan_off, zero)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [1, W - 1, W, W + 1])
def test_late_tie_fixtures(ref, dtype, c):
    for drop in (0, 2):
        lh.late_ties_case(ref, dtype, c, R, drop)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaled_fixtures(ref, dtype):
    for which in (0, 1):
        lh.scaled_case(ref, dtype, W, which)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_loop_of_the_library_on_non_finite_data(pkg, ref, dtype):
    """The checker stops at a zero pivot column and the library's loop returns an error there; on these two fixtures neither does, and
    the loop the contract names must agree with the checker where a NaN or an Inf sits in the searched column."""
    nan_off, max_off = lh.nan_hidden_offsets(R)[1]
    for A, LU, ipiv in (lh.nan_hidden_case(ref, dtype, 1, R, nan_off, max_off), lh.inf_pair_case(ref, dtype, R)):
        b = lh.vector(A.shape[0], dtype)
        Ah, bh = A.copy(order="F"), b.copy()
        pkg.lu_solve_(Ah, bh)
        assert np.isnan(LU).any() and lh.same_bits(Ah, LU), lh.first_difference(Ah, LU)
        assert lh.same_bits(bh, ref.solve(LU, ipiv, b))
