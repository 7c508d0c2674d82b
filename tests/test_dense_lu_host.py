"""The checker of the dense LU tests (tests/dense_ref/dense_lu_ref.c, the bit contract restated as unblocked loops) against what needs no
device: the library's host loop mik_lu_solve, the exactly representable fixture, the pivot-rule fixtures, and a blocked numpy plan.
Every comparison is np.array_equal."""
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
    """panels of W columns, interchanges outside the panel, strip solve, trailing update: k stays ascending per element"""
    for n in (1, 2, 7, 8, 9, 30):
        A = lh.random(n, dtype)
        LU, ipiv, _ = ref.factor(A)
        Lb, pb = lh.blocked(A, W)
        assert Lb.dtype == dtype and np.array_equal(pb, ipiv) and np.array_equal(Lb, LU), (n, W)
