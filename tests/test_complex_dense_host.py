"""Complex dense operators without a GPU: the C restatement of the two orders
(tests/complex_ref/complex_dense_ref.c) against exact rational sums, against the sparse row sum up to one chunk and against the complex dot
per column; the complex Matrix{T} test sets of test/cg.jl:27-47,99-121 and test/gmres.jl:16-36,76-98 on the dense numpy double, bit for bit
what the CSR double gives (n = 10 <= C); one system beyond a chunk; the binding of the new entry."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import complex_dense_host as cdh
import complex_host as ch
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)

CT = [np.complex128, np.complex64]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_ints(rng, T, *shape):
    """complex values with small integer parts: every product and sum below is exact in either precision"""
    return (rng.integers(-4, 5, shape) + 1j * rng.integers(-4, 5, shape)).astype(T)


def frac(z):
    return Fraction(int(z.real)), Fraction(int(z.imag))


def as_c(f, T):
    return T(complex(float(f[0]), float(f[1])))


def spmv_of(ref, A, x, **kw):
    M = ch.NpCSR(ref, ch.dense_csr(A))
    return ref.spmv(M.rowptr, M.col, M.val, np.ascontiguousarray(x), M.n_rows, **kw)


@pytest.mark.parametrize("T", CT)
def test_checker_against_exact_sums(dref, T):
    rng = np.random.default_rng(3)
    for (m, n), chunk, shape in (((1, 1), 64, (1, 2)), ((7, 5), 2, (2, 2)), ((3, 130), 64, (1, 1)), ((600, 3), 64, (1, 2)), ((1100, 2), 4, (2, 2)),
                                 ((0, 3), 64, (1, 2)), ((3, 0), 64, (1, 2))):
        A, x, u = small_ints(rng, T, m, n), small_ints(rng, T, n), small_ints(rng, T, m)
        want_n, want_t = [], []
        for i in range(m):
            re = sum(frac(A[i, j])[0] * frac(x[j])[0] - frac(A[i, j])[1] * frac(x[j])[1] for j in range(n))
            im = sum(frac(A[i, j])[0] * frac(x[j])[1] + frac(A[i, j])[1] * frac(x[j])[0] for j in range(n))
            want_n.append(as_c((re, im), T))
        for j in range(n):
            re = sum(frac(A[i, j])[0] * frac(u[i])[0] + frac(A[i, j])[1] * frac(u[i])[1] for i in range(m))      # conj(a) u
            im = sum(frac(A[i, j])[0] * frac(u[i])[1] - frac(A[i, j])[1] * frac(u[i])[0] for i in range(m))
            want_t.append(as_c((re, im), T))
        assert np.array_equal(dref.mul_n(A, x, chunk), np.array(want_n, T)), (m, n)
        assert np.array_equal(dref.mul_t(A, u, shape), np.array(want_t, T)), (m, n)
    # a leading dimension larger than m: the padding rows are never read
    A, x = small_ints(rng, T, 5, 3), small_ints(rng, T, 3)
    store = np.full((8, 3), np.nan, T, order="F")
    store[:5] = A
    y = np.full(5, np.nan, T)
    dref._fn("cd_mul_n", T)(5, 3, store.ctypes.data_as(C.c_void_p), 8, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), 64)
    assert np.array_equal(y, dref.mul_n(A, x, 64))


@pytest.mark.parametrize("T", CT)
def test_one_chunk_is_the_row_sum_and_a_second_chunk_is_not(pkg, ref, dref, T):
    chunk, rows = cdh.mul_shape(pkg, T)
    assert chunk == 64 and rows > 0 and chunk <= 256                   # 256: mik_spmv_long_row
    rng = np.random.default_rng(17)
    for m, n in ((5, 1), (33, chunk - 1), (130, chunk)):
        A, x = ch.rand_t(rng, T, m, n), ch.rand_t(rng, T, n)
        assert np.array_equal(dref.mul_n(A, x, chunk), spmv_of(ref, A, x)), (m, n)
    # n = C + 1: p_1 is ONE rounded product and +0 + p = p, so p_0 + p_1 is still the serial chain.  The first width at which the
    # chunking can show is C + 2 (p_0 + (a + b) against (p_0 + a) + b), and there it does, on a random matrix
    A, x = ch.rand_t(rng, T, 200, chunk + 2), ch.rand_t(rng, T, chunk + 2)
    assert np.array_equal(dref.mul_n(A[:, :chunk + 1], x[:chunk + 1], chunk), spmv_of(ref, A[:, :chunk + 1], x[:chunk + 1]))
    got, serial = dref.mul_n(A, x, chunk), spmv_of(ref, A, x)
    assert np.any(got != serial)                                       # the chunking is real
    np.testing.assert_allclose(got, serial, rtol=1e-4 if T == np.complex64 else 1e-12)
    assert np.array_equal(dref.mul_n(A, x, chunk + 2), serial)


@pytest.mark.parametrize("T", CT)
def test_adjoint_is_the_complex_dot_per_column_and_conjugates(pkg, ref, dref, T):
    shape = ch.HostOps(pkg, ref).shape(T)
    S = 256 * shape[0] * shape[1]
    rng = np.random.default_rng(23)
    for m, n in ((1, 3), (S - 1, 2), (S + 1, 2), (3 * S + 5, 3)):
        A, u = np.asfortranarray(ch.rand_t(rng, T, m, n)), ch.rand_t(rng, T, m)
        got = dref.mul_t(A, u, shape)
        for j in range(n):
            assert got[j] == ref.dot(np.ascontiguousarray(A[:, j]), u, shape), (m, n, j)
    A, u = ch.rand_t(rng, T, 40, 6), ch.rand_t(rng, T, 40)
    assert np.all(A.imag != 0)
    adj, plain = dref.mul_t(A, u, shape), dref.mul_n(np.asfortranarray(A.T), u, 64)
    assert np.all(adj != plain)                                        # A' u is not transpose(A) u
    np.testing.assert_allclose(adj, A.conj().T @ u, rtol=1e-4 if T == np.complex64 else 1e-12)


# ---------------------------------------------------------------------------------------------
# the reference's complex Matrix{T} test sets on the dense double
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hosts(pkg, ref, dref):
    return cdh.DenseHostBackend(pkg, ref, dref), ch.HostBackend(pkg, ref)


@pytest.mark.parametrize("T", CT)
def test_cg_complex_full_system(hosts, T):
    dense, csr = (ch.cg_full(be, T) for be in hosts)
    ch.check_cg_full(dense)
    ch.same(dense, csr)                                                # n = 10 <= C: the dense order is the row sum


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_termination_criterion(hosts, T, solver):
    dense, csr = (ch.termination(be, T, solver) for be in hosts)
    ch.check_termination(dense)
    ch.same(dense, csr)


@pytest.mark.parametrize("T", CT)
def test_gmres_complex_sets(hosts, T):
    dense, csr = (ch.gmres_sets(be, T, False) for be in hosts)
    ch.check_gmres_sets(dense)
    ch.same(dense, csr)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_system_beyond_a_chunk(hosts, T, seed):
    """n = 197 = 3 C + 5.  Plain numpy CG on these systems (cond(A) about 100) converges in 6 steps to 1.3e-4 - 1.4e-4 against 3.45e-4
    (ComplexF32) and in 11 steps to 3.5e-9 - 4.1e-9 against 1.49e-8 (ComplexF64): the reference order alone holds the condition with
    more than 2x to spare."""
    be, n = hosts[0], 197
    A, b, reltol = cdh.beyond_a_chunk(T, seed, n)
    x, h = be.pkg.cg_(be.vector(np.zeros(n, T)), be.operator(A), be.vector(b), initially_zero=True, reltol=reltol, maxiter=n, log=True, ops=be.ops)
    A, b = A.astype(np.complex128), b.astype(np.complex128)
    assert h.isconverged and np.linalg.norm(A @ x.to_numpy() - b) / np.linalg.norm(b) <= reltol


def test_the_new_entry_is_declared_bound_and_answers_for_all_four_codes(pkg):
    header = open(os.path.join(ROOT, "include", "mik.h")).read()
    section = header[header.index("---- dense operator"):header.index("---- measurement")]
    decl = re.search(r"\bint mik_dense_mul_shape_for\(([^;]*)\);", section).group(1)
    assert len(decl.split(",")) == len(pkg._lib.SIGNATURES["mik_dense_mul_shape_for"][1]) == 3
    assert "MIK_C64 / MIK_C32" in section and "interleaved (re, im)" in section and "MIK_ERR_NOTIMPL" in section
    L = pkg.lib()
    c0, r0 = C.c_int(), C.c_int()
    assert L.mik_dense_mul_shape(C.byref(c0), C.byref(r0)) == 0
    for T in (np.float64, np.float32):
        assert cdh.mul_shape(pkg, T) == (c0.value, r0.value)
    assert cdh.mul_shape(pkg, np.complex128)[0] == cdh.mul_shape(pkg, np.complex64)[0] == c0.value
    assert all(cdh.mul_shape(pkg, T)[1] % 256 == 0 for T in CT)
    assert L.mik_dense_mul_shape_for(7, C.byref(c0), C.byref(r0)) == 1 and L.mik_dense_mul_shape_for(2, None, None) == 0
