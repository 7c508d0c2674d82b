"""Complex bicgstabl, minres and chebyshev without a GPU: the C restatement of the layer they stand on
(tests/complex_ref/complex_solvers_ref.c) against exact rational sums, the complex LU solve of the library against numpy and against that
restatement with the pivot rule pinned, and the three solvers on the numpy double of the device types -- the complex test sets of
test/bicgstabl.jl:13-70, test/minres.jl:32-96 and test/chebyshev.jl:26-94 with the reference's own conditions, fused and unfused."""
from fractions import Fraction

import numpy as np
import pytest

import complex_host as ch
import complex_solvers_host as cs
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)
from complex_solvers_host import sref  # noqa: F401  (fixture)

CT = [np.complex128, np.complex64]
SHAPE = (1, 1)                       # segments of 256 elements: n = 300 spans two of them
N = 300


def small_ints(rng, T, *shape):
    """complex values with small integer parts: every product and sum below is exact in either precision"""
    return (rng.integers(-3, 4, shape) + 1j * rng.integers(-3, 4, shape)).astype(T)


def fdot(x, y):
    """sum conj(x) y in exact rationals"""
    re = sum(Fraction(int(a.real)) * Fraction(int(b.real)) + Fraction(int(a.imag)) * Fraction(int(b.imag)) for a, b in zip(x, y))
    im = sum(Fraction(int(a.real)) * Fraction(int(b.imag)) - Fraction(int(a.imag)) * Fraction(int(b.real)) for a, b in zip(x, y))
    return complex(float(re), float(im))


@pytest.mark.parametrize("T", CT)
def test_checker_gram_and_gemv_t_against_exact_sums(sref, T):
    rng = np.random.default_rng(3)
    k, ld = 4, N + 4
    V = np.zeros(ld * k, T)
    for j in range(k):
        V[j * ld: j * ld + N] = small_ints(rng, T, N)
    w = small_ints(rng, T, N)
    col = lambda j: V[j * ld: j * ld + N]
    assert np.array_equal(sref.gemv_t(V, ld, k, w, SHAPE), np.array([fdot(col(j), w) for j in range(k)], T))
    M = sref.gram(V, ld, N, k, SHAPE)
    assert np.array_equal(M, np.array([[fdot(col(r), col(c)) for c in range(k)] for r in range(k)], T))
    assert np.array_equal(M, M.conj().T) and not np.signbit(M.diagonal().imag).any()


@pytest.mark.parametrize("T", CT)
def test_checker_reducing_sweeps_against_exact_sums(sref, T):
    rng = np.random.default_rng(4)
    rt = ch.real_of(T).type
    x, y0, z = (small_ints(rng, T, N) for _ in range(3))
    for alpha in (rt(2), T(1 - 2j)):                                    # the real and the complex alpha
        y = y0.copy()
        d = sref.axpy_dot(alpha, x, y, z, SHAPE)
        assert np.array_equal(y, (y0 + alpha * x).astype(T)) and d == T(fdot(z, y))
        y = y0.copy()
        nrm = sref.axpy_dot(alpha, x, y, None, SHAPE)
        assert np.array_equal(y, (y0 + alpha * x).astype(T)) and nrm == rt(np.sqrt(fdot(y, y).real))
    y = y0.copy()
    assert sref.axpy_dot(T(0), None, y, z, SHAPE) == T(fdot(z, y0)) and np.array_equal(y, y0)
    # the MR update: integer gammas keep it exact
    l, ld = 2, N + 2
    us, rs = small_ints(rng, T, ld * (l + 1)), small_ints(rng, T, ld * (l + 1))
    xv, gamma = small_ints(rng, T, N), np.array([1 + 1j, -2j], T)
    cu = lambda a, j: a[j * ld: j * ld + N].copy()
    want_u = cu(us, 0) - gamma[0] * cu(us, 1) - gamma[1] * cu(us, 2)
    want_x = xv + gamma[0] * cu(rs, 0) + gamma[1] * cu(rs, 1)
    want_r = cu(rs, 0) - gamma[0] * cu(rs, 1) - gamma[1] * cu(rs, 2)
    got = sref.mr_update(us, ld, rs, ld, xv, l, gamma, SHAPE)
    assert np.array_equal(cu(us, 0), want_u.astype(T)) and np.array_equal(xv, want_x.astype(T)) and np.array_equal(cu(rs, 0), want_r.astype(T))
    assert got == rt(np.sqrt(fdot(want_r, want_r).real))
    # both minres_update forms
    for sc in ([rt(2), rt(-1), rt(3), rt(2), rt(-2)], [T(1j), T(1 - 1j), T(2), T(-1j), T(1 + 1j)]):
        vn, vc, wc, wp, xx = (small_ints(rng, T, N) for _ in range(5))
        for wcur, wprev in ((None, None), (wc, None), (wc, wp)):        # iterations 1, 2 and >= 3
            a, wn, xo = vn.copy(), np.zeros(N, T), xx.copy()
            sref.minres_update(xo, a, vc, wcur, wprev, wn, sc)
            w = vc.astype(np.complex128)
            if wcur is not None:
                w = w + sc[1] * wcur
            if wprev is not None:
                w = w + sc[2] * wprev
            w = w * sc[3]
            assert np.array_equal(a, (vn * sc[0]).astype(T)) and np.array_equal(wn, w.astype(T)) and np.array_equal(xo, (xx + sc[4] * w).astype(T))


@pytest.mark.parametrize("T", CT)
def test_complex_lu_solve(pkg, sref, T):
    rng = np.random.default_rng(8)
    eps = np.finfo(ch.real_of(T)).eps
    for n in (1, 2, 4, 5):
        A = np.asfortranarray(ch.rand_t(rng, T, n, n) - T(0.5 + 0.5j))
        b = ch.rand_t(rng, T, n)
        got = pkg.lu_solve_(A.copy(order="F"), b.copy())
        want = np.linalg.solve(A.astype(np.complex128), b.astype(np.complex128))
        assert np.linalg.norm(got - want) <= 50 * n * eps * np.linalg.cond(A.astype(np.complex128)) * np.linalg.norm(want)
        Ac, bc = A.copy(order="F"), b.copy()
        assert sref.lu_solve(Ac, bc) == 0 and np.array_equal(bc, got)    # bit for bit the restatement
    # |re| + |im| picks 3 + 3 i (6 against 5), the modulus would pick 5 (5 against 4.24): the two pivots give different factors
    A = np.asfortranarray(np.array([[3 + 3j, 1], [5, 2 - 1j]], T))
    F, b = A.copy(order="F"), np.array([1, 1j], T)
    x = pkg.lu_solve_(F, b.copy())
    # no row exchange: the pivot is 3 + 3 i and the multiplier 5 / (3 + 3 i) is LARGER than 1 in modulus, which pivoting by modulus never leaves
    assert F[0, 0] == T(3 + 3j) and abs(F[1, 0] - 5 / (3 + 3j)) <= 4 * eps and abs(F[1, 0]) > 1
    assert np.linalg.norm(A.astype(np.complex128) @ x - b) <= 20 * eps
    Ac, bc = A.copy(order="F"), b.copy()
    assert sref.lu_solve(Ac, bc) == 0 and np.array_equal(bc, x) and np.array_equal(Ac, F)
    # a zero column: MIK_ERR_SINGULAR
    Z = np.asfortranarray(np.array([[1, 0], [2j, 0]], T))
    with pytest.raises(np.linalg.LinAlgError):
        pkg.lu_solve_(Z.copy(order="F"), b.copy())
    assert pkg.lib().mik_lu_solve(pkg._lib.dtype_code(T), Z.ctypes.data, 2, 2, b.copy().ctypes.data) == 8
    assert sref.lu_solve(Z.copy(order="F"), b.copy()) == 8


@pytest.fixture(scope="module")
def host(pkg, ref, dref, sref):
    return cs.HostBackend(pkg, ref, dref, sref)


@pytest.mark.parametrize("T", CT)
def test_seeds_leave_room(T):
    """the plain complex128 restatements meet every condition of the three test sets with the room the seeds were chosen for"""
    cs.room_bicgstabl(T)
    cs.room_minres(T)
    cs.room_cheb(T)


@pytest.mark.parametrize("T", CT)
def test_bicgstabl_complex_sets(host, T):
    fused, unfused = cs.bicgstabl_sets(host, T, True), cs.bicgstabl_sets(host, T, False)
    cs.check_bicgstabl_sets(fused)
    cs.same(fused, unfused)


@pytest.mark.parametrize("T", CT)
def test_minres_complex_sets(host, T):
    fused, unfused = cs.minres_sets(host, T, True), cs.minres_sets(host, T, False)
    cs.check_minres_sets(fused, T)
    cs.same(fused, unfused)


@pytest.mark.parametrize("T", CT)
def test_chebyshev_complex_sets(host, T):
    fused, unfused = cs.cheb_sets(host, T, True), cs.cheb_sets(host, T, False)
    cs.check_cheb_sets(fused, T)
    cs.same(fused, unfused)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["bicgstabl", "minres", "chebyshev"])
def test_termination_criterion(host, T, solver):
    fused, unfused = cs.termination(host, T, solver, True), cs.termination(host, T, solver, False)
    cs.check_termination(fused, solver)
    cs.same(fused, unfused)


def test_dense_double_gives_the_same_bits(pkg, ref, dref, sref, host):
    """n <= 64: one chunk of the dense product, so the dense operator and the fully stored CSR operator sum a row in the same order"""
    dense = cs.HostBackend(pkg, ref, dref, sref, dense=True)
    for T in CT:
        cs.same(cs.minres_sets(host, T), cs.minres_sets(dense, T))
        cs.same(cs.bicgstabl_sets(host, T), cs.bicgstabl_sets(dense, T))


def test_device_types_are_required_without_ops(pkg, host):
    T = np.complex64
    A = host.operator(ch.dense_csr(np.eye(3, dtype=T)))
    b = host.vector(np.ones(3, T))
    x = lambda: host.vector(np.zeros(3, T))
    for call in (lambda: pkg.minres_(x(), A, b), lambda: pkg.minres_iterable_(x(), A, b),
                 lambda: pkg.chebyshev_(x(), A, b, 0.5, 1.5), lambda: pkg.chebyshev_iterable_(x(), A, b, 0.5, 1.5),
                 lambda: pkg.bicgstabl_(x(), A, b), lambda: pkg.bicgstabl_iterator_(x(), A, b)):
        with pytest.raises(TypeError, match=r"complex64.*device types.*ops"):
            call()
    # with the backend's ops the same operands run
    assert np.allclose(pkg.minres_(x(), A, b, ops=host.ops).to_numpy(), np.ones(3, T), atol=1e-5)
    assert pkg.bicgstabl_(x(), A, b, ops=host.ops).to_numpy().dtype == np.dtype(T)
    assert np.allclose(pkg.chebyshev_(x(), A, b, 0.5, 1.5, ops=host.ops).to_numpy(), np.ones(3, T), atol=1e-3)
    # JacobiPrec is refused on a complex operator before anything runs
    for call in (lambda: pkg.bicgstabl_(x(), A, b, Pl=pkg.JacobiPrec(b), ops=host.ops), lambda: pkg.chebyshev_(x(), A, b, 0.5, 1.5, Pl=pkg.JacobiPrec(b), ops=host.ops)):
        with pytest.raises(TypeError, match="JacobiPrec.*complex"):
            call()
    with pytest.raises(TypeError, match="complex"):
        pkg._lib.real_dtype_code(np.complex64, "svdl")
