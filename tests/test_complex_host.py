"""Complex element types without a GPU: the C restatement of the orders (tests/complex_ref/complex_ref.c) against
exact rational sums, the complex Givens rotation and Hessenberg least squares on H2 of test/hessenberg.jl:20-26, and the generic cg /
gmres iterables on a numpy double of the device types whose L1 / L2 operations are that C checker -- the complex test sets of
test/cg.jl:27-47,99-121 and test/gmres.jl:16-57,76-98 with the reference's own conditions."""
from fractions import Fraction

import numpy as np
import pytest

import complex_host as ch
from complex_host import ref  # noqa: F401  (fixture)

CT = [np.complex128, np.complex64]


def small_ints(rng, T, *shape):
    """complex values with small integer parts: every product and sum below is exact in either precision"""
    return (rng.integers(-4, 5, shape) + 1j * rng.integers(-4, 5, shape)).astype(T)


def frac(z):
    return Fraction(int(z.real)), Fraction(int(z.imag))


def fmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def as_c(f, T):
    return T(complex(float(f[0]), float(f[1])))


@pytest.mark.parametrize("T", CT)
def test_checker_dot_and_axpy_family_against_exact_sums(ref, T):
    rng = np.random.default_rng(7)
    for n, shape in ((1, (1, 2)), (5, (2, 2)), (37, (1, 1)), (700, (1, 2)), (1100, (2, 2))):
        x, y = small_ints(rng, T, n), small_ints(rng, T, n)
        re = sum(frac(a)[0] * frac(b)[0] + frac(a)[1] * frac(b)[1] for a, b in zip(x, y))       # sum conj(x) y
        im = sum(frac(a)[0] * frac(b)[1] - frac(a)[1] * frac(b)[0] for a, b in zip(x, y))
        assert ref.dot(x, y, shape) == as_c((re, im), T)
        assert ref.nrm2(x, shape) == ch.real_of(T).type(np.sqrt(float(sum(frac(a)[0] ** 2 + frac(a)[1] ** 2 for a in x))))
    x, y = small_ints(rng, T, 9), small_ints(rng, T, 9)
    alpha = T(2 - 3j)
    for name, want in (("axpy", [tuple(p + q for p, q in zip(frac(b), fmul(frac(alpha), frac(a)))) for a, b in zip(x, y)]),
                       ("xpby", [tuple(p + q for p, q in zip(frac(a), fmul(frac(alpha), frac(b)))) for a, b in zip(x, y)]),
                       ("scal", [fmul(frac(b), frac(alpha)) for b in y])):
        got = y.copy()
        {"axpy": lambda: ref.axpy(alpha, x, got), "xpby": lambda: ref.xpby(x, alpha, got), "scal": lambda: ref.scal(alpha, got)}[name]()
        assert np.array_equal(got, np.array([as_c(w, T) for w in want], T)), name
    r = ch.real_of(T).type(3)                                                                       # a real scalar: (a zr) + (a zi) i
    got = y.copy(); ref.axpy(r, x, got); assert np.array_equal(got, y + 3 * x)
    got = y.copy(); ref.xpby(x, r, got); assert np.array_equal(got, x + 3 * y)
    got = y.copy(); ref.scal(r, got); assert np.array_equal(got, 3 * y)
    got = y.copy(); ref.sub(x, got); assert np.array_equal(got, y - x)


@pytest.mark.parametrize("T", CT)
def test_checker_spmv_orders_mgs_and_gemv_against_exact_sums(ref, T):
    import scipy.sparse as sp
    rng = np.random.default_rng(11)
    lens = [0, 1, 7, 12, 30]                                          # with long_row = 8, segment = 12, group = 4: serial, one segment, cut rows
    m = 40
    rows = []
    for ln in lens:
        r = np.zeros(m, T)
        r[np.sort(rng.choice(m, ln, replace=False))] = small_ints(rng, T, ln) + T(1)
        rows.append(r)
    A = ch.NpCSR(ref, sp.csr_matrix(np.array(rows)))
    x = small_ints(rng, T, m)
    want = []
    for i in range(len(lens)):
        acc = (Fraction(0), Fraction(0))
        for k in range(A.rowptr[i], A.rowptr[i + 1]):
            p = fmul(frac(A.val[k]), frac(x[A.col[k]]))
            acc = (acc[0] + p[0], acc[1] + p[1])
        want.append(as_c(acc, T))
    for kw in (dict(), dict(long_row=8, segment=12, group=4)):
        assert np.array_equal(ref.spmv(A.rowptr, A.col, A.val, x, len(lens), **kw), np.array(want, T))
    # Modified Gram-Schmidt: h and the un-normalised w are exact; gemv_n is exact
    n, k, ld = 6, 2, 8
    V = np.zeros(ld * k, T)
    V[0], V[ld + 1] = T(1), T(1j)                                     # e_1 and i e_2: orthonormal
    w0 = small_ints(rng, T, n)
    w = w0.copy()
    h, nrm = ref.mgs(V, ld, k, w, (1, 2))
    assert np.array_equal(h, np.array([w0[0], np.conj(T(1j)) * w0[1]], T))
    rest = w0.copy(); rest[:2] = 0
    assert nrm == ch.real_of(T).type(np.sqrt(float(np.sum(np.abs(rest.astype(np.complex128)) ** 2))))
    assert np.array_equal(w, (rest * (ch.real_of(T).type(1) / nrm)).astype(T))
    Vd = small_ints(rng, T, ld * 3)
    c, y0, alpha = small_ints(rng, T, 3), small_ints(rng, T, n), T(1 + 1j)
    y = y0.copy()
    ref.gemv_n(Vd, ld, 3, c, alpha, y)
    assert np.array_equal(y, (y0 + sum(alpha * c[j] * Vd[j * ld: j * ld + n] for j in range(3))).astype(T))


H2 = np.array([[1.14661 + 1.00222j, 1.38611 + 0.0100307j, -0.0280623 + 0.00494128j, 0.0205642 - 0.00867472j],
               [1.43066 + 0.0j, 4.11145 + 1.0144j, 0.883563 + 0.00583816j, -0.00332255 - 0.0274278j],
               [0.0, 1.0865 + 0.0j, 3.2653 + 0.990342j, 0.942434 + 0.00586481j],
               [0.0, 0.0, 1.31146 + 0.0j, 3.11491 + 1.01587j],
               [0.0, 0.0, 0.0, 1.42175 + 0.0j]])                       # test/hessenberg.jl:20-26


@pytest.mark.parametrize("T", CT)
def test_complex_givens_on_h2(pkg, T):
    """G [f; g] = [r; 0] and G unitary, both to 4 ulp of the element type, for every rotation the Hessenberg solve of H2 starts from"""
    eps = np.finfo(ch.real_of(T)).eps
    H = H2.astype(T)
    pairs = [(H[i, i], H[i + 1, i]) for i in range(4)] + [(T(0), T(1 + 2j)), (T(3 - 1j), T(0)), (T(1e-30j), T(2.0))]
    for f, g in pairs:
        c, s, r = pkg.givens_algorithm(f, g, T)
        assert np.isrealobj(c) or c.imag == 0
        c, s, r, f, g = (np.complex128(v) for v in (c, s, r, f, g))
        scale = max(abs(f), abs(g))
        assert abs(c * f + s * g - r) <= 4 * eps * scale and abs(-np.conj(s) * f + c * g) <= 4 * eps * scale
        G = np.array([[c, s], [-np.conj(s), c]])
        assert np.max(np.abs(G @ G.conj().T - np.eye(2))) <= 4 * eps


@pytest.mark.parametrize("T", CT)
def test_complex_hessenberg_ldiv_on_h2(pkg, T):
    """test/hessenberg.jl:28-44 for H2"""
    H = np.asfortranarray(H2.astype(T))
    rhs = np.zeros(5, T)
    rhs[0] = 1
    sol = pkg.hessenberg_ldiv_(H.copy(order="F"), rhs.copy())
    want = np.linalg.lstsq(H2, rhs.astype(np.complex128), rcond=None)[0]
    rtol = np.sqrt(np.finfo(ch.real_of(T)).eps)                        # Julia's isapprox default
    assert np.linalg.norm(sol[:4] - want) <= rtol * np.linalg.norm(want)                                     # :40
    rn = np.linalg.norm(H2 @ want - rhs)
    assert abs(abs(sol[4]) - rn) <= rtol * rn                                                                # :43


@pytest.fixture(scope="module")
def host(pkg, ref):
    return ch.HostBackend(pkg, ref)


@pytest.mark.parametrize("T", CT)
def test_cg_complex_full_system(host, T):
    ch.check_cg_full(ch.cg_full(host, T))


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_termination_criterion(host, T, solver):
    ch.check_termination(ch.termination(host, T, solver))


@pytest.mark.parametrize("T,sparse", [(np.complex128, False), (np.complex64, False), (np.complex128, True)])   # :38: the sparse set runs ComplexF64 only
def test_gmres_complex_sets(host, T, sparse):
    ch.check_gmres_sets(ch.gmres_sets(host, T, sparse))


def test_all_zero_rhs_and_mv_products_quirk(host):
    """test/cg.jl:50-51 (an all-zeros rhs gives an all-zeros x) and the mv_products count of src/gmres.jl:122"""
    pkg, T = host.pkg, np.complex128
    A = host.operator(ch.dense_csr(np.eye(4, dtype=T) * 2))
    x = pkg.cg_(host.vector(np.zeros(4, T)), A, host.vector(np.zeros(4, T)), initially_zero=True, ops=host.ops)
    assert np.array_equal(x.to_numpy(), np.zeros(4, T))
    kw = dict(abstol=0.0, reltol=1e-8, restart=4, maxiter=4, orth_meth=pkg.ModifiedGramSchmidt(), ops=host.ops)
    g0 = pkg.GenericGMRESIterable(host.vector(np.zeros(4, T)), A, host.vector(np.ones(4, T)), initially_zero=True, **kw)
    g1 = pkg.GenericGMRESIterable(host.vector(np.zeros(4, T)), A, host.vector(np.ones(4, T)), initially_zero=False, **kw)
    assert (g0.mv_products, g1.mv_products) == (1, 0)                  # as the reference counts, :122


def test_jacobi_prec_is_refused_for_complex(pkg, host):
    T = np.complex128
    A = host.operator(ch.dense_csr(np.eye(3, dtype=T)))
    b = host.vector(np.ones(3, T))
    P = pkg.JacobiPrec(b)
    with pytest.raises(TypeError, match="JacobiPrec.*complex"):
        pkg.cg_(host.vector(np.zeros(3, T)), A, b, Pl=P, ops=host.ops)
    with pytest.raises(TypeError, match="JacobiPrec.*complex"):
        pkg.gmres_(host.vector(np.zeros(3, T)), A, b, Pr=P, ops=host.ops)
    assert pkg._lib.dtype_code(np.complex128) == 2 and pkg._lib.dtype_code(np.complex64) == 3
    with pytest.raises(TypeError):
        pkg._lib.dtype_code(np.int32)
    # what stays real says so before anything reaches the library
    for call in (lambda: pkg.minres_(host.vector(np.zeros(3, T)), A, b), lambda: pkg.chebyshev_(host.vector(np.zeros(3, T)), A, b, 0.5, 1.5),
                 lambda: pkg.bicgstabl_(host.vector(np.zeros(3, T)), A, b), lambda: pkg._lib.real_dtype_code(np.complex64, "svdl")):
        with pytest.raises(TypeError, match="complex"):
            call()
