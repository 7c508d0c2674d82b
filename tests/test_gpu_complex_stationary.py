"""jacobi / gauss_seidel / sor / ssor and their building blocks on a ComplexF64 / ComplexF32 device CSR operator
(csrc/mik_stationary_complex.h), np.array_equal against tests/complex_ref/complex_stationary_ref.c -- the reference's CSC column loops on
(re, im) pairs, which tests/test_complex_stationary_host.py holds to exact quotients and to an independent row-view restatement.

The operators are the staged fixtures of tests/stationary_fixtures.py with a random unit-modulus phase on every stored entry
(tests/complex_stationary_host.py): edges / stairs / hubs, 2049 / 2047 / 2048 rows -- the switch between k_cst_tri_run and k_cst_tri_level at
256 | 257 rows, full and one-row last workgroups, runs between wide launches, rows of more than 256 entries inside a wide level.  The plan
is checked first (StationaryOperator.info() against level_widths / launch_plan), so that a wrong plan is reported as a wrong plan.

The case that launches each instance of k_cst_tri_level (each also of k_cst_tri_run, every fixture having runs):

    <double, double, false>   test_substitutions, ComplexF64, plain
    <double, double, true>    ... ComplexF64, omega 1.2 / np.float32(0.8) / 1
    <float, float, false>     ... ComplexF32, plain
    <float, double, true>     ... ComplexF32, omega 1.2 (a Float64 omega: the 64-bit division, one rounding per component at the store)
    <float, float, true>      ... ComplexF32, omega np.float32(0.8) and 1 (the widened 32-bit division)"""
import math

import numpy as np
import pytest

import complex_stationary_host as ch
import stationary_fixtures as fx
import stationary_host as sh
from complex_stationary_host import cref  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
CTYPES = ch.CTYPES
NAMES = list(fx.STAGED)
SIZES = (1, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def op(pkg, ctx):
    """(M, A, S) of a complexified fixture: uploaded and analysed once per module"""
    made = {}

    def get(name, T, i32=False):
        key = (name, np.dtype(T), i32)
        if key not in made:
            M = ch.fixture(name, T)
            A = fx.dev(pkg, M, i32=i32)
            made[key] = (M, A, pkg.StationaryOperator(A))
        return made[key]

    yield get
    made.clear()


def _plan_of(info):
    return (info["levels_forward"], info["launches_forward"], info["levels_backward"], info["launches_backward"])


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_plan_is_the_one_of_the_real_pattern(pkg, ctx, op, name, T):
    M, A, S = op(name, T)
    assert ctx.spmv_long_row() == fx.LONG_ROW and A.dtype == np.dtype(T)
    want = (len(M.widths[0]), len(M.plans[0]), len(M.widths[1]), len(M.plans[1]))
    assert _plan_of(S.info()) == want
    Mr = fx.fixture(name, np.float64)                                   # ... and the plan the real operator of the same pattern gets
    assert _plan_of(pkg.StationaryOperator(fx.dev(pkg, Mr)).info()) == want


@pytest.mark.parametrize("omega", (None,) + ch.OMEGAS, ids=["plain"] + ch.OMEGA_IDS)
@pytest.mark.parametrize("upper", (False, True), ids=["forward", "backward"])
@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_substitutions(pkg, ctx, cref, op, name, T, upper, omega):
    """forward_sub! / backward_sub!, plain and relaxed, omega a Python float, an np.float32 and an int: all six instances of level and run"""
    M, A, S = op(name, T)
    assert cref.diag(M) == 0
    rng = np.random.default_rng(11)
    x, y = ch.cnormal(rng, T, M.n), ch.cnormal(rng, T, M.n)
    sub = S.backward_sub_ if upper else S.forward_sub_
    xd = pkg.HipVector.from_numpy(x)
    if omega is None:
        assert sub(xd) is xd
        assert np.array_equal(xd.to_numpy(), cref.sub(M, upper, x))
        return
    yd = pkg.HipVector.from_numpy(y)
    assert sub(xd, omega, yd) is xd
    want = cref.sub(M, upper, x, omega, y)
    assert np.all(np.isfinite(want))
    assert np.array_equal(xd.to_numpy(), want) and np.array_equal(yd.to_numpy(), y)


@pytest.mark.parametrize("omega", ch.OMEGAS, ids=ch.OMEGA_IDS)
@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_whole_methods(pkg, ctx, cref, op, name, T, omega):
    """jacobi! / gauss_seidel! / sor! (the returned vector and the caller's x) / ssor!, 3 iterations"""
    M, A, _ = op(name, T)
    ch.check_methods(pkg, cref, M, A, omega, 3, np.random.default_rng(42))


@pytest.mark.parametrize("T", CTYPES)
def test_int32_upload_gives_the_same_bits(pkg, ctx, cref, op, T):
    """SparseMatrixCSC{T, Int32}: the same plan and the same bits"""
    M, A, S = op("edges", T, i32=True)
    assert _plan_of(S.info()) == _plan_of(op("edges", T)[2].info())
    ch.check_methods(pkg, cref, M, A, 1.2, 2, np.random.default_rng(7))
    assert cref.diag(M) == 0
    rng = np.random.default_rng(12)
    x, y = ch.cnormal(rng, T, M.n), ch.cnormal(rng, T, M.n)
    V = pkg.HipVector.from_numpy
    for upper in (False, True):
        sub = S.backward_sub_ if upper else S.forward_sub_
        assert np.array_equal(sub(V(x)).to_numpy(), cref.sub(M, upper, x)), upper
        assert np.array_equal(sub(V(x), 1.2, V(y)).to_numpy(), cref.sub(M, upper, x, 1.2, y)), upper


def _branch_operator(n, T):
    """n rows whose diagonal cycles through the divisors of the branch-covering quotients, and the matching numerators"""
    br = ch.branches(T)
    z = np.array([br[i % len(br)][0] for i in range(n)], np.complex128).astype(T)
    w = np.array([br[i % len(br)][1] for i in range(n)], np.complex128).astype(T)
    assert np.all(np.isfinite(z)) and np.all(np.isfinite(w)) and np.all(w != 0)
    return ch.sprand_complex(n, 6, T, 300 + n, diagonal=w), z


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_row_parallel_kernels(pkg, ctx, cref, n, T):
    """ldiv! (also y === x) on a diagonal that takes every branch of the division, mul! on OffDiagonal in its three beta modes, both
    gauss_seidel_multiply! forms (z === x and not): one row, n on either side of a multiple of 256, more than one workgroup"""
    M, z = _branch_operator(n, T)
    assert cref.diag(M) == 0
    S = pkg.StationaryOperator(fx.dev(pkg, M))
    V = pkg.HipVector.from_numpy
    rng = np.random.default_rng(5)
    x, y, b = (ch.cnormal(rng, T, n) for _ in range(3))
    want = cref.ldiv(M, z)
    assert np.all(np.isfinite(want))
    if n >= len(ch.branches(T)):                                        # every quotient is the checker's scalar division of that pair
        for i, (zz, ww, what) in enumerate(ch.branches(T)):
            assert want[i] == cref.div(zz, ww, T), what
    assert np.array_equal(S.diag_ldiv_(V(np.zeros(n, T)), V(z)).to_numpy(), want)
    zv = V(z)
    assert np.array_equal(S.diag_ldiv_(zv, zv).to_numpy(), want)
    for a, be in ((1.0, 0.0), (1.0, 1.0), (complex(2.0, -0.5), complex(3.0, 0.25)), (complex(-1.0, -0.0), 1.0), (complex(0.0, 1.0), complex(1.0, 1e-3)),
                  (1.5, complex(0.0, -0.0)), (1.5, complex(1.0, -0.0))):
        xv = V(x)
        assert np.array_equal(S.offdiag_mul_(a, xv, be, V(y)).to_numpy(), cref.offdiag_mul(M, a, x, be, y)), (a, be)
        assert np.array_equal(xv.to_numpy(), x)
    nan = np.full(n, np.nan + 1j * np.nan, T)                           # beta == 0 is fill!: what y held does not matter
    assert np.array_equal(S.offdiag_mul_(1.5, V(x), 0.0, V(nan)).to_numpy(), cref.offdiag_mul(M, 1.5, x, 0.0, y))
    for upper in (True, False):
        xv = V(x)
        assert np.array_equal(S.gs_multiply_(upper, complex(-1.0, -0.0), xv, 1.0, V(b), xv).to_numpy(),
                              cref.gs_mul(M, upper, complex(-1.0, -0.0), x, 1.0, b)), upper                                    # z === x
        xv = V(x)
        assert np.array_equal(S.gs_multiply_(upper, complex(2.0, -0.5), xv, complex(3.0, 0.25), V(b), V(y)).to_numpy(),
                              cref.gs_mul(M, upper, complex(2.0, -0.5), x, complex(3.0, 0.25), b, y)), upper
        assert np.array_equal(xv.to_numpy(), x)


@pytest.mark.parametrize("T", CTYPES)
def test_vectors_not_aligned_to_their_element_give_the_same_bits(pkg, ctx, cref, op, T):
    """vectors that start half an element into an allocation take the per-component loads and stores"""
    M, A, S = op("stairs", T)
    assert cref.diag(M) == 0
    half = np.dtype(T).itemsize // 2
    rng = np.random.default_rng(21)
    x, y, b = (ch.cnormal(rng, T, M.n) for _ in range(3))

    def U(a):
        buf = pkg.HipVector(M.n + 1, T, ctx)
        v = pkg.HipVector.wrap(buf.ptr + half, M.n, T, ctx, owner=buf).copy_from_host(a)
        assert v.ptr % np.dtype(T).itemsize == half
        return v

    assert np.array_equal(S.diag_ldiv_(U(y), U(x)).to_numpy(), cref.ldiv(M, x))
    assert np.array_equal(S.offdiag_mul_(complex(2.0, -0.5), U(x), complex(3.0, 0.25), U(y)).to_numpy(),
                          cref.offdiag_mul(M, complex(2.0, -0.5), x, complex(3.0, 0.25), y))
    for upper in (True, False):
        xv = U(x)
        assert np.array_equal(S.gs_multiply_(upper, complex(-1.0, -0.0), xv, 1.0, U(b), xv).to_numpy(), cref.gs_mul(M, upper, complex(-1.0, -0.0), x, 1.0, b))
        sub = S.backward_sub_ if upper else S.forward_sub_
        assert np.array_equal(sub(U(x)).to_numpy(), cref.sub(M, upper, x)), upper
        assert np.array_equal(sub(U(x), 1.2, U(y)).to_numpy(), cref.sub(M, upper, x, 1.2, y)), upper
        assert np.array_equal(sub(U(x), 1, pkg.HipVector.from_numpy(y)).to_numpy(), cref.sub(M, upper, x, 1, y)), upper     # one aligned, one not


@pytest.mark.parametrize("T", CTYPES)
def test_reference_set_on_the_device(pkg, ctx, cref, T):
    """test/stationary.jl:21-52 for a complex T, the sparse half: all eight call forms, maxiter = 2n, omega = 1.2"""
    M, A, b, x0 = ch.reference_set(T, 1234322)
    n = M.n
    Ad = fx.dev(pkg, M)
    tol = math.sqrt(np.finfo(ch.real_of(T)).eps)
    Ah = A.toarray().astype(np.complex128)
    res = lambda x: np.linalg.norm(b - Ah @ x.astype(np.complex128)) / np.linalg.norm(b)
    V = pkg.HipVector.from_numpy
    zero = np.zeros(n, T)
    got = [pkg.jacobi(Ad, V(b), maxiter=2 * n), pkg.gauss_seidel(Ad, V(b), maxiter=2 * n), pkg.sor(Ad, V(b), 1.2, maxiter=2 * n),
           pkg.ssor(Ad, V(b), 1.2, maxiter=2 * n),
           pkg.jacobi_(V(x0), Ad, V(b), maxiter=2 * n), pkg.gauss_seidel_(V(x0), Ad, V(b), maxiter=2 * n), pkg.sor_(V(x0), Ad, V(b), 1.2, maxiter=2 * n),
           pkg.ssor_(V(x0), Ad, V(b), 1.2, maxiter=2 * n)]
    want = [cref.jacobi(M, b, zero, 2 * n)[0], cref.gauss_seidel(M, b, zero, 2 * n)[0], cref.sor(M, b, zero, 1.2, 2 * n)[1], cref.ssor(M, b, zero, 1.2, 2 * n)[0],
            cref.jacobi(M, b, x0, 2 * n)[0], cref.gauss_seidel(M, b, x0, 2 * n)[0], cref.sor(M, b, x0, 1.2, 2 * n)[1], cref.ssor(M, b, x0, 1.2, 2 * n)[0]]
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.to_numpy()
        assert g.dtype == np.dtype(T) and res(g) <= tol, k
        assert np.array_equal(g, w), k


@pytest.mark.parametrize("T", CTYPES)
def test_singular_diagonals(pkg, ctx, T):
    """SingularException(col) for a missing and for a (0, -0.0) diagonal; a (0, tiny) diagonal is not singular"""
    for M, col in ch.singular_cases(T):
        A = fx.dev(pkg, M)
        b = pkg.HipVector.from_numpy(np.ones(3, T))
        if col == 0:
            assert pkg.StationaryOperator(A).info()["levels_forward"] >= 1
            continue
        for call in (lambda: pkg.StationaryOperator(A), lambda: pkg.jacobi(A, b), lambda: pkg.gauss_seidel(A, b), lambda: pkg.sor(A, b, 0.5),
                     lambda: pkg.ssor(A, b, 0.5)):
            with pytest.raises(pkg.SingularException) as e:
                call()
            assert e.value.col == col


def test_real_run_keeps_its_bits_around_a_complex_one(pkg, ctx, cref, tmp_path):
    """laplace_matrix(10, 3), the smallest operator of tests/test_gpu_stationary.py that has levels: the same bits before and after a
    complex run, and the real checker's"""
    ref = sh.build(tmp_path)
    M = sh.Mat.from_csc(*pkg.fixtures.laplace_matrix(10, 3))
    A = fx.dev(pkg, M)
    rng = np.random.default_rng(3)
    b, x0 = rng.standard_normal(M.n), rng.standard_normal(M.n)
    V = pkg.HipVector.from_numpy

    def real_run():
        return [pkg.jacobi_(V(x0), A, V(b), maxiter=3).to_numpy(), pkg.gauss_seidel_(V(x0), A, V(b), maxiter=3).to_numpy(),
                pkg.sor_(V(x0), A, V(b), 1.3, maxiter=3).to_numpy(), pkg.ssor_(V(x0), A, V(b), 1.3, maxiter=3).to_numpy()]

    before = real_run()
    Mc = ch.fixture("edges", np.complex128)
    ch.check_methods(pkg, cref, Mc, fx.dev(pkg, Mc), 1.2, 2, np.random.default_rng(4))
    after = real_run()
    want = [ref.jacobi(M, b, x0, 3)[0], ref.gauss_seidel(M, b, x0, 3)[0], ref.sor(M, b, x0, 1.3, 3)[1], ref.ssor(M, b, x0, 1.3, 3)[0]]
    for p, q, w in zip(before, after, want):
        assert p.dtype == np.float64 and np.array_equal(p, q) and np.array_equal(p, w)


def test_the_other_complex_refusals_still_hold(pkg, ctx):
    """JacobiPrec on complex vectors, the fused handles, mik_dense_mm on a complex matrix, complex CGS / DGKS, and the dense stationary
    methods on a complex HipMatrix"""
    import ctypes as C
    T = np.complex128
    M = ch.fixture("edges", T)
    A = fx.dev(pkg, M)
    bv = pkg.HipVector.from_numpy(ch.cnormal(np.random.default_rng(1), T, M.n))
    with pytest.raises(TypeError, match="JacobiPrec.*complex"):
        pkg.cg(A, bv, Pl=pkg.JacobiPrec(bv))
    x0 = bv.zero()
    with pytest.raises(pkg.MikError) as e:
        pkg.CGIterable(A, x0, bv, pkg.CGStateVariables(x0.zero(), x0.similar(), x0.similar()), pkg.Identity(), abstol=0.0, reltol=1e-8, maxiter=3,
                       initially_zero=True)
    assert e.value.code == 5
    with pytest.raises(pkg.MikError) as e:
        pkg.GMRESIterable(x0, A, bv, abstol=0.0, reltol=1e-8, restart=3, maxiter=3, initially_zero=True, orth_meth=pkg.ModifiedGramSchmidt())
    assert e.value.code == 5
    D = pkg.HipMatrix(5, 5, T, ctx)
    X = pkg.HipMatrix(5, 2, T, ctx)
    with pytest.raises(TypeError, match=str(np.dtype(T))):
        D.mm_(X, X)
    V = pkg.HipMatrix(8, 3, T, ctx)
    w = pkg.HipVector.from_numpy(ch.cnormal(np.random.default_rng(2), T, 8))
    for method in (pkg.ClassicalGramSchmidt(), pkg.DGKS()):
        with pytest.raises(pkg.MikError, match=type(method).__name__) as e:
            pkg.orthogonalize_and_normalize_(V, 2, w, np.zeros(2, T), method)
        assert e.value.code == 5
    d5 = pkg.HipVector.from_numpy(np.ones(5, T))
    with pytest.raises(pkg.MikError) as e:                              # the dense family stays real: mik_dense_stationary_create, MIK_ERR_INVALID
        pkg.jacobi(D, d5)
    assert e.value.code == 1
