"""The CPU checker of the complex stationary methods: tests/complex_ref/complex_stationary_ref.c (the reference's CSC column loops on
(re, im) pairs, with the complex division in both forms) against exact rational quotients, against an independent sequential ROW-view
restatement in plain Python over numpy scalars of the component type, bit for bit, and against the assertions of test/stationary.jl for
T in (ComplexF32, ComplexF64).  The last three tests are the host side of the package: the element-type gate, -one(T) and
_relax_scalars.  No GPU.

Observed maxima of the division test (the bounds are the issue's: 4 * 2^-52 and 1 * 2^-23 normwise):
    64-bit,  40 000 random quotients, exponents +-300:   1.168 * 2^-52
    widened 32-bit, 20 000 random quotients, exponents +-20:   0.496 * 2^-23"""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import complex_stationary_host as ch
from complex_stationary_host import cref  # noqa: F401  (fixture)
from conftest import graft

CTYPES = ch.CTYPES


# ---- the division --------------------------------------------------------------------------------------------------------------------
def _wide(rng, count, span):
    return rng.choice([-1.0, 1.0], size=count) * np.exp2(rng.uniform(-span, span, size=count)) * (1 + rng.random(count))


def test_cx_div_64_against_exact_quotients(cref):
    """random components over exponents +-300, |log2(max|z| / max|w|)| < 600 so that the quotient is finite; normwise error <= 4 * 2^-52"""
    rng = np.random.default_rng(52)
    count = 40000
    a, b, c, d = (_wide(rng, count, 300) for _ in range(4))
    bound_sq = Fraction(4, 2 ** 52) ** 2
    worst, used = Fraction(0), 0
    for k in range(count):
        z, w = complex(a[k], b[k]), complex(c[k], d[k])
        if abs(math.log2(max(abs(a[k]), abs(b[k]))) - math.log2(max(abs(c[k]), abs(d[k])))) >= 600:
            continue
        used += 1
        q = cref.div(z, w, np.complex128)
        assert np.isfinite(q)
        worst = max(worst, ch.normwise_error_sq(q, z, w))
    print(f"64-bit division: {used} quotients, largest normwise error {math.sqrt(worst) * 2 ** 52:.3f} * 2^-52")
    assert used > 0.9 * count
    assert worst <= bound_sq


def test_cx_div_widened_32_against_exact_quotients(cref):
    """Float32 components over exponents +-20; normwise error <= 1 * 2^-23"""
    rng = np.random.default_rng(23)
    count = 20000
    a, b, c, d = (_wide(rng, count, 20).astype(np.float32) for _ in range(4))
    bound_sq = Fraction(1, 2 ** 23) ** 2
    worst = Fraction(0)
    for k in range(count):
        z, w = np.complex64(complex(a[k], b[k])), np.complex64(complex(c[k], d[k]))
        q = cref.div(z, w, np.complex64)
        assert np.isfinite(q) and q.dtype == np.complex64
        worst = max(worst, ch.normwise_error_sq(q, z, w))
    print(f"widened 32-bit division: {count} quotients, largest normwise error {math.sqrt(worst) * 2 ** 23:.3f} * 2^-23")
    assert worst <= bound_sq


# which branches a 64-bit quotient takes, from the definition (floatmax / 2, floatmin * 2 / eps, r and b r as the algorithm forms them)
def _branches_taken(z, w):
    fi = np.finfo(np.float64)
    a, b, c, d = (np.float64(v) for v in (z.real, z.imag, w.real, w.imag))
    ab, cd = max(abs(a), abs(b)), max(abs(c), abs(d))
    took = set()
    bs = np.float64(2.0) / (fi.eps * fi.eps)
    if ab >= fi.max / 2:
        took.add("ab-large"); a, b = a / 2, b / 2
    if cd >= fi.max / 2:
        took.add("cd-large"); c, d = c / 2, d / 2
    if ab <= fi.tiny * 2 / fi.eps:
        took.add("ab-small"); a, b = a * bs, b * bs
    if cd <= fi.tiny * 2 / fi.eps:
        took.add("cd-small"); c, d = c * bs, d * bs
    if abs(d) <= abs(c):
        took.add("d<=c")
    else:
        took.add("d>c"); a, b, c, d = b, a, d, c
    r = d / c
    if r == 0:
        took.add("r==0")
    else:
        for bb in (b, -a):
            took.add("br==0" if bb * r == 0 else "br!=0")
    return took


def test_hand_made_quotients_take_every_branch_and_match_the_exact_quotient(cref):
    seen = set()
    bound_sq = Fraction(4, 2 ** 52) ** 2
    with np.errstate(under="ignore"):
        for z, w, what in ch.BRANCHES:
            seen |= _branches_taken(z, w)
            q = cref.div(z, w, np.complex128)
            assert np.isfinite(q), what
            assert ch.normwise_error_sq(q, z, w) <= bound_sq, what
    assert seen == {"ab-large", "cd-large", "ab-small", "cd-small", "d<=c", "d>c", "r==0", "br==0", "br!=0"}
    want = {"ab >= floatmax/2": "ab-large", "cd >= floatmax/2": "cd-large", "ab <= floatmin*2/eps": "ab-small", "cd <= floatmin*2/eps": "cd-small",
            "|d| <= |c|": "d<=c", "|d| > |c|": "d>c", "r == 0: d == 0": "r==0", "r == 0 after the swap: c == 0": "r==0",
            "r == 0: d / c underflows": "r==0", "br == 0: b == 0": "br==0", "br == 0 in the imaginary part: -a == 0": "br==0",
            "br == 0: b * r underflows, r != 0": "br==0"}
    with np.errstate(under="ignore"):
        for z, w, what in ch.BRANCHES:
            assert want[what] in _branches_taken(z, w), what
    bound32 = Fraction(1, 2 ** 23) ** 2
    for z, w, what in ch.BRANCHES32:
        z, w = np.complex64(z), np.complex64(w)
        assert ch.normwise_error_sq(cref.div(z, w, np.complex64), z, w) <= bound32, what


# ---- the independent restatement: a sequential row view over numpy scalars of the component type ----------------------------------------------
class Py:
    """element operations on (re, im) tuples of numpy scalars of one real type E"""

    def __init__(self, E):
        self.E = np.dtype(E).type

    def of(self, z):
        return (self.E(z.real), self.E(z.imag))

    def mul(self, z, w):
        a, b, c, d = z[0] * w[0], z[1] * w[1], z[0] * w[1], z[1] * w[0]
        return (a - b, c + d)

    def add(self, z, w):
        return (z[0] + w[0], z[1] + w[1])

    def sub(self, z, w):
        return (z[0] - w[0], z[1] - w[1])

    def div(self, z, w):
        return self._div32(z, w) if self.E is np.float32 else self._div64(z, w)

    @staticmethod
    def _div32(z, w):
        a, b, c, d = (np.float64(v) for v in (z[0], z[1], w[0], w[1]))
        mag = np.float64(1.0) / ch.fma(c, c, d * d)
        return (np.float32(ch.fma(a, c, b * d) * mag), np.float32(ch.fma(b, c, -(a * d)) * mag))

    @staticmethod
    def _div64(z, w):
        fi = np.finfo(np.float64)
        a, b, c, d = z[0], z[1], w[0], w[1]
        one, two, half = np.float64(1), np.float64(2), np.float64(0.5)
        ab, cd = max(abs(a), abs(b)), max(abs(c), abs(d))
        bs = two / (fi.eps * fi.eps)
        s = one
        if ab >= fi.max / two:
            a, b, s = a * half, b * half, s * two
        if cd >= fi.max / two:
            c, d, s = c * half, d * half, s * half
        if ab <= fi.tiny * two / fi.eps:
            a, b, s = a * bs, b * bs, s / bs
        if cd <= fi.tiny * two / fi.eps:
            c, d, s = c * bs, d * bs, s * bs

        def div2(a, b, c, d, r, t):
            if r != 0:
                br = b * r
                return (a + br) * t if br != 0 else a * t + (b * t) * r
            return (a + d * (b / c)) * t

        def div1(a, b, c, d):
            r = d / c
            t = one / (c + d * r)
            return div2(a, b, c, d, r, t), div2(b, -a, c, d, r, t)

        if abs(d) <= abs(c):
            p, q = div1(a, b, c, d)
        else:
            p, q = div1(b, a, d, c)
            q = -q
        return (p * s, q * s)


def _to_list(P, v):
    return [P.of(z) for z in v]


def _to_array(v, T):
    out = np.empty(len(v), T)
    out.real = np.array([z[0] for z in v], ch.real_of(T))              # part by part: the bits and the signs of zero as they are
    out.imag = np.array([z[1] for z in v], ch.real_of(T))
    return out


class RowView:
    """the building blocks on the rows of a CMat: the term orders of include/mik.h, "Stationary methods" """

    def __init__(self, M):
        self.M, self.T = M, M.dtype
        self.P = Py(ch.real_of(M.dtype))
        rp, cl, vl = M.csr()
        self.rows = [[(int(cl[k]), self.P.of(vl[k])) for k in range(rp[i], rp[i + 1])] for i in range(M.n)]
        self.d = [next(v for j, v in row if j == i) for i, row in enumerate(self.rows)]

    def out(self, v):
        a = _to_array(v, self.T)
        assert a.dtype == self.T
        return a

    def ldiv(self, x):
        P = self.P
        return self.out([P.div(P.of(x[i]), self.d[i]) for i in range(self.M.n)])

    def offdiag_mul(self, alpha, x, beta, y):
        P = self.P
        al, be = P.of(self.T.type(alpha)), P.of(self.T.type(beta))
        out = []
        for i, row in enumerate(self.rows):
            acc = P.of(self.T.type(0)) if be == (0, 0) else (P.of(y[i]) if be == (1, 0) else P.mul(be, P.of(y[i])))
            for j, a in row:
                if j != i:
                    acc = P.add(acc, P.mul(a, P.mul(al, P.of(x[j]))))
            out.append(acc)
        return self.out(out)

    def gs_mul(self, upper, alpha, x, beta, y):
        P = self.P
        al, be = P.of(self.T.type(alpha)), P.of(self.T.type(beta))
        out = []
        for i, row in enumerate(self.rows):
            acc = P.mul(be, P.of(y[i]))
            terms = [(j, a) for j, a in row if j > i] if upper else [(j, a) for j, a in reversed(row) if j < i]
            for j, a in terms:
                acc = P.add(acc, P.mul(a, P.mul(al, P.of(x[j]))))
            out.append(acc)
        return self.out(out)

    def sub(self, upper, x, omega=None, y=None):
        P, n = self.P, self.M.n
        x = _to_list(P, x)
        if omega is not None:
            E = np.float32 if ch.omega32(omega, self.T) else np.float64
            PE = Py(E)
            al = PE.E(omega)
            be = (PE.E(1) - al, PE.E(0.0))
        for i in (range(n - 1, -1, -1) if upper else range(n)):
            acc = x[i]
            terms = [(j, a) for j, a in reversed(self.rows[i]) if j > i] if upper else [(j, a) for j, a in self.rows[i] if j < i]
            for j, a in terms:
                acc = P.sub(acc, P.mul(a, x[j]))
            if omega is None:
                x[i] = P.div(acc, self.d[i])
            else:
                ax = (al * PE.E(acc[0]), al * PE.E(acc[1]))
                q = PE.div(ax, (PE.E(self.d[i][0]), PE.E(self.d[i][1])))
                r = PE.mul(be, (PE.E(y[i].real), PE.E(y[i].imag)))
                x[i] = (P.E(q[0] + r[0]), P.E(q[1] + r[1]))
        return self.out(x)

    # the four iterations, composed as the iterables compose them
    def jacobi(self, b, x, k):
        for _ in range(k):
            x = self.ldiv(self.offdiag_mul(complex(-1.0, -0.0), x, 1, b))
        return x

    def gauss_seidel(self, b, x, k):
        for _ in range(k):
            x = self.sub(False, self.gs_mul(True, complex(-1.0, -0.0), x, 1, b))
        return x

    def sor(self, b, x, omega, k):
        for _ in range(k):
            x = self.sub(False, self.gs_mul(True, complex(-1.0, -0.0), x, 1, b), omega, x)
        return x

    def ssor(self, b, x, omega, k):
        for _ in range(k):
            t = self.sub(False, self.gs_mul(True, complex(-1.0, -0.0), x, 1, b), omega, x)
            x = self.sub(True, self.gs_mul(False, complex(-1.0, -0.0), t, 1, b), omega, t)
        return x


@pytest.fixture(scope="module")
def rowview():
    made = {}

    def get(T):
        T = np.dtype(T)
        if T not in made:
            made[T] = RowView(ch.fixture("edges", T))
        return made[T]

    return get


@pytest.mark.parametrize("T", CTYPES)
def test_complexified_fixtures_keep_pattern_dominance_and_plans(T):
    """every staged fixture: ch.fixture asserts the pattern, |d| > 1.9 off + 0.9 on the rounded values and the plans pinned in FIXTURES"""
    import stationary_fixtures as fx
    for name in fx.STAGED:
        M = ch.fixture(name, T)
        Mr = fx.fixture(name, np.float64)
        assert M.dtype == np.dtype(T) and M.n == Mr.n and [len(p) for p in M.plans] == [len(p) for p in Mr.plans]


@pytest.mark.parametrize("T", CTYPES)
def test_row_parallel_routines_equal_the_python_loop(cref, rowview, T):
    M = ch.fixture("edges", T)
    R = rowview(T)
    assert cref.diag(M) == 0
    rng = np.random.default_rng(31)
    x, y, b = (ch.cnormal(rng, T, M.n) for _ in range(3))
    assert np.array_equal(cref.ldiv(M, x), R.ldiv(x))
    for al, be in ((1.0, 0.0), (1.0, 1.0), (complex(2.0, -0.5), complex(3.0, 0.25)), (complex(-1.0, -0.0), 1.0), (complex(0.0, 1.0), complex(1.0, 1e-3))):
        assert np.array_equal(cref.offdiag_mul(M, al, x, be, y), R.offdiag_mul(al, x, be, y)), (al, be)
    for upper in (True, False):
        want = R.gs_mul(upper, complex(2.0, -0.5), x, complex(3.0, 0.25), b)
        assert np.array_equal(cref.gs_mul(M, upper, complex(2.0, -0.5), x, complex(3.0, 0.25), b, y), want), upper
        assert np.array_equal(cref.gs_mul(M, upper, complex(-1.0, -0.0), x, 1.0, b), R.gs_mul(upper, complex(-1.0, -0.0), x, 1.0, b)), upper   # z === x


@pytest.mark.parametrize("omega", (None,) + ch.OMEGAS, ids=["plain"] + ch.OMEGA_IDS)
@pytest.mark.parametrize("upper", (False, True), ids=["forward", "backward"])
@pytest.mark.parametrize("T", CTYPES)
def test_substitutions_equal_the_python_loop(cref, rowview, T, upper, omega):
    M = ch.fixture("edges", T)
    R = rowview(T)
    assert cref.diag(M) == 0
    rng = np.random.default_rng(32)
    x, y = ch.cnormal(rng, T, M.n), ch.cnormal(rng, T, M.n)
    got = cref.sub(M, upper, x, omega, None if omega is None else y)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, R.sub(upper, x, omega, None if omega is None else y))


@pytest.mark.parametrize("omega", ch.OMEGAS, ids=ch.OMEGA_IDS)
@pytest.mark.parametrize("T", CTYPES)
def test_iterables_equal_the_python_loop(cref, rowview, T, omega):
    M = ch.fixture("edges", T)
    R = rowview(T)
    rng = np.random.default_rng(33)
    b, x0 = ch.cnormal(rng, T, M.n), ch.cnormal(rng, T, M.n)
    k = 2
    assert np.array_equal(cref.jacobi(M, b, x0, k)[0], R.jacobi(b, x0, k))
    assert np.array_equal(cref.gauss_seidel(M, b, x0, k)[0], R.gauss_seidel(b, x0, k))
    xs, it_x, which = cref.sor(M, b, x0, omega, k)
    assert which == 0 and np.array_equal(it_x, R.sor(b, x0, omega, k))
    xs, it_x, which = cref.sor(M, b, x0, omega, 1)
    assert which == 1 and np.array_equal(it_x, R.sor(b, x0, omega, 1)) and np.array_equal(xs, x0)
    assert np.array_equal(cref.ssor(M, b, x0, omega, k)[0], R.ssor(b, x0, omega, k))


# ---- the reference's assertions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (1234322, 7))
@pytest.mark.parametrize("T", CTYPES)
def test_reference_set_converges_in_all_eight_call_forms(cref, T, seed):
    """test/stationary.jl:21-52 for T in (ComplexF32, ComplexF64), the sparse half: sprand(T, n, n, 4/n) + 2n I, maxiter = 2n, omega = 1.2"""
    M, A, b, x0 = ch.reference_set(T, seed)
    n = M.n
    tol = math.sqrt(np.finfo(ch.real_of(T)).eps)
    Ad = A.toarray().astype(np.complex128)
    res = lambda x: np.linalg.norm(b - Ad @ x.astype(np.complex128)) / np.linalg.norm(b)
    for x in (np.zeros(n, T), x0):                                      # solver(A, b) starts from zerox; solver!(copy(x0), A, b)
        assert res(cref.jacobi(M, b, x, maxiter=2 * n)[0]) <= tol
        assert res(cref.gauss_seidel(M, b, x, maxiter=2 * n)[0]) <= tol
        assert res(cref.sor(M, b, x, 1.2, maxiter=2 * n)[1]) <= tol
        assert res(cref.ssor(M, b, x, 1.2, maxiter=2 * n)[0]) <= tol


@pytest.mark.parametrize("T", CTYPES)
def test_gauss_seidel_and_sor_with_omega_one_coincide(cref, T):
    """test/stationary.jl:56-68"""
    M, A, _, _ = ch.reference_set(T, 11)
    b = (A.astype(np.complex128) @ np.ones(M.n)).astype(T)
    for k in range(1, 6):
        xg, _ = cref.gauss_seidel(M, b, np.zeros(M.n, T), maxiter=k)
        _, xs, _ = cref.sor(M, b, np.zeros(M.n, T), 1.0, maxiter=k)
        assert np.allclose(xg, xs, rtol=math.sqrt(np.finfo(ch.real_of(T)).eps), atol=0)


@pytest.mark.parametrize("T", CTYPES)
def test_singular_diagonals(cref, T):
    """DiagonalIndices :14-19 with iszero(::Complex): a missing diagonal and a (0, -0.0) one throw with the column; (0, tiny) does not"""
    for M, col in ch.singular_cases(T):
        assert cref.diag(M) == col
        assert cref.jacobi(M, np.ones(3, T), np.zeros(3, T))[1] == col
        assert cref.sor(M, np.ones(3, T), np.zeros(3, T), 0.5)[2] == col
        assert cref.ssor(M, np.ones(3, T), np.zeros(3, T), 0.5)[1] == col


# ---- the host side of the package ------------------------------------------------------------------------------------------------------------
def _stationary():
    from importlib import import_module
    return import_module(graft.load_package().__name__ + ".stationary")


@pytest.mark.parametrize("T,rt,ct", [(np.complex128, np.float64, np.complex128), (np.complex64, np.float32, np.complex64)])
def test_relax_scalars_for_a_complex_element_type(T, rt, ct):
    """E = the real type of promote(real(T), typeof(omega)); alpha = E(omega) REAL; beta = one(T) - omega COMPLEX with imaginary part +0.0"""
    st = _stationary()
    a, b, E = st._relax_scalars(T, 1.2)                                  # a Float64 omega widens ComplexF32 to Float64
    assert E == np.float64 and type(a) is np.float64 and a == 1.2
    assert type(b) is np.complex128 and b.real == np.float64(1) - np.float64(1.2) and b.imag == 0 and not np.signbit(b.imag)
    a, b, E = st._relax_scalars(T, np.float32(0.8))                      # a Float32 omega keeps ComplexF32 in Float32
    assert E == rt and type(a) is rt and a == rt(np.float32(0.8))
    assert type(b) is ct and b.real == rt(1) - rt(np.float32(0.8)) and b.imag == 0 and not np.signbit(b.imag)
    a, b, E = st._relax_scalars(T, 1)                                    # an Int omega evaluates in real(T)
    assert E == rt and type(a) is rt and a == 1
    assert type(b) is ct and b.real == 0 and not np.signbit(b.real) and b.imag == 0 and not np.signbit(b.imag)
    a, b, E = st._relax_scalars(T, 2)
    assert b.real == -1 and b.imag == 0 and not np.signbit(b.imag)
    with pytest.raises(TypeError):
        st._relax_scalars(T, 1.2 + 0j)


def test_relax_scalars_for_a_real_element_type_are_unchanged():
    st = _stationary()
    for T, omega, S in ((np.float64, 1.2, np.float64), (np.float32, 1.2, np.float64), (np.float32, np.float32(0.8), np.float32), (np.float32, 1, np.float32),
                        (np.float64, np.float32(0.8), np.float64)):
        a, b, got = st._relax_scalars(T, omega)
        assert got == S and type(a) is S and type(b) is S and a == S(omega) and b == S(1) - S(omega)


def test_minus_one_of_a_complex_type_negates_both_parts():
    """-one(T) for a complex T is (-1.0, -0.0): Julia's unary minus negates the imaginary part too"""
    st = _stationary()
    for T in CTYPES:
        m = np.asarray([st._minus_one(T)], T)[0]
        assert m.real == -1 and m.imag == 0 and np.signbit(m.imag)
    assert st._minus_one(np.float64) == -1 and st._minus_one(np.float32) == -1
