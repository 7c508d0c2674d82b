"""What tests/test_complex_stationary_host.py and tests/test_gpu_complex_stationary.py share: the ctypes binding of
tests/complex_ref/complex_stationary_ref.c (`CRef`, with the methods of stationary_host.Ref), the complex operators -- the real
fixtures of tests/stationary_fixtures.py with a random unit-modulus phase on every stored entry, pattern and moduli kept -- the
reference's n = 10 set, and the quotients that take every branch of the 64-bit division.  Test infrastructure only."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import stationary_fixtures as fx
import stationary_host as sh

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "complex_ref", "complex_stationary_ref.c")
_i64p = C.POINTER(C.c_int64)
_vp = C.c_void_p
CTYPES = (np.complex128, np.complex64)
OMEGAS = (1.2, np.float32(0.8), 1)              # a Float64, a Float32 and an Int omega
OMEGA_IDS = ["float", "float32", "int"]


def real_of(dtype):
    return np.dtype(np.dtype(dtype).type(0).real.dtype)


def build(outdir):
    """gcc -std=c99 -O2 -ffp-contract=off -lm -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "complex_stationary_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    return CRef(C.CDLL(so))


@pytest.fixture(scope="session")
def cref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("complex_stationary_ref"))


def _p(a):
    return a.ctypes.data_as(_vp)


class CMat(sh.Mat):
    """sh.Mat with a complex nzval: 0-based int64 colptr / rowval, sorted row indices"""

    def __init__(self, m, dtype):
        super().__init__(m, dtype)
        assert self.dtype.kind == "c"
        self.sfx = "f64" if self.dtype == np.complex128 else "f32"

    def csr(self):
        """(rowptr, col, val) with ascending columns: the row view of the independent restatements"""
        R = sp.csc_matrix((self.nz, self.rv, self.cp), shape=(self.n, self.n)).tocsr()
        R.sort_indices()
        assert R.nnz == self.nz.size                            # explicit zeros survive
        return R.indptr.astype(np.int64), R.indices.astype(np.int64), R.data.astype(self.dtype)


def omega32(omega, dtype):
    """True when the relaxed substitutions of ComplexF32 data run in Float32: a Float32 or an Int omega (Julia's promotion)"""
    return np.dtype(dtype) == np.complex64 and isinstance(omega, (np.float32, int, np.integer))


class CRef:
    """the C checker; the methods and return values of stationary_host.Ref.  Scalars of offdiag_mul / gs_mul are complex."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("cst_jacobi", "cst_gauss_seidel", "cst_sor", "cst_ssor", "cst_diag"):
                getattr(lib, f"{name}_{sfx}").restype = C.c_int64
        lib.cst_div_f64.argtypes = [C.c_double] * 4 + [_vp]
        lib.cst_div_f32.argtypes = [C.c_float] * 4 + [_vp]

    def _fn(self, name, M):
        return getattr(self.L, f"{name}_{M.sfx}")

    def div(self, z, w, dtype):
        """z / w in `dtype` (complex128: the robust division; complex64: the widened one)"""
        out = np.zeros(1, dtype)
        z, w = np.dtype(dtype).type(z), np.dtype(dtype).type(w)
        (self.L.cst_div_f64 if np.dtype(dtype) == np.complex128 else self.L.cst_div_f32)(float(z.real), float(z.imag), float(w.real), float(w.imag), _p(out))
        return out[0]

    def diag(self, M):
        return self._fn("cst_diag", M)(*M.args(), M.diag.ctypes.data_as(_i64p))

    # ---- whole methods ------------------------------------------------------------------------------------------------------------
    def jacobi(self, M, b, x, maxiter=10):
        x, w = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        s = self._fn("cst_jacobi", M)(*M.args(), _p(np.ascontiguousarray(b, M.dtype)), _p(x), _p(w), C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    def gauss_seidel(self, M, b, x, maxiter=10):
        x = np.array(x, M.dtype)
        s = self._fn("cst_gauss_seidel", M)(*M.args(), _p(np.ascontiguousarray(b, M.dtype)), _p(x), C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    def sor(self, M, b, x, omega, maxiter=10):
        """(caller's x, iterable.x, which) -- which = 1: iterable.x is the internal buffer (odd maxiter)"""
        x, w = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        which = C.c_int()
        s = self._fn("cst_sor", M)(*M.args(), _p(np.ascontiguousarray(b, M.dtype)), _p(x), _p(w), C.c_double(float(omega)), int(omega32(omega, M.dtype)),
                                   C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p), C.byref(which))
        if s:
            return None, None, s
        return x, (w if which.value else x), which.value

    def ssor(self, M, b, x, omega, maxiter=10):
        x, t = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        s = self._fn("cst_ssor", M)(*M.args(), _p(np.ascontiguousarray(b, M.dtype)), _p(x), _p(t), C.c_double(float(omega)), int(omega32(omega, M.dtype)),
                                    C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    # ---- building blocks (diag() first) -------------------------------------------------------------------------------------------
    def ldiv(self, M, x):
        y = np.zeros(M.n, M.dtype)
        self._fn("cst_ldiv", M)(C.c_int64(M.n), _p(M.nz), M.diag.ctypes.data_as(_i64p), _p(y), _p(np.ascontiguousarray(x, M.dtype)))
        return y

    def offdiag_mul(self, M, alpha, x, beta, y):
        y = np.array(y, M.dtype)
        self._fn("cst_offdiag_mul", M)(*M.args(), M.diag.ctypes.data_as(_i64p), _p(np.asarray([alpha], M.dtype)), _p(np.ascontiguousarray(x, M.dtype)),
                                       _p(np.asarray([beta], M.dtype)), _p(y))
        return y

    def gs_mul(self, M, upper, alpha, x, beta, y, z=None):
        """z = None: z is x (in place)"""
        x = np.array(x, M.dtype)
        z = x if z is None else np.array(z, M.dtype)
        self._fn("cst_gs_mul_upper" if upper else "cst_gs_mul_lower", M)(*M.args(), M.diag.ctypes.data_as(_i64p), _p(np.asarray([alpha], M.dtype)), _p(x),
                                                                          _p(np.asarray([beta], M.dtype)), _p(np.ascontiguousarray(y, M.dtype)), _p(z))
        return z

    def sub(self, M, upper, x, omega=None, y=None):
        """forward_sub! / backward_sub!, plain (omega None) or relaxed with alpha = omega, beta = one(T) - omega"""
        x = np.array(x, M.dtype)
        kind = "cst_backward_sub" if upper else "cst_forward_sub"
        dbl, flt = C.c_double, C.c_float
        if omega is None:
            ct = dbl if M.sfx == "f64" else flt
            getattr(self.L, f"{kind}_{M.sfx}")(*M.args(), M.diag.ctypes.data_as(_i64p), 0, ct(0), _p(x), ct(0), ct(0), None)
            return x
        y = np.ascontiguousarray(y, M.dtype)
        if M.sfx == "f64":
            a = np.float64(omega)
            getattr(self.L, f"{kind}_f64")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, dbl(a), _p(x), dbl(1.0 - a), dbl(0.0), _p(y))
        elif omega32(omega, M.dtype):
            a = np.float32(omega)
            getattr(self.L, f"{kind}_f32")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, flt(a), _p(x), flt(np.float32(1) - a), flt(0.0), _p(y))
        else:
            a = float(omega)
            getattr(self.L, f"{kind}_f32w")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, dbl(a), _p(x), dbl(1.0 - a), dbl(0.0), _p(y))
        return x


# ---- operators -------------------------------------------------------------------------------------------------------------------------
def complexify(Mr, T, seed):
    """every stored entry of a real sh.Mat (diagonal included) times its own random unit-modulus phase, rounded to T: the pattern is
    kept, so are the moduli up to the rounding -- strict row dominance is asserted on the rounded values"""
    rng = np.random.default_rng(seed)
    phase = np.exp(2j * np.pi * rng.random(Mr.nz.size))
    nz = (Mr.nz.astype(np.float64) * phase).astype(T)
    M = CMat(sp.csc_matrix((nz, Mr.rv, Mr.cp), shape=(Mr.n, Mr.n)), T)
    assert np.array_equal(M.cp, Mr.cp) and np.array_equal(M.rv, Mr.rv) and M.nz.size == Mr.nz.size
    mod = np.abs(M.nz.astype(np.complex128))
    col = np.repeat(np.arange(M.n), np.diff(M.cp))
    isd = M.rv == col
    off = np.bincount(M.rv[~isd], weights=mod[~isd], minlength=M.n)
    d = np.zeros(M.n)
    d[M.rv[isd]] = mod[isd]
    assert np.all(d > 1.9 * off + 0.9), "complexify: the rounded operator is not strictly dominant"
    assert np.all(np.isfinite(M.nz)) and np.any(M.nz.imag != 0)
    return M


@functools.lru_cache(maxsize=None)
def fixture(name, T):
    """the complexified fixture `name` of tests/stationary_fixtures.py (built once per session and type; nobody writes to it), with
    M.widths and M.plans recomputed on the complex operator and asserted to be the ones pinned in fx.FIXTURES"""
    Mr = fx.fixture(name, np.float64)
    M = complexify(Mr, np.dtype(T).type, seed=900 + sorted(fx.FIXTURES).index(name))
    M.widths = fx.level_widths(M)
    M.plans = tuple(fx.launch_plan(w) for w in M.widths)
    assert M.widths == Mr.widths
    assert (fx.kinds(M.plans[0]), fx.kinds(M.plans[1])) == fx.FIXTURES[name][1:]
    return M


def crand(rng, T, n):
    """rand(T, n): re and im uniform in [0, 1)"""
    rt = real_of(T)
    return (rng.random(n).astype(rt) + 1j * rng.random(n).astype(rt)).astype(T)


def cnormal(rng, T, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(T)


def reference_set(T, seed):
    """test/stationary.jl:16-31 for a complex T: A = sprand(T, 10, 10, 4/10) + 20 I, b = rand(T, 10), x0 = rand(T, 10)"""
    rng = np.random.default_rng(seed)
    n = 10
    S = sp.random(n, n, density=0.4, random_state=rng, format="csc", dtype=np.float64)
    S = sp.csc_matrix((crand(rng, np.complex128, S.nnz), S.indices, S.indptr), shape=(n, n))
    A = (S + 2 * n * sp.identity(n, format="csc")).tocsc().astype(T)
    return CMat(A, T), A, crand(rng, T, n), crand(rng, T, n)


def sprand_complex(n, per_row, T, seed, diagonal=None):
    """n x n, about `per_row` off-diagonal entries a row with mixed signs and magnitudes 2^-10 .. 2^10 in either part, and the given
    diagonal (default: of the same kind): for the row-parallel kernels, which do not iterate"""
    rng = np.random.default_rng(seed)

    def wide(k):
        part = lambda: rng.choice([-1.0, 1.0], size=k) * np.exp2(rng.uniform(-10, 10, size=k)) * (1 + rng.random(k))
        return part() + 1j * part()

    if n > 1:
        S = sp.random(n, n, density=min(1.0, per_row / n), random_state=rng, format="coo", dtype=np.float64)
        keep = S.row != S.col
        i, j = S.row[keep], S.col[keep]
    else:
        i = j = np.zeros(0, np.int64)
    d = wide(n) if diagonal is None else np.asarray(diagonal, np.complex128)
    assert d.size == n
    A = sp.csc_matrix((np.concatenate([wide(i.size), d]).astype(T), (np.concatenate([i, np.arange(n)]), np.concatenate([j, np.arange(n)]))), shape=(n, n))
    M = CMat(A, T)
    assert M.nz.size == i.size + n and np.all(np.isfinite(M.nz))
    return M


def singular_cases(T):
    """(CMat, singular column or 0): a missing diagonal, a stored (0, -0.0) diagonal, and a (0, 1e-300) / (0, 1e-30) one that is NOT singular"""
    tiny = 1e-300 if np.dtype(T) == np.complex128 else 1e-30
    out = [(CMat(sp.csc_matrix(np.array([[1 + 1j, 0, 0], [0, 1j, 2], [0, 3, 0]], T)), T), 3)]
    for dz, col in ((complex(0.0, -0.0), 2), (complex(-0.0, 0.0), 2), (complex(0.0, tiny), 0)):
        A = sp.csc_matrix((np.array([2 + 1j, 1.0, 3 - 1j], T), (np.array([0, 1, 2]), np.array([0, 1, 2]))), shape=(3, 3))
        A.data[1] = dz
        M = CMat(A, T)
        assert M.nz.size == 3 and M.nz[1].imag == T(dz).imag
        out.append((M, col))
    return out


def check_methods(pkg, ref, M, A, omega, k, rng):
    """stationary_fixtures.check_methods with complex vectors: jacobi! / gauss_seidel! / sor! (the returned vector and the caller's x) / ssor!"""
    T = M.dtype
    b, x0 = cnormal(rng, T, M.n), cnormal(rng, T, M.n)
    bd = pkg.HipVector.from_numpy(b)
    x = pkg.HipVector.from_numpy(x0)
    assert np.array_equal(pkg.jacobi_(x, A, bd, maxiter=k).to_numpy(), ref.jacobi(M, b, x0, k)[0]), "jacobi"
    x = pkg.HipVector.from_numpy(x0)
    assert np.array_equal(pkg.gauss_seidel_(x, A, bd, maxiter=k).to_numpy(), ref.gauss_seidel(M, b, x0, k)[0]), "gauss_seidel"
    x = pkg.HipVector.from_numpy(x0)
    xr, rr, _ = ref.sor(M, b, x0, omega, k)
    r = pkg.sor_(x, A, bd, omega, maxiter=k)
    assert np.array_equal(r.to_numpy(), rr) and np.array_equal(x.to_numpy(), xr), "sor"
    x = pkg.HipVector.from_numpy(x0)
    want = ref.ssor(M, b, x0, omega, k)[0]
    assert np.all(np.isfinite(want))
    assert np.array_equal(pkg.ssor_(x, A, bd, omega, maxiter=k).to_numpy(), want), "ssor"


# ---- the 64-bit division: quotients (z, w, what they are for) that take every branch ----------------------------------------------------------
BRANCHES = [
    (complex(1.5e308, 1.0e308), complex(3.0, 2.0), "ab >= floatmax/2"),
    (complex(1.0e300, -2.0e300), complex(1.2e308, -1.0e308), "cd >= floatmax/2"),
    (complex(1.0e-300, 3.0e-301), complex(1.5, 2.5), "ab <= floatmin*2/eps"),
    (complex(1.0e-10, -1.0e-12), complex(1.0e-300, -2.0e-300), "cd <= floatmin*2/eps"),
    (complex(1.0, 2.0), complex(3.0, 1.0), "|d| <= |c|"),
    (complex(1.0, 2.0), complex(-1.0, 3.0), "|d| > |c|"),
    (complex(1.5, 2.5), complex(3.0, 0.0), "r == 0: d == 0"),
    (complex(1.5, -2.5), complex(0.0, 3.0), "r == 0 after the swap: c == 0"),
    (complex(0.7, 1.3), complex(1.0e200, 1.0e-200), "r == 0: d / c underflows"),
    (complex(1.0, 0.0), complex(3.0, 1.0), "br == 0: b == 0"),
    (complex(0.0, 1.0), complex(3.0, -1.0), "br == 0 in the imaginary part: -a == 0"),
    (complex(1.0, 1.0e-200), complex(1.0, 1.0e-150), "br == 0: b * r underflows, r != 0"),
]
# for ComplexF32 the division has no branches: the same shapes with exponents a Float32 holds
BRANCHES32 = [
    (complex(1.5e30, 1.0e30), complex(3.0, 2.0), "large numerator"),
    (complex(1.0e10, -2.0e10), complex(1.2e18, -1.0e18), "large divisor"),
    (complex(1.0e-30, 3.0e-31), complex(1.5, 2.5), "small numerator"),
    (complex(1.0e-10, -1.0e-12), complex(1.0e-18, -2.0e-18), "small divisor"),
    (complex(1.0, 2.0), complex(3.0, 1.0), "|d| <= |c|"),
    (complex(1.0, 2.0), complex(-1.0, 3.0), "|d| > |c|"),
    (complex(1.5, 2.5), complex(3.0, 0.0), "d == 0"),
    (complex(1.5, -2.5), complex(0.0, 3.0), "c == 0"),
    (complex(1.0, 0.0), complex(3.0, 1.0), "b == 0"),
]


def branches(T):
    return BRANCHES if np.dtype(T) == np.complex128 else BRANCHES32


def exact_quotient(z, w):
    """(re, im) of z / w as Fractions (z, w: complex scalars whose parts are exact binary floats)"""
    a, b, c, d = (Fraction(float(v)) for v in (z.real, z.imag, w.real, w.imag))
    den = c * c + d * d
    return (a * c + b * d) / den, (b * c - a * d) / den


def normwise_error_sq(got, z, w):
    """|got - z/w|^2 / |z/w|^2, exactly"""
    er, ei = exact_quotient(z, w)
    gr, gi = Fraction(float(got.real)), Fraction(float(got.imag))
    return ((gr - er) ** 2 + (gi - ei) ** 2) / (er ** 2 + ei ** 2)


def fma(a, b, c):
    """the correctly rounded a * b + c of three doubles (float() of a Fraction rounds to nearest even)"""
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))
