"""ctypes binding of tests/stationary_ref/stationary_ref.c (the CSC-column-loop restatement of src/stationary_sparse.jl) and the
test matrices of the stationary tests.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "stationary_ref", "stationary_ref.c")

_i64p = C.POINTER(C.c_int64)
_vp = C.c_void_p


def build(outdir):
    """gcc -O2 -ffp-contract=off (Julia never fuses here) -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "stationary_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return Ref(C.CDLL(so))


def _p(a):
    return a.ctypes.data_as(_vp)


class Mat:
    """A SparseMatrixCSC as the restatement reads it: 0-based int64 colptr / rowval, sorted row indices, nzval of dtype."""

    def __init__(self, m, dtype=np.float64):
        m = sp.csc_matrix(m)
        m.sort_indices()
        self.n = m.shape[0]
        self.cp = np.ascontiguousarray(m.indptr, np.int64)
        self.rv = np.ascontiguousarray(m.indices, np.int64)
        self.nz = np.ascontiguousarray(m.data, dtype)
        self.dtype = np.dtype(dtype)
        self.sfx = "f64" if self.dtype == np.float64 else "f32"
        self.diag = np.zeros(self.n, np.int64)

    @classmethod
    def from_csc(cls, n, colptr, rowval, nzval, index_base=1):
        """from SparseMatrixCSC fields (no copy through scipy: the 256^3 Laplacian has 117 M entries)"""
        self = cls.__new__(cls)
        self.n = int(n)
        self.cp = np.ascontiguousarray(np.asarray(colptr, np.int64) - index_base)
        self.rv = np.ascontiguousarray(np.asarray(rowval, np.int64) - index_base)
        self.nz = np.ascontiguousarray(nzval)
        self.dtype = self.nz.dtype
        self.sfx = "f64" if self.dtype == np.float64 else "f32"
        self.diag = np.zeros(self.n, np.int64)
        return self

    def args(self):
        return (C.c_int64(self.n), self.cp.ctypes.data_as(_i64p), self.rv.ctypes.data_as(_i64p), _p(self.nz))


def omega32(omega, dtype):
    """True when the relaxed substitutions of Float32 data run in Float32: a Float32 or an Int omega (Julia's promotion)."""
    return np.dtype(dtype) == np.float32 and (isinstance(omega, (np.float32, int, np.integer)))


class Ref:
    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("st_jacobi", "st_gauss_seidel", "st_sor", "st_ssor", "st_diag"):
                getattr(lib, f"{name}_{sfx}").restype = C.c_int64

    def _fn(self, name, M):
        return getattr(self.L, f"{name}_{M.sfx}")

    def diag(self, M):
        return self._fn("st_diag", M)(*M.args(), M.diag.ctypes.data_as(_i64p))

    # ---- whole methods: (x, returned vector, singular column) ----------------------------------------------------------------
    def jacobi(self, M, b, x, maxiter=10):
        x, w = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        s = self._fn("st_jacobi", M)(*M.args(), _p(np.asarray(b, M.dtype)), _p(x), _p(w), C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    def gauss_seidel(self, M, b, x, maxiter=10):
        x = np.array(x, M.dtype)
        s = self._fn("st_gauss_seidel", M)(*M.args(), _p(np.asarray(b, M.dtype)), _p(x), C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    def sor(self, M, b, x, omega, maxiter=10):
        """(caller's x, iterable.x, which) -- which = 1: iterable.x is the internal buffer (odd maxiter)"""
        x, w = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        b = np.asarray(b, M.dtype)
        which = C.c_int()
        s = self._fn("st_sor", M)(*M.args(), _p(b), _p(x), _p(w), C.c_double(float(omega)), int(omega32(omega, M.dtype)), C.c_int64(maxiter),
                                  M.diag.ctypes.data_as(_i64p), C.byref(which))
        if s:
            return None, None, s
        return x, (w if which.value else x), which.value

    def ssor(self, M, b, x, omega, maxiter=10):
        x, t = np.array(x, M.dtype), np.zeros(M.n, M.dtype)
        s = self._fn("st_ssor", M)(*M.args(), _p(np.asarray(b, M.dtype)), _p(x), _p(t), C.c_double(float(omega)), int(omega32(omega, M.dtype)),
                                   C.c_int64(maxiter), M.diag.ctypes.data_as(_i64p))
        return x, s

    # ---- building blocks (diag() first) ----------------------------------------------------------------------------------------
    def ldiv(self, M, x):
        y = np.zeros(M.n, M.dtype)
        self._fn("st_ldiv", M)(C.c_int64(M.n), _p(M.nz), M.diag.ctypes.data_as(_i64p), _p(y), _p(np.asarray(x, M.dtype)))
        return y

    def _scal(self, M, v):
        return (C.c_double if M.dtype == np.float64 else C.c_float)(v)

    def offdiag_mul(self, M, alpha, x, beta, y):
        y = np.array(y, M.dtype)
        self._fn("st_offdiag_mul", M)(*M.args(), M.diag.ctypes.data_as(_i64p), self._scal(M, alpha), _p(np.asarray(x, M.dtype)), self._scal(M, beta), _p(y))
        return y

    def gs_mul(self, M, upper, alpha, x, beta, y, z=None):
        """z = None: z is x (in place)"""
        x = np.array(x, M.dtype)
        z = x if z is None else np.array(z, M.dtype)
        self._fn("st_gs_mul_upper" if upper else "st_gs_mul_lower", M)(*M.args(), M.diag.ctypes.data_as(_i64p), self._scal(M, alpha), _p(x),
                                                                        self._scal(M, beta), _p(np.asarray(y, M.dtype)), _p(z))
        return z

    def sub(self, M, upper, x, omega=None, y=None):
        """forward_sub! / backward_sub!, plain (omega None) or relaxed with alpha = omega, beta = one(T) - omega"""
        x = np.array(x, M.dtype)
        kind = "st_backward_sub" if upper else "st_forward_sub"
        if omega is None:
            getattr(self.L, f"{kind}_{M.sfx}")(*M.args(), M.diag.ctypes.data_as(_i64p), 0, self._scal(M, 0), _p(x), self._scal(M, 0), None)
            return x
        y = np.asarray(y, M.dtype)
        if M.dtype == np.float64:
            a = np.float64(omega)
            getattr(self.L, f"{kind}_f64")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, C.c_double(a), _p(x), C.c_double(1.0 - a), _p(y))
        elif omega32(omega, M.dtype):
            a = np.float32(omega)
            getattr(self.L, f"{kind}_f32")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, C.c_float(a), _p(x), C.c_float(np.float32(1) - a), _p(y))
        else:
            a = float(omega)
            getattr(self.L, f"{kind}_f32w")(*M.args(), M.diag.ctypes.data_as(_i64p), 1, C.c_double(a), _p(x), C.c_double(1.0 - a), _p(y))
        return x


# ---- test matrices ------------------------------------------------------------------------------------------------------------
def sprand_dominant(n, density, seed, dtype=np.float64):
    """sprand(T, n, n, density) + 2n*I -- test/stationary.jl:23 (a seeded numpy stand-in for Julia's sprand)"""
    rng = np.random.default_rng(seed)
    m = sp.random(n, n, density=density, random_state=rng, format="csc", dtype=np.float64)
    return (m + 2 * n * sp.identity(n, format="csc")).astype(dtype).tocsc()


def arrow(n, long_row, dtype=np.float64, seed=5):
    """diagonally dominant with two dense rows and columns (rows longer than mik_spmv_long_row) plus a tridiagonal band"""
    rng = np.random.default_rng(seed)
    m = sp.lil_matrix((n, n))
    for i in range(n):
        m[i, i] = 4.0 + rng.random()
        if i + 1 < n:
            m[i, i + 1] = -rng.random()
            m[i + 1, i] = -rng.random()
    for hub in (0, n // 2):                 # two long rows / columns: one with an empty strict-lower part, one in the middle
        cols = rng.choice(np.setdiff1d(np.arange(n), [hub]), size=min(n - 1, long_row), replace=False)
        for j in cols:
            m[hub, j] = 0.01 * rng.random()
            m[j, hub] = 0.01 * rng.random()
        m[hub, hub] = 10.0
    return m.tocsc().astype(dtype)


def tridiag(n, dtype=np.float64):
    return sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csc", dtype=dtype)
