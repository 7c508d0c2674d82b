"""ctypes binding of tests/stationary_ref/stationary_dense_ref.c (the column-loop restatement of src/stationary.jl), the per-row forms of
the same methods as explicit numpy chains, and the test matrices of the dense stationary tests.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "stationary_ref", "stationary_dense_ref.c")

_vp = C.c_void_p


def build(outdir):
    """gcc -O2 -ffp-contract=off (Julia never fuses here) -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "stationary_dense_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return Ref(C.CDLL(so))


def _p(a):
    return a.ctypes.data_as(_vp)


def wide(omega, dtype):
    """True when Float32 data meets a Float64 omega (a Python float or an np.float64): Julia's promotion widens the update."""
    return np.dtype(dtype) == np.float32 and not isinstance(omega, (np.float32, int, np.integer))


class Ref:
    """Every method copies its vectors, runs `maxiter` iterations of the reference's loops and returns the vectors and check_diag's
    1-based index (0: none).  `ld` > n embeds A in a taller column-major array, as a HipMatrix stores it."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("dst_check_diag", "dst_jacobi", "dst_gauss_seidel", "dst_sor"):
                getattr(lib, f"{name}_{sfx}").restype = C.c_int64

    @staticmethod
    def _mat(A, dtype, ld=None):
        A = np.asarray(A)
        n = A.shape[0]
        assert A.shape == (n, n)
        ld = n if ld is None else int(ld)
        store = np.full((ld, n), np.nan, dtype, order="F")        # the padding rows must never be read
        store[:n, :] = A
        return n, ld, store

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")

    def check_diag(self, A, dtype=None, ld=None):
        dtype = np.dtype(dtype or np.asarray(A).dtype)
        n, ld, store = self._mat(A, dtype, ld)
        return self._fn("dst_check_diag", dtype)(C.c_int64(n), _p(store), C.c_int64(ld))

    def jacobi(self, A, b, x, maxiter=10, ld=None):
        dtype = np.asarray(A).dtype
        n, ld, store = self._mat(A, dtype, ld)
        x, nxt = np.array(x, dtype), np.zeros(n, dtype)
        s = self._fn("dst_jacobi", dtype)(C.c_int64(n), _p(store), C.c_int64(ld), _p(np.ascontiguousarray(b, dtype)), _p(x), _p(nxt), C.c_int64(maxiter))
        return x, nxt, s

    def gauss_seidel(self, A, b, x, maxiter=10, ld=None):
        dtype = np.asarray(A).dtype
        n, ld, store = self._mat(A, dtype, ld)
        x = np.array(x, dtype)
        s = self._fn("dst_gauss_seidel", dtype)(C.c_int64(n), _p(store), C.c_int64(ld), _p(np.ascontiguousarray(b, dtype)), _p(x), C.c_int64(maxiter))
        return x, s

    def _sor(self, A, b, x, omega, maxiter, symmetric, ld, is_wide=None):
        dtype = np.asarray(A).dtype
        n, ld, store = self._mat(A, dtype, ld)
        x, tmp = np.array(x, dtype), np.zeros(n, dtype)
        is_wide = wide(omega, dtype) if is_wide is None else is_wide
        s = self._fn("dst_sor", dtype)(C.c_int64(n), _p(store), C.c_int64(ld), _p(np.ascontiguousarray(b, dtype)), _p(x), _p(tmp),
                                       C.c_double(float(omega)), int(is_wide), int(symmetric), C.c_int64(maxiter))
        return x, tmp, s

    def sor(self, A, b, x, omega, maxiter=10, ld=None, is_wide=None):
        return self._sor(A, b, x, omega, maxiter, False, ld, is_wide)

    def ssor(self, A, b, x, omega, maxiter=10, ld=None, is_wide=None):
        return self._sor(A, b, x, omega, maxiter, True, ld, is_wide)


# ---- the per-row forms, as explicit chains of numpy scalars (one rounded product, one rounded difference per term) -----------------
def _chain(acc, A, r, cols, x):
    for c in cols:
        p = A[r, c] * x[c]
        acc = acc - p
    return acc


def _relax(T, xo, q, omega):
    """x + omega * (q - x) with Julia's types"""
    dq = q - xo
    if wide(omega, T):
        return T(np.float64(xo) + np.float64(omega) * np.float64(dq))
    w = T(omega)
    return xo + w * dq


def rows_jacobi(A, b, x):
    """(x, next) after one iteration: next[r] = b[r] - sum over c != r ascending (old x); x[r] = next[r] / d"""
    n = len(b)
    nxt = np.array([_chain(b[r], A, r, [c for c in range(n) if c != r], x) for r in range(n)], A.dtype)
    return np.array([nxt[r] / A[r, r] for r in range(n)], A.dtype), nxt


def rows_forward(A, b, x, omega=None):
    """(x, t) after one Gauss-Seidel (omega None) or SOR sweep: t = b[r] - upper part (old x, ascending) - lower part (new x, ascending)"""
    n = len(b)
    T = A.dtype.type
    new, t = x.copy(), np.zeros(n, A.dtype)
    for r in range(n):
        acc = _chain(b[r], A, r, range(r + 1, n), x)
        acc = _chain(acc, A, r, range(r), new)
        t[r] = acc
        q = acc / A[r, r]
        new[r] = q if omega is None else _relax(T, x[r], q, omega)
    return new, t


def rows_backward(A, b, x, omega):
    """(x, tmp) after the backward half of SSOR: both parts DESCENDING, every product with the x the half started from; row-parallel"""
    n = len(b)
    T = A.dtype.type
    new, t = x.copy(), np.zeros(n, A.dtype)
    for r in range(n):
        acc = _chain(b[r], A, r, range(r - 1, -1, -1), x)
        acc = _chain(acc, A, r, range(n - 1, r, -1), x)
        t[r] = acc
        new[r] = _relax(T, x[r], acc / A[r, r], omega)
    return new, t


# ---- test matrices ----------------------------------------------------------------------------------------------------------------
def dominant(n, dtype, seed=0):
    """strictly diagonally dominant, non-symmetric, mixed signs (diagonal included)"""
    rng = np.random.default_rng(seed + 1000 * n)
    A = rng.uniform(-1.0, 1.0, (n, n))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, sign * (np.abs(A).sum(axis=1) + 1.0 + rng.random(n)))
    return np.asfortranarray(A.astype(dtype))


def non_dominant(n, dtype, seed=0):
    """a diagonal of 0.4 times its off-diagonal row sum, mixed signs: not diagonally dominant, yet a few iterations of every method stay finite"""
    rng = np.random.default_rng(seed + 77 * n)
    A = rng.uniform(-1.0, 1.0, (n, n))
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, np.where(rng.random(n) < 0.5, -1.0, 1.0) * 0.4 * np.abs(A).sum(axis=1))
    return np.asfortranarray(A.astype(dtype))
