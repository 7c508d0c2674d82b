"""ctypes binding of tests/dense_ref/dense_mul_ref.c (the chunked and the serial order of y = A x) and the matrices of the dense operator
tests.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dense_ref", "dense_mul_ref.c")

_vp = C.c_void_p


def build(outdir):
    """gcc -O2 -ffp-contract=off (no product is ever fused into a sum) -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "dense_mul_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return Ref(C.CDLL(so))


def _p(a):
    return a.ctypes.data_as(_vp)


class Ref:
    """`ld` > m embeds A in a taller column-major array whose padding rows are NaN: they must never be read."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("dmr_mul_chunked", "dmr_mul_serial"):
                getattr(lib, f"{name}_{sfx}").restype = None

    @staticmethod
    def _mat(A, ld=None):
        A = np.asarray(A)
        m, n = A.shape
        ld = max(m, 1) if ld is None else int(ld)
        store = np.full((ld, max(n, 1)), np.nan, A.dtype, order="F")
        store[:m, :n] = A
        return m, n, ld, store

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")

    def chunked(self, A, x, chunk, ld=None):
        m, n, ld, store = self._mat(A, ld)
        x = np.ascontiguousarray(x, store.dtype)
        assert x.size == n
        y = np.full(m, np.nan, store.dtype)
        self._fn("dmr_mul_chunked", store.dtype)(C.c_int64(m), C.c_int64(n), _p(store), C.c_int64(ld), _p(x), _p(y), C.c_int64(int(chunk)))
        return y

    def serial(self, A, x, ld=None):
        m, n, ld, store = self._mat(A, ld)
        x = np.ascontiguousarray(x, store.dtype)
        assert x.size == n
        y = np.full(m, np.nan, store.dtype)
        self._fn("dmr_mul_serial", store.dtype)(C.c_int64(m), C.c_int64(n), _p(store), C.c_int64(ld), _p(x), _p(y))
        return y


# ---- test matrices: seeded, no zero entries ---------------------------------------------------------------------------------------
def _nonzero(a):
    a = np.array(a)
    a[a == 0] = 0.5
    return a


def rect(m, n, dtype, seed=0):
    """m x n, mixed signs and magnitudes over several binades, no zero entries"""
    rng = np.random.default_rng(seed + 131 * m + n)
    return np.asfortranarray(_nonzero(rng.standard_normal((m, n)) * np.exp2(rng.integers(-3, 4, (m, n)))).astype(dtype))


def vec(n, dtype, seed=0):
    return _nonzero(np.random.default_rng(seed + 7 * n + 1).standard_normal(n)).astype(dtype)


def spd(n, dtype, seed=0):
    """A = R'R + I"""
    R = np.random.default_rng(seed + n).random((n, n))
    return np.asfortranarray(_nonzero(R.T @ R + np.eye(n)).astype(dtype))


def shifted(n, dtype, seed=0):
    """rand + n I: non-symmetric, well conditioned"""
    R = np.random.default_rng(seed + 3 * n).random((n, n))
    return np.asfortranarray(_nonzero(R + n * np.eye(n)).astype(dtype))


def oracle_spmv(orc, A, x):
    """the oracle's mul!(y, A::SparseMatrixCSC, x) (column scatter) on the m x n matrix A with every entry stored"""
    A = np.asarray(A)
    m, n = A.shape
    suf, ct = ("f64", C.c_double) if A.dtype == np.float64 else ("f32", C.c_float)
    cp = np.arange(0, m * n + 1, m, dtype=np.int64)
    rv = np.tile(np.arange(m, dtype=np.int64), n)
    val = np.ascontiguousarray(A.T).reshape(-1).copy()
    xa, out = np.ascontiguousarray(x, A.dtype), np.empty(m, A.dtype)
    getattr(orc.lib(), f"orc_csc_spmv_{suf}")(m, n, cp.ctypes.data_as(C.POINTER(C.c_int64)), rv.ctypes.data_as(C.POINTER(C.c_int64)),
                                             val.ctypes.data_as(C.POINTER(ct)), 0, xa.ctypes.data_as(C.POINTER(ct)), out.ctypes.data_as(C.POINTER(ct)))
    return out
