"""What tests/test_complex_dense_host.py and tests/test_gpu_complex_dense.py share: the ctypes binding of
tests/complex_ref/complex_dense_ref.c (`DenseRef`), a numpy double of a complex `HipMatrix` used as an operator (`NpDense`), the `ops`
whose `mul_` calls that checker (`DenseHostOps`), and two backends (`DenseHostBackend`, `DenseDeviceBackend`) that take what the scenarios
of tests/complex_host.py pass -- a scipy matrix -- and build the dense form from `m.toarray()`.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import complex_host as ch

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "complex_ref", "complex_dense_ref.c")
_vp = C.c_void_p
_i64 = C.c_int64


def _p(a):
    return a.ctypes.data_as(_vp)


class DenseRef:
    """The C checker.  A: an (m, n) complex array in Fortran order or a flat column-major store with leading dimension `lda` (elements)."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            f = getattr(lib, f"cd_mul_n_{sfx}")
            f.restype, f.argtypes = None, [_i64, _i64, _vp, _i64, _vp, _vp, C.c_int]
            f = getattr(lib, f"cd_mul_t_{sfx}")
            f.restype, f.argtypes = None, [_i64, _i64, _vp, _i64, _vp, _vp, C.c_int, C.c_int]

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.complex128 else 'f32'}")

    @staticmethod
    def _store(A, lda):
        if A.ndim == 2:
            A = np.asfortranarray(A)
            return A, A.shape[0], A.shape[1], (A.shape[0] if lda is None else lda)
        raise ValueError("A: a 2-d array")

    def mul_n(self, A, x, chunk, lda=None):
        A, m, n, lda = self._store(A, lda)
        x = np.ascontiguousarray(x, A.dtype)
        y = np.full(m, np.nan, A.dtype)
        self._fn("cd_mul_n", A.dtype)(m, n, _p(A), max(lda, 1), _p(x), _p(y), int(chunk))
        return y

    def mul_t(self, A, x, shape, lda=None):
        A, m, n, lda = self._store(A, lda)
        x = np.ascontiguousarray(x, A.dtype)
        y = np.full(n, np.nan, A.dtype)
        self._fn("cd_mul_t", A.dtype)(m, n, _p(A), max(lda, 1), _p(x), _p(y), int(shape[0]), int(shape[1]))
        return y


def build(outdir):
    """gcc -std=c99 -O2 -ffp-contract=off -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "complex_dense_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return DenseRef(C.CDLL(so))


@pytest.fixture(scope="session")
def dref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("complex_dense_ref"))


def mul_shape(pkg, dtype):
    """(C, rows per workgroup) of mik_dense_mul_shape_for"""
    c, r = C.c_int(), C.c_int()
    assert pkg.lib().mik_dense_mul_shape_for(pkg._lib.dtype_code(dtype), C.byref(c), C.byref(r)) == 0
    return c.value, r.value


class NpDense:
    """a complex matrix as the operator of the numpy double: what a complex `HipMatrix` is on the device"""

    def __init__(self, A, adjoint_of=None):
        self.A = np.asfortranarray(A)
        self.dtype = self.A.dtype
        self.parent = adjoint_of
        self.n_rows, self.n_cols = self.A.shape if adjoint_of is None else self.A.shape[::-1]

    @property
    def adj(self):
        return self.parent if self.parent is not None else NpDense(self.A, adjoint_of=self)

    def size(self, d=None):
        return (self.n_rows, self.n_cols) if d is None else (self.n_rows, self.n_cols)[d - 1]


class DenseHostOps(ch.HostOps):
    """HostOps whose product of an `NpDense` is the dense checker's"""

    def __init__(self, pkg, ref, dref):
        super().__init__(pkg, ref)
        self.dref = dref

    def mul_(self, y, A, x):
        if not isinstance(A, NpDense):
            return super().mul_(y, A, x)
        if A.parent is not None:
            y.a[:] = self.dref.mul_t(A.A, x.a, self.shape(A.dtype))
        else:
            y.a[:] = self.dref.mul_n(A.A, x.a, mul_shape(self.pkg, A.dtype)[0])
        return y


class DenseHostBackend(ch.HostBackend):
    name = "dense-host"

    def __init__(self, pkg, ref, dref):
        super().__init__(pkg, ref)
        self.ops = DenseHostOps(pkg, ref, dref)

    def operator(self, m):
        return NpDense(np.asarray(m.toarray() if hasattr(m, "toarray") else m))


class DenseDeviceBackend(ch.DeviceBackend):
    name = "dense-device"

    def operator(self, m):
        return self.pkg.HipMatrix.from_numpy(np.asarray(m.toarray() if hasattr(m, "toarray") else m), self.ctx)


def beyond_a_chunk(T, seed, n=197):
    """the system of n = 3 C + 5 unknowns: A = B' B / n + I (Hermitian positive definite, cond about 100), b, reltol = sqrt(eps(real(T)))"""
    rng = np.random.default_rng(seed)
    B = ch.rand_t(rng, T, n, n)
    A = (B.conj().T @ B / n + np.eye(n)).astype(T)
    b = ch.rand_t(rng, T, n)
    return A, b, np.sqrt(np.finfo(ch.real_of(T)).eps)
