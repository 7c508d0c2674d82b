"""Dense operators for the numpy double of lobpcg (tests/lobpcg_double.py): a host matrix whose product is the chunked order of
mik_dense_mul / mik_dense_mm restated in C (tests/dense_ref/dense_mul_ref.c), and stand-ins of the device operator types that need no
device, for the type checks of ``lobpcg.DeviceOps``.  Test infrastructure only."""
import numpy as np

from host_double import FakeCtx


class DenseOperator:
    """A (dense, host) as an operator of ``NumpyOps``: ``mul(y, x)`` is ``Ref.chunked(A, x, C)``"""

    def __init__(self, ref, A, chunk):
        self.ref, self.A, self.chunk = ref, np.asfortranarray(A), int(chunk)
        self.n_rows, self.n_cols = self.A.shape
        self.dtype = self.A.dtype
        self.ctx = FakeCtx()

    def size(self, d=None):
        return (self.n_rows, self.n_cols) if d is None else (self.n_rows, self.n_cols)[d - 1]

    def mul(self, y, x):
        y.a[:] = self.ref.chunked(self.A, x.a, self.chunk)
        return y


def sym(n, dt, seed, shift=20):
    """test/lobpcg.jl:38-39 with numpy's generator: ``A = rand(n, n); A = A' + A + 20I`` (positive definite: see tests/test_lobpcg_host.py; the
    bulk of the spectrum lies within 2 sqrt(n / 6) of the shift, so a size well above 10 needs a larger one to stay so)"""
    R = np.random.default_rng(seed).random((n, n))
    M = R + R.T + shift * np.eye(n)
    assert np.linalg.eigvalsh(M)[0] > 10
    return M.astype(dt)


def separated(n, dt, seed, k=4):
    """a full symmetric matrix Q diag(d) Q' with k well separated eigenvalues at either end of a cluster in [1, 2): a block of k converges to
    them in a few tens of iterations whatever n is"""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    d = np.concatenate([10.0 * np.arange(k, 0, -1), 1 + np.arange(n - 2 * k) / n, -10.0 * np.arange(1, k + 1)])
    M = (Q * d) @ Q.T
    return ((M + M.T) / 2).astype(dt)


def device_type_doubles(pkg):
    """(Dense, CSR): subclasses of ``pkg.HipMatrix`` / ``pkg.HipCSR`` that hold their shape and element type and nothing on a device"""

    class Dense(pkg.HipMatrix):
        def __init__(self, n, cols, dtype):
            self.n, self.cols, self.dtype, self.ctx, self.reserved = int(n), int(cols), np.dtype(dtype), FakeCtx(), 0

        def reserve_block_(self):
            self.reserved += 1
            return self

        def __del__(self):
            pass

    class CSR(pkg.HipCSR):
        def __init__(self, n_rows, n_cols, dtype):
            self.n_rows, self.n_cols, self.dtype, self.ctx = int(n_rows), int(n_cols), np.dtype(dtype), FakeCtx()

        def __del__(self):
            pass

    return Dense, CSR
