"""A numpy double of the dense-operator entries of libmik.so (test infrastructure): ``api.lib`` is replaced by a ``DoubleLib`` whose
``mik_dense_create`` / ``mik_dense_mul`` work on numpy arrays registered under fake device pointers, the N form through
tests/dense_ref/dense_mul_ref.c with the library's chunk and the T form as one serial dot per column.  The Python layer -- ``HipMatrix`` as an
operator, its adjoint view, ``mul_``, ``_Bound.operator`` and the constructors of the fused iterables -- runs on it unchanged; the
``mik_cg_create_op`` / ``mik_gmres_create_op`` calls are recorded instead of carried out."""
import ctypes as C
import itertools

import numpy as np

from host_double import FakeCtx, FakeVector

_ptrs = itertools.count(0x1000, 0x1000)
REG = {}


class DoubleVector(FakeVector):
    """a FakeVector with a fake device pointer the DoubleLib can resolve"""

    def __init__(self, a):
        super().__init__(a)
        self._ptr = next(_ptrs)
        REG[self._ptr] = self.a

    @property
    def ptr(self):
        return self._ptr

    def similar(self):
        return DoubleVector(np.empty_like(self.a))

    def zero(self):
        return DoubleVector(np.zeros_like(self.a))


def matrix(pkg, A):
    """a ``pkg.HipMatrix`` (the real class: its operator methods are what is tested) over numpy storage, ld = m"""
    A = np.asfortranarray(A)
    M = pkg.HipMatrix.__new__(pkg.HipMatrix)
    M.ctx, M.n, M.cols, M.dtype, M.ld = FakeCtx(), A.shape[0], A.shape[1], A.dtype, max(A.shape[0], 1)
    M.buf = DoubleVector(A.reshape(-1, order="F"))
    M.host = A
    return M


def _val(p):
    return p.value if isinstance(p, C.c_void_p) else p


class DoubleLib:
    def __init__(self, real, ref, chunk):
        self.real, self.ref, self.chunk = real, ref, int(chunk)
        self.handles, self.calls, self.created, self.destroyed = {}, [], [], []
        self.mik_dense_mul_fn, self.mik_dense_mul_adj_fn = real.mik_dense_mul_fn, real.mik_dense_mul_adj_fn    # the native callbacks

    def mik_last_error(self, _ctx):
        return b""

    def mik_dense_create(self, _ctx, code, m, n, A, lda, out):
        h = next(_ptrs)
        dtype = np.float64 if code == 0 else np.float32
        self.handles[h] = np.asarray(REG[_val(A)], dtype).reshape((lda, n), order="F")[:m, :]
        out._obj.value = h
        self.created.append(h)
        return 0

    def mik_dense_destroy(self, h):
        self.destroyed.append(_val(h))
        return 0

    def mik_dense_mul(self, h, adjoint, x, y):
        A, xa, ya = self.handles[_val(h)], REG[_val(x)], REG[_val(y)]
        self.calls.append(("mul", _val(h), int(adjoint)))
        if adjoint:
            ya[:] = self.ref.chunked(np.ascontiguousarray(A.T), xa, max(A.shape[0], 1))       # one serial dot per column
        else:
            ya[:] = self.ref.chunked(A, xa, self.chunk)
        return 0

    def _record(self, name, op):
        op = op._obj
        self.calls.append((name, op.dtype, op.n, op.csr, C.cast(op.mul, C.c_void_p).value, op.user))
        return 0

    def mik_cg_create_op(self, _ctx, op, *rest):
        return self._record("mik_cg_create_op", op)

    def mik_gmres_create_op(self, _ctx, op, *rest):
        return self._record("mik_gmres_create_op", op)

    def mik_cg_state(self, *a):
        return 0

    def mik_gmres_state(self, *a):
        return 0

    def mik_cg_destroy(self, *a):
        return 0

    def mik_gmres_destroy(self, *a):
        return 0
