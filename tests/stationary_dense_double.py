"""A numpy double of ``stationary_dense.DenseStationaryOperator`` (test infrastructure): the four step methods evaluated on the host by one
iteration of tests/stationary_ref/stationary_dense_ref.c on ``host_double.FakeVector``s.  The iterables, builders and public names of
stationary_dense.py run on it unchanged.  Like the real operator it runs check_diag at construction, types omega through
``stationary._relax_scalars`` and counts its calls."""
import numpy as np

from host_double import FakeCtx


class DoubleOperator:
    def __init__(self, pkg, ref, A):
        A = np.asarray(A)
        if A.shape[0] != A.shape[1]:
            raise ValueError(f"DimensionMismatch: the matrix is {A.shape[0]} x {A.shape[1]}, not square")
        self.pkg, self.ref, self.M = pkg, ref, np.asfortranarray(A)
        self.dtype, self.n, self.ctx = self.M.dtype, A.shape[0], FakeCtx()
        self.calls = []
        s = ref.check_diag(self.M)
        if s:
            raise pkg.SingularException(s)

    def _vec(self, v, name):
        if v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {v.n}/{v.dtype}, the operator {self.n}/{self.dtype}")
        return v.a

    def jacobi_step_(self, x, next, b):
        self.calls.append("jacobi")
        xa, na, ba = self._vec(x, "x"), self._vec(next, "next"), self._vec(b, "b")
        xa[:], na[:], _ = self.ref.jacobi(self.M, ba, xa, 1)

    def gs_step_(self, x, b):
        self.calls.append("gs")
        xa, ba = self._vec(x, "x"), self._vec(b, "b")
        xa[:], _ = self.ref.gauss_seidel(self.M, ba, xa, 1)

    def _relaxed(self, fn, x, tmp, b, omega):
        w, _, S = self.pkg.stationary._relax_scalars(self.dtype, omega)      # what DenseStationaryOperator._relaxed hands to the C entry
        self.scalar = (w, np.dtype(S))
        xa, ta, ba = self._vec(x, "x"), self._vec(tmp, "tmp"), self._vec(b, "b")
        xa[:], ta[:], _ = fn(self.M, ba, xa, float(w), 1, is_wide=(self.dtype == np.float32 and np.dtype(S) == np.float64))

    def sor_step_(self, x, tmp, b, omega):
        self.calls.append("sor")
        self._relaxed(self.ref.sor, x, tmp, b, omega)

    def ssor_step_(self, x, tmp, b, omega):
        self.calls.append("ssor")
        self._relaxed(self.ref.ssor, x, tmp, b, omega)
