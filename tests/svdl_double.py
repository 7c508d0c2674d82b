"""A numpy double of the device side of svdl.py (test infrastructure): the methods of ``svdl.DeviceOps`` evaluated on the host, the two new
entries of include/mik.h (``mik_basis_rotate``, ``mik_svdl_reorth``) implemented literally from their definitions there.  Dots and norms go
through the CPU oracle, either with the device's reduction tree (``mode="tree"``, the shape of ``mik_reduce_shape``) or as plain sequential
sums (``mode="seq"``); the sparse products are the oracle's column scatter.  The driver of svdl.py runs on it unchanged (``ops=``)."""
import numpy as np

from host_double import FakeMatrix, FakeOperator

TREE_SHAPE = {np.dtype(np.float64): (2, 2), np.dtype(np.float32): (4, 2)}      # (W, L) of mik_reduce_shape


def basis_rotate(V, F):
    """``Y[:, j] = (...(V[:, 0]*F[0, j] + V[:, 1]*F[1, j]) + ...) + V[:, k-1]*F[k-1, j]``: the definition of mik_basis_rotate, literally."""
    k, l = F.shape
    Y = np.empty((V.shape[0], l), V.dtype)
    for j in range(l):
        acc = V[:, 0] * F[0, j]
        for c in range(1, k):
            acc = acc + V[:, c] * F[c, j]
        Y[:, j] = acc
    return Y


class Matrix(FakeMatrix):
    def to_numpy(self):
        return self.m.T.copy()


class NumpyOps:
    def __init__(self, orc, S, mode="tree"):
        S = S.tocsc()
        S.sort_indices()
        self.orc, self.S, self.mode = orc, S, mode
        self.dtype = np.dtype(S.dtype)
        self.m, self.n = S.shape
        self.A = FakeOperator(orc, S)          # .adj: the transposed matrix, products by the oracle's column scatter
        self.W, self.L = TREE_SHAPE[self.dtype] if mode == "tree" else (1, 1)
        self.passes = []                     # Gram-Schmidt passes of every reorth call

    # -- storage ----------------------------------------------------------------------------------
    def matrix(self, rows, cols):
        return Matrix(rows, cols, self.dtype)

    def set_col(self, M, j, host):
        M.m[j, :] = np.asarray(host, self.dtype)

    # -- L1 ---------------------------------------------------------------------------------------
    def mul(self, y, x):
        return self.A.mul(y, x)

    def mul_adj(self, y, x):
        return self.A.adj.mul(y, x)

    def _dot(self, x, y):
        return self.dtype.type(self.orc.dot(np.ascontiguousarray(x), np.ascontiguousarray(y), self.mode, self.W, self.L))

    def _nrm(self, x):
        return self.dtype.type(self.orc.nrm2(np.ascontiguousarray(x), self.mode, self.W, self.L))

    def norm(self, x):
        return self._nrm(x.a)

    def dot(self, x, y):
        return self._dot(x.a, y.a)

    def scal(self, x, a):
        x.a[:] = x.a * self.dtype.type(a)
        return x

    def copy(self, dst, src):
        dst.a[:] = src.a
        return dst

    def axpy_nrm2(self, alpha, x, y):
        t = self.dtype.type(alpha) * x.a
        y.a[:] = y.a + t
        return self._nrm(y.a)

    # -- L2 ---------------------------------------------------------------------------------------
    def gemv_t(self, V, k, w):
        return np.array([self._dot(V.m[j], w.a) for j in range(k)], self.dtype)

    def gemv_n(self, y, V, k, c, alpha):
        T = self.dtype.type
        for j in range(k):
            temp = T(alpha) * T(c[j])
            y.a[:] = y.a + temp * V.m[j]
        return y

    def reorth(self, Q, k, q, alpha):
        """old = norm(q); q -= Q*(Q'q); if norm(q) <= alpha*old: q -= Q*(Q'q); beta = norm(q); q .*= inv(beta) -- as the chain of
        mik_nrm2 / mik_gemv_t / mik_gemv_n / mik_scal that defines mik_svdl_reorth."""
        T = self.dtype.type
        old = self._nrm(q.a)
        self.gemv_n(q, Q, k, self.gemv_t(Q, k, q), -1)
        nw = self._nrm(q.a)
        passes = 1
        if nw <= T(alpha) * old:
            self.gemv_n(q, Q, k, self.gemv_t(Q, k, q), -1)
            nw = self._nrm(q.a)
            passes = 2
        self.passes.append(passes)
        if nw != 0:
            q.a[:] = q.a * (T(1) / nw)
        return nw, passes

    def rotate(self, V, k, F, Y):
        F = np.asarray(F, self.dtype)
        Y.m[:F.shape[1], :] = basis_rotate(V.m[:k].T, F).T
        return Y
