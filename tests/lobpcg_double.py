"""A numpy double of the device side of lobpcg.py (test infrastructure): the methods of ``lobpcg.DeviceOps`` evaluated on the host, the four
block entries of include/mik.h (``mik_spmm``, ``mik_block_gram``, ``mik_block_rdiv``, ``mik_block_update``) implemented literally from their
definitions there.  Dots and norms go through the CPU oracle with the device's reduction tree (``mode="tree"``, the shape of
``mik_reduce_shape``) or as sequential sums (``mode="seq"``); sparse products are the oracle's column scatter (``host_double.FakeOperator``).
The driver of lobpcg.py runs on it unchanged (``ops=``); operators are ``FakeOperator``s, a Jacobi preconditioner is ``HostJacobi``."""
import numpy as np

from host_double import FakeMatrix, FakeOperator
from svdl_double import TREE_SHAPE, basis_rotate


class Matrix(FakeMatrix):
    def to_numpy(self):
        return self.m.T.copy()


class HostJacobi:
    """``JacobiPrec`` on the host: ``x ./ diagonal``."""

    def __init__(self, diagonal):
        self.diagonal = np.asarray(diagonal)


def block_rdiv(X, R):
    """the loop of rdiv! (src/lobpcg.jl:345-355), literally; X is n x s, updated in place"""
    s = R.shape[0]
    for i in range(s):
        for j in range(i):
            X[:, i] = X[:, i] - X[:, j] * R[j, i]
        X[:, i] = X[:, i] / R[i, i]
    return X


def block_update(sx, b1, b2, X, R, P, V):
    """(Xout, Pout) of mik_block_update from its definition, with rot = svdl_double.basis_rotate; Pout is None when b1 == 0"""
    Vx, Vr, Vp = V[:sx], V[sx:sx + b1], V[sx + b1:sx + b1 + b2]
    Pout = None
    if b1 > 0:
        Pout = basis_rotate(R[:, :b1], Vr)
        if b2 > 0:
            Pout = Pout + basis_rotate(P[:, :b2], Vp)
    Xout = basis_rotate(X[:, :sx], Vx)
    if b1 > 0:
        Xout = Xout + Pout
    return Xout, Pout


def operator(orc, S):
    return FakeOperator(orc, S)


class NumpyOps:
    def __init__(self, orc, n, dtype, mode="tree"):
        self.orc, self.mode = orc, mode
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.W, self.L = TREE_SHAPE[self.dtype] if mode == "tree" else (1, 1)

    # -- storage ----------------------------------------------------------------------------------
    def matrix(self, rows, cols):
        return Matrix(rows, max(int(cols), 1), self.dtype)

    def upload(self, M, host, c0=0):
        host = np.asarray(host, self.dtype)
        M.m[c0:c0 + host.shape[1], :] = host.T

    def download(self, M, cols):
        return M.m[:cols].T.copy()

    def copy_cols(self, dst, d0, src, s0, count):
        for j in range(count):
            dst.m[d0 + j, :] = src.m[s0 + j]

    def _dot(self, x, y):
        return self.dtype.type(self.orc.dot(np.ascontiguousarray(x), np.ascontiguousarray(y), self.mode, self.W, self.L))

    def _nrm(self, x):
        return self.dtype.type(self.orc.nrm2(np.ascontiguousarray(x), self.mode, self.W, self.L))

    # -- the four block entries -------------------------------------------------------------------
    def spmm(self, A, X, b, Y):
        for j in range(b):
            A.mul(Y.col(j), X.col(j))

    def gram(self, X, p, Y, q, x0=0, y0=0):
        G = np.zeros((p, q), self.dtype)
        for i in range(p):
            for j in range(q):
                G[i, j] = self._dot(X.m[x0 + i], Y.m[y0 + j])
        return G

    def rdiv(self, X, s, R):
        Xh = X.m[:s].T.copy()
        X.m[:s] = block_rdiv(Xh, np.asarray(R, self.dtype)).T

    def update(self, sx, b1, b2, X, R, P, V, Xout, Pout):
        V = np.asarray(V, self.dtype)
        xo, po = block_update(sx, b1, b2, X.m.T, R.m.T if R is not None else None, P.m.T if P is not None else None, V)
        Xout.m[:sx] = xo.T
        if po is not None:
            Pout.m[:sx] = po.T

    # -- composed from the vector entries ---------------------------------------------------------
    def residuals(self, AX, BX, lam, R, sx):
        T = self.dtype.type
        out = np.zeros(sx, self.dtype)
        for j in range(sx):
            t = T(-lam[j]) * BX.m[j]
            R.m[j, :] = AX.m[j] + t
            out[j] = self._nrm(R.m[j])
        return out

    def gather_cols(self, dst, src, mask):
        k = 0
        for j in np.flatnonzero(mask):
            dst.m[k, :] = src.m[j]
            k += 1

    def constrain(self, X, sx, Y, sy, tmp):
        T = self.dtype.type
        for j in range(sx):
            for i in range(sy):
                temp = T(-1) * T(tmp[i, j])
                X.m[j, :] = X.m[j] + temp * Y.m[i]

    def precond(self, P, X, bs, temp):
        if P is None:
            return
        for j in range(bs):
            X.m[j, :] = X.m[j] / P.diagonal.astype(self.dtype)
