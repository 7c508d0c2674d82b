"""``svdl`` -- Golub-Kahan-Lanczos bidiagonalisation with thick restart for a device CSR operator (src/svdl.jl, v0.9.4), restated
statement by statement; Julia's ``f!`` is spelled ``f_``.  Citations are file:line in the reference checkout.

What runs where
  device   everything of length m or n: ``A*q`` / ``A'p`` (``mik_spmv`` on the operator and on the adjoint uploaded next to it),
           ``p .-= beta*P[:, j]`` with its norm in one sweep (``mik_axpy_dot``), ``f -= L.P*rho`` (``mik_gemv_n``), ``P'f`` (``mik_gemv_t``), the
           double classical Gram-Schmidt of extend! with its norm test and the normalisation (``mik_svdl_reorth``), every basis rotation
           of the restarts and the singular vectors (``mik_basis_rotate``);
  host     in numpy, in the element type: ``svd(L.B)``, the full SVD and the QR of harmonicrestart!, ``ldiv!`` / ``pinv``, isconverged.
``L.P`` (m x k) and ``L.Q`` (n x (k+1)) are allocated once at full width together with ONE spare pair that is the target of a rotation
and is then swapped in; the reference's ``[L.Q q]`` concatenations are a column counter.  Nothing is allocated on the device inside the
restart loop.

Differences from the reference, all deliberate:
  * the operator is a ``HipCSR`` uploaded with its adjoint (``extras.with_adjoint`` / ``with_adjoint_from_scipy``) or a ``HipMatrix`` (its ``.adj`` is a view), rectangular allowed;
    ``LinearOperator`` callbacks are not supported;
  * the default ``v0`` is a random unit vector from numpy's generator, not from Julia's stream; a caller's ``v0`` is copied (build scales
    ``q`` in place, :357: that happens on the copy the factorisation owns);
  * ``beta == 0`` in extend! (an exactly invariant subspace): the reference divides by zero and fills the basis with Inf / NaN; here a
    ``MikError`` that is also a ``ZeroDivisionError`` is raised;
  * with ``vecs`` the singular vectors stay on the device: ``F.U`` is a ``HipMatrix`` (m x nsv), ``F.V`` a ``HipMatrix`` (n x nsv);
    ``F.Vt`` materialises the nsv x n host array the reference returns;
  * the singular vectors are formed with the SVD of the final ``L.B`` instead of the one taken before the last restart (:230-237, see
    svdl_method_): the reference's product is only right once B has stopped changing;
  * extend! re-uses the name of its keyword ``alpha = 1/sqrt(2)`` for ``norm(p)`` (:596), so from the second Lanczos vector of a call on the
    second-pass test of :571 compares with the last ``norm(p)``: restated as written.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import api
from ._lib import MikError, check, dtype_code, lib, real_dtype_code
from .api import ConvergenceHistory, HipCSR, HipMatrix, HipVector
from .extras import with_adjoint, with_adjoint_from_scipy       # noqa: F401  (how an operator gets its adjoint)

_vp = C.c_void_p


class ArgumentError(ValueError):
    """Julia's ``ArgumentError``."""


class BoundsError(IndexError):
    """Julia's ``BoundsError``."""


class SvdlBreakdown(MikError, ZeroDivisionError):
    """``beta == 0`` in extend!: the Krylov space is exactly invariant (the reference divides by zero, src/svdl.jl:577)."""


# ==============================================================================================
# BrokenArrowBidiagonal, PartialFactorization  -- src/svdl.jl:19-81
# ==============================================================================================
class BrokenArrowBidiagonal:
    """``BrokenArrowBidiagonal{T}`` (:19-23): diagonal ``dv``, the arrow column ``av`` (column ``len(av) + 1``) and the superdiagonal ``ev``
    behind it.  Indices are 1-based like the reference's; an empty ``av`` is the ``Bidiagonal(dv, ev, :U)`` of build (:361)."""

    def __init__(self, dv, av, ev):
        self.dv, self.av, self.ev = list(dv), list(av), list(ev)

    def size(self, n=None):                                              # :25-33
        if n is None:
            return (len(self.dv), len(self.dv))
        if n == 1 or n == 2:
            return len(self.dv)
        raise ArgumentError(f"invalid dimension {n}")

    def __getitem__(self, ij):                                           # :35-51
        i, j = ij
        n = self.size(1)
        k = len(self.av)
        if not (1 <= i <= n and 1 <= j <= n):
            raise BoundsError()
        if i == j:
            return self.dv[i - 1]
        if i <= k and j == k + 1:
            return self.av[i - 1]
        if i > k and j == i + 1:
            return self.ev[i - k - 1]
        return type(self.dv[0])(0)

    def Matrix(self, dtype=None):                                        # :53-67
        n = self.size(1)
        k = len(self.av)
        M = np.zeros((n, n), dtype if dtype is not None else np.asarray(self.dv).dtype)
        for i in range(n):
            M[i, i] = self.dv[i]
        for i in range(k):
            M[i, k] = self.av[i]
        for i in range(k, n - 1):
            M[i, i + 1] = self.ev[i - k]
        return M

    def svd(self):                                                       # :69
        return SVD(*np.linalg.svd(self.Matrix()))

    def copy(self):
        return BrokenArrowBidiagonal(self.dv, self.av, self.ev)


class SVD:
    """``LinearAlgebra.SVD``: ``U``, ``S``, ``Vt`` and ``V = Vt'``.  For the k x k problems of a restart the factors are host arrays; in the
    result of ``svdl(..., vecs=...)`` ``U`` / ``V`` are device matrices (m x nsv / n x nsv) and ``Vt`` materialises the nsv x n host array."""

    def __init__(self, U, S, Vt=None, V=None):
        self.U, self.S = U, S
        self._Vt, self._V = Vt, V

    @property
    def V(self):
        return self._V if self._V is not None else self._Vt.T

    @property
    def Vt(self):
        if self._Vt is not None:
            return self._Vt
        return self._V.to_numpy().T if hasattr(self._V, "to_numpy") else np.asarray(self._V).T


class PartialFactorization:
    """``A ~ P * [B 0; 0 beta] * Q`` (:76-81).  ``P`` / ``Q`` are full-width device blocks of which the first ``np_`` / ``nq`` columns are the
    reference's ``L.P`` / ``L.Q``; ``Pt`` / ``Qt`` the spare pair the rotations write to."""

    def __init__(self, P, Q, B, beta, np_=0, nq=0, Pt=None, Qt=None):
        self.P, self.Q, self.B, self.beta = P, Q, B, beta
        self.np_, self.nq, self.Pt, self.Qt = np_, nq, Pt, Qt

    def P_host(self):
        return self.P.to_numpy()[:, :self.np_]

    def Q_host(self):
        return self.Q.to_numpy()[:, :self.nq]


def _Bsize(B):
    return B.size(1) if isinstance(B, BrokenArrowBidiagonal) else B.shape[0]


def _Bsvd(B):
    return B.svd() if isinstance(B, BrokenArrowBidiagonal) else SVD(*np.linalg.svd(B))


# ==============================================================================================
# the device side
# ==============================================================================================
class DeviceOps:
    """Every statement of length m or n, on the device.  (tests/svdl_double.py implements the same methods in numpy.)"""

    def __init__(self, A):
        if not isinstance(A, (HipCSR, HipMatrix)):
            raise TypeError("svdl needs a HipCSR or a HipMatrix operator (LinearOperator callbacks are not supported)")
        if getattr(A, "adj", None) is None:
            raise MikError(5, "svdl", "this operator was uploaded without its adjoint: create it with extras.with_adjoint(...) / "
                                      "with_adjoint_from_scipy(m)")
        self.A, self.ctx, self.dtype = A, A.ctx, np.dtype(A.dtype)
        self.code = real_dtype_code(self.dtype, "svdl")
        self.m, self.n = A.n_rows, A.n_cols

    def matrix(self, rows, cols):
        return HipMatrix(rows, cols, self.dtype, self.ctx)

    def set_col(self, M, j, host):
        M.col(j).copy_from_host(np.ascontiguousarray(host, self.dtype))

    def mul(self, y, x):                                                 # mul!(y, A, x)
        return api.mul_(y, self.A, x)

    def mul_adj(self, y, x):                                             # mul!(y, adjoint(A), x)
        return api.mul_(y, self.A.adj, x)

    def norm(self, x):
        return api.norm(x)

    def dot(self, x, y):
        return api.dot(x, y)

    def scal(self, x, a):
        return x.scal_(a)

    def copy(self, dst, src):
        return dst.copyto_(src)

    def axpy_nrm2(self, alpha, x, y):                                    # y .+= alpha .* x; norm(y), one sweep
        return api.axpy_dot_(alpha, x, y, None)

    def gemv_t(self, V, k, w):
        return api.gemv_t_(V, k, w)

    def gemv_n(self, y, V, k, c, alpha):
        return api.gemv_n_(y, V, k, np.asarray(c, self.dtype), alpha)

    def reorth(self, Q, k, q, alpha):                                    # src/svdl.jl:567-577 -> (beta, passes)
        a = np.asarray([alpha], self.dtype)
        beta = np.zeros(1, self.dtype)
        passes = C.c_int(0)
        check(lib().mik_svdl_reorth(self.ctx.handle, self.code, Q.n, int(k), _vp(Q.buf.ptr), Q.ld, _vp(q.ptr), a.ctypes.data_as(_vp),
                                    beta.ctypes.data_as(_vp), C.byref(passes)), "mik_svdl_reorth", self.ctx.handle)
        return beta[0], passes.value

    def rotate(self, V, k, F, Y):                                        # Y[:, :l] = V[:, :k] * F (k x l, host)
        F = np.asfortranarray(F, self.dtype)
        check(lib().mik_basis_rotate(self.ctx.handle, self.code, V.n, int(k), int(F.shape[1]), _vp(V.buf.ptr), V.ld, F.ctypes.data_as(_vp),
                                     max(int(F.shape[0]), 1), _vp(Y.buf.ptr), Y.ld), "mik_basis_rotate", self.ctx.handle)
        return Y


def _ops_for(A, ops):
    return ops if ops is not None else DeviceOps(A)


# ==============================================================================================
# API  -- src/svdl.jl:157-171
# ==============================================================================================
class _Log:
    """The keys svdl reserves in its ConvergenceHistory (:161-167) hold one entry per restart: lists while running, arrays (``:Bs``: a list)
    after shrink!; ``partial`` keeps the last entry only."""
    KEYS = ("conv", "ritz", "resnorm", "Bs", "betas")

    @staticmethod
    def reserve(history):
        if not history.partial:
            for key in _Log.KEYS:
                history.data[key] = []

    @staticmethod
    def push(history, key, val):
        if history.partial:
            history.data[key] = val
        else:
            history.data[key].append(val)

    @staticmethod
    def shrink(history):
        if not history.partial:
            for key in ("conv", "ritz", "resnorm", "betas"):
                if isinstance(history.data.get(key), list):
                    history.data[key] = np.asarray(history.data[key])


def svdl(A, *, nsv: int = 6, k: int = None, tol=None, maxiter: int = None, method: str = "ritz", log: bool = False, ops=None, **kwargs):
    """``svdl(A; nsv, v0, k, j, maxiter, tol, reltol, verbose, method, vecs, dolock, log)`` -> ``(X, L)`` or ``(X, L, history)`` (:157-171).
    ``X``: the ``nsv`` largest singular values, or an ``SVD`` with the vectors asked for by ``vecs`` ("none", "left", "right", "both").
    ``method``: "ritz" or "harmonic".  History keys: "conv", "ritz", "resnorm", "Bs", "betas" (and "tol")."""
    ops = _ops_for(A, ops)
    if k is None:
        k = 2 * nsv
    if tol is None:
        tol = math.sqrt(np.finfo(ops.dtype).eps)
    if maxiter is None:
        maxiter = min(ops.m, ops.n)
    history = ConvergenceHistory(partial=not log)                        # :161
    history["tol"] = tol
    _Log.reserve(history)                                                # :163-167
    X, L = svdl_method_(history, A, nsv, k=k, tol=tol, maxiter=maxiter, method=method, ops=ops, **kwargs)
    return (X, L, history) if log else (X, L)


# ==============================================================================================
# method  -- src/svdl.jl:177-247
# ==============================================================================================
def svdl_method_(log, A, l: int = None, *, k: int = None, j: int = None, v0=None, maxiter: int = None, tol=None, reltol=None,
                 verbose: bool = False, method: str = "ritz", vecs: str = "none", dolock: bool = False, ops=None):
    ops = _ops_for(A, ops)
    T = ops.dtype.type
    if l is None:
        l = min(6, ops.m)
    k = 2 * l if k is None else k
    j = l if j is None else j
    maxiter = min(ops.m, ops.n) if maxiter is None else maxiter
    tol = math.sqrt(np.finfo(ops.dtype).eps) if tol is None else tol
    reltol = math.sqrt(np.finfo(ops.dtype).eps) if reltol is None else reltol
    if v0 is None:                                                       # :178 (numpy's generator, not Julia's stream)
        v0 = np.random.default_rng().standard_normal(ops.n).astype(ops.dtype)
        v0 = v0 * T(1 / np.linalg.norm(v0))
    v0 = np.array(v0, dtype=ops.dtype, copy=True)
    if v0.shape != (ops.n,):
        raise ValueError(f"DimensionMismatch: v0 has length {v0.size}, the operator {ops.n} columns")
    method = str(method).lstrip(":")
    vecs = str(vecs).lstrip(":")

    T0 = time.perf_counter()
    if not k > 1:                                                        # :183
        raise AssertionError("k > 1")
    if k + 1 > 64:
        raise MikError(5, "svdl", f"k = {k}: the basis rotation handles up to 63 Lanczos vectors")
    L = build(log, A, v0, k, ops=ops)                                    # :184

    F = None
    for it in range(1, maxiter + 1):                                     # :188
        log.nextiter_()                                                  # :189
        F = _Bsvd(L.B)                                                   # :192
        if method == "ritz":                                             # :194-200
            thickrestart_(A, L, F, j, ops=ops)
        elif method == "harmonic":
            harmonicrestart_(A, L, F, j, ops=ops)
        else:
            raise ArgumentError(f"Unknown restart method {method}")
        extend_(log, A, L, k, ops=ops)                                   # :201
        if verbose:
            print(f"Iteration {it}: {round(time.perf_counter() - T0, 3)} seconds")

        conv = isconverged(L, F, l, tol, reltol, log, verbose)           # :207

        _Log.push(log, "conv", conv)                                     # :209-212
        _Log.push(log, "ritz", np.array(F.S[:k]))
        _Log.push(log, "Bs", L.B.copy())
        _Log.push(log, "betas", L.beta)

        if method == "ritz" and dolock:                                  # :215-221
            for i in range(len(conv)):
                if conv[i]:
                    L.B.av[i] = T(0)
        if np.all(conv):                                                 # :222
            log.setconv(True)
            break
    _Log.shrink(log)                                                     # :224

    values = np.array(F.S[:l])                                           # :227
    if vecs == "none":                                                   # :242-243
        return values, L
    # :230-237 multiply the factorisation AFTER the last restart and extension by the factors of the B BEFORE it, which are only close to the
    # right ones once B has stopped changing; a run that converges in its first restart then returns vectors with A v != sigma u.  Here the
    # vectors come from the SVD of the B that belongs to L.P and L.Q (one more k x k SVD on the host); the values stay the reference's.
    FL = _Bsvd(L.B)
    leftvecs = rightvecs = None
    if vecs in ("left", "both"):                                         # :230-231  L.P * view(F.U, :, 1:l)
        leftvecs = ops.rotate(L.P, L.np_, FL.U[:, :l], ops.matrix(ops.m, l))
    if vecs in ("right", "both"):                                        # :236-237  (view(L.Q, :, 1:size(L.Q, 2) - 1) * view(F.V, :, 1:l))'
        rightvecs = ops.rotate(L.Q, L.nq - 1, FL.V[:, :l], ops.matrix(ops.n, l))
    return SVD(leftvecs, values, V=rightvecs), L                         # :245


def isconverged(L, F, k: int, tol, reltol, log, verbose: bool = False):
    """:290-350.  ``conv[i]``: the error bound of Ritz value i is below ``max(tol, reltol * sigma[1])``."""
    assert tol >= 0                                                      # :294
    sigma = np.array(F.S[:k])                                            # :296
    T = sigma.dtype.type
    Dsigma = T(L.beta) * np.abs(F.U[-1, :k])                             # :297
    dsigma = Dsigma.copy()                                               # :300
    if k > 1:                                                            # :307
        d = T(np.inf)
        for i in range(len(sigma)):                                      # :309-311
            for jj in range(i):
                d = min(d, abs(sigma[i] - sigma[jj]))
        if verbose:
            print("Smallest empirical spectral gap: ", d)
            print("Normwise backward error associated with subspace: ", L.beta / sigma[0])
        for i in range(len(Dsigma)):                                     # :316
            alpha = Dsigma[i]
            if 2 * alpha <= d:                                           # :320
                y = alpha ** 2 / d                                       # :326
                dsigma[i] = min(dsigma[i], y)                            # :328
            if verbose:
                print("Ritz value ", i + 1, ": ", sigma[i], " +- ", dsigma[i])
    if verbose and (F.S[0] / F.S[-1]) > 1 / math.sqrt(np.finfo(sigma.dtype).eps):   # :344-346
        print("Warning: Two-sided reorthogonalization should be used but is not implemented")
    _Log.push(log, "resnorm", dsigma[:k].copy())                         # :348
    return dsigma[:k] < max(tol, reltol * sigma[0])                      # :349


def build(log, A, q, k: int, ops=None):
    """:353-363 (Hernandez 2008).  ``q``: host array, owned by the factorisation from here on."""
    ops = _ops_for(A, ops)
    T = ops.dtype.type
    P, Pt = ops.matrix(ops.m, k), ops.matrix(ops.m, k)                   # the only device allocations of a run (+ the vectors asked for)
    Q, Qt = ops.matrix(ops.n, k + 1), ops.matrix(ops.n, k + 1)
    ops.set_col(Q, 0, q)
    qd, pd = Q.col(0), P.col(0)
    beta = ops.norm(qd)                                                  # :356
    ops.scal(qd, T(1) / beta)                                            # :357
    ops.mul(pd, qd)                                                      # :358
    alpha = ops.norm(pd)                                                 # :359
    ops.scal(pd, T(1) / alpha)                                           # :360
    bidiag = BrokenArrowBidiagonal([alpha], [], [])                      # :361
    return extend_(log, A, PartialFactorization(P, Q, bidiag, beta, 1, 1, Pt, Qt), k, ops=ops)   # :362


def thickrestart_(A, L, F, l: int, ops=None):
    """Thick restart with ordinary Ritz values, :376-405."""
    ops = _ops_for(A, ops)
    T = ops.dtype.type
    k = F.V.shape[0]                                                     # :379
    ops.rotate(L.Q, k, F.V[:, :l], L.Qt)                                 # :384
    ops.copy(L.Qt.col(l), L.Q.col(k))                                    # :385
    L.Q, L.Qt, L.nq = L.Qt, L.Q, l + 1

    rho = (T(L.beta) * F.U[-1, :l]).astype(ops.dtype)                    # :391
    ops.rotate(L.P, k, F.U[:, :l], L.Pt)                                 # :392
    L.P, L.Pt, L.np_ = L.Pt, L.P, l
    f = L.P.col(l)
    ops.mul(f, L.Q.col(l))                                               # :390

    ops.gemv_n(f, L.P, l, rho, -1)                                       # :395
    alpha = ops.norm(f)                                                  # :396
    ops.scal(f, T(1) / alpha)                                            # :397
    L.np_ = l + 1                                                        # :398

    g = L.Q.col(l + 1)                                                   # the next free column: extend! overwrites it
    ops.mul_adj(g, f)                                                    # :400
    L.beta = ops.axpy_nrm2(-alpha, L.Q.col(l), g)                        # :400-401
    L.B = BrokenArrowBidiagonal(list(F.S[:l]) + [alpha], list(rho), [])  # :402
    return L


def harmonicrestart_(A, L, F, k: int, ops=None):
    """Thick restart with harmonic Ritz values, :424-494."""
    ops = _ops_for(A, ops)
    dt = ops.dtype
    T = dt.type
    B = L.B.Matrix() if isinstance(L.B, BrokenArrowBidiagonal) else L.B
    m = B.shape[0]                                                       # :427
    F0 = F                                                               # :430
    rho = (T(L.beta) * F0.U[-1, :]).astype(dt)                           # :431
    BA = np.hstack([np.diag(F0.S).astype(dt), rho.reshape(m, 1)])        # :435
    U2, S2, V2t = np.linalg.svd(BA, full_matrices=True)                  # :436
    Sigma = S2[:k]                                                       # :439
    U = F0.U @ U2[:, :k]                                                 # :440
    M = np.eye(m + 1, dtype=dt)                                          # :441
    M[:m, :m] = F0.V                                                     # :442
    M = M @ V2t.T                                                        # :443
    Mend = M[-1, :k].copy()                                              # :444
    r0 = np.zeros(m, dt)                                                 # :446-447
    r0[-1] = 1
    try:                                                                 # :451-459
        r = np.linalg.solve(B, r0).astype(dt)
        if not np.all(np.isfinite(r)):
            raise np.linalg.LinAlgError("singular")
    except np.linalg.LinAlgError:
        r = (np.linalg.pinv(B) @ r0).astype(dt)
    r = r * T(L.beta)                                                    # :460
    M = M[:m, :] + np.outer(r, M[m, :])                                  # :461

    M2 = np.zeros((m + 1, k + 1), dt)                                    # :463-466
    M2[:m, :k] = M[:, :k]
    M2[:m, k] = -r
    M2[m, k] = 1
    Qf, R = np.linalg.qr(M2)                                             # :467-468

    ops.rotate(L.Q, m + 1, Qf[:, :k + 1], L.Qt)                          # :470
    ops.rotate(L.P, m, U[:, :k], L.Pt)                                   # :471
    L.Q, L.Qt, L.nq = L.Qt, L.Q, k + 1
    L.P, L.Pt, L.np_ = L.Pt, L.P, k

    R = R[:k + 1, :k] + np.outer(R[:, k], Mend)                          # :473

    f = L.P.col(k)
    ops.mul(f, L.Q.col(k))                                               # :475
    if k > 0:
        h = ops.gemv_t(L.P, k, f)                                        # :476
        ops.gemv_n(f, L.P, k, h, -1)
    alpha = ops.norm(f)                                                  # :477
    ops.scal(f, T(1) / alpha)                                            # :478
    L.np_ = k + 1                                                        # :479
    Bn = np.zeros((k + 1, k + 1), dt)                                    # :480
    Bn[:k, :] = np.diag(Sigma) @ np.triu(R.T)
    Bn[k, k] = alpha
    g = L.Q.col(k + 1)                                                   # the next free column: extend! overwrites it
    ops.mul_adj(g, f)                                                    # :482
    q = L.Q.col(k)                                                       # :483
    L.beta = ops.axpy_nrm2(-ops.dot(g, q), q, g)                         # :485-486
    L.B = Bn                                                             # :489-492
    return L


def extend_(log, A, L, k: int, orthleft: bool = False, orthright: bool = True, alpha=None, ops=None):
    """Extend the factorisation to k pairs of Lanczos vectors, :542-609.  The new vectors are formed in place, in the next free columns of
    ``L.Q`` / ``L.P``.  Raises ``SvdlBreakdown`` when a new right vector vanishes (``beta == 0``)."""
    ops = _ops_for(A, ops)
    T = ops.dtype.type
    alpha = T(1 / math.sqrt(2)) if alpha is None else T(alpha)           # :544
    l = _Bsize(L.B) - 1                                                  # :547
    p = L.P.col(l)                                                       # :548
    if not isinstance(L.B, BrokenArrowBidiagonal):                       # :554-559
        Bk = np.zeros((k, k), ops.dtype)
        Bk[:L.B.shape[0], :L.B.shape[1]] = L.B
        L.B = Bk
    beta = L.beta                                                        # :561
    for j in range(l + 1, k + 1):                                        # :563
        log.mtvps += 1                                                   # :564
        q = L.Q.col(L.nq)
        ops.mul_adj(q, p)                                                # :565
        if orthright:                                                    # :567-577
            beta, _ = ops.reorth(L.Q, L.nq, q, alpha)
        else:
            beta = ops.norm(q)                                           # :576
            if beta != 0:
                ops.scal(q, T(1) / beta)                                 # :577
        if beta == 0:
            raise SvdlBreakdown(8, "svdl", "extend!: the new right Lanczos vector is zero (beta == 0); the reference divides by zero here")
        L.nq += 1                                                        # :579
        if j == k:                                                       # :580
            break
        log.mvps += 1                                                    # :582
        pn = L.P.col(L.np_)
        ops.mul(pn, q)                                                   # :584
        if orthleft:                                                     # :585-597
            ops.axpy_nrm2(-beta, L.P.col(j - 1), pn)
            alpha, _ = ops.reorth(L.P, L.np_, pn, alpha)
        else:
            alpha = ops.axpy_nrm2(-beta, L.P.col(j - 1), pn)             # :585, :596
            ops.scal(pn, T(1) / alpha)                                   # :597
        if isinstance(L.B, BrokenArrowBidiagonal):                       # :598-604
            L.B.dv.append(alpha)
            L.B.ev.append(beta)
        else:
            L.B[j, j] = alpha
            L.B[j - 1, j] = beta
        L.np_ += 1                                                       # :605
        p = pn
    L.beta = beta                                                        # :607
    return L
