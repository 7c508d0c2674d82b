"""``lobpcg`` -- the Locally Optimal Block Preconditioned Conjugate Gradient method for the extreme eigenpairs of ``A x = lambda B x`` on
device operators, sparse (``HipCSR``) or dense (``HipMatrix``) (src/lobpcg.jl, v0.9.4), restated function by function; Julia's ``f!`` is spelled ``f_``.  Citations are file:line in
the reference checkout.

What runs where
  device   everything of length n, a block of columns at a time: ``A*X`` / ``B*X`` (``mik_spmm`` for a ``HipCSR``, ``mik_dense_mm`` for a
           ``HipMatrix``), every cross product ``X'Y`` of the block
           Gram matrices, of CholQR and of the constraint (``mik_block_gram``), ``X * inv(R)`` of CholQR (``mik_block_rdiv``), the Ritz update
           of X, AX, BX and P, AP, BP (``mik_block_update``); column by column the residuals with their norms (``mik_copy`` +
           ``mik_axpy_dot``), the gather of the active columns (``mik_copy``), ``X -= Y*tmp`` of the constraint (``mik_gemv_n``) and the
           preconditioner (``mik_divide`` for ``JacobiPrec``, else ``ldiv_`` per column);
  host     in numpy, in the element type: the Cholesky factorisations, the triangular solves of the constraint, and the Rayleigh-Ritz
           problem of at most 96 x 96 (``eigh``; the generalised problem reduced by the Cholesky factor of ``gramB``; a stable argsort).
Every block, and the block workspace of a dense operator, is allocated when the iterator is built; the update writes into a spare X triple that is then swapped in.  Nothing is allocated
on the device inside the iteration loop.

Differences from the reference, all deliberate:
  * ``A`` and ``B`` are ``HipCSR``, or -- with ``dense=True`` -- each a ``HipCSR`` or a square ``HipMatrix`` (the two may differ).  Without the
    keyword a ``HipMatrix`` is refused as it always was: that refusal is behaviour callers and the suite rely on, so the dense route is asked for;
    real float32 / float64 -- and, for ``HipCSR`` operators, complex64 / complex128 (Hermitian ``A``, Hermitian positive definite ``B``;
    DESIGN.md section 20); a block is at most 32 columns wide (the width of the device entries);
  * where the reference calls ``rand`` the functions take ``rng=`` (a ``numpy.random.Generator``), so that runs repeat;
  * ``results.X`` stays on the device (a ``HipMatrix``); ``X0`` and ``C`` are ``HipMatrix`` or numpy arrays and are copied;
  * a Cholesky factorisation that fails (a block that lost rank, a ``B`` that is not positive definite) raises ``LobpcgCholeskyError``,
    a ``MikError``, where the reference lets LAPACK's PosDefException through;
  * the refusals of :833-834 and :933-934 throw strings in the reference; here ``LobpcgRefusal``, a ``ValueError``;
  * the residual column is formed as ``AX + (-lambda) * BX`` (the same value as ``AX - BX * lambda``: a negation is exact) and its norm is
    the device's ``norm`` of the stored column instead of a serial sum of squares (:538-545);
  * the constraint subtracts ``Y * tmp`` one column of Y at a time (``X[:, j] += (-tmp[i, j]) * Y[:, i]``, i ascending) instead of forming
    the product first (:220-221);
  * complex element types: ``rdiv!`` (:345-355) divides a column by ``R[i, i]``, a complex number whose imaginary part ``realdiag!``
    (:357-363) has set to zero; ``mik_block_rdiv`` divides re and im by ``real(R[i, i])`` -- two real divisions, no complex division on the
    device -- and refuses a factor whose diagonal is not real.  A complex ``HipMatrix`` and ``JacobiPrec`` on complex vectors stay refused;
  * every call of ``lobpcg_`` starts a trace of its own; the reference keeps pushing into the one vector the iterator owns (:883), so the
    batches of the multi-batch driver would share one growing trace.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import MikError, check, dtype_code, lib
from .api import HipCSR, HipMatrix, Identity, JacobiPrec
from .dense_factor import DenseFactor

_vp = C.c_void_p
MAX_BLOCK = 32                                                           # widest block of mik_spmm / mik_dense_mm / mik_block_gram / mik_block_rdiv / mik_block_update


class LobpcgRefusal(ValueError):
    """The reference's ``throw("...")`` of :833-834 and :933-934."""


class LobpcgCholeskyError(MikError, ArithmeticError):
    """A Gram matrix that CholQR, the constraint or the Rayleigh-Ritz problem has to factor is not positive definite."""


# ==============================================================================================
# LOBPCGState, LOBPCGResults  -- src/lobpcg.jl:36-91
# ==============================================================================================
class LOBPCGState:
    """``LOBPCGState`` (:36-40): one entry of the trace."""

    def __init__(self, iteration, residual_norms, ritz_values):
        self.iteration, self.residual_norms, self.ritz_values = iteration, residual_norms, ritz_values

    def __repr__(self):                                                  # :41-44
        return f"{self.iteration:8d}    {np.max(self.residual_norms):14e}" if self.residual_norms is not None else f"{self.iteration:8d}"


class LOBPCGResults:
    """``LOBPCGResults`` (:56-65).  ``lam`` is ``λ``; ``X`` is a device matrix."""

    def __init__(self, lam, X, tolerance, residual_norms, iterations, maxiter, converged, trace):
        self.lam, self.X, self.tolerance, self.residual_norms = lam, X, tolerance, residual_norms
        self.iterations, self.maxiter, self.converged, self.trace = iterations, maxiter, converged, trace

    λ = property(lambda self: self.lam)

    def __repr__(self):                                                  # :92-115
        return ("Results of LOBPCG Algorithm\n * Algorithm: LOBPCG - CholQR\n"
                f" * λ: {np.asarray(self.lam).tolist()}\n * Residual norm(s): {np.asarray(self.residual_norms).tolist()}\n * Convergence\n"
                f"   * Iterations: {self.iterations}\n   * Converged: {bool(np.all(self.converged))}\n   * Iterations limit: {self.maxiter}\n")


def _real_dtype(dtype):
    """``real(T)``: the type of a residual norm and of the tolerance."""
    return np.zeros(0, dtype).real.dtype


def _rand(rng, shape, dtype):
    """``rand(T, shape...)`` from ``rng``: a complex type draws re and im."""
    if np.dtype(dtype).kind == "c":
        return rng.random(shape) + 1j * rng.random(shape)
    return rng.random(shape)


def _empty_results(ops, blocksize, k, tolerance, maxiter):
    """``EmptyLOBPCGResults`` (:66-77)."""
    lam = np.zeros(k, ops.dtype)
    return LOBPCGResults(lam, ops.matrix(ops.n, k), tolerance, np.zeros(k, _real_dtype(ops.dtype)), np.zeros(-(-k // blocksize), np.int64), maxiter, np.zeros(k, bool),
                         [[] for _ in range(k // blocksize + 1)])


def _append(ops, r1, r2, n1, n2=None):
    """``append!(r1, r2, n1, n2)`` (:79-91): the LAST n2 pairs of r2 become pairs n1 .. n1 + n2 of r1."""
    m = len(r2.lam)
    n2 = m if n2 is None else n2
    r1.lam[n1:n1 + n2] = r2.lam[m - n2:]
    r1.residual_norms[n1:n1 + n2] = r2.residual_norms[m - n2:]
    ops.copy_cols(r1.X, n1, r2.X, m - n2, n2)
    ind = n1 // m
    r1.iterations[ind] = r2.iterations
    r1.converged[n1:n1 + n2] = r2.converged
    r1.trace[ind] = r2.trace
    return r1


# ==============================================================================================
# the device side
# ==============================================================================================
class DeviceOps:
    """Every statement of length n, on the device.  (tests/lobpcg_double.py implements the same methods in numpy.)"""

    def __init__(self, A, B=None, dense=False):
        for M, name in ((A, "A"), (B, "B")):
            if M is None and name == "B":
                continue
            if isinstance(M, HipMatrix) and not dense:
                raise TypeError(f"lobpcg needs HipCSR operators ({name} is a HipMatrix: pass dense=True to run it through mik_dense_mm)")
            if not isinstance(M, (HipCSR, HipMatrix)):
                raise TypeError(f"lobpcg needs HipCSR operators, or HipMatrix ones with dense=True ({name} is {type(M).__name__}; callbacks are not supported)")
        if A.n_rows != A.n_cols or (B is not None and (B.n_rows, B.n_cols, np.dtype(B.dtype)) != (A.n_rows, A.n_cols, np.dtype(A.dtype))):
            raise ValueError("DimensionMismatch: lobpcg needs square A and B of one size and element type")
        self.ctx, self.dtype, self.n = A.ctx, np.dtype(A.dtype), A.n_rows
        if self.dtype.kind == "c" and (isinstance(A, HipMatrix) or isinstance(B, HipMatrix)):
            raise TypeError(f"lobpcg is not offered for a {self.dtype} HipMatrix (the block product mik_dense_mm is real only)")
        self.code = dtype_code(self.dtype)                               # complex: the complex instances of the four block entries
        for M in (A, B):
            if isinstance(M, HipMatrix):
                M.reserve_block_()                                       # the partials of mik_dense_mm: allocated here, not in the loop

    # -- storage ----------------------------------------------------------------------------------
    def matrix(self, rows, cols):
        return HipMatrix(rows, max(int(cols), 1), self.dtype, self.ctx)

    def upload(self, M, host, c0=0):
        host = np.asarray(host, self.dtype)
        for j in range(host.shape[1]):
            M.col(c0 + j).copy_from_host(host[:, j])

    def download(self, M, cols):
        return np.stack([M.col(j).to_numpy() for j in range(cols)], axis=1) if cols else np.zeros((M.n, 0), self.dtype)

    def copy_cols(self, dst, d0, src, s0, count):
        for j in range(count):
            dst.col(d0 + j).copyto_(src.col(s0 + j))

    def _at(self, M, j):
        return _vp(M.buf.ptr + j * M.ld * self.dtype.itemsize)

    # -- the four block entries -------------------------------------------------------------------
    def spmm(self, A, X, b, Y):                                          # mul!(Y[:, 1:b], A, X[:, 1:b]), :124-139
        if isinstance(A, HipMatrix):
            A.mm_(Y, X, b)
            return
        check(lib().mik_spmm(self.ctx.handle, A.handle, int(b), _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld), "mik_spmm", self.ctx.handle)

    def gram(self, X, p, Y, q, x0=0, y0=0):                              # X[:, x0:x0+p]' * Y[:, y0:y0+q] -> host
        G = np.zeros((p, q), self.dtype, order="F")
        if p and q:
            check(lib().mik_block_gram(self.ctx.handle, self.code, X.n, int(p), int(q), self._at(X, x0), X.ld, self._at(Y, y0), Y.ld,
                                       G.ctypes.data_as(_vp), p), "mik_block_gram", self.ctx.handle)
        return G

    def rdiv(self, X, s, R):                                             # rdiv!(X[:, 1:s], UpperTriangular(R)), :345-355
        R = np.asfortranarray(R, self.dtype)
        check(lib().mik_block_rdiv(self.ctx.handle, self.code, X.n, int(s), R.ctypes.data_as(_vp), R.shape[0], _vp(X.buf.ptr), X.ld),
              "mik_block_rdiv", self.ctx.handle)

    def update(self, sx, b1, b2, X, R, P, V, Xout, Pout):                # one block triple of update_X_P!, :629-690
        V = np.asfortranarray(V, self.dtype)
        check(lib().mik_block_update(self.ctx.handle, self.code, X.n, int(sx), int(b1), int(b2), _vp(X.buf.ptr), X.ld, _vp(R.buf.ptr), R.ld,
                                     _vp(P.buf.ptr), P.ld, V.ctypes.data_as(_vp), V.shape[0], _vp(Xout.buf.ptr), Xout.ld, _vp(Pout.buf.ptr), Pout.ld),
              "mik_block_update", self.ctx.handle)

    # -- composed from the vector entries ---------------------------------------------------------
    def residuals(self, AX, BX, lam, R, sx):                             # residuals!, :533-547
        from . import api
        out = np.zeros(sx, _real_dtype(self.dtype))
        lam = np.real(lam)                                               # Ritz values are real: real x complex on a complex block
        for j in range(sx):
            r = R.col(j)
            r.copyto_(AX.col(j))
            out[j] = api.axpy_dot_(-lam[j], BX.col(j), r, None)
        return out

    def gather_cols(self, dst, src, mask):                               # dst[:, 1:bs] .= src[:, mask], :557-562
        k = 0
        for j in np.flatnonzero(mask):
            dst.col(k).copyto_(src.col(int(j)))
            k += 1

    def constrain(self, X, sx, Y, sy, tmp):                              # X .-= Y * tmp, :220-221
        from . import api
        for j in range(sx):
            api.gemv_n_(X.col(j), Y, sy, np.ascontiguousarray(tmp[:, j], self.dtype), -1)

    def precond(self, P, X, bs, temp):                                   # RPreconditioner, :236-242
        if P is None or isinstance(P, Identity):
            return
        if isinstance(P, JacobiPrec):
            for j in range(bs):
                P.ldiv_(X.col(j))
            return
        if not callable(getattr(P, "ldiv_", None)):
            raise MikError(5, "lobpcg", "the preconditioner needs ldiv_(y, x)")
        if isinstance(P, DenseFactor) and bs >= P.block_min_cols:        # lu(A) / cholesky(A): one block solve in place, the bits of bs vector solves
            P.ldiv_(X, cols=bs)
            return
        for j in range(bs):
            P.ldiv_(temp.col(j), X.col(j))
            X.col(j).copyto_(temp.col(j))


# ==============================================================================================
# host helpers: Hermitian(.) reads the upper triangle; the factorisations in the element type
# ==============================================================================================
def _hermitian(G):
    """``Hermitian(G)``: the upper triangle, its conjugate below, a real diagonal.  (The real path is the code it always was.)"""
    U = np.triu(G)
    if not np.iscomplexobj(G):
        return U + np.triu(G, 1).T
    H = U + np.triu(G, 1).conj().T
    np.fill_diagonal(H, np.diagonal(H).real)
    return H


def _adjoint(M):
    return M.conj().T if np.iscomplexobj(M) else M.T


def _cholesky_upper(G, what):
    """``cholesky!(Hermitian(G)).factors``: the upper factor R with R'R = G; complex: the diagonal made real, as ``realdiag!`` (:357-363)."""
    try:
        R = np.ascontiguousarray(_adjoint(np.linalg.cholesky(_hermitian(G))))
    except np.linalg.LinAlgError as e:
        raise LobpcgCholeskyError(8, "lobpcg", f"{what} is not positive definite ({e})") from None
    if np.iscomplexobj(R):
        np.fill_diagonal(R, np.diagonal(R).real)
    return R


def _solve_upper_t(R, b):
    """x with R' x = b (R' the conjugate transpose), R upper triangular; columns of b one after another, forward substitution in the
    element type."""
    x = np.array(b, dtype=R.dtype, copy=True)
    Rc = R.conj() if np.iscomplexobj(R) else R
    for i in range(R.shape[0]):
        x[i] = (x[i] - Rc[:i, i] @ x[:i]) / Rc[i, i]
    return x


def _solve_upper(R, b):
    """x with R x = b, R upper triangular: back substitution."""
    x = np.array(b, dtype=R.dtype, copy=True)
    for i in range(R.shape[0] - 1, -1, -1):
        x[i] = (x[i] - R[i, i + 1:] @ x[i + 1:]) / R[i, i]
    return x


# ==============================================================================================
# Blocks, Constraint, CholQR  -- src/lobpcg.jl:117-224, :340-393
# ==============================================================================================
class Blocks:
    """``Blocks{Generalized}`` (:117-123): a block with its A- and B-image; without B the B-image IS the block."""

    def __init__(self, block, A_block, B_block=None):
        self.block, self.A_block = block, A_block
        self.B_block = block if B_block is None else B_block
        self.generalized = B_block is not None

    def triple(self):
        return ("block", "A_block", "B_block") if self.generalized else ("block", "A_block")


def _new_blocks(ops, sizeX, generalized, block=None):
    block = ops.matrix(ops.n, sizeX) if block is None else block
    return Blocks(block, ops.matrix(ops.n, sizeX), ops.matrix(ops.n, sizeX) if generalized else None)


class Constraint:
    """``Constraint`` (:144-224): keeps blocks B-orthogonal to the columns of ``Y``.  ``Y`` / ``BY`` are device matrices of full capacity of
    which the first ``sizeY`` columns count (the reference's views into a parent); ``chol`` is the upper Cholesky factor of ``Y'BY``
    embedded in an identity of the capacity's size, so that ``update_`` only has to move ``sizeY`` (:200-204)."""

    def __init__(self, ops, Y, BY, sizeY):                               # :171-186
        self.ops, self.Y, self.BY, self.sizeY = ops, Y, BY, int(sizeY)
        if Y is None:
            return
        cap = Y.cols
        self.chol = np.eye(cap, dtype=ops.dtype)
        if self.sizeY:
            self.chol[:self.sizeY, :self.sizeY] = _cholesky_upper(_gram(ops, Y, self.sizeY, BY, self.sizeY), "the constraint's Y'BY")

    def update_(self, X, BX, sizeX):                                     # update!, :188-206
        ops = self.ops
        ops.copy_cols(self.Y, self.sizeY, X, 0, sizeX)
        if X is not BX:
            ops.copy_cols(self.BY, self.sizeY, BX, 0, sizeX)
        self.sizeY += sizeX
        return self

    def __call__(self, X, sizeX):                                        # :208-224
        if self.Y is None or self.sizeY == 0 or sizeX == 0:
            return
        ops, sy = self.ops, self.sizeY
        gramYBV = _gram(ops, self.BY, sy, X, sizeX)                      # :217
        R = self.chol[:sy, :sy]
        tmp = _solve_upper(R, _solve_upper_t(R, gramYBV))                # :219
        ops.constrain(X, sizeX, self.Y, sy, tmp)                         # :220-221


def _gram(ops, X, p, Y, q):
    """``X[:, 1:p]' * Y[:, 1:q]`` on the host, in tiles of at most MAX_BLOCK columns a side."""
    G = np.zeros((p, q), ops.dtype)
    for i0 in range(0, p, MAX_BLOCK):
        for j0 in range(0, q, MAX_BLOCK):
            pi, qj = min(MAX_BLOCK, p - i0), min(MAX_BLOCK, q - j0)
            G[i0:i0 + pi, j0:j0 + qj] = ops.gram(X, pi, Y, qj, i0, j0)
    return G


def cholqr_(ops, blocks, sizeX, update_AX=False, update_BX=False):
    """``CholQR`` (:365-393): B-orthonormalise the first ``sizeX`` columns of ``blocks.block``; BX is assumed premultiplied."""
    R = _cholesky_upper(ops.gram(blocks.block, sizeX, blocks.B_block, sizeX), "CholQR: X'BX")     # :375-381
    ops.rdiv(blocks.block, sizeX, R)                                     # :383
    if update_AX:
        ops.rdiv(blocks.A_block, sizeX, R)                               # :384
    if blocks.generalized and update_BX:
        ops.rdiv(blocks.B_block, sizeX, R)                               # :385


# ==============================================================================================
# LOBPCGIterator  -- src/lobpcg.jl:395-522, :524-749
# ==============================================================================================
def _host(M):
    return M.to_numpy() if hasattr(M, "to_numpy") else np.asarray(M)


class LOBPCGIterator:
    """``LOBPCGIterator(A, [B,] largest, X, [nev,] P, C)`` (:435-522).  ``X``: the initial Ritz vectors (``HipMatrix`` or numpy, copied).
    With ``nev`` the constraint gets room for the pairs the multi-batch driver deflates (:497-522)."""

    def __init__(self, A, B, largest, X, nev=None, P=None, C=None, ops=None, dense=False):
        ops = self.ops = ops if ops is not None else DeviceOps(A, B, dense)
        self.A, self.B, self.largest, self.P = A, B, bool(largest), P
        Xh = np.asarray(_host(X), ops.dtype)
        if Xh.ndim != 2 or Xh.shape[0] != ops.n:
            raise ValueError(f"DimensionMismatch: X is {Xh.shape}, the operator has {ops.n} rows")
        sizeX = self.sizeX = Xh.shape[1]
        if not 1 <= sizeX <= MAX_BLOCK:
            raise MikError(5, "lobpcg", f"block size {sizeX}: the device entries take 1 to {MAX_BLOCK} columns")
        T = ops.dtype
        generalized = self.generalized = B is not None
        # constr! -- :452, :501-519
        Ch = None if C is None else np.asarray(_host(C), T)
        sizeC = 0 if Ch is None else Ch.shape[1]
        if nev is None and Ch is None:
            self.constr = Constraint(ops, None, None, 0)                 # Constraint{Nothing}, :154-158
        else:
            cap = sizeC + (0 if nev is None else (nev // sizeX) * sizeX)
            Y = ops.matrix(ops.n, cap)
            if sizeC:
                ops.upload(Y, Ch)
            BY = Y
            if generalized:
                BY = ops.matrix(ops.n, cap)
                for j0 in range(0, sizeC, MAX_BLOCK):                    # :167, :516-518
                    jb = min(MAX_BLOCK, sizeC - j0)
                    Yt, BYt = ops.matrix(ops.n, jb), ops.matrix(ops.n, jb)
                    ops.copy_cols(Yt, 0, Y, j0, jb)
                    ops.spmm(B, Yt, jb, BYt)
                    ops.copy_cols(BY, j0, BYt, 0, jb)
            self.constr = Constraint(ops, Y, BY, sizeC)
        # the blocks -- :458-472 (RBlocks needs its block only)
        self.XBlocks = _new_blocks(ops, sizeX, generalized)
        ops.upload(self.XBlocks.block, Xh)
        self.tempXBlocks = _new_blocks(ops, sizeX, generalized)
        self.RBlocks = Blocks(ops.matrix(ops.n, sizeX), None)
        self.activeRBlocks = _new_blocks(ops, sizeX, generalized)
        self.PBlocks = _new_blocks(ops, sizeX, generalized)
        self.activePBlocks = _new_blocks(ops, sizeX, generalized)
        self.ritz_values = np.zeros(3 * sizeX, T)                        # :473-479
        self.lam = np.zeros(sizeX, T)
        self.V = np.zeros((3 * sizeX, 3 * sizeX), T)
        self.residuals = np.full(sizeX, np.nan, _real_dtype(T))
        self.iteration = 1
        self.currentBlockSize = sizeX
        self.gramA = np.zeros((3 * sizeX, 3 * sizeX), T)                 # :486-487
        self.gramB = np.zeros((3 * sizeX, 3 * sizeX), T)
        self.activeMask = np.ones(sizeX, bool)                           # :489
        self.trace = []

    @property
    def X(self):
        return self.XBlocks.block

    # -- :524-532 ---------------------------------------------------------------------------------
    def _ortho_AB_mul_X(self, blocks, bs):
        ops = self.ops
        if blocks.generalized:
            ops.spmm(self.B, blocks.block, bs, blocks.B_block)           # B_mul_X!
        cholqr_(ops, blocks, bs, update_BX=True)
        ops.spmm(self.A, blocks.block, bs, blocks.A_block)               # A_mul_X!

    def _residuals(self):                                                # :533-547
        X = self.XBlocks
        self.residuals[:] = self.ops.residuals(X.A_block, X.B_block, self.ritz_values[:self.sizeX], self.RBlocks.block, self.sizeX)

    def _update_mask(self, tol):                                         # :549-555
        self.activeMask[:] = self.residuals[:self.sizeX] > tol
        self.currentBlockSize = int(np.sum(self.activeMask))

    def _precond_constr(self, block, bs):                                # :564-569
        self.ops.precond(self.P, block, bs, self.tempXBlocks.block)
        self.constr(block, bs)

    # -- the Gram blocks, :570-605 and :282-338 ---------------------------------------------------
    def _block_grams(self, bs, with_p):
        ops, sx = self.ops, self.sizeX
        X, R, P = self.XBlocks, self.activeRBlocks, self.activePBlocks
        gA, gB = self.gramA, self.gramB
        xr, rr, pr = slice(0, sx), slice(sx, sx + bs), slice(sx + bs, sx + 2 * bs)
        gA[xr, xr] = np.diag(self.ritz_values[:sx])                      # :289
        gB[xr, xr] = np.eye(sx, dtype=ops.dtype)                         # :312
        gA[xr, rr] = ops.gram(X.block, sx, R.A_block, bs)                # XAR!
        gA[rr, rr] = ops.gram(R.block, bs, R.A_block, bs)                # RAR!
        gB[xr, rr] = ops.gram(X.block, sx, R.B_block, bs)                # XBR!
        gB[rr, rr] = np.eye(bs, dtype=ops.dtype)
        if with_p:
            gA[xr, pr] = ops.gram(X.block, sx, P.A_block, bs)            # XAP!
            gA[rr, pr] = ops.gram(R.A_block, bs, P.block, bs)            # RAP!
            gA[pr, pr] = ops.gram(P.block, bs, P.A_block, bs)            # PAP!
            gB[xr, pr] = ops.gram(X.block, sx, P.B_block, bs)            # XBP!
            gB[rr, pr] = ops.gram(R.B_block, bs, P.block, bs)            # RBP!
            gB[pr, pr] = np.eye(bs, dtype=ops.dtype)

    def _sub_problem(self, bs1, bs2):                                    # :607-627
        sx = self.sizeX
        subdim = sx + bs1 + bs2
        if bs1 == 0:
            X = self.XBlocks
            values, vectors = np.linalg.eigh(_hermitian(self.ops.gram(X.block, sx, X.A_block, sx)))      # XAX!, :572, :610-613
        else:
            GA, GB = _hermitian(self.gramA[:subdim, :subdim]), self.gramB[:subdim, :subdim]
            Rb = _cholesky_upper(GB, "the Rayleigh-Ritz Gram matrix of B")       # GB = Rb' Rb
            Cm = _adjoint(_solve_upper_t(Rb, _adjoint(_solve_upper_t(Rb, GA))))      # inv(Rb') GA inv(Rb)
            values, Z = np.linalg.eigh(_hermitian(Cm))
            vectors = _solve_upper(Rb, Z)                                # :620: vectors' GB vectors = I
        values = values.astype(self.ops.dtype)
        key = values.real if np.iscomplexobj(values) else values         # Ritz values are real (eigh), stored in the element type
        perm = np.argsort(-key if self.largest else key, kind="stable")[:sx]       # :623
        self.ritz_values[:sx] = values[perm]                             # :624
        self.V[:subdim, :sx] = vectors[:, perm]                          # :625

    def _update_X_P(self, bs1, bs2):                                     # :629-690
        sx = self.sizeX
        V = self.V[:sx + bs1 + bs2, :sx]
        X, tX, R, P, Pn = self.XBlocks, self.tempXBlocks, self.activeRBlocks, self.activePBlocks, self.PBlocks
        for name in X.triple():
            self.ops.update(sx, bs1, bs2, getattr(X, name), getattr(R, name), getattr(P, name), V, getattr(tX, name), getattr(Pn, name))
        self.XBlocks, self.tempXBlocks = tX, X                           # the spare triple becomes X

    # -- one iteration, :692-749 ------------------------------------------------------------------
    def step(self, residualTolerance, log):
        ops, sx = self.ops, self.sizeX
        iteration = self.iteration
        if iteration == 1:
            self._ortho_AB_mul_X(self.XBlocks, sx)                       # :696
            self._sub_problem(0, 0)                                      # :698-699
            self._update_X_P(0, 0)
        else:
            bs = self.currentBlockSize
            ops.gather_cols(self.activeRBlocks.block, self.RBlocks.block, self.activeMask)     # :707, :723-727
            if iteration > 2:
                for name in self.PBlocks.triple():
                    ops.gather_cols(getattr(self.activePBlocks, name), getattr(self.PBlocks, name), self.activeMask)
            self._precond_constr(self.activeRBlocks.block, bs)           # :709, :729
            self._ortho_AB_mul_X(self.activeRBlocks, bs)                 # :711, :731
            if iteration > 2:
                cholqr_(ops, self.activePBlocks, bs, update_AX=True, update_BX=True)           # :733
            self._block_grams(bs, iteration > 2)                         # :713, :735
            self._sub_problem(bs, bs if iteration > 2 else 0)            # :715, :737
            self._update_X_P(bs, bs if iteration > 2 else 0)             # :716, :740
        self._residuals()
        self._update_mask(residualTolerance)
        if log:                                                          # :744-748
            return LOBPCGState(iteration, self.residuals[:sx].copy(), self.ritz_values[:sx].copy())
        return LOBPCGState(iteration, None, None)

    __call__ = step


def default_tolerance(dtype):
    """``eps(real(T))^(real(T)(3)/10)`` (:751)."""
    T = _real_dtype(dtype).type
    return T(np.finfo(T).eps) ** (T(3) / T(10))


# ==============================================================================================
# lobpcg!, lobpcg  -- src/lobpcg.jl:787-962
# ==============================================================================================
def lobpcg_(iterator, *, log=False, maxiter=200, not_zeros=False, tol=None, rng=None):
    """``lobpcg!(iterator; log, maxiter, not_zeros, tol)`` (:865-893)."""
    ops, sx = iterator.ops, iterator.sizeX
    tol = default_tolerance(ops.dtype) if tol is None else tol
    iterator.constr(iterator.X, sx)                                      # :868
    if not not_zeros:                                                    # :869-876
        Xh = ops.download(iterator.X, sx)
        rng = np.random.default_rng() if rng is None else rng
        for j in range(sx):
            if not np.any(Xh[:, j]):
                ops.upload(iterator.X, _rand(rng, (ops.n, 1), ops.dtype), j)
        iterator.constr(iterator.X, sx)
    iterator.iteration = 1                                               # :879
    iterator.trace = []
    while iterator.iteration <= maxiter:                                 # :880-887
        state = iterator.step(tol, log)
        if log:
            iterator.trace.append(state)
        if iterator.currentBlockSize == 0:
            break
        iterator.iteration += 1
    iterator.lam[:] = iterator.ritz_values[:sx]                          # :888
    converged = bool(np.all(np.abs(iterator.residuals[:sx]) <= tol))     # :890
    return LOBPCGResults(iterator.lam.copy(), iterator.X, tol, iterator.residuals.copy(), iterator.iteration, maxiter, converged, iterator.trace)


def _split_args(args):
    """``(A, largest, ...)`` or ``(A, B, largest, ...)`` -> ``(B, largest, rest)``."""
    if args and isinstance(args[0], (bool, np.bool_)):
        return None, bool(args[0]), args[1:]
    if len(args) >= 2 and isinstance(args[1], (bool, np.bool_)):
        return args[0], bool(args[1]), args[2:]
    raise TypeError("lobpcg(A, [B,] largest::Bool, nev | X0 [, nev]; ...)")


def lobpcg(A, *args, not_zeros=False, log=False, P=None, maxiter=200, C=None, tol=None, rng=None, ops=None, dense=False):
    """``lobpcg(A, [B,] largest, nev | X0 [, nev]; not_zeros, log, P, C, maxiter, tol)`` -> ``LOBPCGResults`` (:787-839, :925-962).

    ``largest``: True for the largest eigenvalues, False for the smallest.  ``nev`` alone: that many pairs from a random start.  ``X0``: the
    initial block, its width the number of pairs -- or, followed by ``nev``, the width of the batches in which ``nev`` pairs are found, each
    batch deflated against the ones before it.  ``P``: ``JacobiPrec``, ``Identity`` or an object with ``ldiv_(y, x)``; ``C``: a block the
    result is kept B-orthogonal to; ``rng``: the generator behind every random column; ``ops``: the device side (tests swap it); ``dense=True``: ``A`` and ``B`` may be square
    ``HipMatrix`` operators (``mik_dense_mm``), refused otherwise."""
    B, largest, rest = _split_args(args)
    ops = ops if ops is not None else DeviceOps(A, B, dense)
    n = ops.n
    tol = default_tolerance(ops.dtype) if tol is None else tol
    rng = np.random.default_rng() if rng is None else rng
    if len(rest) == 1 and isinstance(rest[0], (int, np.integer)):        # :790-792
        X0, not_zeros = _rand(rng, (n, int(rest[0])), ops.dtype).astype(ops.dtype), True
        rest = (X0,)
    if len(rest) == 1:                                                   # :827-839
        Xh = np.asarray(_host(rest[0]), ops.dtype)
        sizeX = Xh.shape[1]
        if sizeX > n:
            raise LobpcgRefusal("X column dimension exceeds the row dimension")
        if 3 * sizeX > n:
            raise LobpcgRefusal("The LOBPCG algorithms is not stable to use when the matrix size is less than 3 times the block size. "
                                "Please use a dense solver instead.")
        iterator = LOBPCGIterator(A, B, largest, Xh, None, P, C, ops=ops)
        return lobpcg_(iterator, log=log, tol=tol, maxiter=maxiter, not_zeros=not_zeros, rng=rng)
    if len(rest) != 2:
        raise TypeError("lobpcg(A, [B,] largest::Bool, nev | X0 [, nev]; ...)")
    # the multi-batch driver, :928-962
    Xh, nev = np.asarray(_host(rest[0]), ops.dtype), int(rest[1])
    sizeX = Xh.shape[1]
    if nev > n:
        raise LobpcgRefusal("Number of eigenvectors desired exceeds the row dimension.")
    if 3 * sizeX > n:
        raise LobpcgRefusal("The LOBPCG algorithms is not stable to use when the matrix size is less than 3 times the block size. "
                            "Please use a dense solver instead.")
    sizeX = min(nev, sizeX)                                              # :936
    iterator = LOBPCGIterator(A, B, largest, Xh[:, :sizeX], nev, P, C, ops=ops)
    r = _empty_results(ops, sizeX, nev, tol, maxiter)
    rnext = lobpcg_(iterator, log=log, tol=tol, maxiter=maxiter, not_zeros=not_zeros, rng=rng)
    _append(ops, r, rnext, 0)
    converged_x = sizeX
    while converged_x < nev:                                             # :944-960
        X = iterator.XBlocks
        if nev - converged_x < sizeX:
            cutoff = sizeX - (nev - converged_x)
            iterator.constr.update_(X.block, X.B_block, cutoff)          # :947
            ops.copy_cols(X.block, 0, X.block, cutoff, sizeX - cutoff)   # :948
            ops.upload(X.block, _rand(rng, (n, sizeX - cutoff), ops.dtype), cutoff)  # :949
            rnext = lobpcg_(iterator, log=log, tol=tol, maxiter=maxiter, not_zeros=True, rng=rng)
            _append(ops, r, rnext, converged_x, sizeX - cutoff)
            converged_x += sizeX - cutoff
        else:
            iterator.constr.update_(X.block, X.B_block, sizeX)           # :954
            ops.upload(X.block, _rand(rng, (n, sizeX), ops.dtype))       # :955
            rnext = lobpcg_(iterator, log=log, tol=tol, maxiter=maxiter, not_zeros=True, rng=rng)
            _append(ops, r, rnext, converged_x)
            converged_x += sizeX
    return r
