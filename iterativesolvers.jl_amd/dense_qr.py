"""``qr(A)`` / ``qr!(A)`` (Householder, no pivoting) of an m x n dense device matrix, m >= n, its products with ``Q`` and ``Q'``, the
least-squares solve ``F \\ b`` and the thin ``Q`` -- over the ``mik_dense_qr_*`` entries of include/mik.h.  ``A \\ b`` for a tall matrix is
what the reference's tests hold ``lsqr`` and ``lsmr`` to (test/lsqr.jl:15-19, test/lsmr.jl:68-72); ``Matrix(qr(A).Q)`` is how they build an
orthonormal basis (test/orthogonalize.jl:17-18).

Everything runs on the device.  The factors, ``tau``, the products and the solution are bit for bit those of the unblocked loops stated in
csrc/mik_dense_qr.h (tests/dense_ref/dense_qr_ref.c restates them).  The sums of squares are not rescaled: data whose squares overflow or
turn subnormal follow those loops into Inf / 0 / reduced accuracy.  Rows are not split across workgroups: a tall matrix of very few columns
runs on few compute units.

    reference (LinearAlgebra)            here
    ---------------------------------    -----------------------------------------
    qr(A)                                qr(A)          factors a copy
    qr!(A)                               qr_(A)         factors in place, keeps A alive
    F.factors, F.τ                       F.factors, F.tau
    F.R, Matrix(F.Q)                     F.R(), F.Q()   new HipMatrix: n x n upper triangular, m x n
    lmul!(F.Q, Y), lmul!(F.Q', Y)        F.lmul_Q_(Y), F.lmul_Qt_(Y)     Y a HipVector of m or a HipMatrix of m rows
    F \\ b, ldiv!(x, F, b)                F.solve(b), F.ldiv_(x, b)       vectors, or HipMatrix blocks with ``cols``
    A \\ b                                ldiv(A, b)     square: lu; tall: qr; wide: refused

``qr`` never raises for a rank-deficient matrix; ``solve`` raises ``SingularException(k)`` where ``R[k,k] == 0``.  A square ``DenseQR`` is
accepted wherever a preconditioner is; the fused ``cg`` / ``gmres`` iterables reach it through ``mik_dense_qr_ldiv_fn`` inside the library
(``_Bound.precond`` in api.py), with no Python frame per application.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check
from .api import HipMatrix, HipVector
from . import dense_factor
from .dense_factor import DenseFactor
from .dense_lu import lu
from .stationary import SingularException

_vp = C.c_void_p


def _lib_():
    return dense_factor.lib()            # one place to put a double of the library (the tests of dense_factor.py's subclasses do)


class DenseQR(DenseFactor):
    """The factorisation of an m x n ``HipMatrix`` of float64 / float32, m >= n, made in place in ``factors``: ``R`` on and above the
    diagonal, the reflectors' ``v`` below it, ``tau`` (numpy, n entries) beside it."""

    _entry, _name, _failure = "mik_dense_qr", "qr", SingularException
    _no_complex = "complex QR needs complex reflectors: a complex tau and conjugated products"
    _info_keys = ("W", "accumulators", "resident_rows", "resident", "launches_factor", "launches_solve", "bytes", "zero_diag")

    @classmethod
    def _admit(cls, A):
        """the refusals: not a HipMatrix, a complex element type, more columns than rows"""
        if not isinstance(A, HipMatrix):
            raise TypeError(f"{cls._name} takes a HipMatrix, got {type(A).__name__}")
        if np.dtype(A.dtype).kind == "c":
            raise TypeError(f"{cls._name} is not offered for a {np.dtype(A.dtype)} matrix ({cls._no_complex})")
        if A.n < A.cols:
            raise ValueError(f"DimensionMismatch: the matrix is {A.n} x {A.cols}: qr of a wide matrix (m < n) is not offered")

    def __init__(self, factors: HipMatrix, resident_rows: int = 0):
        self._admit(factors)
        self.factors = factors
        self.ctx = factors.ctx
        self.dtype = np.dtype(factors.dtype)
        self.m, self.n = factors.n, factors.cols
        h, col = _vp(), C.c_int64()
        plan = C.c_int64(int(resident_rows))
        code = _lib_().mik_dense_qr_create(self.ctx.handle, _vp(factors.buf.ptr), self.m, self.n, factors.ld, _lib.dtype_code(self.dtype),
                                           C.byref(plan) if resident_rows else None, C.byref(col), C.byref(h))
        check(code, "mik_dense_qr_create", self.ctx.handle)
        self.handle = h
        self.zero_diag = int(col.value)
        tau = np.zeros(self.n, self.dtype)
        check(_lib_().mik_dense_qr_tau(h, tau.ctypes.data_as(_vp)), "mik_dense_qr_tau", self.ctx.handle)
        self.tau = tau

    @classmethod
    def _of_copy(cls, A: HipMatrix, *args):
        cls._admit(A)
        copy = HipMatrix(A.n, A.cols, A.dtype, A.ctx)
        copy.buf.copyto_(A.buf)
        return cls(copy, *args)

    # ---- the argument checks: a vector or a block of `rows` rows --------------------------------------------------------------------------
    def _arg(self, v, rows: int, name: str):
        kind = HipMatrix if isinstance(v, HipMatrix) else HipVector
        if not isinstance(v, (HipVector, HipMatrix)) or v.n != rows or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {getattr(v, 'n', '?')} rows/{getattr(v, 'dtype', type(v).__name__)}, the factorisation needs {rows}/{self.dtype}")
        return _vp(v.buf.ptr if kind is HipMatrix else v.ptr)

    def _usable(self):
        if self.zero_diag:
            raise SingularException(self.zero_diag)

    # ---- lmul!(Q, Y), lmul!(Q', Y) ---------------------------------------------------------------------------------------------------------
    def _lmul(self, adjoint: int, Y, cols: Optional[int]):
        p = self._arg(Y, self.m, "Y")
        if isinstance(Y, HipMatrix):
            cols = Y.cols if cols is None else int(cols)
            if not 1 <= cols <= Y.cols:
                raise ValueError(f"DimensionMismatch: {cols} columns of Y with {Y.cols}")
            ld = Y.ld
        else:
            if cols is not None:
                raise ValueError("DimensionMismatch: cols is for a block, Y is a vector")
            cols, ld = 1, self.m
        check(_lib_().mik_dense_qr_lmul(self.handle, adjoint, p, ld, cols), "mik_dense_qr_lmul", self.ctx.handle)
        return Y

    def lmul_Q_(self, Y, cols: Optional[int] = None):
        """``lmul!(F.Q, Y)`` in place: a ``HipVector`` of m, or the leading ``cols`` columns (default: all) of a ``HipMatrix`` of m rows."""
        return self._lmul(0, Y, cols)

    def lmul_Qt_(self, Y, cols: Optional[int] = None):
        """``lmul!(F.Q', Y)`` in place."""
        return self._lmul(1, Y, cols)

    # ---- F \ b ------------------------------------------------------------------------------------------------------------------------------
    def ldiv_(self, x, b=None, cols: Optional[int] = None):
        """``ldiv!(x, F, b)``: ``x`` of n (rows), ``b`` of m (rows), not modified; with one argument ``ldiv!(F, b)``: the first n entries
        (rows) of ``b`` become the solution.  Two ``HipVector`` or two ``HipMatrix``: a block solves its leading ``cols`` columns (default:
        all of ``b``) in one call, each with the bits of the vector solve of that column.  ``SingularException(k)`` where ``R[k,k] == 0``."""
        b = x if b is None else b
        if isinstance(x, HipMatrix) or isinstance(b, HipMatrix):
            if not (isinstance(x, HipMatrix) and isinstance(b, HipMatrix)):
                raise ValueError(f"DimensionMismatch: ldiv! of a {type(x).__name__} and a {type(b).__name__}: two vectors or two matrices")
            xp, bp = self._arg(x, self.m if x is b else self.n, "X"), self._arg(b, self.m, "B")
            cols = b.cols if cols is None else int(cols)
            if not 1 <= cols <= min(x.cols, b.cols):
                raise ValueError(f"DimensionMismatch: {cols} columns of B with {b.cols} and X with {x.cols}")
            self._usable()
            check(_lib_().mik_dense_qr_solve_block(self.handle, xp, x.ld, bp, b.ld, cols), "mik_dense_qr_solve_block", self.ctx.handle)
            return x
        if cols is not None:
            raise ValueError("DimensionMismatch: cols is for a block of right-hand sides, x and b are vectors")
        xp, bp = self._arg(x, self.m if x is b else self.n, "x"), self._arg(b, self.m, "b")
        if not isinstance(x, HipVector) or not isinstance(b, HipVector):
            raise ValueError("DimensionMismatch: ldiv! takes two vectors or two matrices")
        self._usable()
        check(_lib_().mik_dense_qr_solve(self.handle, xp, bp), "mik_dense_qr_solve", self.ctx.handle)
        return x

    def solve(self, b):
        """``F \\ b``: a new vector of n, or for a ``HipMatrix`` of m rows a new n-row matrix of as many columns: the least-squares
        solution(s) of ``A x = b``."""
        self._arg(b, self.m, "b")
        if isinstance(b, HipMatrix):
            return self.ldiv_(HipMatrix(self.n, b.cols, b.dtype, b.ctx), b)
        return self.ldiv_(HipVector(self.n, self.dtype, self.ctx), b)

    def block_plan(self, nrhs: int) -> dict:
        raise NotImplementedError("qr has no block_plan query: a block solve is one stage launch, one launch of Q' and the LU's backward passes per 32 columns")

    # ---- F.R, Matrix(F.Q) -------------------------------------------------------------------------------------------------------------------
    def R(self) -> HipMatrix:
        """``F.R``: a new n x n upper-triangular ``HipMatrix``."""
        out = HipMatrix(self.n, self.n, self.dtype, self.ctx)
        check(_lib_().mik_dense_qr_r(self.handle, _vp(out.buf.ptr), out.ld), "mik_dense_qr_r", self.ctx.handle)
        return out

    def Q(self) -> HipMatrix:
        """``Matrix(F.Q)``: a new m x n ``HipMatrix`` with orthonormal columns."""
        out = HipMatrix(self.m, self.n, self.dtype, self.ctx)
        check(_lib_().mik_dense_qr_thin_q(self.handle, _vp(out.buf.ptr), out.ld), "mik_dense_qr_thin_q", self.ctx.handle)
        return out

    def info(self) -> dict:
        """Panel width ``W``, the ``accumulators`` of a reduction, the row limit of the LDS-resident form in use (``resident_rows``) and
        whether this handle is within it (``resident``), launches of the factorisation and of one solve, device bytes held, ``zero_diag``
        (``mik_dense_qr_info``)."""
        return self._read_info()

    def _read_info(self) -> dict:
        v = [C.c_int64() for _ in self._info_keys]
        check(_lib_().mik_dense_qr_info(self.handle, *[C.byref(q) for q in v]), "mik_dense_qr_info", self.ctx.handle)
        return {k: q.value for k, q in zip(self._info_keys, v)}

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                _lib_().mik_dense_qr_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def qr_(A: HipMatrix, resident_rows: int = 0) -> DenseQR:
    """``qr!(A)``: ``A`` is overwritten by its factors and kept alive by the result (``F.factors is A``).  ``resident_rows``: the row limit
    below which a workgroup keeps its column in LDS (0: as many as fit); the bits do not depend on it."""
    return DenseQR(A, resident_rows)


def qr(A: HipMatrix, resident_rows: int = 0) -> DenseQR:
    """``qr(A)``: factors a copy; ``A`` is left as it is."""
    return DenseQR._of_copy(A, resident_rows)


def ldiv(A: HipMatrix, b):
    """Julia's ``A \\ b`` on a ``HipMatrix``: ``lu(A).solve(b)`` for a square matrix, ``qr(A).solve(b)`` (least squares) for a tall one.
    A wide matrix is refused: the minimum-norm solution is not offered."""
    if not isinstance(A, HipMatrix):
        raise TypeError(f"ldiv takes a HipMatrix, got {type(A).__name__}")
    if A.n < A.cols:
        raise ValueError(f"DimensionMismatch: ldiv of a wide matrix ({A.n} x {A.cols}, m < n): the minimum-norm solution is not offered")
    return lu(A).solve(b) if A.n == A.cols else qr(A).solve(b)
