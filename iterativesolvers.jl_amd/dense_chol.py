"""``cholesky(A)`` / ``cholesky!(A)`` of a square dense device matrix, real or complex, and ``ldiv!(y, F, x)`` -- what the reference's
tests pass as ``Pl`` to ``cg`` (test/cg.jl:44-47) and to ``chebyshev`` (test/chebyshev.jl:59-66) in Float32, Float64, ComplexF32 and
ComplexF64 -- over the ``mik_dense_chol_*`` entries of include/mik.h.

The factorisation and both substitutions run on the device, in the LOWER form: ``A = L L^H``.  The factor and the solution are bit for
bit those of the unblocked loops stated in include/mik.h and csrc/mik_dense_chol.h (tests/dense_ref/dense_chol_ref.c restates them).
Only the lower triangle of ``A`` and the real parts of its diagonal are read, which is LAPACK's rule; the strict upper triangle is
never read and never written.  Whether the input is Hermitian is NOT checked (Julia's ``PosDefException(-1)`` is out of scope): the
caller vouches for it, as with ``cholesky(Hermitian(A, :L))``.

    reference (LinearAlgebra)              here
    -----------------------------------    -----------------------------------------
    cholesky(Hermitian(A, :L))             cholesky(A)        factors a copy
    cholesky!(Hermitian(A, :L))            cholesky_(A)       factors in place, keeps A alive
    ldiv!(y, F, x) / ldiv!(F, x)           F.ldiv_(y, x) / F.ldiv_(y)
    F \\ b                                  F.solve(b)
    F.uplo, F.info, issuccess(F)           F.uplo == "L", F.info, F.issuccess()
    cholesky(A; check=false)               cholesky(A, check=False)
    PosDefException(k)                     PosDefException(k)

A ``DenseCholesky`` is accepted wherever a preconditioner is.  The fused real ``cg`` / ``gmres`` iterables reach it through
``mik_dense_chol_ldiv_fn`` inside the library (``_Bound.precond`` in api.py), with no Python frame per application; the complex
generic iterables and every other solver call ``ldiv_`` like on any user preconditioner.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MikError, check, lib
from .api import HipMatrix, HipVector
from .stationary import PosDefException

_vp = C.c_void_p


def _admit(A):
    """the refusals of cholesky / cholesky!: not a HipMatrix, not square"""
    if not isinstance(A, HipMatrix):
        raise TypeError(f"cholesky takes a HipMatrix, got {type(A).__name__}")
    if A.n != A.cols:
        raise ValueError(f"DimensionMismatch: the matrix is {A.n} x {A.cols}, not square")


class DenseCholesky:
    """The factorisation of a square ``HipMatrix`` of float64 / float32 / complex128 / complex64, made in place in the lower triangle
    of ``factors``."""

    uplo = "L"

    def __init__(self, factors: HipMatrix, check: bool = True):
        _admit(factors)
        self.factors = factors
        self.ctx = factors.ctx
        self.dtype = np.dtype(factors.dtype)
        self.n = factors.n
        h = _vp()
        col = C.c_int64()
        code = lib().mik_dense_chol_create(self.ctx.handle, _vp(factors.buf.ptr), self.n, factors.ld, _lib.dtype_code(self.dtype), 1 if check else 0,
                                           C.byref(col), C.byref(h))
        if code == 8:
            raise PosDefException(col.value)
        _lib.check(code, "mik_dense_chol_create", self.ctx.handle)
        self.handle = h
        self.info = int(col.value)

    def issuccess(self) -> bool:
        return self.info == 0

    def _vec(self, v: HipVector, name: str):
        if not isinstance(v, HipVector) or v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {getattr(v, 'n', '?')}/{getattr(v, 'dtype', type(v).__name__)}, the factorisation {self.n}/{self.dtype}")
        return _vp(v.ptr)

    def ldiv_(self, y: HipVector, x: HipVector = None) -> HipVector:
        """``ldiv!(y, F, x)``; with one argument ``ldiv!(F, y)``.  ``x`` is not modified; ``y`` may be ``x``.  Refused on a failed
        factorisation (``info != 0``)."""
        x = y if x is None else x
        yp, xp = self._vec(y, "y"), self._vec(x, "x")
        if self.info:
            raise MikError(1, "mik_dense_chol_solve", f"the factorisation failed: PosDefException({self.info})")
        check(lib().mik_dense_chol_solve(self.handle, yp, xp), "mik_dense_chol_solve", self.ctx.handle)
        return y

    def solve(self, b: HipVector) -> HipVector:
        """``F \\ b``: a new vector."""
        self._vec(b, "b")
        return self.ldiv_(b.similar(), b)

    def plan(self) -> dict:
        """Panel width W, rows per workgroup of the panel kernel R, tile of the trailing update, launches of the factorisation and of one
        solve, device bytes held, and ``info`` -- for this handle's element type (``mik_dense_chol_info``).  ``F.info`` itself is the
        reference's field, an integer."""
        v = [C.c_int64() for _ in range(8)]
        check(lib().mik_dense_chol_info(self.handle, *[C.byref(q) for q in v]), "mik_dense_chol_info", self.ctx.handle)
        keys = ("W", "R", "tile_rows", "tile_cols", "launches_factor", "launches_solve", "bytes", "info")
        return {k: q.value for k, q in zip(keys, v)}

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                lib().mik_dense_chol_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def cholesky_(A: HipMatrix, check: bool = True) -> DenseCholesky:
    """``cholesky!(Hermitian(A, :L))``: the lower triangle of ``A`` is overwritten by ``L``; ``A`` is kept alive by the result
    (``F.factors is A``).  ``check=False`` never raises for a matrix that is not positive definite: ``F.info`` is the failing column."""
    return DenseCholesky(A, check)


def cholesky(A: HipMatrix, check: bool = True) -> DenseCholesky:
    """``cholesky(Hermitian(A, :L))``: factors a copy; ``A`` is left as it is."""
    _admit(A)
    copy = HipMatrix(A.n, A.cols, A.dtype, A.ctx)
    copy.buf.copyto_(A.buf)
    return DenseCholesky(copy, check)
