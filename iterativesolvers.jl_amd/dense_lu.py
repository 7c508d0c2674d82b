"""``lu(A)`` / ``lu!(A)`` of a square dense device matrix and ``ldiv!(y, F, x)`` -- what the reference's tests pass as ``Pl`` / ``Pr``
(test/gmres.jl:28-35, test/bicgstabl.jl:40-42, test/idrs.jl:55) and as the operator of ``invpowm``
(test/simple_eigensolvers.jl:40) -- over the ``mik_dense_lu_*`` entries of include/mik.h.

The factorisation (partial pivoting) and both substitutions run on the device.  The factors, the pivots and the solution are bit for
bit those of the unblocked loops of ``mik_lu_solve`` (the contract is stated in include/mik.h and csrc/mik_dense_lu.h).

    reference (LinearAlgebra)            here
    ---------------------------------    -----------------------------------------
    lu(A)                                lu(A)          factors a copy
    lu!(A)                               lu_(A)         factors in place, keeps A alive
    ldiv!(y, F, x) / ldiv!(F, x)         F.ldiv_(y, x) / F.ldiv_(y)
    F \\ b                                F.solve(b)
    F.ipiv                               F.ipiv         1-based, numpy int64
    F.factors                            F.factors      the HipMatrix holding L\\U

A ``DenseLU`` is accepted wherever a preconditioner is.  The fused ``cg`` / ``gmres`` iterables reach it through
``mik_dense_lu_ldiv_fn`` inside the library (``_Bound.precond`` in api.py), with no Python frame per application; every other solver
calls ``ldiv_`` like on any user preconditioner.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import HipMatrix, HipVector
from .stationary import SingularException

_vp = C.c_void_p


def _admit(A):
    """the refusals of lu / lu!: not a HipMatrix, a complex element type, not square"""
    if not isinstance(A, HipMatrix):
        raise TypeError(f"lu takes a HipMatrix, got {type(A).__name__}")
    if np.dtype(A.dtype).kind == "c":
        raise TypeError(f"lu is not offered for a {np.dtype(A.dtype)} matrix (complex LU needs |re| + |im| pivots and a complex division on the device)")
    if A.n != A.cols:
        raise ValueError(f"DimensionMismatch: the matrix is {A.n} x {A.cols}, not square")


class DenseLU:
    """The factorisation of a square ``HipMatrix`` of float64 / float32, made in place in ``factors``."""

    def __init__(self, factors: HipMatrix):
        _admit(factors)
        self.factors = factors
        self.ctx = factors.ctx
        self.dtype = np.dtype(factors.dtype)
        self.n = factors.n
        h = _vp()
        col = C.c_int64()
        code = lib().mik_dense_lu_create(self.ctx.handle, _vp(factors.buf.ptr), self.n, factors.ld, _lib.dtype_code(self.dtype), C.byref(col), C.byref(h))
        if code == 8:
            raise SingularException(col.value)
        check(code, "mik_dense_lu_create", self.ctx.handle)
        self.handle = h
        ipiv = np.zeros(self.n, np.int64)
        check(lib().mik_dense_lu_ipiv(self.handle, ipiv.ctypes.data_as(C.POINTER(C.c_int64))), "mik_dense_lu_ipiv", self.ctx.handle)
        self.ipiv = ipiv

    def _vec(self, v: HipVector, name: str):
        if not isinstance(v, HipVector) or v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {getattr(v, 'n', '?')}/{getattr(v, 'dtype', type(v).__name__)}, the factorisation {self.n}/{self.dtype}")
        return _vp(v.ptr)

    def ldiv_(self, y: HipVector, x: HipVector = None) -> HipVector:
        """``ldiv!(y, F, x)``; with one argument ``ldiv!(F, y)``.  ``x`` is not modified; ``y`` may be ``x``."""
        x = y if x is None else x
        check(lib().mik_dense_lu_solve(self.handle, self._vec(y, "y"), self._vec(x, "x")), "mik_dense_lu_solve", self.ctx.handle)
        return y

    def solve(self, b: HipVector) -> HipVector:
        """``F \\ b``: a new vector."""
        self._vec(b, "b")
        return self.ldiv_(b.similar(), b)

    def info(self) -> dict:
        """Panel width W, rows per workgroup of the pivot search R, tile of the trailing update, the row limit of the one-launch panel
        (0: not built), launches of the factorisation and of one solve, device bytes held (``mik_dense_lu_info``)."""
        v = [C.c_int64() for _ in range(8)]
        check(lib().mik_dense_lu_info(self.handle, *[C.byref(q) for q in v]), "mik_dense_lu_info", self.ctx.handle)
        keys = ("W", "R", "tile_rows", "tile_cols", "one_launch_rows", "launches_factor", "launches_solve", "bytes")
        return {k: q.value for k, q in zip(keys, v)}

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                lib().mik_dense_lu_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def lu_(A: HipMatrix) -> DenseLU:
    """``lu!(A)``: ``A`` is overwritten by its factors and kept alive by the result (``F.factors is A``)."""
    return DenseLU(A)


def lu(A: HipMatrix) -> DenseLU:
    """``lu(A)``: factors a copy; ``A`` is left as it is."""
    _admit(A)
    copy = HipMatrix(A.n, A.cols, A.dtype, A.ctx)
    copy.buf.copyto_(A.buf)
    return DenseLU(copy)
