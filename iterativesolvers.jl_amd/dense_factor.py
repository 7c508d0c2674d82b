"""What the factorisations of a square dense device matrix share (``dense_lu.py``, ``dense_chol.py``): the refusals, the handle over the
``<entry>_create`` / ``_solve`` / ``_solve_block`` / ``_info`` / ``_destroy`` entries of include/mik.h, ``ldiv_`` and ``solve`` on a vector
or on a block of right-hand sides (a ``HipMatrix``), and "factor a copy".

A subclass names its entries (``_entry``), itself in messages (``_name``), the exception of a failed factorisation (``_failure``), the
keys of its ``_info`` entry, and -- where complex matrices are refused -- why (``_no_complex``).  A ``DenseFactor`` is accepted wherever a
preconditioner is; the fused ``cg`` / ``gmres`` iterables reach it through ``<entry>_ldiv_fn`` inside the library (``_Bound.precond`` in
api.py), with no Python frame per application.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import HipMatrix, HipVector

_vp = C.c_void_p


class DenseFactor:
    _entry = _name = ""
    _failure = None
    _info_keys = ()
    _no_complex = None
    block_min_cols = 2               # fewer columns are cheaper as vector solves (a block of one costs 1.0 to 1.4 vector solves: DESIGN.md section 26)

    @classmethod
    def _admit(cls, A):
        """the refusals: not a HipMatrix, an element type that is not offered, not square"""
        if not isinstance(A, HipMatrix):
            raise TypeError(f"{cls._name} takes a HipMatrix, got {type(A).__name__}")
        if cls._no_complex and np.dtype(A.dtype).kind == "c":
            raise TypeError(f"{cls._name} is not offered for a {np.dtype(A.dtype)} matrix ({cls._no_complex})")
        if A.n != A.cols:
            raise ValueError(f"DimensionMismatch: the matrix is {A.n} x {A.cols}, not square")

    def _create(self, factors: HipMatrix, *args) -> int:
        """factors ``factors`` in place; ``args`` go between the dtype and the failing column, which is returned"""
        self._admit(factors)
        self.factors = factors
        self.ctx = factors.ctx
        self.dtype = np.dtype(factors.dtype)
        self.n = factors.n
        h = _vp()
        col = C.c_int64()
        who = f"{self._entry}_create"
        code = getattr(lib(), who)(self.ctx.handle, _vp(factors.buf.ptr), self.n, factors.ld, _lib.dtype_code(self.dtype), *args, C.byref(col), C.byref(h))
        if code == 8:
            raise self._failure(col.value)
        check(code, who, self.ctx.handle)
        self.handle = h
        return int(col.value)

    @classmethod
    def _of_copy(cls, A: HipMatrix, *args):
        cls._admit(A)
        copy = HipMatrix(A.n, A.cols, A.dtype, A.ctx)
        copy.buf.copyto_(A.buf)
        return cls(copy, *args)

    def _vec(self, v: HipVector, name: str):
        if not isinstance(v, HipVector) or v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {getattr(v, 'n', '?')}/{getattr(v, 'dtype', type(v).__name__)}, the factorisation {self.n}/{self.dtype}")
        return _vp(v.ptr)

    def _usable(self):
        """raises where the factorisation cannot solve"""

    def _block(self, M: HipMatrix, name: str):
        if not isinstance(M, HipMatrix) or M.n != self.n or M.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {getattr(M, 'n', '?')} rows/{getattr(M, 'dtype', type(M).__name__)}, the factorisation {self.n}/{self.dtype}")
        return _vp(M.buf.ptr)

    def ldiv_(self, y, x=None, cols: int = None):
        """``ldiv!(y, F, x)``; with one argument ``ldiv!(F, y)``.  ``x`` is not modified; ``y`` may be ``x``.  Two ``HipVector`` or two
        ``HipMatrix`` of ``n`` rows: a block solves its leading ``cols`` columns (default: all of ``x``; ``y`` needs as many) in one call
        (``<entry>_solve_block``), each with the bits of the vector solve of that column; the other columns of ``y`` are not written."""
        x = y if x is None else x
        if isinstance(y, HipMatrix) or isinstance(x, HipMatrix):
            if not (isinstance(y, HipMatrix) and isinstance(x, HipMatrix)):
                raise ValueError(f"DimensionMismatch: ldiv! of a {type(y).__name__} and a {type(x).__name__}: two vectors or two matrices")
            yp, xp = self._block(y, "Y"), self._block(x, "X")
            cols = x.cols if cols is None else int(cols)
            if not 1 <= cols <= min(x.cols, y.cols):
                raise ValueError(f"DimensionMismatch: {cols} columns of X with {x.cols} and Y with {y.cols}")
            self._usable()
            who = f"{self._entry}_solve_block"
            check(getattr(lib(), who)(self.handle, yp, y.ld, xp, x.ld, cols), who, self.ctx.handle)
            return y
        if cols is not None:
            raise ValueError("DimensionMismatch: cols is for a block of right-hand sides, y and x are vectors")
        yp, xp = self._vec(y, "y"), self._vec(x, "x")
        self._usable()
        who = f"{self._entry}_solve"
        check(getattr(lib(), who)(self.handle, yp, xp), who, self.ctx.handle)
        return y

    def solve(self, b):
        """``F \\ b``: a new vector, or for a ``HipMatrix`` a new matrix of as many columns."""
        if isinstance(b, HipMatrix):
            self._block(b, "B")
            return self.ldiv_(HipMatrix(b.n, b.cols, b.dtype, b.ctx), b)
        self._vec(b, "b")
        return self.ldiv_(b.similar(), b)

    def block_plan(self, nrhs: int) -> dict:
        """How ``ldiv_`` runs a block of ``nrhs`` columns on this handle (``mik_dev_dense_<lu|chol>_block_plan``): ``NB`` columns per lane,
        ``G`` columns per pass, ``passes``, ``launches`` (passes x the launches of one vector solve), ``workspace_bytes``."""
        keys = ("NB", "G", "passes", "launches", "workspace_bytes")
        v = [C.c_int64() for _ in keys]
        who = self._entry.replace("mik_", "mik_dev_") + "_block_plan"
        check(getattr(lib(), who)(self.handle, int(nrhs), *[C.byref(q) for q in v]), who, self.ctx.handle)
        return {k: q.value for k, q in zip(keys, v)}

    def _read_info(self) -> dict:
        v = [C.c_int64() for _ in self._info_keys]
        who = f"{self._entry}_info"
        check(getattr(lib(), who)(self.handle, *[C.byref(q) for q in v]), who, self.ctx.handle)
        return {k: q.value for k, q in zip(self._info_keys, v)}

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                getattr(lib(), f"{self._entry}_destroy")(self.handle)
                self.handle = None
        except Exception:
            pass
