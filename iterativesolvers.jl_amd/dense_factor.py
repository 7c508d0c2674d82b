"""What the factorisations of a square dense device matrix share (``dense_lu.py``, ``dense_chol.py``): the refusals, the handle over the
``<entry>_create`` / ``_solve`` / ``_info`` / ``_destroy`` entries of include/mik.h, ``ldiv_`` and ``solve``, and "factor a copy".

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

    def ldiv_(self, y: HipVector, x: HipVector = None) -> HipVector:
        """``ldiv!(y, F, x)``; with one argument ``ldiv!(F, y)``.  ``x`` is not modified; ``y`` may be ``x``."""
        x = y if x is None else x
        yp, xp = self._vec(y, "y"), self._vec(x, "x")
        self._usable()
        who = f"{self._entry}_solve"
        check(getattr(lib(), who)(self.handle, yp, xp), who, self.ctx.handle)
        return y

    def solve(self, b: HipVector) -> HipVector:
        """``F \\ b``: a new vector."""
        self._vec(b, "b")
        return self.ldiv_(b.similar(), b)

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
