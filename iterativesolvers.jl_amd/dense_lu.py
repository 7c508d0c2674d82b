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
    ldiv!(Y, F, X) / ldiv!(F, X), F \\ B   F.ldiv_(Y, X) / F.ldiv_(Y), F.solve(B)   HipMatrix blocks: one call, each column's bits those of its vector solve
    F.ipiv                               F.ipiv         1-based, numpy int64
    F.factors                            F.factors      the HipMatrix holding L\\U

A ``DenseLU`` is accepted wherever a preconditioner is.  The fused ``cg`` / ``gmres`` iterables reach it through
``mik_dense_lu_ldiv_fn`` inside the library (``_Bound.precond`` in api.py), with no Python frame per application; every other solver
calls ``ldiv_`` like on any user preconditioner.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, lib
from .api import HipMatrix
from .dense_factor import DenseFactor
from .stationary import SingularException


class DenseLU(DenseFactor):
    """The factorisation of a square ``HipMatrix`` of float64 / float32, made in place in ``factors``."""

    _entry, _name, _failure = "mik_dense_lu", "lu", SingularException
    _no_complex = "complex LU needs |re| + |im| pivots and a complex division on the device"
    _info_keys = ("W", "R", "tile_rows", "tile_cols", "one_launch_rows", "launches_factor", "launches_solve", "bytes")

    def __init__(self, factors: HipMatrix):
        self._create(factors)
        ipiv = np.zeros(self.n, np.int64)
        check(lib().mik_dense_lu_ipiv(self.handle, ipiv.ctypes.data_as(C.POINTER(C.c_int64))), "mik_dense_lu_ipiv", self.ctx.handle)
        self.ipiv = ipiv

    def info(self) -> dict:
        """Panel width W, rows per workgroup of the pivot search R, tile of the trailing update, the row limit of the one-launch panel
        (0: not built), launches of the factorisation and of one solve, device bytes held (``mik_dense_lu_info``)."""
        return self._read_info()


def lu_(A: HipMatrix) -> DenseLU:
    """``lu!(A)``: ``A`` is overwritten by its factors and kept alive by the result (``F.factors is A``)."""
    return DenseLU(A)


def lu(A: HipMatrix) -> DenseLU:
    """``lu(A)``: factors a copy; ``A`` is left as it is."""
    return DenseLU._of_copy(A)
