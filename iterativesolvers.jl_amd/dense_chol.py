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
    ldiv!(Y, F, X) / ldiv!(F, X), F \\ B     F.ldiv_(Y, X) / F.ldiv_(Y), F.solve(B)   HipMatrix blocks: one call, each column's bits those of its vector solve
    F.uplo, F.info, issuccess(F)           F.uplo == "L", F.info, F.issuccess()
    cholesky(A; check=false)               cholesky(A, check=False)
    PosDefException(k)                     PosDefException(k)

A ``DenseCholesky`` is accepted wherever a preconditioner is.  The fused real ``cg`` / ``gmres`` iterables reach it through
``mik_dense_chol_ldiv_fn`` inside the library (``_Bound.precond`` in api.py), with no Python frame per application; the complex
generic iterables and every other solver call ``ldiv_`` like on any user preconditioner.
"""
from __future__ import annotations

from ._lib import MikError
from .api import HipMatrix
from .dense_factor import DenseFactor
from .stationary import PosDefException


class DenseCholesky(DenseFactor):
    """The factorisation of a square ``HipMatrix`` of float64 / float32 / complex128 / complex64, made in place in the lower triangle
    of ``factors``."""

    _entry, _name, _failure = "mik_dense_chol", "cholesky", PosDefException
    _info_keys = ("W", "R", "tile_rows", "tile_cols", "launches_factor", "launches_solve", "bytes", "info")
    uplo = "L"

    def __init__(self, factors: HipMatrix, check: bool = True):
        self.info = self._create(factors, 1 if check else 0)

    def issuccess(self) -> bool:
        return self.info == 0

    def _usable(self):
        """``ldiv_`` is refused on a failed factorisation (``info != 0``)"""
        if self.info:
            raise MikError(1, "mik_dense_chol_solve", f"the factorisation failed: PosDefException({self.info})")

    def plan(self) -> dict:
        """Panel width W, rows per workgroup of the panel kernel R, tile of the trailing update, launches of the factorisation and of one
        solve, device bytes held, and ``info`` -- for this handle's element type (``mik_dense_chol_info``).  ``F.info`` itself is the
        reference's field, an integer."""
        return self._read_info()


def cholesky_(A: HipMatrix, check: bool = True) -> DenseCholesky:
    """``cholesky!(Hermitian(A, :L))``: the lower triangle of ``A`` is overwritten by ``L``; ``A`` is kept alive by the result
    (``F.factors is A``).  ``check=False`` never raises for a matrix that is not positive definite: ``F.info`` is the failing column."""
    return DenseCholesky(A, check)


def cholesky(A: HipMatrix, check: bool = True) -> DenseCholesky:
    """``cholesky(Hermitian(A, :L))``: factors a copy; ``A`` is left as it is."""
    return DenseCholesky._of_copy(A, check)
