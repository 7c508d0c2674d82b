"""Jacobi, Gauss-Seidel, SOR and SSOR on a dense device matrix -- the dense stationary methods of IterativeSolvers.jl
(src/stationary.jl), over the ``mik_dense_*`` entries of include/mik.h -- and the public names of both stationary families,
which dispatch on the operator: a ``HipCSR`` runs stationary.py (src/stationary_sparse.jl), a ``HipMatrix`` the code here.

One C call is one whole iteration; every row is summed by one lane in the order the reference's column loops give it, so the
iterates (and ``next`` / ``tmp``) are bit-identical to the reference's.

    reference                                     here
    ------------------------------------------    ------------------------------------------------
    check_diag                          :6-12     DenseStationaryOperator  (mik_dense_stationary_create)
    DenseJacobiIterable / iterate       :38-72    DenseJacobiIterable      (mik_dense_jacobi_step)
    DenseGaussSeidelIterable / iterate  :98-129   DenseGaussSeidelIterable (mik_dense_gs_step)
    DenseSORIterable / iterate          :156-188  DenseSORIterable         (mik_dense_sor_step)
    DenseSSORIterable / iterate         :216-263  DenseSSORIterable        (mik_dense_ssor_step)
    jacobi! gauss_seidel! sor! ssor!    :31 :91 :149 :209    jacobi_ gauss_seidel_ sor_ ssor_
    jacobi gauss_seidel sor ssor        :19 :79 :136 :195    jacobi gauss_seidel sor ssor

The relaxation parameter keeps Julia's types, as in stationary.py: with Float32 data and a Float64 omega,
``x + omega * (tmp / d - x)`` has its inner difference in Float32, the product and the sum in Float64, one rounding at the store.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, stationary as _sparse
from ._lib import check, lib
from .api import HipCSR, HipMatrix, HipVector
from .stationary import SingularException, _host, _relax_scalars, _StationaryIterable

_vp = C.c_void_p
FORMS = {"auto": _lib.MIK_DENSE_AUTO, "panel": _lib.MIK_DENSE_PANEL, "chained": _lib.MIK_DENSE_CHAINED}
_FORM_NAMES = {v: k for k, v in FORMS.items()}


class DenseStationaryOperator:
    """``check_diag(A)`` (src/stationary.jl:6-12) and the work vectors of the four dense iterations on one square ``HipMatrix``.
    Raises ``SingularException(i)`` for the first zero diagonal entry (``-0.0`` included).  ``A`` is read at every step and
    must outlive the operator.  ``form``: how the strict-lower phase runs ("auto" / "panel"; "chained" is refused by the
    library, which does not build it); ``spin_limit`` travels with it in the plan (0 = default)."""

    def __init__(self, A: HipMatrix, *, form: str = "auto", spin_limit: int = 0):
        if A.n != A.cols:
            raise ValueError(f"DimensionMismatch: the matrix is {A.n} x {A.cols}, not square")
        self.A = A
        self.ctx = A.ctx
        self.dtype = np.dtype(A.dtype)
        self.n = A.n
        plan = _lib.MikDensePlan(FORMS[form], int(spin_limit))
        h = _vp()
        col = C.c_int64()
        code = lib().mik_dense_stationary_create(self.ctx.handle, _vp(A.buf.ptr), self.n, A.ld, _lib.dtype_code(self.dtype), C.byref(plan),
                                                 C.byref(col), C.byref(h))
        if code == 8:
            raise SingularException(col.value)
        check(code, "mik_dense_stationary_create", self.ctx.handle)
        self.handle = h

    def _check(self, code, where):
        check(code, where, self.ctx.handle)

    def _vec(self, v: HipVector, name: str):
        if v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {v.n}/{v.dtype}, the operator {self.n}/{self.dtype}")
        return _vp(v.ptr)

    def info(self) -> dict:
        """Panel width W, rows per workgroup R, launches of one forward substitution, the form in use, whether a chained launch
        has given up, device bytes held (``mik_dense_stationary_info``)."""
        w, r, la, b = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        form, gave_up = C.c_int(), C.c_int()
        self._check(lib().mik_dense_stationary_info(self.handle, C.byref(w), C.byref(r), C.byref(la), C.byref(form), C.byref(gave_up), C.byref(b)),
                    "mik_dense_stationary_info")
        return {"W": w.value, "R": r.value, "launches_forward": la.value, "form": _FORM_NAMES[form.value], "gave_up": bool(gave_up.value),
                "bytes": b.value}

    def jacobi_step_(self, x: HipVector, next: HipVector, b: HipVector) -> None:                  # iterate  :48-72
        self._check(lib().mik_dense_jacobi_step(self.handle, self._vec(x, "x"), self._vec(next, "next"), self._vec(b, "b")), "mik_dense_jacobi_step")

    def gs_step_(self, x: HipVector, b: HipVector) -> None:                                       # iterate  :108-129
        self._check(lib().mik_dense_gs_step(self.handle, self._vec(x, "x"), self._vec(b, "b")), "mik_dense_gs_step")

    def _relaxed(self, fn, where, x, tmp, b, omega):
        w, _, S = _relax_scalars(self.dtype, omega)
        _w, pw = _host(S, w)
        self._check(fn(self.handle, self._vec(x, "x"), self._vec(tmp, "tmp"), self._vec(b, "b"), pw, _lib.dtype_code(S)), where)

    def sor_step_(self, x: HipVector, tmp: HipVector, b: HipVector, omega) -> None:               # iterate  :167-188
        self._relaxed(lib().mik_dense_sor_step, "mik_dense_sor_step", x, tmp, b, omega)

    def ssor_step_(self, x: HipVector, tmp: HipVector, b: HipVector, omega) -> None:              # iterate  :227-263
        self._relaxed(lib().mik_dense_ssor_step, "mik_dense_ssor_step", x, tmp, b, omega)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                lib().mik_dense_stationary_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class DenseJacobiIterable(_StationaryIterable):                                     # :38-44
    def __init__(self, A, x, next, b, maxiter: int):
        self.A, self.x, self.next, self.b, self.maxiter = A, x, next, b, int(maxiter)

    def _step(self):                                                                # :48-72
        self.A.jacobi_step_(self.x, self.next, self.b)


class DenseGaussSeidelIterable(_StationaryIterable):                                # :98-103
    def __init__(self, A, x, b, maxiter: int):
        self.A, self.x, self.b, self.maxiter = A, x, b, int(maxiter)

    def _step(self):                                                                # :108-129
        self.A.gs_step_(self.x, self.b)


class DenseSORIterable(_StationaryIterable):                                        # :156-163
    def __init__(self, A, x, tmp, b, omega, maxiter: int):
        self.A, self.x, self.tmp, self.b, self.omega, self.maxiter = A, x, tmp, b, omega, int(maxiter)

    def _step(self):                                                                # :167-188 (in place: no swap, unlike the sparse SOR)
        self.A.sor_step_(self.x, self.tmp, self.b, self.omega)


class DenseSSORIterable(_StationaryIterable):                                       # :216-223
    def __init__(self, A, x, tmp, b, omega, maxiter: int):
        self.A, self.x, self.tmp, self.b, self.omega, self.maxiter = A, x, tmp, b, omega, int(maxiter)

    def _step(self):                                                                # :227-263
        self.A.ssor_step_(self.x, self.tmp, self.b, self.omega)


# ---- the public names of both families ------------------------------------------------------------------------------------------
def _dense(A):
    """The dense operator behind ``A``: a square ``HipMatrix`` (check_diag runs here), or an operator that is one already."""
    if isinstance(A, HipMatrix):
        return DenseStationaryOperator(A)
    if hasattr(A, "jacobi_step_") and hasattr(A, "ssor_step_"):
        return A
    raise TypeError(f"the stationary methods take a HipCSR or a HipMatrix, got {type(A).__name__}")


def _zerox(b):                                                                      # zerox(A, b), src/common.jl:18-23; A is square
    return b.similar().fill_(0)


def jacobi_iterable(x, A, b, *, maxiter: int = 10):
    if isinstance(A, HipCSR):
        return _sparse.jacobi_iterable(x, A, b, maxiter=maxiter)
    return DenseJacobiIterable(_dense(A), x, x.similar(), b, maxiter)               # :33


def gauss_seidel_iterable(x, A, b, *, maxiter: int = 10):
    if isinstance(A, HipCSR):
        return _sparse.gauss_seidel_iterable(x, A, b, maxiter=maxiter)
    return DenseGaussSeidelIterable(_dense(A), x, b, maxiter)                       # :93


def sor_iterable(x, A, b, omega, *, maxiter: int = 10):
    if isinstance(A, HipCSR):
        return _sparse.sor_iterable(x, A, b, omega, maxiter=maxiter)
    return DenseSORIterable(_dense(A), x, x.similar(), b, omega, maxiter)           # :151


def ssor_iterable(x, A, b, omega, *, maxiter: int = 10):
    if isinstance(A, HipCSR):
        return _sparse.ssor_iterable(x, A, b, omega, maxiter=maxiter)
    return DenseSSORIterable(_dense(A), x, x.similar(), b, omega, maxiter)          # :211


def _run(iterable):
    for _ in iterable:
        pass
    return iterable.x


def jacobi_(x, A, b, *, maxiter: int = 10):                                         # jacobi!  :31-36 / stationary_sparse.jl:251-255
    return _run(jacobi_iterable(x, A, b, maxiter=maxiter))


def gauss_seidel_(x, A, b, *, maxiter: int = 10):                                   # gauss_seidel!  :91-96 / :298-302
    return _run(gauss_seidel_iterable(x, A, b, maxiter=maxiter))


def sor_(x, A, b, omega, *, maxiter: int = 10):                                     # sor!  :149-154 / :356-360
    """Dense: ``x`` itself.  Sparse: ``iterable.x``, the internal buffer after an odd number of iterations (stationary.py)."""
    return _run(sor_iterable(x, A, b, omega, maxiter=maxiter))


def ssor_(x, A, b, omega, *, maxiter: int = 10):                                    # ssor!  :209-214 / :422-426
    return _run(ssor_iterable(x, A, b, omega, maxiter=maxiter))


def jacobi(A, b, **kwargs):                                                         # :19
    return _sparse.jacobi(A, b, **kwargs) if isinstance(A, HipCSR) else jacobi_(_zerox(b), A, b, **kwargs)


def gauss_seidel(A, b, **kwargs):                                                   # :79
    return _sparse.gauss_seidel(A, b, **kwargs) if isinstance(A, HipCSR) else gauss_seidel_(_zerox(b), A, b, **kwargs)


def sor(A, b, omega, **kwargs):                                                     # :136
    return _sparse.sor(A, b, omega, **kwargs) if isinstance(A, HipCSR) else sor_(_zerox(b), A, b, omega, **kwargs)


def ssor(A, b, omega, **kwargs):                                                    # :195
    return _sparse.ssor(A, b, omega, **kwargs) if isinstance(A, HipCSR) else ssor_(_zerox(b), A, b, omega, **kwargs)
