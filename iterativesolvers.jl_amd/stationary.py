"""Jacobi, Gauss-Seidel, SOR and SSOR on a device CSR operator -- the sparse stationary methods of
IterativeSolvers.jl (src/stationary_sparse.jl), over the ``mik_stationary`` entries of include/mik.h.

Each ``iterate`` restates the reference's body line by line; every building block is one C call whose
rows are summed in the reference's order, so the iterates are bit-identical to the reference's.

    reference                                        here
    ---------------------------------------------    ---------------------------------------
    DiagonalIndices + the triangular views :6-64     StationaryOperator  (mik_stationary_create)
    ldiv!(y, D, x)                        :30-35     StationaryOperator.diag_ldiv_
    mul!(a, O::OffDiagonal, x, b, y)      :148-171   StationaryOperator.offdiag_mul_
    gauss_seidel_multiply!                :178-208   StationaryOperator.gs_multiply_
    forward_sub! / backward_sub!          :67-142    StationaryOperator.forward_sub_ / backward_sub_
    jacobi_iterable / jacobi!             :213-255   jacobi_iterable / jacobi_  (jacobi: src/stationary.jl:19)
    gauss_seidel_iterable / gauss_seidel! :261-302   gauss_seidel_iterable / gauss_seidel_
    sor_iterable / sor!                   :308-360   sor_iterable / sor_
    ssor_iterable / ssor!                 :366-426   ssor_iterable / ssor_

The relaxation parameter keeps Julia's types: a Python ``float`` (or ``np.float64``) is a Float64 omega, an
``np.float32`` a Float32 one, an ``int`` an Int (promoted to the element type, as Julia does).  With Float32
data and a Float64 omega, ``alpha * x / d + beta * y`` runs in Float64 and rounds once at the store.

A ``complex128`` / ``complex64`` operator runs the same statements on ComplexF64 / ComplexF32:
omega stays real, ``one(T) - omega`` is complex with imaginary part ``+0.0``, and ``-one(T)`` is ``(-1.0, -0.0)``.
"""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib
from .api import HipCSR, HipVector, zerox

_vp = C.c_void_p


class SingularException(np.linalg.LinAlgError):
    """``LinearAlgebra.SingularException(col)``: the diagonal entry of column ``col`` (1-based) is missing or zero."""

    def __init__(self, col: int):
        self.col = int(col)
        super().__init__(f"SingularException({self.col})")


class PosDefException(np.linalg.LinAlgError):
    """``LinearAlgebra.PosDefException(k)``: the pivot of column ``k`` (1-based) of a Cholesky factorisation is not positive."""

    def __init__(self, k: int):
        self.k = int(k)
        super().__init__(f"PosDefException({self.k}): matrix is not positive definite; the factorisation failed at column {self.k}")


def _host(dtype, value):
    a = np.asarray([value], dtype=dtype)
    return a, a.ctypes.data_as(_vp)


def _minus_one(T):
    """``-one(T)``: Julia's unary minus negates both parts, so a complex T gives ``(-1.0, -0.0)``."""
    return complex(-1.0, -0.0) if np.dtype(T).kind == "c" else -1


def _relax_scalars(T, omega):
    """(alpha, beta, scalar dtype) of forward_sub!(omega, L, x, one(T) - omega, y) with Julia's promotion.  For a complex T the
    scalar dtype E is the REAL type of promote(real(T), typeof(omega)); alpha is a real of E, beta a complex of E with
    imaginary part +0.0 (``one(T) - omega`` subtracts a real from the real part only)."""
    T = np.dtype(T)
    if T.kind == "c":
        a, _, E = _relax_scalars(T.type(0).real.dtype, omega)
        CE = np.result_type(E, np.complex64)
        return a, CE.type(complex(E.type(E.type(1) - a), 0.0)), E
    if isinstance(omega, np.floating):
        S = np.result_type(T, omega.dtype)
    elif isinstance(omega, (bool, np.bool_)) or isinstance(omega, numbers.Integral):
        S = T                                       # Int omega: one(T) - omega and omega * x[i] are of type T
    elif isinstance(omega, numbers.Real):
        S = np.result_type(T, np.float64)           # a Python float is a Float64
    else:
        raise TypeError(f"omega must be real, got {type(omega).__name__}")
    a = S.type(omega)
    b = S.type(S.type(1) - a)
    return a, b, S


class StationaryOperator:
    """``DiagonalIndices(A)`` and the triangular views built on it (src/stationary_sparse.jl:6-64), plus the level schedules
    of the two triangular sweeps.  Raises ``SingularException(col)`` for the first zero or missing diagonal entry."""

    def __init__(self, A: HipCSR):
        self.A = A                                  # the handle reads A's arrays at creation only, but A must outlive it
        self.ctx = A.ctx
        self.dtype = np.dtype(A.dtype)
        self.n = A.size(1)
        h = _vp()
        col = C.c_int64()
        code = lib().mik_stationary_create(self.ctx.handle, A.handle, C.byref(col), C.byref(h))
        if code == 8:
            raise SingularException(col.value)
        check(code, "mik_stationary_create", self.ctx.handle)
        self.handle = h

    def _check(self, code, where):
        check(code, where, self.ctx.handle)

    def _vec(self, v: HipVector, name: str):
        if v.n != self.n or v.dtype != self.dtype:
            raise ValueError(f"DimensionMismatch: {name} has {v.n}/{v.dtype}, the operator {self.n}/{self.dtype}")
        return _vp(v.ptr)

    def info(self) -> dict:
        """Levels and launches per triangular sweep (forward = strict lower, backward = strict upper), device bytes held,
        analysis time (``mik_stationary_info``)."""
        lv, la = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        b, ms = C.c_int64(), C.c_double()
        self._check(lib().mik_stationary_info(self.handle, lv, la, C.byref(b), C.byref(ms)), "mik_stationary_info")
        return {"levels_forward": lv[0], "levels_backward": lv[1], "launches_forward": la[0], "launches_backward": la[1],
                "bytes": b.value, "analysis_ms": ms.value}

    def diag_ldiv_(self, y: HipVector, x: HipVector) -> HipVector:               # ldiv!(y, D, x)  :30-35
        self._check(lib().mik_diag_ldiv(self.handle, self._vec(y, "y"), self._vec(x, "x")), "mik_diag_ldiv")
        return y

    def offdiag_mul_(self, alpha, x: HipVector, beta, y: HipVector) -> HipVector:   # mul!(alpha, O, x, beta, y)  :148-171
        _a, pa = _host(self.dtype, alpha)
        _b, pb = _host(self.dtype, beta)
        self._check(lib().mik_offdiag_mul(self.handle, pa, self._vec(x, "x"), pb, self._vec(y, "y")), "mik_offdiag_mul")
        return y

    def gs_multiply_(self, upper: bool, alpha, x: HipVector, beta, y: HipVector, z: HipVector) -> HipVector:
        """``gauss_seidel_multiply!(alpha, U | L, x, beta, y, z)`` -- :178-191 / :196-208; z may be x."""
        _a, pa = _host(self.dtype, alpha)
        _b, pb = _host(self.dtype, beta)
        self._check(lib().mik_gs_multiply(self.handle, int(bool(upper)), pa, self._vec(x, "x"), pb, self._vec(y, "y"), self._vec(z, "z")),
                    "mik_gs_multiply")
        return z

    def _sub(self, fn, where, x, omega, y):
        px = self._vec(x, "x")
        if y is None:
            self._check(fn(self.handle, None, px, None, None, _lib.MIK_F64), where)
            return x
        a, b, S = _relax_scalars(self.dtype, omega)
        _a, pa = _host(S, a)
        _b, pb = _host(b.dtype, b)                  # of S, or (complex operator) the complex type over S
        self._check(fn(self.handle, pa, px, pb, self._vec(y, "y"), _lib.dtype_code(S)), where)
        return x

    def forward_sub_(self, x: HipVector, omega=None, y: Optional[HipVector] = None) -> HipVector:
        """``forward_sub!(L, x)`` (y None) or ``forward_sub!(omega, L, x, one(T) - omega, y)`` -- :67-103."""
        return self._sub(lib().mik_forward_sub, "mik_forward_sub", x, omega, y)

    def backward_sub_(self, x: HipVector, omega=None, y: Optional[HipVector] = None) -> HipVector:
        """``backward_sub!(U, x)`` (y None) or ``backward_sub!(omega, U, x, one(T) - omega, y)`` -- :109-142."""
        return self._sub(lib().mik_backward_sub, "mik_backward_sub", x, omega, y)

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.ctx.handle:
                lib().mik_stationary_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _StationaryIterable:
    """start / done / iterate of the four iterables (exactly ``maxiter`` iterations, no convergence test)."""

    def start(self) -> int:
        return 1

    def done(self, iteration: int) -> bool:
        return iteration > self.maxiter

    def iterate(self, iteration: Optional[int] = None):
        iteration = self.start() if iteration is None else iteration
        if self.done(iteration):
            return None
        self._step()
        return None, iteration + 1

    def __iter__(self):
        iteration = self.start()
        while True:
            nxt = self.iterate(iteration)
            if nxt is None:
                return
            item, iteration = nxt
            yield item


class JacobiIterable(_StationaryIterable):                                          # :213-221
    def __init__(self, O: StationaryOperator, x: HipVector, next: HipVector, b: HipVector, maxiter: int):
        self.O, self.x, self.next, self.b, self.maxiter = O, x, next, b, int(maxiter)

    def _step(self):                                                                # :225-234
        m1 = _minus_one(self.x.dtype)                                               # T = eltype(x); -one(T)  
        self.next.copyto_(self.b)                                                   # copyto!(j.next, j.b)
        self.O.offdiag_mul_(m1, self.x, 1, self.next)                               # mul!(-one(T), j.O, j.x, one(T), j.next)
        self.O.diag_ldiv_(self.x, self.next)                                        # ldiv!(j.x, j.O.diag, j.next)


class GaussSeidelIterable(_StationaryIterable):                                     # :261-269
    def __init__(self, S: StationaryOperator, x: HipVector, b: HipVector, maxiter: int):
        self.U = self.L = S
        self.x, self.b, self.maxiter = x, b, int(maxiter)

    def _step(self):                                                                # :278-288
        m1 = _minus_one(self.x.dtype)                                               # T = eltype(x); -one(T)  
        self.U.gs_multiply_(True, m1, self.x, 1, self.b, self.x)                    # gauss_seidel_multiply!(-one(T), g.U, g.x, one(T), g.b, g.x)
        self.L.forward_sub_(self.x)                                                 # forward_sub!(g.L, g.x)


class SORIterable(_StationaryIterable):                                             # :308-318
    def __init__(self, S: StationaryOperator, omega, x: HipVector, next: HipVector, b: HipVector, maxiter: int):
        self.U = self.L = S
        self.omega = omega
        self.x, self.next, self.b, self.maxiter = x, next, b, int(maxiter)

    def _step(self):                                                                # :322-336
        m1 = _minus_one(self.x.dtype)                                               # T = eltype(x); -one(T)  
        self.U.gs_multiply_(True, m1, self.x, 1, self.b, self.next)                 # next = b - U * x
        self.L.forward_sub_(self.next, self.omega, self.x)                          # next = omega * inv(L) * next + (1 - omega) * x
        self.x, self.next = self.next, self.x                                       # switch current and next iterate


class SSORIterable(_StationaryIterable):                                            # :366-376
    def __init__(self, S: StationaryOperator, omega, x: HipVector, tmp: HipVector, b: HipVector, maxiter: int):
        self.sL = self.sU = self.L = self.U = S
        self.omega = omega
        self.x, self.tmp, self.b, self.maxiter = x, tmp, b, int(maxiter)

    def _step(self):                                                                # :392-418
        m1 = _minus_one(self.x.dtype)                                               # T = eltype(x); -one(T)  
        self.sU.gs_multiply_(True, m1, self.x, 1, self.b, self.tmp)                 # tmp = b - U * x
        self.L.forward_sub_(self.tmp, self.omega, self.x)                           # tmp = omega * inv(L) * tmp + (1 - omega) * x
        self.sL.gs_multiply_(False, m1, self.tmp, 1, self.b, self.x)                # x = b - L * tmp
        self.U.backward_sub_(self.x, self.omega, self.tmp)                          # x = omega * inv(U) * x + (1 - omega) * tmp


def jacobi_iterable(x: HipVector, A: HipCSR, b: HipVector, *, maxiter: int = 10) -> JacobiIterable:   # :236-238
    return JacobiIterable(StationaryOperator(A), x, x.similar(), b, maxiter)


def gauss_seidel_iterable(x: HipVector, A: HipCSR, b: HipVector, *, maxiter: int = 10) -> GaussSeidelIterable:   # :271-274
    return GaussSeidelIterable(StationaryOperator(A), x, b, maxiter)


def sor_iterable(x: HipVector, A: HipCSR, b: HipVector, omega, *, maxiter: int = 10) -> SORIterable:   # :338-344
    return SORIterable(StationaryOperator(A), omega, x, x.similar(), b, maxiter)


def ssor_iterable(x: HipVector, A: HipCSR, b: HipVector, omega, *, maxiter: int = 10) -> SSORIterable:   # :378-387
    return SSORIterable(StationaryOperator(A), omega, x, x.similar(), b, maxiter)


def _run(iterable):
    for _ in iterable:
        pass
    return iterable.x


def jacobi_(x: HipVector, A: HipCSR, b: HipVector, *, maxiter: int = 10) -> HipVector:            # jacobi!  :251-255
    return _run(jacobi_iterable(x, A, b, maxiter=maxiter))


def gauss_seidel_(x: HipVector, A: HipCSR, b: HipVector, *, maxiter: int = 10) -> HipVector:      # gauss_seidel!  :298-302
    return _run(gauss_seidel_iterable(x, A, b, maxiter=maxiter))


def sor_(x: HipVector, A: HipCSR, b: HipVector, omega, *, maxiter: int = 10) -> HipVector:        # sor!  :356-360
    """Returns ``iterable.x``: after an odd number of iterations that is the internal buffer, and the caller's ``x``
    holds iterate ``maxiter - 1`` (the swap at :334)."""
    return _run(sor_iterable(x, A, b, omega, maxiter=maxiter))


def ssor_(x: HipVector, A: HipCSR, b: HipVector, omega, *, maxiter: int = 10) -> HipVector:       # ssor!  :422-426
    return _run(ssor_iterable(x, A, b, omega, maxiter=maxiter))


def jacobi(A: HipCSR, b: HipVector, **kwargs) -> HipVector:                         # src/stationary.jl:19
    return jacobi_(zerox(A, b), A, b, **kwargs)


def gauss_seidel(A: HipCSR, b: HipVector, **kwargs) -> HipVector:                   # src/stationary.jl:79
    return gauss_seidel_(zerox(A, b), A, b, **kwargs)


def sor(A: HipCSR, b: HipVector, omega, **kwargs) -> HipVector:                     # src/stationary.jl:136
    return sor_(zerox(A, b), A, b, omega, **kwargs)


def ssor(A: HipCSR, b: HipVector, omega, **kwargs) -> HipVector:                    # src/stationary.jl:195
    return ssor_(zerox(A, b), A, b, omega, **kwargs)
