"""The stationary methods in the Julia shim (MIK.jl), checked statically like the rest of the shim (no Julia toolchain here), and the
C ABI / ctypes entries behind them.  No GPU."""
import os
import re

from conftest import ROOT

JL = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "julia", "MIK.jl")).read()
HEADER = open(os.path.join(ROOT, "include", "mik.h")).read()
ENTRIES = ("mik_stationary_create", "mik_stationary_destroy", "mik_stationary_info", "mik_diag_ldiv", "mik_offdiag_mul", "mik_gs_multiply",
           "mik_forward_sub", "mik_backward_sub")


def test_header_and_binding_declare_the_stationary_entries(pkg):
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", HEADER), name
        assert name in pkg._lib.SIGNATURES, name
    assert "MIK_ABI_VERSION 6" in HEADER and "stationary" in HEADER.split("enum {")[0]


def test_every_stationary_entry_is_called_by_the_shim_with_the_c_arity(pkg):
    calls = {}
    for m in re.finditer(r"ccall\(\(:(mik_\w+), libmik\),\s*\w+,\s*\(([^)]*)\)", JL):
        calls.setdefault(m.group(1), set()).add(len([a for a in m.group(2).split(",") if a.strip()]))
    for name in ENTRIES:
        assert calls.get(name) == {len(pkg._lib.SIGNATURES[name][1])}, (name, calls.get(name))


def test_the_reference_methods_exist_with_their_keyword_defaults():
    """src/stationary_sparse.jl: jacobi! / gauss_seidel! (x, A, b; maxiter = 10), sor! / ssor! (x, A, b, ω; maxiter = 10), the
    four iterables, the non-! forms through zerox (src/stationary.jl:19, :79, :136, :195)"""
    for fn in ("jacobi!", "gauss_seidel!"):
        assert f"function IterativeSolvers.{fn}(x::HipVector{{T}}, A::HipCSR{{T}}, b::HipVector{{T}}; maxiter::Int = 10)" in JL, fn
    for fn in ("sor!", "ssor!"):
        assert f"function IterativeSolvers.{fn}(x::HipVector{{T}}, A::HipCSR{{T}}, b::HipVector{{T}}, ω::Real; maxiter::Int = 10)" in JL, fn
    for fn in ("jacobi_iterable", "gauss_seidel_iterable"):
        assert f"IterativeSolvers.{fn}(x::HipVector{{T}}, A::HipCSR{{T}}, b::HipVector{{T}}; maxiter::Int = 10)" in JL, fn
    for fn in ("sor_iterable", "ssor_iterable"):
        assert f"IterativeSolvers.{fn}(x::HipVector{{T}}, A::HipCSR{{T}}, b::HipVector{{T}}, ω::Real; maxiter::Int = 10)" in JL, fn
    for fn in ("jacobi", "gauss_seidel", "sor", "ssor"):
        assert re.search(rf"IterativeSolvers\.{fn}\(A::HipCSR\{{T\}}, b::HipVector\{{T\}}.*= IterativeSolvers\.{fn}!\(IterativeSolvers\.zerox\(A, b\)", JL), fn
    for it in ("HipJacobiIterable", "HipGaussSeidelIterable", "HipSORIterable", "HipSSORIterable"):
        assert re.search(rf"function Base\.iterate\(\w+::{it}\{{T\}}, iteration::Int = 1\)", JL), it


def test_singular_status_throws_singular_exception_with_the_column():
    i = JL.index("function HipStationary(A::HipCSR{T})")
    body = JL[i:JL.index("\nend", i)]
    assert "code == 8 && throw(LinearAlgebra.SingularException(Int(col[])))" in body


def test_sor_iterate_swaps_like_the_reference():
    """:334 -- the swap that makes sor! return the internal buffer after an odd number of iterations"""
    i = JL.index("function Base.iterate(s::HipSORIterable{T}")
    body = JL[i:JL.index("\nend", i)]
    assert "s.x, s.next = s.next, s.x" in body
