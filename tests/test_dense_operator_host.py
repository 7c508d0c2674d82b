"""The dense operator (mul!(y, A::Matrix, x) and its adjoint) without a GPU: the C restatement tests/dense_ref/dense_mul_ref.c of the
chunked order held to the plain column loop and to the oracle's sparse product on the fully stored matrix; header, binding and library
export of the seven entries; the Python layer (HipMatrix as an operator, its adjoint view, mul_, the native-callback operator of the
fused iterables) on a numpy double of the library; and the Julia shim, statically."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dense_operator_host as dh
from conftest import ROOT
from dense_operator_double import DoubleLib, DoubleVector, matrix
from test_julia_shim import ccalls

ENTRIES = ("mik_dense_mul_shape", "mik_dense_create", "mik_dense_destroy", "mik_dense_mul", "mik_dense_mul_fn", "mik_dense_mul_adj_fn")
HEADER = open(os.path.join(ROOT, "include", "mik.h")).read()
JL = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "julia", "MIK.jl")).read()
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dense_mul_ref"))


def _shape(pkg):
    c, r = C.c_int(), C.c_int()
    assert pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r)) == 0
    return c.value, r.value


# ---- 1: the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chunk", [32, 64, 256])
def test_up_to_one_chunk_the_chunked_order_is_the_plain_column_loop(ref, dtype, chunk):
    for m, n in ((1, 1), (7, chunk - 1), (65, chunk), (3, 5)):
        A, x = dh.rect(m, n, dtype), dh.vec(n, dtype)
        assert np.array_equal(ref.chunked(A, x, chunk), ref.serial(A, x)), (m, n)
    A, x = dh.rect(9, 3 * chunk + 5, dtype), dh.vec(3 * chunk + 5, dtype)
    assert not np.array_equal(ref.chunked(A, x, chunk), ref.serial(A, x))          # beyond one chunk it is another order ...
    p = [ref.serial(A[:, j:j + chunk], x[j:j + chunk]) for j in range(0, A.shape[1], chunk)]
    tot = p[0]
    for q in p[1:]:
        tot = tot + q                                                              # ... the chunk sums added left to right
    assert np.array_equal(ref.chunked(A, x, chunk), tot)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_restatement_reads_no_padding_and_the_empty_sum_is_plus_zero(ref, dtype):
    A, x = dh.rect(13, 70, dtype), dh.vec(70, dtype)
    assert np.array_equal(ref.chunked(A, x, 32), ref.chunked(A, x, 32, ld=20))       # the padding rows are NaN
    y = ref.chunked(np.zeros((4, 0), dtype), np.zeros(0, dtype), 64)
    assert np.array_equal(y, np.zeros(4, dtype)) and not np.signbit(y).any()
    y = ref.chunked(np.full((3, 5), -0.0, dtype), np.ones(5, dtype), 64)           # a row of -0.0 products: +0 + -0 = +0
    assert np.array_equal(y, np.zeros(3, dtype)) and not np.signbit(y).any()
    A = dh.rect(4, 6, dtype)
    A[2, 3] = 0
    x = dh.vec(6, dtype)
    x[3] = np.inf
    y = ref.chunked(A, x, 64)
    assert np.isnan(y[2]) and np.isinf(y[[0, 1, 3]]).all()                         # Inf * 0 = NaN in that row only


@pytest.mark.parametrize("dtype", DTYPES)
def test_up_to_one_chunk_it_is_the_oracles_sparse_product_of_the_fully_stored_matrix(pkg, orc, ref, dtype):
    chunk, _ = _shape(pkg)
    for m, n in ((5, 1), (64, 48), (33, min(chunk, 256)), (130, min(chunk, 256) - 1)):
        A, x = dh.rect(m, n, dtype, seed=5), dh.vec(n, dtype, seed=5)
        assert np.count_nonzero(A) == A.size
        assert np.array_equal(ref.chunked(A, x, chunk), dh.oracle_spmv(orc, A, x)), (m, n)


# ---- 2: header, binding, export ------------------------------------------------------------------------------------------------
def test_header_binding_and_export_agree_on_the_entries(pkg):
    L = pkg.lib()
    assert "MIK_ABI_VERSION 6" in HEADER and L.mik_abi_version() == 6
    section = HEADER[HEADER.index("---- dense operator"):HEADER.index("---- measurement")]
    assert HEADER.index("---- lobpcg") < HEADER.index("---- dense operator")
    assert "typedef struct mik_dense mik_dense;" in section
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", section), name
        decl = re.search(rf"\bint {name}\(([^;]*)\);", section).group(1)
        assert len(decl.split(",")) == len(pkg._lib.SIGNATURES[name][1]), name
        assert callable(getattr(L, name))
    for cite in ("src/cg.jl:54,137", "src/gmres.jl:245,287", "src/lsqr.jl:", "src/lsmr.jl:", "src/qmr.jl:", "src/svdl.jl:"):
        assert cite in section, cite
    chunk, rows = _shape(pkg)
    assert chunk in (32, 64, 128, 256) and rows > 0
    assert L.mik_dense_mul(None, 0, None, None) == 1 and L.mik_dense_mul_fn(None, None, None) == 1 and L.mik_dense_mul_adj_fn(None, None, None) == 1
    assert L.mik_dense_create(None, 0, 1, 1, None, 1, None) == 1 and L.mik_dense_destroy(None) == 0       # MIK_ERR_INVALID, no device needed


def test_the_launch_plan_query_is_a_development_entry_and_fails_cleanly_without_a_handle(pkg):
    dev = open(os.path.join(ROOT, "include", "mik_dev.h")).read()
    assert "mik_dev_dense_plan" not in HEADER and re.search(r"\bint mik_dev_dense_plan\(const mik_dense \*D, int adjoint,", dev)
    v, s = C.c_int(-1), C.c_int(-1)
    g = [C.c_int64(-1) for _ in range(4)]
    assert pkg.lib().mik_dev_dense_plan(None, 0, None, None, C.byref(v), C.byref(s), *[C.byref(q) for q in g]) == 1       # MIK_ERR_INVALID
    assert (v.value, s.value) == (-1, -1) and all(q.value == -1 for q in g)                                              # nothing was written
    src = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "csrc", "mik_dense_mul.hip")).read()
    hdr = open(os.path.join(ROOT, "iterativesolvers.jl_amd", "csrc", "mik_dense_mul.h")).read()
    assert "192.0e6" not in src and hdr.count("192.0e6") == 1 and "MIK_DM_STREAM_BYTES" in src     # the streaming threshold has one home
    for fn in ("dm_mul_n", "dm_mul_t"):                                                             # launch and query share the helper
        body = src[src.index(f"int {fn}("):]
        assert f"dm_plan_{fn[-1]}<T>(D, x, y)" in body[:body.index("return MIK_OK;\n}")]
    q = src[src.index('extern "C" int mik_dev_dense_plan('):]
    assert "dm_plan_n<double>" in q and "dm_plan_t<float>" in q[:q.index("\n}\n")]


# ---- 3: the Python layer on the numpy double ------------------------------------------------------------------------------------
@pytest.fixture
def double(pkg, ref, monkeypatch):
    D = DoubleLib(pkg.lib(), ref, _shape(pkg)[0])
    monkeypatch.setattr(pkg.api, "lib", lambda: D)
    return D


@pytest.mark.parametrize("dtype", DTYPES)
def test_mul_dispatches_a_matrix_and_its_adjoint_view(pkg, ref, double, dtype):
    A = dh.rect(37, 150, dtype)
    M = matrix(pkg, A)
    assert (M.n_rows, M.n_cols, M.size(), M.size(1), M.size(2), M.eltype()) == (37, 150, (37, 150), 37, 150, np.dtype(dtype))
    x, y = DoubleVector(dh.vec(150, dtype)), DoubleVector(np.zeros(37, dtype))
    assert pkg.mul_(y, M, x) is y and np.array_equal(y.a, ref.chunked(A, x.a, double.chunk))
    assert len(double.created) == 1                                              # the handle is created at the first product ...
    Mt = M.adj
    assert isinstance(Mt, pkg.HipMatrixAdjoint) and Mt.adj is M and M.adj is Mt and M.adj.adj is M
    assert (Mt.n_rows, Mt.n_cols, Mt.size(), Mt.size(1), Mt.eltype()) == (150, 37, (150, 37), 150, np.dtype(dtype))
    assert pkg.extras.adjoint(M) is Mt and pkg.extras.adjoint(Mt) is M
    u, v = DoubleVector(dh.vec(37, dtype)), DoubleVector(np.zeros(150, dtype))
    assert pkg.mul_(v, Mt, u) is v
    np.testing.assert_allclose(v.a, A.T.astype(np.float64) @ u.a, rtol=1e-4 if dtype == np.float32 else 1e-12)
    assert len(double.created) == 1 and [c[2] for c in double.calls] == [0, 1]   # ... and shared with the adjoint view
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.mul_(y, Mt, u)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.mul_(DoubleVector(np.zeros(37, np.float32 if dtype == np.float64 else np.float64)), M, x)


def test_cg_and_gmres_hand_the_native_callback_to_the_library(pkg, double):
    A = dh.spd(40, np.float64)
    M = matrix(pkg, A)
    native = C.cast(pkg.lib().mik_dense_mul_fn, C.c_void_p).value
    native_adj = C.cast(pkg.lib().mik_dense_mul_adj_fn, C.c_void_p).value
    assert native and native_adj and native != native_adj
    b = DoubleVector(dh.vec(40, np.float64))
    it = pkg.cg_iterator_(DoubleVector(np.zeros(40)), M, b)
    assert isinstance(it, pkg.CGIterable)
    g = pkg.gmres_iterable_(DoubleVector(np.zeros(40)), M, b)
    assert isinstance(g, pkg.GMRESIterable)
    handle = double.created[0]
    assert double.calls == [("mik_cg_create_op", 0, 40, None, native, handle), ("mik_gmres_create_op", 0, 40, None, native, handle)]
    assert it._bound.keep == [M] and g._bound.keep == [M]                       # the matrix is kept alive; no Python callback was made
    double.calls.clear()
    pkg.gmres_iterable_(DoubleVector(np.zeros(40)), M.adj, b)
    assert double.calls == [("mik_gmres_create_op", 0, 40, None, native_adj, handle)]


def test_a_rectangular_or_mistyped_matrix_never_reaches_the_native_callback(pkg, double):
    """the library's callback cannot see the vector lengths: the binding refuses what mul_ would refuse"""
    M = matrix(pkg, dh.rect(40, 50, np.float64))
    for A, n in ((M, 40), (M.adj, 50)):
        b = DoubleVector(dh.vec(n, np.float64))
        with pytest.raises(ValueError, match="DimensionMismatch"):
            pkg.cg_iterator_(DoubleVector(np.zeros(n)), A, b)
        with pytest.raises(ValueError, match="DimensionMismatch"):
            pkg.gmres_iterable_(DoubleVector(np.zeros(n)), A, b)
    S = matrix(pkg, dh.spd(40, np.float64))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.api._Bound(S.ctx, 39, np.float64).operator(S)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.api._Bound(S.ctx, 40, np.float32).operator(S)
    assert double.calls == [] and double.created == []                  # nothing was created, nothing was handed to the library


def test_the_adjoint_view_does_not_keep_the_matrix_alive(pkg, double):
    import gc
    import weakref
    gc.disable()
    try:
        M = matrix(pkg, dh.rect(6, 4, np.float64))
        view = M.adj
        assert M.adj is view and view.adj is M
        alive = weakref.ref(M)
        del M
        assert alive() is view.adj                                       # the view holds the matrix ...
        del view
        assert alive() is None                                           # ... and no cycle holds either: freed without the cycle collector
    finally:
        gc.enable()


def test_svdl_and_lobpcg_keep_their_refusals(pkg, double):
    with pytest.raises(TypeError):
        pkg.svdl(object())
    ops = pkg.svdl.__globals__["DeviceOps"](matrix(pkg, dh.rect(6, 4, np.float64)))      # a HipMatrix is accepted, its adjoint is the view
    assert (ops.m, ops.n) == (6, 4) and ops.A.adj.adj is ops.A
    M = matrix(pkg, dh.spd(8, np.float64))
    with pytest.raises(TypeError, match="HipCSR"):
        pkg.lobpcg(M, False, 2)


# ---- 4: the Julia shim, statically ----------------------------------------------------------------------------------------------
def _body(start):
    i = JL.index(start)
    return JL[i:JL.index("\nend", i)]


def test_the_shim_binds_the_dense_operator(pkg):
    calls = {}
    for sym, ret, nargs in ccalls(JL):
        calls.setdefault(sym, set()).add((ret, nargs))
    for name in ("mik_dense_mul_shape", "mik_dense_create", "mik_dense_destroy", "mik_dense_mul"):
        assert calls.get(name) == {("Cint", len(pkg._lib.SIGNATURES[name][1]))}, (name, calls.get(name))
    assert "function LinearAlgebra.mul!(y::HipVector{T}, A::HipDenseMatrix{T}, x::HipVector{T}) where {T}" in JL
    assert "function LinearAlgebra.mul!(y::HipVector{T}, A::HipDenseAdjoint{T}, x::HipVector{T}) where {T}" in JL
    assert "LinearAlgebra.adjoint(A::HipDenseMatrix) = HipDenseAdjoint(A)" in JL and "LinearAlgebra.adjoint(A::HipDenseAdjoint) = A.parent" in JL
    body = _body("function dense_mul!(")
    assert [c[0] for c in ccalls(body)] == ["mik_dense_mul"] and "throw(DimensionMismatch(" in body.split("ccall")[0]
    assert re.search(r"mutable struct HipDenseMatrix\{T<:MikFloat\}\s+ptr::Ptr\{Cvoid\}\s+n::Int\s+cols::Int\s+ld::Int\s+ctx::Context\s+end", JL)   # untouched
    # the operator of the fused iterables: the library's own function pointer and the handle, no trampoline
    assert "MikOperator(dtype_code(T), n, C_NULL, cglobal((:mik_dense_mul_fn, libmik)), dense_operator(A).handle)" in JL
    assert "MikOperator(dtype_code(T), n, C_NULL, cglobal((:mik_dense_mul_adj_fn, libmik)), dense_operator(A.parent).handle)" in JL
    for kind in ("HipDenseMatrix", "HipDenseAdjoint"):                   # a rectangular or mistyped matrix is refused before the pointer is handed over
        b = _body(f"function dense_operator_struct(A::{kind}")
        assert b.index("dense_square(A, T, n)") < b.index("MikOperator(")
    assert "throw(DimensionMismatch(" in JL[JL.index("dense_square(A, ::Type{T}"):JL.index("function dense_operator_struct(A::HipDenseMatrix")]
    body = _body("function operator_struct(")
    assert body.index("A isa HipDenseMatrix") < body.index("@cfunction(mul_trampoline") and "push!(keep, A)" in body
