# MIK.jl -- Julia-side shim: binds libmik.so (include/mik.h) behind IterativeSolvers.jl's own
# dispatch points so that the UNMODIFIED `cg!` / `gmres!` drivers run the HIP path.
#
# STATUS: written against include/mik.h and IterativeSolvers v0.9.4; NOT EXECUTED -- no Julia
# toolchain exists in the build environment (SURVEY.md F3).  The Python mirror
# (iterativesolvers.jl_amd/api.py) issues the same C calls in the same order and IS tested on
# MI355X; keep the two in step.
#
# Plug points (file:line in the reference):
#   cg!(x, A, b; ...)        src/cg.jl:209  calls cg_iterator!(x, A, b, Pl; ...) at :224
#       -> method cg_iterator!(x::HipVector, A::HipCSR, b::HipVector, Pl; ...) below returns a
#          HipCGIterable; the driver's loop (:229-235) then uses Base.iterate, `iterable.residual`,
#          `iterable.mv_products`, `iterable.x` and IterativeSolvers.converged -- all defined here.
#   gmres!(x, A, b; ...)     src/gmres.jl:184 calls gmres_iterable!(x, A, b; ...) at :200
#       -> method gmres_iterable!(x::HipVector, A::HipCSR, b::HipVector; ...) returns a
#          HipGMRESIterable (needed because ArnoldiDecomp pins V to a host Matrix, src/gmres.jl:7,13).
#   bicgstabl!(x, A, b, l)   src/bicgstabl.jl:181 calls bicgstabl_iterator!(x, A, b, l; ...) at :197 -> HipBiCGStabIterable
#   minres!(x, A, b)         src/minres.jl:197 calls minres_iterable!(x, A, b; ...) at :208 -> HipMINRESIterable
#       (one C call per iteration each: mik_bicgstab_step, mik_minres_step)
#   lsqr! / lsmr! / qmr!     run UNMODIFIED on HipVector / HipCSR: adjoint(A) is the operator uploaded by MIK.with_adjoint (the CSC arrays read
#       as CSR), their vector statements lower through the broadcast style and axpy! / rmul! / dot / norm below (one L1 call per statement)
#   idrs!(x, A, b)           src/idrs.jl:49 -> idrs_method! (:150) calls idrs_iterable!(log, X, A, C, s, Pl, ...) at :156 -> HipIDRSIterable
#       (one C call per step: mik_idrs_step)
#   Generic code paths (any other solver of the package) see HipVector/HipCSR through
#   mul!, dot, norm, axpy!, rmul!, ldiv!, copyto!, fill!, similar, zero and the broadcast style below (the four
#   vector-update shapes of src/cg.jl), so the unmodified iterate(::CGIterable) runs on device vectors as well.
module MIK

using LinearAlgebra
using SparseArrays
import IterativeSolvers
import IterativeSolvers: Identity, OrthogonalizationMethod, ModifiedGramSchmidt, ClassicalGramSchmidt, DGKS

const libmik = get(ENV, "LIBMIK", joinpath(@__DIR__, "..", "libmik.so"))

const MIK_F64 = Cint(0); const MIK_F32 = Cint(1)
dtype_code(::Type{Float64}) = MIK_F64
dtype_code(::Type{Float32}) = MIK_F32
const MikFloat = Union{Float32, Float64}

struct MikError <: Exception
    code::Cint
    where::String
    detail::String
end

function check(code::Cint, where::AbstractString, ctx::Ptr{Cvoid} = C_NULL)
    code == 0 && return
    msg = ccall((:mik_last_error, libmik), Cstring, (Ptr{Cvoid},), ctx)
    throw(MikError(code, where, msg == C_NULL ? "" : unsafe_string(msg)))
end

# ---- context ------------------------------------------------------------------------------------
mutable struct Context
    handle::Ptr{Cvoid}
    function Context(device::Integer = 0)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mik_ctx_create, libmik), Cint, (Cint, Ref{Ptr{Cvoid}}), device, h), "mik_ctx_create")
        ctx = new(h[])
        # Julia gives no finalizer order at exit: the context marks itself dead (handle = C_NULL) and every child's
        # finalizer checks `alive(ctx)` first -- a child outliving its context leaks device memory of a dying process
        # instead of handing mik_free a context that no longer exists.
        finalizer(ctx) do c
            c.handle == C_NULL || ccall((:mik_ctx_destroy, libmik), Cint, (Ptr{Cvoid},), c.handle)
            c.handle = C_NULL
        end
        ctx
    end
end
alive(c::Context) = c.handle != C_NULL
struct DeviceInfo                    # same field order and types as the C struct mik_device_info
    device::Cint
    compute_units::Cint
    xcds::Cint
    wavefront_size::Cint
    lds_bytes_per_cu::Int64
    l2_bytes::Int64
    hbm_bytes::Int64
    arch::NTuple{64, UInt8}
    planned_compute_units::Cint
    planned_xcds::Cint
    xcd_maps::Cint
    resident_workgroup_cap::Cint
    gs_single_launch_max_segments::Cint
    gs_xcd_local_max_workgroups::Cint
    sweep_grid_cap::Cint
    mgs_resident_max_segments::Cint
    reserved::NTuple{7, Cint}
end
"The machine behind a context as the library queried it, and the launch caps it derived (mik_ctx_info)."
function device_info(ctx::Context = context())
    r = Ref{DeviceInfo}()
    check(ccall((:mik_ctx_info, libmik), Cint, (Ptr{Cvoid}, Ref{DeviceInfo}), ctx.handle, r), "mik_ctx_info", ctx.handle)
    r[]
end
const default_ctx = Ref{Union{Nothing, Context}}(nothing)
context() = (default_ctx[] === nothing && (default_ctx[] = Context(0)); default_ctx[]::Context)

# ---- device vector ------------------------------------------------------------------------------
mutable struct HipVector{T<:MikFloat} <: AbstractVector{T}
    ptr::Ptr{Cvoid}
    n::Int
    ctx::Context
    function HipVector{T}(::UndefInitializer, n::Integer, ctx::Context = context()) where {T<:MikFloat}
        p = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mik_malloc, libmik), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), ctx.handle, n * sizeof(T), p), "mik_malloc", ctx.handle)
        v = new{T}(p[], n, ctx)
        finalizer(x -> alive(x.ctx) && ccall((:mik_free, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.handle, x.ptr), v)
        v
    end
    # a view of device memory owned by somebody else (no finalizer): what the operator / preconditioner callbacks receive
    HipVector{T}(ptr::Ptr{Cvoid}, n::Integer, ctx::Context, ::Val{:unowned}) where {T<:MikFloat} = new{T}(ptr, n, ctx)
end
function HipVector(a::Vector{T}, ctx::Context = context()) where {T<:MikFloat}
    v = HipVector{T}(undef, length(a), ctx)
    GC.@preserve a check(ccall((:mik_memcpy_h2d, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                               ctx.handle, v.ptr, pointer(a), sizeof(a)), "mik_memcpy_h2d", ctx.handle)
    v
end
Base.size(v::HipVector) = (v.n,)
Base.similar(v::HipVector{T}) where {T} = HipVector{T}(undef, v.n, v.ctx)
Base.similar(v::HipVector, ::Type{T}, n::Integer) where {T<:MikFloat} = HipVector{T}(undef, n, v.ctx)
Base.similar(v::HipVector, ::Type{T}, dims::Tuple{Int}) where {T<:MikFloat} = HipVector{T}(undef, dims[1], v.ctx)
Base.zero(v::HipVector{T}) where {T} = fill!(similar(v), zero(T))
function Base.Array(v::HipVector{T}) where {T}
    a = Vector{T}(undef, v.n)
    GC.@preserve a check(ccall((:mik_memcpy_d2h, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                               v.ctx.handle, pointer(a), v.ptr, sizeof(a)), "mik_memcpy_d2h", v.ctx.handle)
    a
end
# Scalar indexing would copy the WHOLE vector device-to-host per element (134 MB at 256^3): any generic AbstractVector
# fallback that reaches it -- show, a missed broadcast, a generic dot -- must fail loudly instead of crawling.
const scalar_indexing_allowed = Ref(false)
"allowscalar(true) permits v[i] (one full device-to-host copy per call) for debugging at the REPL."
allowscalar(flag::Bool) = (scalar_indexing_allowed[] = flag)
function Base.getindex(v::HipVector, i::Int)
    scalar_indexing_allowed[] || error("scalar indexing of a HipVector is disabled (it copies the whole vector per element); ",
                                       "use Array(v), or MIK.allowscalar(true) at the REPL")
    Array(v)[i]
end
Base.setindex!(v::HipVector, x, i::Int) = error("setindex! on a HipVector is not supported; build a Vector and upload it with HipVector(a)")
Base.show(io::IO, v::HipVector{T}) where {T} = print(io, "HipVector{", T, "}(n = ", v.n, ") on device memory")
Base.show(io::IO, ::MIME"text/plain", v::HipVector) = show(io, v)
function Base.fill!(v::HipVector{T}, val) where {T}
    check(ccall((:mik_fill, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{T}, Ptr{Cvoid}), v.ctx.handle, dtype_code(T), v.n, T(val), v.ptr), "mik_fill", v.ctx.handle)
    v
end
function Base.copyto!(y::HipVector{T}, x::HipVector{T}) where {T}
    check(ccall((:mik_copy, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), y.ctx.handle, dtype_code(T), y.n, x.ptr, y.ptr), "mik_copy", y.ctx.handle)
    y
end
function LinearAlgebra.dot(x::HipVector{T}, y::HipVector{T}) where {T}
    out = Ref{T}()
    check(ccall((:mik_dot, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}), x.ctx.handle, dtype_code(T), x.n, x.ptr, y.ptr, out), "mik_dot", x.ctx.handle)
    out[]
end
function LinearAlgebra.norm(x::HipVector{T}) where {T}
    out = Ref{T}()
    check(ccall((:mik_nrm2, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ref{T}), x.ctx.handle, dtype_code(T), x.n, x.ptr, out), "mik_nrm2", x.ctx.handle)
    out[]
end
function LinearAlgebra.axpy!(a, x::HipVector{T}, y::HipVector{T}) where {T}           # y .+= a .* x
    check(ccall((:mik_axpy, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{T}, Ptr{Cvoid}, Ptr{Cvoid}), y.ctx.handle, dtype_code(T), y.n, T(a), x.ptr, y.ptr), "mik_axpy", y.ctx.handle)
    y
end
function xpby!(x::HipVector{T}, b, y::HipVector{T}) where {T}                          # y .= x .+ b .* y
    check(ccall((:mik_xpby, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}), y.ctx.handle, dtype_code(T), y.n, x.ptr, T(b), y.ptr), "mik_xpby", y.ctx.handle)
    y
end
function LinearAlgebra.rmul!(x::HipVector{T}, a::Number) where {T}                    # x .*= a
    check(ccall((:mik_scal, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ref{T}, Ptr{Cvoid}), x.ctx.handle, dtype_code(T), x.n, T(a), x.ptr), "mik_scal", x.ctx.handle)
    x
end

function sub!(x::HipVector{T}, y::HipVector{T}) where {T}                               # y .-= x
    check(ccall((:mik_sub, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), y.ctx.handle, dtype_code(T), y.n, x.ptr, y.ptr), "mik_sub", y.ctx.handle)
    y
end

# ---- broadcast: SURVEY.md section 8b plug point (1) -----------------------------------------------------------------------
# The UNMODIFIED iterate(::CGIterable) writes its vector updates as fused broadcasts.  With this style they lower to
# the L1 entry points instead of falling into scalar indexing; the four shapes of src/cg.jl are
#     u .= r .+ beta .* u      (:51, :86)   -> mik_xpby
#     x .+= alpha .* u         (:58, :93)   -> mik_axpy(alpha)
#     r .-= alpha .* c         (:59, :94)   -> mik_axpy(-alpha)        [same rounded product, then a rounded subtract]
#     r .-= c                  (:138)       -> mik_sub
# and the scaled-sum shapes of src/lsqr.jl / src/lsmr.jl (`dest .= a .* v .+ w`, `dest .= v .+ w .* a`, `dest .= v .* a`, scale on either side)
#                                              -> mik_copy (when dest is not the scaled vector) + mik_xpby / mik_scal
# plus  x .= value (fill!) and  y .= x (copyto!).  Anything else throws -- by design: a shape that is not listed here
# would otherwise run as n scalar device-to-host copies.
struct HipStyle <: Base.Broadcast.AbstractArrayStyle{1} end
HipStyle(::Val{1}) = HipStyle()
HipStyle(::Val{N}) where {N} = Base.Broadcast.DefaultArrayStyle{N}()
Base.BroadcastStyle(::Type{<:HipVector}) = HipStyle()
const Bc = Base.Broadcast.Broadcasted

is_scaled(b) = b isa Bc && b.f === (*) && length(b.args) == 2 && b.args[1] isa Number && b.args[2] isa HipVector
# (scale, vector) of a term `v`, `a .* v` or `v .* a` (scale === nothing: unscaled); nothing for anything else.  The second form is how
# src/lsqr.jl:151,159 and src/lsmr.jl:161,167,199,201 write their updates; a rounded product is commutative, so both lower to the same call.
term(t::HipVector) = (nothing, t)
function term(t)
    (t isa Bc && t.f === (*) && length(t.args) == 2) || return nothing
    p, q = t.args
    p isa Number && q isa HipVector && return (p, q)
    q isa Number && p isa HipVector && return (q, p)
    nothing
end
function Base.copyto!(dest::HipVector{T}, bc::Bc{HipStyle}) where {T}
    f, a = bc.f, bc.args
    if f === identity && length(a) == 1
        return a[1] isa Number ? fill!(dest, a[1]) : copyto!(dest, a[1]::HipVector{T})
    elseif f === (+) && length(a) == 2 && is_scaled(a[2]) && (a[1] === dest || (a[2].args[2] === dest && a[1] isa HipVector))
        s, v = a[2].args
        a[1] === dest && return LinearAlgebra.axpy!(s, v, dest)                    # x .+= alpha .* u
        return xpby!(a[1], s, dest)                                                  # u .= r .+ beta .* u
    elseif f === (-) && length(a) == 2 && a[1] === dest
        is_scaled(a[2]) && return LinearAlgebra.axpy!(-a[2].args[1], a[2].args[2], dest)   # r .-= alpha .* c
        a[2] isa HipVector && return sub!(a[2], dest)                                # r .-= c
    elseif f === (+) && length(a) == 2 && term(a[1]) !== nothing && term(a[2]) !== nothing
        (s1, v1), (s2, v2) = term(a[1]), term(a[2])
        if s1 !== nothing && s2 === nothing                                          # dest .= s1 .* v1 .+ v2
            v2 === dest && v1 !== dest && return LinearAlgebra.axpy!(s1, v1, dest)
            v1 === dest || copyto!(dest, v1)                                         #   (u .= -alpha .* u .+ tmpm; w = t2 .* w .+ v; hbar .= hbar .* c .+ h)
            return xpby!(v2, s1, dest)
        elseif s1 === nothing && s2 !== nothing                                      # dest .= v1 .+ s2 .* v2   (u .= tmp_u .+ u .* -α)
            v2 === dest || (v1 === dest ? (return LinearAlgebra.axpy!(s2, v2, dest)) : copyto!(dest, v2))
            return xpby!(v1, s2, dest)
        elseif s1 === nothing && s2 === nothing && v1 === dest                       # x .+= (t1 * w)  with the product formed first (src/lsqr.jl:189)
            return LinearAlgebra.axpy!(one(T), v2, dest)
        end
    elseif f === (*) && length(a) == 2 && term(bc) !== nothing                       # u .*= inv(beta); wrho .= w .* inv(rho)
        s1, v1 = term(bc)
        v1 === dest || copyto!(dest, v1)
        return LinearAlgebra.rmul!(dest, s1)
    end
    error("broadcast shape not lowered for HipVector (MIK.jl lists the supported ones); expression: ", f, " over ", map(typeof, a))
end
Base.similar(bc::Bc{HipStyle}, ::Type{T}) where {T<:MikFloat} = HipVector{T}(undef, length(bc), first(x for x in Base.Broadcast.flatten(bc).args if x isa HipVector).ctx)

# ---- operator -----------------------------------------------------------------------------------
mutable struct HipCSR{T<:MikFloat}
    handle::Ptr{Cvoid}
    m::Int
    n::Int
    ctx::Context
    adj::Union{HipCSR{T}, Nothing}   # partner uploaded by with_adjoint: a reference cycle the GC collects as a whole (no global table keeps it alive)
    HipCSR{T}(handle, m, n, ctx) where {T<:MikFloat} = new{T}(handle, m, n, ctx, nothing)
end
"Upload a SparseMatrixCSC{T,Int} (colptr/rowval/nzval, 1-based Int64: test/laplace_matrix.jl:12)."
function HipCSR(A::SparseMatrixCSC{T, Int64}, ctx::Context = context()) where {T<:MikFloat}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A check(ccall((:mik_csr_create, libmik), Cint,
        (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
        ctx.handle, dtype_code(T), size(A, 1), size(A, 2), nnz(A), pointer(A.colptr), pointer(A.rowval), pointer(A.nzval), 1, 1, h),
        "mik_csr_create", ctx.handle)
    op = HipCSR{T}(h[], size(A, 1), size(A, 2), ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_csr_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), op)
    op
end
"SparseMatrixCSC{T,Int32} -- the reference's tests run `Ti in (Int64, Int32)` (test/gmres.jl:38): 32-bit colptr / rowval."
function HipCSR(A::SparseMatrixCSC{T, Int32}, ctx::Context = context()) where {T<:MikFloat}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A check(ccall((:mik_csr_create_i32, libmik), Cint,
        (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
        ctx.handle, dtype_code(T), size(A, 1), size(A, 2), nnz(A), pointer(A.colptr), pointer(A.rowval), pointer(A.nzval), 1, 1, h),
        "mik_csr_create_i32", ctx.handle)
    op = HipCSR{T}(h[], size(A, 1), size(A, 2), ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_csr_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), op)
    op
end
"""
The same upload from arrays that already live in DEVICE memory -- the colPtr / rowVal / nzVal buffers of an AMDGPU.jl
ROCSparseMatrixCSC, passed as raw device pointers: mik_csr_create detects the placement and starts its device-side pipeline
from them (no host copy).  The arrays are only read during the call.
"""
function HipCSR(::Type{T}, m::Integer, n::Integer, nz::Integer, colptr::Ptr{Int64}, rowval::Ptr{Int64}, nzval::Ptr{Cvoid},
                ctx::Context = context()) where {T<:MikFloat}
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_csr_create, libmik), Cint,
        (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
        ctx.handle, dtype_code(T), m, n, nz, colptr, rowval, nzval, 1, 1, h), "mik_csr_create", ctx.handle)
    op = HipCSR{T}(h[], m, n, ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_csr_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), op)
    op
end
# adjoint(A) for lsqr! / lsmr! / qmr! (src/lsqr.jl:120, src/lsmr.jl:113, src/qmr.jl:51): the SAME colptr / rowval / nzval read as a CSR matrix
# are A' (row j of A' = column j of A, entries in storage order = the order mul!(y, adjoint(A), x) of SparseArrays sums them in), so the
# adjoint is a second upload with is_csc = 0 -- no transpose is formed for it.  `with_adjoint(A)` returns the operator; `adjoint(op)` / `op'`
# its partner.  (Real element types.)
function with_adjoint(A::SparseMatrixCSC{T, Int64}, ctx::Context = context()) where {T<:MikFloat}
    op = HipCSR(A, ctx)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A check(ccall((:mik_csr_create, libmik), Cint,
        (Ptr{Cvoid}, Cint, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}),
        ctx.handle, dtype_code(T), size(A, 2), size(A, 1), nnz(A), pointer(A.colptr), pointer(A.rowval), pointer(A.nzval), 1, 0, h),
        "mik_csr_create", ctx.handle)
    adj = HipCSR{T}(h[], size(A, 2), size(A, 1), ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_csr_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), adj)
    op.adj = adj; adj.adj = op
    op
end
function LinearAlgebra.adjoint(A::HipCSR)
    A.adj === nothing && throw(MikError(Cint(5), "adjoint", "this operator was uploaded without its adjoint: use MIK.with_adjoint(A)"))
    A.adj
end
Base.:*(a::Number, x::HipVector{T}) where {T} = LinearAlgebra.rmul!(copyto!(similar(x), x), T(a))       # t1*w (src/lsqr.jl:189)

"Release the CSR arrays of an operator that runs on one of the sliced layouts (mik_csr_compact); false if it needs them."
function compact!(A::HipCSR)
    rc = ccall((:mik_csr_compact, libmik), Cint, (Ptr{Cvoid},), A.handle)
    rc == 5 && return false
    check(rc, "mik_csr_compact", A.ctx.handle)
    true
end
"Name of the kernel mul!(y, A, x) launches for this operator (mik_spmv_kernel; for profiles)."
function spmv_kernel(A::HipCSR)
    buf = zeros(UInt8, 64)
    check(ccall((:mik_spmv_kernel, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint), A.handle, buf, 64), "mik_spmv_kernel", A.ctx.handle)
    unsafe_string(pointer(buf))
end
Base.eltype(::HipCSR{T}) where {T} = T
Base.size(A::HipCSR) = (A.m, A.n)
Base.size(A::HipCSR, d::Integer) = d == 1 ? A.m : d == 2 ? A.n : 1
function LinearAlgebra.mul!(y::HipVector{T}, A::HipCSR{T}, x::HipVector{T}) where {T}
    check(ccall((:mik_spmv, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), A.ctx.handle, A.handle, x.ptr, y.ptr), "mik_spmv", A.ctx.handle)
    y
end
Base.:*(A::HipCSR{T}, x::HipVector{T}) where {T} = mul!(HipVector{T}(undef, A.m, A.ctx), A, x)

"Diagonal (Jacobi) left preconditioner on the device: ldiv!(y, P, x) = y .= x ./ P.diagonal (test/cg.jl:14-18)."
struct HipJacobi{T}
    diagonal::HipVector{T}
end
# ldiv!(y, P, x) / ldiv!(P, x): the contract of docs/src/preconditioning.md:5-14, so the GENERIC iterables (PCGIterable of
# src/cg.jl:72-100 through the broadcast style above, or any other solver of the package) accept it too
function LinearAlgebra.ldiv!(y::HipVector{T}, P::HipJacobi{T}, x::HipVector{T}) where {T}
    check(ccall((:mik_divide, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), y.ctx.handle, dtype_code(T), y.n, x.ptr, P.diagonal.ptr, y.ptr),
          "mik_divide", y.ctx.handle)
    y
end
LinearAlgebra.ldiv!(P::HipJacobi{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(x, P, x)
Base.:\(P::HipJacobi{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(similar(x), P, x)

# ---- CGIterable ---------------------------------------------------------------------------------
mutable struct HipCGIterable{T, Tx<:HipVector{T}}
    handle::Ptr{Cvoid}
    A                                # HipCSR or any operator with mul!
    ctx::Context
    keep::Vector{Any}                # callback boxes: must outlive the handle
    x::Tx
    r::Tx; c::Tx; u::Tx; b::Tx       # keep the vectors alive while the handle uses their pointers
    Pl
    tol::T
    residual::T
    prev_residual::T
    maxiter::Int
    mv_products::Int
end

function refresh!(it::HipCGIterable{T}) where {T}
    res = Ref{Cdouble}(); prev = Ref{Cdouble}(); tol = Ref{Cdouble}(); mx = Ref{Int64}(); mv = Ref{Int64}(); cv = Ref{Cint}()
    check(ccall((:mik_cg_state, libmik), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cdouble}, Ref{Int64}, Ref{Int64}, Ref{Cint}),
                it.handle, res, prev, tol, mx, mv, cv), "mik_cg_state", it.ctx.handle)
    it.residual = T(res[]); it.prev_residual = T(prev[]); it.tol = T(tol[]); it.mv_products = mv[]
    it
end

# ---- any operator / any preconditioner: C callbacks (include/mik.h mik_mul_fn, mik_ldiv_fn) ------------------------------
# `user` carries a pointer to a Julia object that holds the operator and a template vector; the trampolines wrap the raw
# device pointers in non-owning HipVectors and call the ordinary mul! / ldiv! methods, so LinearMaps.jl maps over
# HipVectors, or any struct with mul! / ldiv! methods for HipVector, work unchanged (test/gmres.jl:59-66, :28-35).
struct MikOperator          # same field order and types as the C struct mik_operator
    dtype::Cint
    n::Int64
    csr::Ptr{Cvoid}
    mul::Ptr{Cvoid}
    user::Ptr{Cvoid}
end
struct MikPrecond           # mik_precond
    diag::Ptr{Cvoid}
    ldiv::Ptr{Cvoid}
    user::Ptr{Cvoid}
end
mutable struct CallbackBox{T}
    obj::Any
    n::Int
    ctx::Context
end
unowned(::Type{T}, p::Ptr{Cvoid}, n::Int, ctx::Context) where {T} = HipVector{T}(p, n, ctx, Val(:unowned))
function mul_trampoline(user::Ptr{Cvoid}, x::Ptr{Cvoid}, y::Ptr{Cvoid})::Cint
    box = unsafe_pointer_to_objref(user)::CallbackBox
    T = typeof(box).parameters[1]
    try
        LinearAlgebra.mul!(unowned(T, y, box.n, box.ctx), box.obj, unowned(T, x, box.n, box.ctx))
        return Cint(0)
    catch
        return Cint(1)          # surfaces as MIK_ERR_CALLBACK; never unwind through the C frame
    end
end
function ldiv_trampoline(user::Ptr{Cvoid}, y::Ptr{Cvoid}, x::Ptr{Cvoid})::Cint
    box = unsafe_pointer_to_objref(user)::CallbackBox
    T = typeof(box).parameters[1]
    try
        LinearAlgebra.ldiv!(unowned(T, y, box.n, box.ctx), box.obj, unowned(T, x, box.n, box.ctx))
        return Cint(0)
    catch
        return Cint(1)
    end
end
function operator_struct(A, ::Type{T}, n::Int, ctx::Context, keep::Vector{Any}) where {T}
    A isa HipCSR && return MikOperator(dtype_code(T), n, A.handle, C_NULL, C_NULL)
    if A isa HipDenseMatrix || A isa HipDenseAdjoint             # the library's own callback: no Julia frame per product
        push!(keep, A)
        return dense_operator_struct(A, T, n)
    end
    box = CallbackBox{T}(A, n, ctx); push!(keep, box)
    MikOperator(dtype_code(T), n, C_NULL, @cfunction(mul_trampoline, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), pointer_from_objref(box))
end
function precond_struct(P, ::Type{T}, n::Int, ctx::Context, keep::Vector{Any}) where {T}
    P isa Identity && return nothing
    P isa HipJacobi && return MikPrecond(P.diagonal.ptr, C_NULL, C_NULL)
    if P isa HipLU                                               # the library's own callback: no Julia frame per ldiv!
        push!(keep, P)
        return lu_precond_struct(P, T, n)
    end
    if P isa HipCholesky
        push!(keep, P)
        return chol_precond_struct(P, T, n)
    end
    if P isa HipQR                                               # a square one only
        push!(keep, P)
        return qr_precond_struct(P, T, n)
    end
    box = CallbackBox{T}(P, n, ctx); push!(keep, box)
    MikPrecond(C_NULL, @cfunction(ldiv_trampoline, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid})), pointer_from_objref(box))
end
refptr(::Nothing) = C_NULL
refptr(r::Ref) = Base.unsafe_convert(Ptr{Cvoid}, r)

# cg_iterator!(x, A, b, Pl; ...)  -- src/cg.jl:120-155, specialised on the device vector type: A may be a HipCSR (fully fused
# step) or ANY operator with mul!(::HipVector, A, ::HipVector); Pl Identity(), HipJacobi (fused) or anything with ldiv!.
function IterativeSolvers.cg_iterator!(x::HipVector{T}, A, b::HipVector{T}, Pl = Identity();
        abstol::Real = zero(T), reltol::Real = sqrt(eps(T)), maxiter::Int = size(A, 2),
        statevars::IterativeSolvers.CGStateVariables = IterativeSolvers.CGStateVariables(zero(x), similar(x), similar(x)),
        initially_zero::Bool = false) where {T}
    ctx = x.ctx
    keep = Any[]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if A isa HipCSR && (Pl isa Identity || Pl isa HipJacobi)
        diag = Pl isa HipJacobi ? Pl.diagonal.ptr : C_NULL
        check(ccall((:mik_cg_create, libmik), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Int64, Cint, Ref{Ptr{Cvoid}}),
            ctx.handle, A.handle, x.ptr, b.ptr, statevars.u.ptr, statevars.r.ptr, statevars.c.ptr, diag,
            Float64(abstol), Float64(reltol), maxiter, initially_zero ? 1 : 0, h), "mik_cg_create", ctx.handle)
    else
        op = Ref(operator_struct(A, T, x.n, ctx, keep))
        pl = precond_struct(Pl, T, x.n, ctx, keep)
        plref = pl === nothing ? nothing : Ref(pl)
        GC.@preserve op plref keep check(ccall((:mik_cg_create_op, libmik), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Int64, Cint, Ref{Ptr{Cvoid}}),
            ctx.handle, refptr(op), refptr(plref), x.ptr, b.ptr, statevars.u.ptr, statevars.r.ptr, statevars.c.ptr,
            Float64(abstol), Float64(reltol), maxiter, initially_zero ? 1 : 0, h), "mik_cg_create_op", ctx.handle)
    end
    it = HipCGIterable{T, typeof(x)}(h[], A, ctx, keep, x, statevars.r, statevars.c, statevars.u, b, Pl, zero(T), zero(T), one(T), maxiter, 0)
    finalizer(i -> alive(i.ctx) && ccall((:mik_cg_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), it)
    refresh!(it)
end

IterativeSolvers.converged(it::HipCGIterable) = it.residual ≤ it.tol                      # src/cg.jl:32
IterativeSolvers.start(::HipCGIterable) = 0                                                # src/cg.jl:34
IterativeSolvers.done(it::HipCGIterable, iteration::Int) = iteration ≥ it.maxiter || IterativeSolvers.converged(it)   # :36

# iterate(it, iteration) -- src/cg.jl:43-66 (fused device step; one host-visible residual per call)
function Base.iterate(it::HipCGIterable{T}, iteration::Int = IterativeSolvers.start(it)) where {T}
    res = Ref{Cdouble}(); done = Ref{Cint}()
    check(ccall((:mik_cg_iterate, libmik), Cint, (Ptr{Cvoid}, Int64, Ref{Cdouble}, Ref{Cint}), it.handle, iteration, res, done), "mik_cg_iterate", it.ctx.handle)
    done[] != 0 && return nothing
    it.prev_residual = it.residual
    it.residual = T(res[])
    it.mv_products += 1
    it.residual, iteration + 1
end

"""
    iterate_many!(it, iteration, max_steps) -> Vector{Float64}

Up to `max_steps` `iterate` calls with ONE host synchronisation (`mik_cg_iterate_many`): the stopping test of src/cg.jl:36
runs on the device after every step.  Returns the residuals of the executed steps.
"""
function iterate_many!(it::HipCGIterable{T}, iteration::Int, max_steps::Int) where {T}
    res = Vector{Cdouble}(undef, max(max_steps, 1)); nd = Ref{Int64}(0)
    check(ccall((:mik_cg_iterate_many, libmik), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ref{Int64}), it.handle, iteration, max_steps, res, nd),
          "mik_cg_iterate_many", it.ctx.handle)
    refresh!(it)
    resize!(res, nd[])
end

# ---- GMRESIterable ------------------------------------------------------------------------------
orth_code(::ModifiedGramSchmidt) = Cint(0)
orth_code(::ClassicalGramSchmidt) = Cint(1)
orth_code(::DGKS) = Cint(2)

mutable struct HipResidual{T}      # stands in for g.residual.current read by the driver (src/gmres.jl:51)
    current::T
end
mutable struct HipGMRESIterable{T, Tx<:HipVector{T}}
    handle::Ptr{Cvoid}
    A
    ctx::Context
    keep::Vector{Any}
    x::Tx
    b::Tx
    residual::HipResidual{T}
    mv_products::Int
    restart::Int
    k::Int
    maxiter::Int
    tol::T
    β::T
end

function refresh!(g::HipGMRESIterable{T}) where {T}
    res = Ref{Cdouble}(); tol = Ref{Cdouble}(); beta = Ref{Cdouble}(); k = Ref{Cint}(); mv = Ref{Int64}(); cv = Ref{Cint}()
    check(ccall((:mik_gmres_state, libmik), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cdouble}, Ref{Cint}, Ref{Int64}, Ref{Cint}),
                g.handle, res, tol, beta, k, mv, cv), "mik_gmres_state", g.ctx.handle)
    g.residual.current = T(res[]); g.tol = T(tol[]); g.β = T(beta[]); g.k = k[]; g.mv_products = mv[]
    g
end

# gmres_iterable!(x, A, b; ...) -- src/gmres.jl:108-136; A: HipCSR or any operator with mul!, Pl / Pr: Identity(), HipJacobi or
# anything with ldiv! (all three expand! methods of src/gmres.jl:285-304 run on the device side of the handle)
function IterativeSolvers.gmres_iterable!(x::HipVector{T}, A, b::HipVector{T};
        Pl = Identity(), Pr = Identity(), abstol::Real = zero(T), reltol::Real = sqrt(eps(T)),
        restart::Int = min(20, size(A, 2)), maxiter::Int = size(A, 2), initially_zero::Bool = false,
        orth_meth::OrthogonalizationMethod = ModifiedGramSchmidt()) where {T}
    ctx = x.ctx
    keep = Any[]
    simple(P) = P isa Identity || P isa HipJacobi
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if A isa HipCSR && simple(Pl) && simple(Pr)
        pl = Pl isa HipJacobi ? Pl.diagonal.ptr : C_NULL
        pr = Pr isa HipJacobi ? Pr.diagonal.ptr : C_NULL
        check(ccall((:mik_gmres_create, libmik), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cint, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
            ctx.handle, A.handle, x.ptr, b.ptr, pl, pr, Float64(abstol), Float64(reltol), restart, maxiter, initially_zero ? 1 : 0, orth_code(orth_meth), h),
            "mik_gmres_create", ctx.handle)
    else
        op = Ref(operator_struct(A, T, x.n, ctx, keep))
        pl = precond_struct(Pl, T, x.n, ctx, keep); plref = pl === nothing ? nothing : Ref(pl)
        pr = precond_struct(Pr, T, x.n, ctx, keep); prref = pr === nothing ? nothing : Ref(pr)
        GC.@preserve op plref prref keep check(ccall((:mik_gmres_create_op, libmik), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cint, Int64, Cint, Cint, Ref{Ptr{Cvoid}}),
            ctx.handle, refptr(op), refptr(plref), refptr(prref), x.ptr, b.ptr, Float64(abstol), Float64(reltol), restart, maxiter,
            initially_zero ? 1 : 0, orth_code(orth_meth), h), "mik_gmres_create_op", ctx.handle)
    end
    g = HipGMRESIterable{T, typeof(x)}(h[], A, ctx, keep, x, b, HipResidual{T}(one(T)), 0, restart, 1, maxiter, zero(T), one(T))
    finalizer(i -> alive(i.ctx) && ccall((:mik_gmres_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), g)
    refresh!(g)
end

IterativeSolvers.converged(g::HipGMRESIterable) = g.residual.current ≤ g.tol                  # src/gmres.jl:51
IterativeSolvers.start(::HipGMRESIterable) = 0
IterativeSolvers.done(g::HipGMRESIterable, iteration::Int) = iteration ≥ g.maxiter || IterativeSolvers.converged(g)

# iterate(g, iteration) -- src/gmres.jl:57-106
function Base.iterate(g::HipGMRESIterable{T}, iteration::Int = IterativeSolvers.start(g)) where {T}
    res = Ref{Cdouble}(); done = Ref{Cint}()
    check(ccall((:mik_gmres_iterate, libmik), Cint, (Ptr{Cvoid}, Int64, Ref{Cdouble}, Ref{Cint}), g.handle, iteration, res, done), "mik_gmres_iterate", g.ctx.handle)
    done[] != 0 && return nothing
    refresh!(g)
    g.residual.current, iteration + 1
end

# ---- BiCGStabIterable ---------------------------------------------------------------------------
# bicgstabl!(x, A, b, l; ...) (src/bicgstabl.jl:181-219) calls bicgstabl_iterator!(x, A, b, l; ...) at :197; the reference's
# iterable keeps rs / us as host Matrices (:39-40), so the device path returns its own iterable with the fields the driver
# reads (`mv_products`, `residual`, `x`) and one C call per outer iteration: rho, beta, sigma, alpha, M, gamma, omega stay
# on the device (include/mik.h, mik_bicgstab_step).  `r_shadow` replaces rand(T, n) (:38) when reproducibility is wanted.
mutable struct HipBiCGStabIterable{T, Tx<:HipVector{T}}
    handle::Ptr{Cvoid}
    A::HipCSR{T}
    l::Int
    x::Tx
    r_shadow::Tx
    rs::Tx                 # n x (l + 1), column-major, leading dimension ld
    us::Tx
    ld::Int
    max_mv_products::Int
    mv_products::Int
    tol::T
    residual::T
    Pl
end
# column j (1-based) of a device block: a view, no finalizer
column(block::HipVector{T}, ld::Int, n::Int, j::Int) where {T} = HipVector{T}(block.ptr + (j - 1) * ld * sizeof(T), n, block.ctx, Val(:unowned))

function IterativeSolvers.bicgstabl_iterator!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, l::Int = 2;
        Pl = Identity(), max_mv_products = size(A, 2), abstol::Real = zero(T), reltol::Real = sqrt(eps(T)), initial_zero = false,
        r_shadow::HipVector{T} = HipVector(rand(T, x.n), x.ctx)) where {T}
    (Pl isa Identity || Pl isa HipJacobi) || throw(MikError(Cint(5), "bicgstabl_iterator!", "Pl must be Identity() or HipJacobi on the device path"))
    1 <= l <= 4 || throw(MikError(Cint(5), "bicgstabl_iterator!", "l must be 1 ... 4 on the device path"))
    n = x.n
    ld = cld(n, 64) * 64
    rs = HipVector{T}(undef, ld * (l + 1), x.ctx)                            # :39
    us = fill!(HipVector{T}(undef, ld * (l + 1), x.ctx), zero(T))            # :40
    residual = column(rs, ld, n, 1)
    mv_products = 0
    if initial_zero
        copyto!(residual, b)                                                 # :46
    else
        mul!(residual, A, x)                                                 # :48
        xpby!(b, -one(T), residual)                                          # residual .= b .- residual  :49
        mv_products += 1
    end
    Pl isa HipJacobi && ldiv!(residual, Pl, residual)                        # :55
    nrm = norm(residual)                                                     # :61
    tolerance = max(T(reltol) * nrm, T(abstol))                              # :69
    h = Ref{Ptr{Cvoid}}(C_NULL)
    pl = Pl isa HipJacobi ? Pl.diagonal.ptr : C_NULL
    check(ccall((:mik_bicgstab_create, libmik), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
        x.ctx.handle, A.handle, l, x.ptr, rs.ptr, ld, us.ptr, ld, r_shadow.ptr, pl, h), "mik_bicgstab_create", x.ctx.handle)
    it = HipBiCGStabIterable{T, typeof(x)}(h[], A, l, x, r_shadow, rs, us, ld, Int(max_mv_products), mv_products, tolerance, nrm, Pl)
    finalizer(i -> alive(i.x.ctx) && ccall((:mik_bicgstab_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), it)
    it
end

IterativeSolvers.converged(it::HipBiCGStabIterable) = it.residual ≤ it.tol                    # src/bicgstabl.jl:75
IterativeSolvers.start(::HipBiCGStabIterable) = 0
IterativeSolvers.done(it::HipBiCGStabIterable, iteration::Int) = it.mv_products ≥ it.max_mv_products || IterativeSolvers.converged(it)   # :77

# iterate(it, iteration) -- src/bicgstabl.jl:79-134, one call
function Base.iterate(it::HipBiCGStabIterable{T}, iteration::Int = IterativeSolvers.start(it)) where {T}
    IterativeSolvers.done(it, iteration) && return nothing
    res = Ref{T}()
    code = ccall((:mik_bicgstab_step, libmik), Cint, (Ptr{Cvoid}, Ref{T}), it.handle, res)
    code == 8 && throw(LinearAlgebra.SingularException(0))                   # MIK_ERR_SINGULAR: lu! at :124
    check(code, "mik_bicgstab_step", it.x.ctx.handle)
    it.mv_products += 2 * it.l                                               # :115
    it.residual = res[]                                                      # :132
    it.residual, iteration + 1
end

# ---- MINRESIterable -----------------------------------------------------------------------------
# minres!(x, A, b; ...) (src/minres.jl:197-230) calls minres_iterable!(x, A, b; ...) at :208; MINRESIterable wants DenseVector
# work vectors (:6), so the device path returns its own iterable with the fields the driver reads (`mv_products`, `x`) and one
# C call per iteration (include/mik.h, mik_minres_step): H, rhs and the rotations stay on the device.
mutable struct HipMINRESIterable{T, Tx<:HipVector{T}}
    handle::Ptr{Cvoid}
    A::HipCSR{T}
    skew_hermitian::Bool
    x::Tx
    v_prev::Tx
    v_curr::Tx
    v_next::Tx
    w_prev::Tx
    w_curr::Tx
    w_next::Tx
    mv_products::Int
    maxiter::Int
    tol::T
    resnorm::T
end

function IterativeSolvers.minres_iterable!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T};
        initially_zero::Bool = false, skew_hermitian::Bool = false, abstol::Real = zero(T), reltol::Real = sqrt(eps(T)), maxiter = size(A, 2)) where {T}
    v_prev = similar(x)
    v_curr = copyto!(similar(x), b)                                          # :47-48
    v_next = similar(x)
    w_prev = zero(x); w_curr = zero(x); w_next = zero(x)                     # :51-53 (similar there; zeros here: read only once written)
    mv_products = 0
    if !initially_zero
        mul!(v_next, A, x)                                                   # :60
        axpy!(-one(T), v_next, v_curr)                                       # :61
        mv_products = 1
    end
    resnorm = norm(v_curr)                                                   # :65
    tolerance = max(T(reltol) * resnorm, T(abstol))                          # :66
    rmul!(v_curr, inv(resnorm))                                              # :74
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_minres_create, libmik), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cint, Ref{Ptr{Cvoid}}),
        x.ctx.handle, A.handle, x.ptr, v_prev.ptr, v_curr.ptr, v_next.ptr, w_prev.ptr, w_curr.ptr, w_next.ptr, Float64(resnorm), skew_hermitian ? 1 : 0, h),
        "mik_minres_create", x.ctx.handle)
    m = HipMINRESIterable{T, typeof(x)}(h[], A, skew_hermitian, x, v_prev, v_curr, v_next, w_prev, w_curr, w_next, mv_products, Int(maxiter), tolerance, resnorm)
    finalizer(i -> alive(i.x.ctx) && ccall((:mik_minres_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), m)
    m
end

IterativeSolvers.converged(m::HipMINRESIterable) = m.resnorm ≤ m.tol                          # src/minres.jl:89
IterativeSolvers.start(::HipMINRESIterable) = 1                                                # :91
IterativeSolvers.done(m::HipMINRESIterable, iteration::Int) = iteration > m.maxiter || IterativeSolvers.converged(m)   # :93

# iterate(m, iteration) -- src/minres.jl:95-159, one call
function Base.iterate(m::HipMINRESIterable{T}, iteration::Int = IterativeSolvers.start(m)) where {T}
    IterativeSolvers.done(m, iteration) && return nothing
    res = Ref{T}()
    check(ccall((:mik_minres_step, libmik), Cint, (Ptr{Cvoid}, Int64, Ref{T}), m.handle, iteration, res), "mik_minres_step", m.x.ctx.handle)
    m.v_prev, m.v_curr, m.v_next = m.v_curr, m.v_next, m.v_prev              # :145 (the handle rotates its pointers alike)
    m.w_prev, m.w_curr, m.w_next = m.w_curr, m.w_next, m.w_prev              # :146
    m.resnorm = res[]                                                        # :154
    m.mv_products += 1
    m.resnorm, iteration + 1
end

# ---- IDRSIterable -------------------------------------------------------------------------------
# idrs!(x, A, b; ...) (src/idrs.jl:49-64) calls idrs_method! (:150-162), which calls idrs_iterable!(log, X, A, C, s, Pl, abstol, reltol,
# maxiter; smoothing, verbose) at :156, reduces over it and returns `iterable.X`.  The reference's IDRSIterable keeps P, U, G as Vectors of
# host vectors and its broadcasts would run statement by statement; the device path returns its own iterable with the fields the driver
# reads (`X`, `normR`) and ONE C call per step (include/mik.h, mik_idrs_step): M, f and omega live in the handle.  `P` (a device n x s
# block, leading dimension cld(n, 64) * 64) replaces rand! (:136) when reproducibility is wanted.
mutable struct HipIDRSIterable{T, Tx<:HipVector{T}}
    handle::Ptr{Cvoid}
    A::HipCSR{T}
    s::Int
    X::Tx
    R::Tx
    X_s::Union{Tx, Nothing}
    R_s::Union{Tx, Nothing}
    P::Tx                  # n x s, column-major, leading dimension ld
    U::Tx
    G::Tx
    ld::Int
    maxiter::Int
    smoothing::Bool
    verbose::Bool
    tol::T
    normR::T
    log
    Pl
end

function IterativeSolvers.idrs_iterable!(log, X::HipVector{T}, A::HipCSR{T}, C::HipVector{T}, s::Number, Pl, abstol::Real, reltol::Real,
        maxiter::Number; smoothing::Bool = false, verbose::Bool = false, P::Union{HipVector{T}, Nothing} = nothing) where {T}
    (Pl isa Identity || Pl isa HipJacobi) || throw(MikError(Cint(5), "idrs_iterable!", "Pl must be Identity() or HipJacobi on the device path"))
    1 <= s <= 32 || throw(MikError(Cint(5), "idrs_iterable!", "s must be 1 ... 32 on the device path"))
    n = X.n
    ld = cld(n, 64) * 64
    R = similar(X)
    mul!(R, A, X)                                                            # R = C - A*X  :119
    xpby!(C, -one(T), R)
    normR = norm(R)                                                          # :120
    tolerance = max(T(reltol) * normR, T(abstol))                            # :121
    X_s = smoothing ? copyto!(similar(X), X) : nothing                       # :123-126
    R_s = smoothing ? copyto!(similar(X), R) : nothing
    if P === nothing                                                         # :136
        Ph = zeros(T, ld * Int(s))
        for k in 1:Int(s)
            Ph[(k - 1) * ld + 1:(k - 1) * ld + n] = rand(T, n)
        end
        P = HipVector(Ph, X.ctx)
    end
    (P.n >= ld * Int(s) && P.ctx === X.ctx) || throw(MikError(Cint(3), "idrs_iterable!", "P must hold ld * s = $(ld * Int(s)) entries (column-major, leading dimension $ld) on X's context"))
    U = fill!(HipVector{T}(undef, ld * Int(s), X.ctx), zero(T))              # :137
    G = fill!(HipVector{T}(undef, ld * Int(s), X.ctx), zero(T))              # :138
    h = Ref{Ptr{Cvoid}}(C_NULL)
    pl = Pl isa HipJacobi ? Pl.diagonal.ptr : C_NULL
    check(ccall((:mik_idrs_create, libmik), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
         Cdouble, Ref{Ptr{Cvoid}}),
        X.ctx.handle, A.handle, s, X.ptr, R.ptr, P.ptr, ld, U.ptr, ld, G.ptr, ld, pl, smoothing ? X_s.ptr : C_NULL, smoothing ? R_s.ptr : C_NULL,
        Float64(normR), h), "mik_idrs_create", X.ctx.handle)
    it = HipIDRSIterable{T, typeof(X)}(h[], A, Int(s), X, R, X_s, R_s, P, U, G, ld, Int(maxiter), smoothing, verbose, tolerance, normR, log, Pl)
    finalizer(i -> alive(i.X.ctx) && ccall((:mik_idrs_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), it)
    it
end

# iterate(it, (iter, step)) -- src/idrs.jl:164-272, one call per step
function Base.iterate(it::HipIDRSIterable{T}, (iter, step) = (1, 1)) where {T}
    if it.normR < it.tol || iter > it.maxiter                                # :168
        it.log !== nothing && IterativeSolvers.setconv(it.log, 0 <= it.normR < it.tol)
        it.smoothing && copyto!(it.X, it.X_s)                                # :171-173
        return nothing
    end
    res = Ref{T}()
    check(ccall((:mik_idrs_step, libmik), Cint, (Ptr{Cvoid}, Cint, Ref{T}), it.handle, step, res), "mik_idrs_step", it.X.ctx.handle)
    it.normR = res[]
    nextstep = step <= it.s ? step + 1 : 1                                   # :240, :267
    if it.log !== nothing
        IterativeSolvers.nextiter!(it.log, mvps = 1)                         # :268-269
        push!(it.log, :resnorm, it.normR)
    end
    it.normR, (iter + 1, nextstep)
end

# zerox(A, b) (src/common.jl:18-23) already works: similar(b, T, size(A, 2)) + fill! are defined above.

# ------------------------------------------------------------------------------------------------
# gmres! over a row partition (one process per GPU): include/mik.h `mik_partition`
# ------------------------------------------------------------------------------------------------
# The handle calls back for the two couplings between ranks -- or, with `link` set, exchanges by itself on the device (Transport 3: no
# host round trip inside an Arnoldi column); everything else is the iterable above.
#   halo(user)::Cint                      -- send_buf is packed (stream-ordered); fill x_ext[n_loc+1:n_ext]
#   reduce(user, dtype, count, values)    -- partial sums in, ((p0 + p1) + p2) + ... in rank order out
struct Partition                     # same field order and types as the C struct
    rank::Cint
    nranks::Cint
    n_ext::Int64
    x_ext::Ptr{Cvoid}
    send_idx::Ptr{Int32}
    n_send::Int64
    send_buf::Ptr{Cvoid}
    halo::Ptr{Cvoid}                 # @cfunction(halo_cb, Cint, (Ptr{Cvoid},))
    reduce::Ptr{Cvoid}               # @cfunction(reduce_cb, Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Cvoid}))
    user::Ptr{Cvoid}
    link::Ptr{Cvoid}                 # C_NULL: the callbacks couple the ranks; a connected PartitionLink's handle: the library does, on the device
end

"""
    gmres_iterable_partitioned!(x, A_loc, b, part; n_global, kwargs...)

`A_loc` is this rank's `n_loc x n_ext` block (halo columns behind the owned ones), `x`, `b` its rows.  Returns the same
`HipGMRESIterable`; drive it with `iterate` / `gmres!`-style loops on every rank in lockstep.  Defaults are those of
`gmres_iterable!` (src/gmres.jl:108-117) evaluated on the GLOBAL size: `restart = min(20, n_global)`,
`maxiter = n_global`, `orth_meth = ModifiedGramSchmidt()` -- switching a solve to the partitioned call does not change
its result.  (ClassicalGramSchmidt() needs one reduction per step instead of k: pass it explicitly at scale.)
"""
function gmres_iterable_partitioned!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, part::Partition; n_global::Int, Pl = Identity(), Pr = Identity(),
        abstol::Real = zero(real(T)), reltol::Real = sqrt(eps(real(T))), restart::Int = min(20, n_global), maxiter::Int = n_global,
        initially_zero::Bool = false, orth_meth::OrthogonalizationMethod = ModifiedGramSchmidt()) where {T}
    all(P -> P isa Identity || P isa HipJacobi, (Pl, Pr)) || throw(MikError(Cint(5), "gmres_iterable_partitioned!", "Pl / Pr must be Identity() or HipJacobi"))
    pl = Pl isa HipJacobi ? Pl.diagonal.ptr : C_NULL
    pr = Pr isa HipJacobi ? Pr.diagonal.ptr : C_NULL
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_gmres_create_partitioned, libmik), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cdouble, Cdouble, Cint, Int64, Cint, Cint, Ref{Partition}, Ref{Ptr{Cvoid}}),
        A.ctx.handle, A.handle, x.ptr, b.ptr, pl, pr, Float64(abstol), Float64(reltol), restart, maxiter, initially_zero ? 1 : 0,
        orth_code(orth_meth), Ref(part), h), "mik_gmres_create_partitioned", A.ctx.handle)
    g = HipGMRESIterable{T, typeof(x)}(h[], A, A.ctx, Any[], x, b, HipResidual{T}(one(T)), 0, restart, 1, maxiter, zero(T), one(T))
    finalizer(i -> alive(i.ctx) && ccall((:mik_gmres_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), g)
    refresh!(g)
end

# ------------------------------------------------------------------------------------------------
# cg! over a row partition, exchanges inside libmik.so (include/mik.h "Transport 1": RCCL over xGMI, one process per GPU)
# ------------------------------------------------------------------------------------------------
"RCCL communicator owned by libmik.so.  `id` = the 128 bytes of `unique_id()` made on rank 0 and broadcast by the host (MPI.jl)."
mutable struct Comm
    handle::Ptr{Cvoid}
    ctx::Context
end
function unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:mik_comm_unique_id, libmik), Cint, (Ptr{UInt8},), id), "mik_comm_unique_id")
    id
end
function Comm(ctx::Context, id::Union{Nothing, Vector{UInt8}}, rank::Integer, nranks::Integer)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve id check(ccall((:mik_comm_create, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint, Ref{Ptr{Cvoid}}),
                                ctx.handle, id === nothing ? C_NULL : pointer(id), rank, nranks, h), "mik_comm_create", ctx.handle)
    c = Comm(h[], ctx)
    finalizer(x -> alive(x.ctx) && ccall((:mik_comm_destroy, libmik), Cint, (Ptr{Cvoid},), x.handle), c)
    c
end

# Transport 3 (include/mik.h): peer-mapped mailboxes -- no collective launch in the step.  `allgather` is whatever the host has for
# small byte vectors (MPI.Allgather!): it carries the 64-byte HIP IPC handles once.
"64-byte HIP IPC handle of this communicator's mailbox (mik_comm_mailbox_export)"
function mailbox_handle(c::Comm)
    h = zeros(UInt8, 64)
    check(ccall((:mik_comm_mailbox_export, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}), c.handle, h), "mik_comm_mailbox_export", c.ctx.handle)
    h
end
"every rank's mailbox handle, rank order, 64 bytes each (mik_comm_mailbox_connect; collective)"
function connect_mailboxes!(c::Comm, handles::Vector{UInt8})
    GC.@preserve handles check(ccall((:mik_comm_mailbox_connect, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}), c.handle, handles), "mik_comm_mailbox_connect", c.ctx.handle)
    c
end
"""
The device-driven links of one row partition on a communicator whose mailboxes are connected (include/mik.h `mik_plink`): halo plan,
landing buffer, peer mappings.  `recv` / `send`: (peer, offset, count) segments of the ghost region / of the packed send buffer.
`allgather(x)` is whatever the host has for small host objects (MPI.Allgather of the 64-byte handle, the ghost count and the receive
segments of every rank); `PartitionLink(...)` is collective.  Its `handle` goes into `Partition.link`.
"""
mutable struct PartitionLink
    handle::Ptr{Cvoid}
    comm::Comm
end
function PartitionLink(comm::Comm, ::Type{T}, n_ghost::Integer, recv::Vector{NTuple{3, Int}}, send::Vector{NTuple{3, Int}}, rank::Integer, allgather) where {T<:MikFloat}
    rp = Cint[p for (p, _, _) in recv]; ro = Int64[o for (_, o, _) in recv]; rc = Int64[k for (_, _, k) in recv]
    sp = Cint[p for (p, _, _) in send]; so = Int64[o for (_, o, _) in send]; sc = Int64[k for (_, _, k) in send]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_plink_create, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Cint}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Cint}, Ptr{Int64}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
                comm.handle, dtype_code(T), n_ghost, length(rp), rp, ro, rc, length(sp), sp, so, sc, h), "mik_plink_create", comm.ctx.handle)
    mine = zeros(UInt8, 64)
    check(ccall((:mik_plink_export, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], mine), "mik_plink_export", comm.ctx.handle)
    info = allgather((mine, Int64(n_ghost), recv))                       # per rank: (handle, ghost count, receive segments)
    handles = reduce(vcat, [i[1] for i in info]); counts = Int64[i[2] for i in info]
    dst = landing_targets(send, info, rank)
    GC.@preserve handles counts dst check(ccall((:mik_plink_connect, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Ptr{Int64}), h[], handles, counts, dst),
                                          "mik_plink_connect", comm.ctx.handle)
    l = PartitionLink(h[], comm)
    finalizer(x -> alive(x.comm.ctx) && ccall((:mik_plink_destroy, libmik), Cint, (Ptr{Cvoid},), x.handle), l)
    l
end
"per SEND segment: the offset of the matching receive segment in the receiver's ghost region (info[q][3] = rank q's receive segments)"
function landing_targets(send, info, rank)
    taken = Dict{Int, Int}(); dst = Int64[]
    for (peer, _, cnt) in send
        cands = [sg for sg in info[peer + 1][3] if sg[1] == rank]
        k = get(taken, peer, 0) + 1; taken[peer] = k
        (k <= length(cands) && cands[k][3] == cnt) || throw(MikError(Cint(3), "landing_targets", "halo plans of ranks $rank and $peer disagree"))
        push!(dst, cands[k][2])
    end
    isempty(dst) ? Int64[0] : dst
end

"Row-partitioned CGIterable: this rank's block, the halo plan and the communicator; `iterate_many!` is ONE ccall per batch."
mutable struct HipDistCG{T}
    handle::Ptr{Cvoid}
    ctx::Context
    keep::Vector{Any}
    residual::Float64
    tol::Float64
    maxiter::Int
end
function dist_cg_iterator!(x::HipVector{T}, A_loc::HipCSR{T}, b::HipVector{T}, comm::Comm, rank::Integer, nranks::Integer;
        send_idx::Vector{Int32}, recv::Vector{NTuple{3, Int}}, send::Vector{NTuple{3, Int}},        # (peer, offset, count)
        abstol::Real = 0.0, reltol::Real = sqrt(eps(T)), maxiter::Int, initially_zero::Bool = true,
        u_ext::Union{Nothing, HipVector{T}} = nothing, ghosts = nothing) where {T}
    ctx = x.ctx
    n_loc, n_ext = size(A_loc)
    u_ext = u_ext === nothing ? fill!(HipVector{T}(undef, n_ext, ctx), 0) : u_ext
    r = similar(x); c = similar(x)
    sbuf = HipVector{T}(undef, max(length(send_idx), 1), ctx)
    dot_all = fill!(HipVector{T}(undef, nranks, ctx), 0); rr_all = fill!(HipVector{T}(undef, nranks, ctx), 0)
    sidx = HipVector{Float32}(undef, max(length(send_idx), 1), ctx)      # 4-byte slots: holds the Int32 indices
    isempty(send_idx) || GC.@preserve send_idx check(ccall((:mik_memcpy_h2d, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                                                           ctx.handle, sidx.ptr, pointer(send_idx), sizeof(send_idx)), "mik_memcpy_h2d", ctx.handle)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_cgd_create, libmik), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint,
         Cdouble, Cdouble, Int64, Cint, Ref{Ptr{Cvoid}}),
        ctx.handle, A_loc.handle, x.ptr, b.ptr, u_ext.ptr, r.ptr, c.ptr, sidx.ptr, length(send_idx), sbuf.ptr, dot_all.ptr, rr_all.ptr, rank, nranks,
        Float64(abstol), Float64(reltol), maxiter, initially_zero ? 1 : 0, h), "mik_cgd_create", ctx.handle)
    rp = Cint[p for (p, _, _) in recv]; ro = Int64[o for (_, o, _) in recv]; rc = Int64[k for (_, _, k) in recv]
    sp = Cint[p for (p, _, _) in send]; so = Int64[o for (_, o, _) in send]; sc = Int64[k for (_, _, k) in send]
    check(ccall((:mik_cgd_set_halo_plan, libmik), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Cint}, Ptr{Int64}, Ptr{Int64}),
                h[], length(rp), rp, ro, rc, length(sp), sp, so, sc), "mik_cgd_set_halo_plan", ctx.handle)
    check(ccall((:mik_cgd_set_comm, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h[], comm.handle), "mik_cgd_set_comm", ctx.handle)
    if ghosts !== nothing
        # transport 3, halo pushed into the neighbours' landing buffers: ghosts = allgather (as for PartitionLink).  Every rank exports the
        # landing buffer the library allocated for its plan, the host gathers (handle, ghost count, receive segments) of every rank
        mine = zeros(UInt8, 64)
        check(ccall((:mik_cgd_ghost_export, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}), h[], mine), "mik_cgd_ghost_export", ctx.handle)
        info = ghosts((mine, Int64(n_ext - n_loc), recv))
        gh = reduce(vcat, [i[1] for i in info]); gcnt = Int64[i[2] for i in info]; gdst = landing_targets(send, info, rank)
        GC.@preserve gh gcnt gdst check(ccall((:mik_cgd_connect_ghosts, libmik), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Ptr{Int64}), h[], gh, gcnt, gdst),
                                        "mik_cgd_connect_ghosts", ctx.handle)
    end
    res = Ref{Cdouble}(); tol = Ref{Cdouble}()
    check(ccall((:mik_cgd_init, libmik), Cint, (Ptr{Cvoid}, Ref{Cdouble}, Ref{Cdouble}), h[], res, tol), "mik_cgd_init", ctx.handle)
    it = HipDistCG{T}(h[], ctx, Any[x, b, u_ext, r, c, sbuf, dot_all, rr_all, sidx, A_loc, comm], res[], tol[], maxiter)
    finalizer(i -> alive(i.ctx) && ccall((:mik_cgd_destroy, libmik), Cint, (Ptr{Cvoid},), i.handle), it)
    it
end
"(runs, rows, merged) -- the contiguous row runs a rank updates, packs and puts on the wire ahead of the sweep over u (0 runs: the halo follows the sweep)"
function halo_early(it::HipDistCG)
    runs = Ref{Cint}(0); rows = Ref{Int64}(0); merged = Ref{Cint}(0)
    check(ccall((:mik_cgd_halo_early, libmik), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}, Ref{Cint}), it.handle, runs, rows, merged), "mik_cgd_halo_early", it.ctx.handle)
    (Int(runs[]), Int(rows[]), merged[] != 0)
end
function iterate_many!(it::HipDistCG, iteration::Int, max_steps::Int)
    res = Vector{Cdouble}(undef, max(max_steps, 1)); nd = Ref{Int64}(0)
    check(ccall((:mik_cgd_iterate_many, libmik), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ref{Int64}), it.handle, iteration, max_steps, res, nd),
          "mik_cgd_iterate_many", it.ctx.handle)
    resize!(res, nd[])
    isempty(res) || (it.residual = res[end])
    res
end

"""
orthogonalize_and_normalize!(V::Vector{Vector}, w, h, ModifiedGramSchmidt()) -- src/orthogonalize.jl:53-65 -- for a basis kept as
separate device vectors: one C call, same arithmetic and bits as the matrix method (mik_orthogonalize_vectors).
"""
function IterativeSolvers.orthogonalize_and_normalize!(V::Vector{HipVector{T}}, w::HipVector{T}, h::AbstractVector{T},
                                                       ::IterativeSolvers.ModifiedGramSchmidt) where {T<:MikFloat}
    k = length(V)
    ptrs = Ptr{Cvoid}[v.ptr for v in V]
    hh = Vector{T}(undef, max(k, 1))
    nrm = Ref{T}(zero(T))
    GC.@preserve V ptrs hh check(ccall((:mik_orthogonalize_vectors, libmik), Cint,
        (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{T}, Ref{T}),
        w.ctx.handle, dtype_code(T), w.n, k, ptrs, w.ptr, hh, nrm), "mik_orthogonalize_vectors", w.ctx.handle)
    copyto!(h, 1, hh, 1, k)
    nrm[]
end

# ---- stationary methods: jacobi / gauss_seidel / sor / ssor on a HipCSR (src/stationary_sparse.jl) ------------------------------
# DiagonalIndices + the level schedules of both triangular sweeps (mik_stationary_create); every building block one C call whose rows
# are summed in the order of the reference's column loops, so the iterates are the reference's bits.
mutable struct HipStationary{T}
    handle::Ptr{Cvoid}
    A::HipCSR{T}                     # read at creation; kept alive with the handle
    ctx::Context
end
function HipStationary(A::HipCSR{T}) where {T}
    h = Ref{Ptr{Cvoid}}(C_NULL); col = Ref{Int64}(0)
    code = ccall((:mik_stationary_create, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}, Ref{Ptr{Cvoid}}), A.ctx.handle, A.handle, col, h)
    code == 8 && throw(LinearAlgebra.SingularException(Int(col[])))             # DiagonalIndices, src/stationary_sparse.jl:19
    check(code, "mik_stationary_create", A.ctx.handle)
    S = HipStationary{T}(h[], A, A.ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_stationary_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), S)
    S
end
function diag_ldiv!(y::HipVector{T}, S::HipStationary{T}, x::HipVector{T}) where {T}                       # ldiv!(y, D, x)  :30-35
    check(ccall((:mik_diag_ldiv, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), S.handle, y.ptr, x.ptr), "mik_diag_ldiv", S.ctx.handle)
    y
end
function offdiag_mul!(α::T, S::HipStationary{T}, x::HipVector{T}, β::T, y::HipVector{T}) where {T}      # mul!(α, O, x, β, y)  :148-171
    check(ccall((:mik_offdiag_mul, libmik), Cint, (Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}), S.handle, α, x.ptr, β, y.ptr),
          "mik_offdiag_mul", S.ctx.handle)
    y
end
# gauss_seidel_multiply!(α, U | L, x, β, y, z) -- :178-191 / :196-208; z may be x
function gs_multiply!(upper::Bool, α::T, S::HipStationary{T}, x::HipVector{T}, β::T, y::HipVector{T}, z::HipVector{T}) where {T}
    check(ccall((:mik_gs_multiply, libmik), Cint, (Ptr{Cvoid}, Cint, Ref{T}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ptr{Cvoid}),
                S.handle, upper, α, x.ptr, β, y.ptr, z.ptr), "mik_gs_multiply", S.ctx.handle)
    z
end
# forward_sub!(L, x) / backward_sub!(U, x) (ω === nothing), or the relaxed forms with α = ω, β = one(T) - ω in Julia's promotion:
# Float32 data with a Float64 ω evaluate α*x/d + β*y in Float64 (scalar dtype MIK_F64)
function triangular_sub!(upper::Bool, S::HipStationary{T}, x::HipVector{T}, ω, y) where {T}
    if ω === nothing
        check(upper ? ccall((:mik_backward_sub, libmik), Cint, (Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Cint), S.handle, zero(T), x.ptr, zero(T), C_NULL, dtype_code(T)) :
                      ccall((:mik_forward_sub, libmik), Cint, (Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Ref{T}, Ptr{Cvoid}, Cint), S.handle, zero(T), x.ptr, zero(T), C_NULL, dtype_code(T)),
              upper ? "mik_backward_sub" : "mik_forward_sub", S.ctx.handle)
        return x
    end
    R = promote_type(T, typeof(ω))
    R <: MikFloat || throw(ArgumentError("ω of type $(typeof(ω)) on $(T) data: the device computes in Float32 / Float64"))
    α = convert(R, ω); β = convert(R, one(T) - ω)
    check(upper ? ccall((:mik_backward_sub, libmik), Cint, (Ptr{Cvoid}, Ref{R}, Ptr{Cvoid}, Ref{R}, Ptr{Cvoid}, Cint), S.handle, α, x.ptr, β, y.ptr, dtype_code(R)) :
                  ccall((:mik_forward_sub, libmik), Cint, (Ptr{Cvoid}, Ref{R}, Ptr{Cvoid}, Ref{R}, Ptr{Cvoid}, Cint), S.handle, α, x.ptr, β, y.ptr, dtype_code(R)),
          upper ? "mik_backward_sub" : "mik_forward_sub", S.ctx.handle)
    x
end
"levels and launches per triangular sweep (forward, backward), device bytes, analysis milliseconds"
function stationary_info(S::HipStationary)
    lv = zeros(Int64, 2); la = zeros(Int64, 2); b = Ref{Int64}(0); ms = Ref{Cdouble}(0)
    check(ccall((:mik_stationary_info, libmik), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{Cdouble}), S.handle, lv, la, b, ms),
          "mik_stationary_info", S.ctx.handle)
    (levels = (lv[1], lv[2]), launches = (la[1], la[2]), bytes = b[], analysis_ms = ms[])
end

mutable struct HipJacobiIterable{T}                      # JacobiIterable  :213-221
    O::HipStationary{T}
    x::HipVector{T}
    next::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
mutable struct HipGaussSeidelIterable{T}                 # GaussSeidelIterable  :261-269
    S::HipStationary{T}
    x::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
mutable struct HipSORIterable{T, numT<:Real}             # SORIterable  :308-318
    S::HipStationary{T}
    ω::numT
    x::HipVector{T}
    next::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
mutable struct HipSSORIterable{T, numT<:Real}            # SSORIterable  :366-376
    S::HipStationary{T}
    ω::numT
    x::HipVector{T}
    tmp::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
const HipStationaryIterable = Union{HipJacobiIterable, HipGaussSeidelIterable, HipSORIterable, HipSSORIterable}

IterativeSolvers.jacobi_iterable(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}; maxiter::Int = 10) where {T} =
    HipJacobiIterable{T}(HipStationary(A), x, similar(x), b, maxiter)
IterativeSolvers.gauss_seidel_iterable(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}; maxiter::Int = 10) where {T} =
    HipGaussSeidelIterable{T}(HipStationary(A), x, b, maxiter)
IterativeSolvers.sor_iterable(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T} =
    HipSORIterable{T, typeof(ω)}(HipStationary(A), ω, x, similar(x), b, maxiter)
IterativeSolvers.ssor_iterable(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T} =
    HipSSORIterable{T, typeof(ω)}(HipStationary(A), ω, x, similar(x), b, maxiter)

function Base.iterate(j::HipJacobiIterable{T}, iteration::Int = 1) where {T}                              # :225-234
    iteration > j.maxiter && return nothing
    copyto!(j.next, j.b)
    offdiag_mul!(-one(T), j.O, j.x, one(T), j.next)
    diag_ldiv!(j.x, j.O, j.next)
    nothing, iteration + 1
end
function Base.iterate(g::HipGaussSeidelIterable{T}, iteration::Int = 1) where {T}                         # :278-288
    iteration > g.maxiter && return nothing
    gs_multiply!(true, -one(T), g.S, g.x, one(T), g.b, g.x)
    triangular_sub!(false, g.S, g.x, nothing, nothing)
    nothing, iteration + 1
end
function Base.iterate(s::HipSORIterable{T}, iteration::Int = 1) where {T}                                 # :322-336
    iteration > s.maxiter && return nothing
    gs_multiply!(true, -one(T), s.S, s.x, one(T), s.b, s.next)                  # next = b - U * x
    triangular_sub!(false, s.S, s.next, s.ω, s.x)                               # next = ω * inv(L) * next + (1 - ω) * x
    s.x, s.next = s.next, s.x                                                   # switch current and next iterate
    nothing, iteration + 1
end
function Base.iterate(s::HipSSORIterable{T}, iteration::Int = 1) where {T}                                # :392-418
    iteration > s.maxiter && return nothing
    gs_multiply!(true, -one(T), s.S, s.x, one(T), s.b, s.tmp)                   # tmp = b - U * x
    triangular_sub!(false, s.S, s.tmp, s.ω, s.x)                                # tmp = ω * inv(L) * tmp + (1 - ω) * x
    gs_multiply!(false, -one(T), s.S, s.tmp, one(T), s.b, s.x)                  # x = b - L * tmp
    triangular_sub!(true, s.S, s.x, s.ω, s.tmp)                                 # x = ω * inv(U) * x + (1 - ω) * tmp
    nothing, iteration + 1
end
Base.length(it::HipStationaryIterable) = it.maxiter

# jacobi! / gauss_seidel! / sor! / ssor! return iterable.x (:251-255, :298-302, :356-360, :422-426): for sor! after an odd maxiter the
# internal buffer, the caller's x then holding iterate maxiter - 1
function IterativeSolvers.jacobi!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}; maxiter::Int = 10) where {T}
    iterable = IterativeSolvers.jacobi_iterable(x, A, b, maxiter = maxiter)
    for item = iterable end
    iterable.x
end
function IterativeSolvers.gauss_seidel!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}; maxiter::Int = 10) where {T}
    iterable = IterativeSolvers.gauss_seidel_iterable(x, A, b, maxiter = maxiter)
    for item = iterable end
    iterable.x
end
function IterativeSolvers.sor!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T}
    iterable = IterativeSolvers.sor_iterable(x, A, b, ω, maxiter = maxiter)
    for item = iterable end
    iterable.x
end
function IterativeSolvers.ssor!(x::HipVector{T}, A::HipCSR{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T}
    iterable = IterativeSolvers.ssor_iterable(x, A, b, ω, maxiter = maxiter)
    for item = iterable end
    iterable.x
end
# the non-! forms start from zerox(A, b) (src/stationary.jl:19, :79, :136, :195)
IterativeSolvers.jacobi(A::HipCSR{T}, b::HipVector{T}; kwargs...) where {T} = IterativeSolvers.jacobi!(IterativeSolvers.zerox(A, b), A, b; kwargs...)
IterativeSolvers.gauss_seidel(A::HipCSR{T}, b::HipVector{T}; kwargs...) where {T} = IterativeSolvers.gauss_seidel!(IterativeSolvers.zerox(A, b), A, b; kwargs...)
IterativeSolvers.sor(A::HipCSR{T}, b::HipVector{T}, ω::Real; kwargs...) where {T} = IterativeSolvers.sor!(IterativeSolvers.zerox(A, b), A, b, ω; kwargs...)
IterativeSolvers.ssor(A::HipCSR{T}, b::HipVector{T}, ω::Real; kwargs...) where {T} = IterativeSolvers.ssor!(IterativeSolvers.zerox(A, b), A, b, ω; kwargs...)

# ---- dense stationary methods: jacobi / gauss_seidel / sor / ssor on a dense device matrix (src/stationary.jl) --------------------
# A device n x cols column-major matrix (leading dimension padded to a multiple of 64 elements), uploaded from a Matrix.
mutable struct HipDenseMatrix{T<:MikFloat}
    ptr::Ptr{Cvoid}
    n::Int
    cols::Int
    ld::Int
    ctx::Context
end
function HipDenseMatrix(a::Matrix{T}, ctx::Context = context()) where {T<:MikFloat}
    n, cols = size(a)
    ld = max(64, cld(n, 64) * 64)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_malloc, libmik), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), ctx.handle, ld * max(cols, 1) * sizeof(T), p), "mik_malloc", ctx.handle)
    m = HipDenseMatrix{T}(p[], n, cols, ld, ctx)
    finalizer(x -> alive(x.ctx) && ccall((:mik_free, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.handle, x.ptr), m)
    padded = zeros(T, ld, cols)
    padded[1:n, :] .= a
    GC.@preserve padded check(ccall((:mik_memcpy_h2d, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t),
                                    ctx.handle, m.ptr, pointer(padded), sizeof(padded)), "mik_memcpy_h2d", ctx.handle)
    m
end
Base.size(m::HipDenseMatrix) = (m.n, m.cols)
Base.size(m::HipDenseMatrix, d::Integer) = d == 1 ? m.n : (d == 2 ? m.cols : 1)
Base.eltype(::HipDenseMatrix{T}) where {T} = T
IterativeSolvers.zerox(A::HipDenseMatrix{T}, b::HipVector{T}) where {T} = fill!(HipVector{T}(undef, size(A, 2), b.ctx), zero(T))

struct DensePlan                     # same field order and types as the C struct mik_dense_plan
    form::Cint                       # 0 auto, 1 panel, 2 chained (not built: refused)
    spin_limit::Cint
end
# check_diag (src/stationary.jl:6-12) + the work vectors of the four iterations (mik_dense_stationary_create); one C call per iteration
mutable struct HipDenseStationary{T}
    handle::Ptr{Cvoid}
    A::HipDenseMatrix{T}             # read at every step; kept alive with the handle
    ctx::Context
end
function HipDenseStationary(A::HipDenseMatrix{T}; form::Integer = 0, spin_limit::Integer = 0) where {T}
    size(A, 1) == size(A, 2) || throw(DimensionMismatch("the matrix is $(size(A, 1)) x $(size(A, 2)), not square"))
    h = Ref{Ptr{Cvoid}}(C_NULL); col = Ref{Int64}(0)
    code = ccall((:mik_dense_stationary_create, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ref{DensePlan}, Ref{Int64}, Ref{Ptr{Cvoid}}),
                 A.ctx.handle, A.ptr, A.n, A.ld, dtype_code(T), DensePlan(form, spin_limit), col, h)
    code == 8 && throw(LinearAlgebra.SingularException(Int(col[])))             # check_diag, src/stationary.jl:9
    check(code, "mik_dense_stationary_create", A.ctx.handle)
    S = HipDenseStationary{T}(h[], A, A.ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_dense_stationary_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), S)
    S
end
"panel width, rows per workgroup, launches of one forward substitution, form in use, whether a chained launch gave up, device bytes"
function dense_stationary_info(S::HipDenseStationary)
    w = Ref{Int64}(0); r = Ref{Int64}(0); la = Ref{Int64}(0); form = Ref{Cint}(0); gave_up = Ref{Cint}(0); b = Ref{Int64}(0)
    check(ccall((:mik_dense_stationary_info, libmik), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Cint}, Ref{Cint}, Ref{Int64}),
                S.handle, w, r, la, form, gave_up, b), "mik_dense_stationary_info", S.ctx.handle)
    (W = w[], R = r[], launches_forward = la[], form = Int(form[]), gave_up = gave_up[] != 0, bytes = b[])
end
# ω in Julia's promotion: Float32 data with a Float64 ω evaluate x + ω * (tmp / d - x) in Float64 (scalar dtype MIK_F64); an Int ω stays in T
function dense_omega(::Type{T}, ω::Real) where {T}
    R = promote_type(T, typeof(ω))
    R <: MikFloat || throw(ArgumentError("ω of type $(typeof(ω)) on $(T) data: the device computes in Float32 / Float64"))
    convert(R, ω)
end

mutable struct HipDenseJacobiIterable{T}                 # DenseJacobiIterable  :38-44
    A::HipDenseStationary{T}
    x::HipVector{T}
    next::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
mutable struct HipDenseGaussSeidelIterable{T}            # DenseGaussSeidelIterable  :98-103
    A::HipDenseStationary{T}
    x::HipVector{T}
    b::HipVector{T}
    maxiter::Int
end
mutable struct HipDenseSORIterable{T, numT<:Real}        # DenseSORIterable  :156-163
    A::HipDenseStationary{T}
    x::HipVector{T}
    tmp::HipVector{T}
    b::HipVector{T}
    ω::numT
    maxiter::Int
end
mutable struct HipDenseSSORIterable{T, numT<:Real}       # DenseSSORIterable  :216-223
    A::HipDenseStationary{T}
    x::HipVector{T}
    tmp::HipVector{T}
    b::HipVector{T}
    ω::numT
    maxiter::Int
end
const HipDenseStationaryIterable = Union{HipDenseJacobiIterable, HipDenseGaussSeidelIterable, HipDenseSORIterable, HipDenseSSORIterable}

function Base.iterate(j::HipDenseJacobiIterable{T}, iteration::Int = 1) where {T}                         # :48-72
    iteration > j.maxiter && return nothing
    check(ccall((:mik_dense_jacobi_step, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), j.A.handle, j.x.ptr, j.next.ptr, j.b.ptr),
          "mik_dense_jacobi_step", j.A.ctx.handle)
    nothing, iteration + 1
end
function Base.iterate(s::HipDenseGaussSeidelIterable{T}, iteration::Int = 1) where {T}                    # :108-129
    iteration > s.maxiter && return nothing
    check(ccall((:mik_dense_gs_step, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), s.A.handle, s.x.ptr, s.b.ptr), "mik_dense_gs_step", s.A.ctx.handle)
    nothing, iteration + 1
end
function Base.iterate(s::HipDenseSORIterable{T}, iteration::Int = 1) where {T}                            # :167-188
    iteration > s.maxiter && return nothing
    ω = dense_omega(T, s.ω); R = typeof(ω)
    check(ccall((:mik_dense_sor_step, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{R}, Cint),
                s.A.handle, s.x.ptr, s.tmp.ptr, s.b.ptr, ω, dtype_code(R)), "mik_dense_sor_step", s.A.ctx.handle)
    nothing, iteration + 1
end
function Base.iterate(s::HipDenseSSORIterable{T}, iteration::Int = 1) where {T}                           # :227-263
    iteration > s.maxiter && return nothing
    ω = dense_omega(T, s.ω); R = typeof(ω)
    check(ccall((:mik_dense_ssor_step, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{R}, Cint),
                s.A.handle, s.x.ptr, s.tmp.ptr, s.b.ptr, ω, dtype_code(R)), "mik_dense_ssor_step", s.A.ctx.handle)
    nothing, iteration + 1
end
Base.length(it::HipDenseStationaryIterable) = it.maxiter

# jacobi! / gauss_seidel! / sor! / ssor! (:31-36, :91-96, :149-154, :209-214): check_diag once, exactly maxiter iterations, x in place
function IterativeSolvers.jacobi!(x::HipVector{T}, A::HipDenseMatrix{T}, b::HipVector{T}; maxiter::Int = 10) where {T}
    iterable = HipDenseJacobiIterable{T}(HipDenseStationary(A), x, similar(x), b, maxiter)
    for item = iterable end
    x
end
function IterativeSolvers.gauss_seidel!(x::HipVector{T}, A::HipDenseMatrix{T}, b::HipVector{T}; maxiter::Int = 10) where {T}
    iterable = HipDenseGaussSeidelIterable{T}(HipDenseStationary(A), x, b, maxiter)
    for item = iterable end
    x
end
function IterativeSolvers.sor!(x::HipVector{T}, A::HipDenseMatrix{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T}
    iterable = HipDenseSORIterable{T, typeof(ω)}(HipDenseStationary(A), x, similar(x), b, ω, maxiter)
    for item = iterable end
    x
end
function IterativeSolvers.ssor!(x::HipVector{T}, A::HipDenseMatrix{T}, b::HipVector{T}, ω::Real; maxiter::Int = 10) where {T}
    iterable = HipDenseSSORIterable{T, typeof(ω)}(HipDenseStationary(A), x, similar(x), b, ω, maxiter)
    for item = iterable end
    x
end
IterativeSolvers.jacobi(A::HipDenseMatrix{T}, b::HipVector{T}; kwargs...) where {T} = IterativeSolvers.jacobi!(IterativeSolvers.zerox(A, b), A, b; kwargs...)
IterativeSolvers.gauss_seidel(A::HipDenseMatrix{T}, b::HipVector{T}; kwargs...) where {T} = IterativeSolvers.gauss_seidel!(IterativeSolvers.zerox(A, b), A, b; kwargs...)
IterativeSolvers.sor(A::HipDenseMatrix{T}, b::HipVector{T}, ω::Real; kwargs...) where {T} = IterativeSolvers.sor!(IterativeSolvers.zerox(A, b), A, b, ω; kwargs...)
IterativeSolvers.ssor(A::HipDenseMatrix{T}, b::HipVector{T}, ω::Real; kwargs...) where {T} = IterativeSolvers.ssor!(IterativeSolvers.zerox(A, b), A, b, ω; kwargs...)

# ---- dense operator: mul!(y, A, x) and mul!(y, adjoint(A), x) for a dense device matrix (csrc/mik_dense_mul.hip) -------------------
# What LinearAlgebra's generic mul! is for a Matrix at src/cg.jl:54,137 and src/gmres.jl:245,287, and for adjoint(A) at src/lsqr.jl:132,172,
# src/lsmr.jl:118,172, src/qmr.jl:76 and src/svdl.jl:565.  The mik_dense handle (opaque: it owns the workspace of the chunk partials and the
# segment sums, no copy of the matrix) is created at the first product of a matrix and kept beside it, not inside HipDenseMatrix.
mutable struct HipDenseOperator
    handle::Ptr{Cvoid}
    ctx::Context
end
const DENSE_OPERATORS = WeakKeyDict{Any, HipDenseOperator}()     # HipDenseMatrix -> its handle; the value holds no reference to the key
function dense_operator(A::HipDenseMatrix{T}) where {T}
    get!(DENSE_OPERATORS, A) do
        h = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mik_dense_create, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}),
                    A.ctx.handle, dtype_code(T), A.n, A.cols, A.ptr, A.ld, h), "mik_dense_create", A.ctx.handle)
        op = HipDenseOperator(h[], A.ctx)
        finalizer(o -> alive(o.ctx) && ccall((:mik_dense_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), op)
        op
    end
end
"(C, R): the columns per chunk of y = A x and the rows a workgroup owns (include/mik.h, dense operator)"
function dense_mul_shape()
    c = Ref{Cint}(0); r = Ref{Cint}(0)
    check(ccall((:mik_dense_mul_shape, libmik), Cint, (Ref{Cint}, Ref{Cint}), c, r), "mik_dense_mul_shape", C_NULL)
    (C = Int(c[]), R = Int(r[]))
end
"adjoint(A) of a HipDenseMatrix: a view, no copy; adjoint(adjoint(A)) === A"
struct HipDenseAdjoint{T<:MikFloat}
    parent::HipDenseMatrix{T}
end
LinearAlgebra.adjoint(A::HipDenseMatrix) = HipDenseAdjoint(A)
LinearAlgebra.adjoint(A::HipDenseAdjoint) = A.parent
Base.size(A::HipDenseAdjoint) = (A.parent.cols, A.parent.n)
Base.size(A::HipDenseAdjoint, d::Integer) = d == 1 ? A.parent.cols : (d == 2 ? A.parent.n : 1)
Base.eltype(::HipDenseAdjoint{T}) where {T} = T
function dense_mul!(y::HipVector{T}, A::HipDenseMatrix{T}, adj::Bool, x::HipVector{T}) where {T}
    (length(x), length(y)) == (adj ? (A.n, A.cols) : (A.cols, A.n)) || throw(DimensionMismatch("mul!(y, A, x)"))
    check(ccall((:mik_dense_mul, libmik), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}), dense_operator(A).handle, adj ? 1 : 0, x.ptr, y.ptr),
          "mik_dense_mul", A.ctx.handle)
    y
end
"Y[:, 1:b] = A * X[:, 1:b] (mik_dense_mm): every column has the bits of dense_mul! on that column; A is read once per group of columns"
function dense_mm!(Y::HipDenseMatrix{T}, A::HipDenseMatrix{T}, X::HipDenseMatrix{T}, b::Integer = X.cols) where {T}
    (X.n == A.cols && Y.n == A.n && 0 <= b <= min(X.cols, Y.cols)) || throw(DimensionMismatch("mul!(Y, A, X)"))
    check(ccall((:mik_dense_mm, libmik), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64), dense_operator(A).handle, b, X.ptr, X.ld, Y.ptr, Y.ld),
          "mik_dense_mm", A.ctx.handle)
    Y
end
function LinearAlgebra.mul!(y::HipVector{T}, A::HipDenseMatrix{T}, x::HipVector{T}) where {T}
    dense_mul!(y, A, false, x)
end
function LinearAlgebra.mul!(y::HipVector{T}, A::HipDenseAdjoint{T}, x::HipVector{T}) where {T}
    dense_mul!(y, A.parent, true, x)
end
Base.:*(A::HipDenseMatrix{T}, x::HipVector{T}) where {T} = mul!(HipVector{T}(undef, A.n, A.ctx), A, x)
Base.:*(A::HipDenseAdjoint{T}, x::HipVector{T}) where {T} = mul!(HipVector{T}(undef, A.parent.cols, A.parent.ctx), A, x)
# mik_operator{dtype, n, NULL, mik_dense_mul_fn, handle}: the fused iterables call the library's product themselves
dense_square(A, ::Type{T}, n::Int) where {T} = (size(A, 1) == size(A, 2) == n && eltype(A) == T) ||
    throw(DimensionMismatch("a $(size(A, 1)) x $(size(A, 2)) $(eltype(A)) matrix as the operator of $(n)-vectors of $(T)"))     # the callback never sees the vector lengths
function dense_operator_struct(A::HipDenseMatrix, ::Type{T}, n::Int) where {T}
    dense_square(A, T, n)
    MikOperator(dtype_code(T), n, C_NULL, cglobal((:mik_dense_mul_fn, libmik)), dense_operator(A).handle)
end
function dense_operator_struct(A::HipDenseAdjoint, ::Type{T}, n::Int) where {T}
    dense_square(A, T, n)
    MikOperator(dtype_code(T), n, C_NULL, cglobal((:mik_dense_mul_adj_fn, libmik)), dense_operator(A.parent).handle)
end

# ---- dense LU: lu(A) / lu!(A) with partial pivoting and ldiv!(y, F, x) on a dense device matrix (csrc/mik_dense_lu.hip) ------------------
# What the reference's tests pass as Pl / Pr (test/gmres.jl:28-35, test/bicgstabl.jl:40-42) and wrap as the operator of
# invpowm (test/simple_eigensolvers.jl:40).  Factors, pivots and solution have the bits of the unblocked loops of mik_lu_solve (include/mik.h).
mutable struct HipLU{T}
    handle::Ptr{Cvoid}
    factors::HipDenseMatrix{T}       # L\U, read at every solve; kept alive with the handle
    ipiv::Vector{Int64}              # 1-based, LAPACK's
    ctx::Context
end
function LinearAlgebra.lu!(A::HipDenseMatrix{T}) where {T}
    size(A, 1) == size(A, 2) || throw(DimensionMismatch("the matrix is $(size(A, 1)) x $(size(A, 2)), not square"))
    h = Ref{Ptr{Cvoid}}(C_NULL); col = Ref{Int64}(0)
    code = ccall((:mik_dense_lu_create, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ref{Int64}, Ref{Ptr{Cvoid}}),
                 A.ctx.handle, A.ptr, A.n, A.ld, dtype_code(T), col, h)
    code == 8 && throw(LinearAlgebra.SingularException(Int(col[])))
    check(code, "mik_dense_lu_create", A.ctx.handle)
    ipiv = Vector{Int64}(undef, A.n)
    check(ccall((:mik_dense_lu_ipiv, libmik), Cint, (Ptr{Cvoid}, Ptr{Int64}), h[], ipiv), "mik_dense_lu_ipiv", A.ctx.handle)
    F = HipLU{T}(h[], A, ipiv, A.ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_dense_lu_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), F)
    F
end
function LinearAlgebra.lu(A::HipDenseMatrix{T}) where {T}        # factors a copy
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_malloc, libmik), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), A.ctx.handle, A.ld * max(A.cols, 1) * sizeof(T), p), "mik_malloc", A.ctx.handle)
    m = HipDenseMatrix{T}(p[], A.n, A.cols, A.ld, A.ctx)
    finalizer(x -> alive(x.ctx) && ccall((:mik_free, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.handle, x.ptr), m)
    check(ccall((:mik_copy, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), A.ctx.handle, dtype_code(T), A.ld * A.cols, A.ptr, m.ptr),
          "mik_copy", A.ctx.handle)
    LinearAlgebra.lu!(m)
end
Base.size(F::HipLU) = size(F.factors)
Base.size(F::HipLU, d::Integer) = size(F.factors, d)
Base.eltype(::HipLU{T}) where {T} = T
function LinearAlgebra.ldiv!(y::HipVector{T}, F::HipLU{T}, x::HipVector{T}) where {T}
    (length(y) == F.factors.n && length(x) == F.factors.n) || throw(DimensionMismatch("ldiv!: vectors of $(length(y)) and $(length(x)), a factorisation of order $(F.factors.n)"))
    check(ccall((:mik_dense_lu_solve, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), F.handle, y.ptr, x.ptr), "mik_dense_lu_solve", F.ctx.handle)
    y
end
LinearAlgebra.ldiv!(F::HipLU{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(x, F, x)
Base.:\(F::HipLU{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(similar(x), F, x)
# ldiv!(Y, F, X) / ldiv!(F, X) / F \ X on a block of right-hand sides: one call, every column with the bits of its vector solve
function LinearAlgebra.ldiv!(Y::HipDenseMatrix{T}, F::HipLU{T}, X::HipDenseMatrix{T}) where {T}
    (Y.n == F.factors.n && X.n == F.factors.n && Y.cols >= X.cols >= 1) ||
        throw(DimensionMismatch("ldiv!: blocks of $(Y.n) x $(Y.cols) and $(X.n) x $(X.cols), a factorisation of order $(F.factors.n)"))
    check(ccall((:mik_dense_lu_solve_block, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64), F.handle, Y.ptr, Y.ld, X.ptr, X.ld, X.cols),
          "mik_dense_lu_solve_block", F.ctx.handle)
    Y
end
LinearAlgebra.ldiv!(F::HipLU{T}, X::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(X, F, X)
Base.:\(F::HipLU{T}, X::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(HipDenseMatrix(zeros(T, X.n, X.cols), X.ctx), F, X)
"panel width, rows per workgroup of the pivot search, tile of the trailing update, row limit of the one-launch panel (0: not built), launches, device bytes"
function dense_lu_info(F::HipLU)
    w = Ref{Int64}(0); r = Ref{Int64}(0); tr = Ref{Int64}(0); tc = Ref{Int64}(0); one = Ref{Int64}(0); lf = Ref{Int64}(0); ls = Ref{Int64}(0); b = Ref{Int64}(0)
    check(ccall((:mik_dense_lu_info, libmik), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                F.handle, w, r, tr, tc, one, lf, ls, b), "mik_dense_lu_info", F.ctx.handle)
    (W = w[], R = r[], tile_rows = tr[], tile_cols = tc[], one_launch_rows = one[], launches_factor = lf[], launches_solve = ls[], bytes = b[])
end
function lu_precond_struct(F::HipLU, ::Type{T}, n::Int) where {T}
    (eltype(F) == T && F.factors.n == n) || throw(DimensionMismatch("the lu of a $(F.factors.n) x $(F.factors.n) $(eltype(F)) matrix as a preconditioner of $n-vectors of $T"))
    MikPrecond(C_NULL, cglobal((:mik_dense_lu_ldiv_fn, libmik)), F.handle)
end

# ---- dense Cholesky: cholesky(A) / cholesky!(A) in the lower form and ldiv!(y, F, x) on a dense device matrix, real or complex ------------
# (csrc/mik_dense_chol.hip).  What the reference's tests pass as Pl to cg (test/cg.jl:44-47) and to chebyshev (test/chebyshev.jl:59-66).
# Only the lower triangle of A and the real parts of its diagonal are read; whether A is Hermitian is not checked.  The factor and the
# solution have the bits of the unblocked loops stated in include/mik.h.
mutable struct HipCholesky{T}
    handle::Ptr{Cvoid}
    factors::HipDenseMatrix{T}       # the lower triangle holds L, read at every solve; kept alive with the handle
    uplo::Char                       # 'L'
    info::Int64                      # 0, or the first column whose pivot was not positive (check = false)
    ctx::Context
end
function LinearAlgebra.cholesky!(A::HipDenseMatrix{T}; check::Bool = true) where {T}
    size(A, 1) == size(A, 2) || throw(DimensionMismatch("the matrix is $(size(A, 1)) x $(size(A, 2)), not square"))
    h = Ref{Ptr{Cvoid}}(C_NULL); col = Ref{Int64}(0)
    code = ccall((:mik_dense_chol_create, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ref{Int64}, Ref{Ptr{Cvoid}}),
                 A.ctx.handle, A.ptr, A.n, A.ld, dtype_code(T), check ? 1 : 0, col, h)
    code == 8 && throw(LinearAlgebra.PosDefException(Int(col[])))
    MIK.check(code, "mik_dense_chol_create", A.ctx.handle)     # `check` is the keyword here
    F = HipCholesky{T}(h[], A, 'L', col[], A.ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_dense_chol_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), F)
    F
end
function LinearAlgebra.cholesky(A::HipDenseMatrix{T}; check::Bool = true) where {T}        # factors a copy
    p = Ref{Ptr{Cvoid}}(C_NULL)
    MIK.check(ccall((:mik_malloc, libmik), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), A.ctx.handle, A.ld * max(A.cols, 1) * sizeof(T), p), "mik_malloc", A.ctx.handle)
    m = HipDenseMatrix{T}(p[], A.n, A.cols, A.ld, A.ctx)
    finalizer(x -> alive(x.ctx) && ccall((:mik_free, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.handle, x.ptr), m)
    MIK.check(ccall((:mik_copy, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), A.ctx.handle, dtype_code(T), A.ld * A.cols, A.ptr, m.ptr),
              "mik_copy", A.ctx.handle)
    LinearAlgebra.cholesky!(m; check = check)
end
Base.size(F::HipCholesky) = size(F.factors)
Base.size(F::HipCholesky, d::Integer) = size(F.factors, d)
Base.eltype(::HipCholesky{T}) where {T} = T
LinearAlgebra.issuccess(F::HipCholesky) = F.info == 0
function LinearAlgebra.ldiv!(y::HipVector{T}, F::HipCholesky{T}, x::HipVector{T}) where {T}
    (length(y) == F.factors.n && length(x) == F.factors.n) || throw(DimensionMismatch("ldiv!: vectors of $(length(y)) and $(length(x)), a factorisation of order $(F.factors.n)"))
    MIK.check(ccall((:mik_dense_chol_solve, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), F.handle, y.ptr, x.ptr), "mik_dense_chol_solve", F.ctx.handle)
    y
end
LinearAlgebra.ldiv!(F::HipCholesky{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(x, F, x)
Base.:\(F::HipCholesky{T}, x::HipVector{T}) where {T} = LinearAlgebra.ldiv!(similar(x), F, x)
# ldiv!(Y, F, X) / ldiv!(F, X) / F \ X on a block of right-hand sides: one call, every column with the bits of its vector solve
function LinearAlgebra.ldiv!(Y::HipDenseMatrix{T}, F::HipCholesky{T}, X::HipDenseMatrix{T}) where {T}
    (Y.n == F.factors.n && X.n == F.factors.n && Y.cols >= X.cols >= 1) ||
        throw(DimensionMismatch("ldiv!: blocks of $(Y.n) x $(Y.cols) and $(X.n) x $(X.cols), a factorisation of order $(F.factors.n)"))
    MIK.check(ccall((:mik_dense_chol_solve_block, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64), F.handle, Y.ptr, Y.ld, X.ptr, X.ld, X.cols),
          "mik_dense_chol_solve_block", F.ctx.handle)
    Y
end
LinearAlgebra.ldiv!(F::HipCholesky{T}, X::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(X, F, X)
Base.:\(F::HipCholesky{T}, X::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(HipDenseMatrix(zeros(T, X.n, X.cols), X.ctx), F, X)
"panel width, rows per workgroup of the panel kernel, tile of the trailing update, launches, device bytes, info"
function dense_chol_info(F::HipCholesky)
    w = Ref{Int64}(0); r = Ref{Int64}(0); tr = Ref{Int64}(0); tc = Ref{Int64}(0); lf = Ref{Int64}(0); ls = Ref{Int64}(0); b = Ref{Int64}(0); info = Ref{Int64}(0)
    MIK.check(ccall((:mik_dense_chol_info, libmik), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                    F.handle, w, r, tr, tc, lf, ls, b, info), "mik_dense_chol_info", F.ctx.handle)
    (W = w[], R = r[], tile_rows = tr[], tile_cols = tc[], launches_factor = lf[], launches_solve = ls[], bytes = b[], info = info[])
end
function chol_precond_struct(F::HipCholesky, ::Type{T}, n::Int) where {T}
    (eltype(F) == T && F.factors.n == n) || throw(DimensionMismatch("the cholesky of a $(F.factors.n) x $(F.factors.n) $(eltype(F)) matrix as a preconditioner of $n-vectors of $T"))
    MikPrecond(C_NULL, cglobal((:mik_dense_chol_ldiv_fn, libmik)), F.handle)
end

# ---- dense QR: qr(A) / qr!(A) (Householder, no pivoting) of an m x n dense device matrix, m >= n; lmul!(F.Q, Y), lmul!(F.Q', Y), F \ b and
# ---- Matrix(F.Q) (csrc/mik_dense_qr.hip).  A \ b for a tall matrix is what the reference's tests hold lsqr and lsmr to (test/lsqr.jl:15-19,
# test/lsmr.jl:68-72); Matrix(qr(A).Q) is their orthonormal basis (test/orthogonalize.jl:17-18).  Factors, tau, products and solution have
# the bits of the unblocked loops stated in include/mik.h.  Float64 / Float32.
mutable struct HipQR{T}
    handle::Ptr{Cvoid}
    factors::HipDenseMatrix{T}       # R on and above the diagonal, the reflectors below it; kept alive with the handle
    τ::Vector{T}
    zero_diag::Int64                 # 0, or the first k with R[k,k] == 0: F \ b then throws SingularException(k)
    ctx::Context
end
struct HipQRQ{T}                     # F.Q
    F::HipQR{T}
end
struct HipQRQAdjoint{T}              # F.Q'
    F::HipQR{T}
end
function LinearAlgebra.qr!(A::HipDenseMatrix{T}; resident_rows::Integer = 0) where {T}
    size(A, 1) >= size(A, 2) || throw(DimensionMismatch("the matrix is $(size(A, 1)) x $(size(A, 2)): qr of a wide matrix is not offered"))
    h = Ref{Ptr{Cvoid}}(C_NULL); col = Ref{Int64}(0); plan = Ref{Int64}(resident_rows)
    check(ccall((:mik_dense_qr_create, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Cint, Ptr{Int64}, Ref{Int64}, Ref{Ptr{Cvoid}}),
                A.ctx.handle, A.ptr, A.n, A.cols, A.ld, dtype_code(T), resident_rows == 0 ? Ptr{Int64}(C_NULL) : Base.unsafe_convert(Ptr{Int64}, plan), col, h),
          "mik_dense_qr_create", A.ctx.handle)
    τ = Vector{T}(undef, A.cols)
    check(ccall((:mik_dense_qr_tau, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), h[], τ), "mik_dense_qr_tau", A.ctx.handle)
    F = HipQR{T}(h[], A, τ, col[], A.ctx)
    finalizer(o -> alive(o.ctx) && ccall((:mik_dense_qr_destroy, libmik), Cint, (Ptr{Cvoid},), o.handle), F)
    F
end
function LinearAlgebra.qr(A::HipDenseMatrix{T}; resident_rows::Integer = 0) where {T}        # factors a copy
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mik_malloc, libmik), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), A.ctx.handle, A.ld * max(A.cols, 1) * sizeof(T), p), "mik_malloc", A.ctx.handle)
    m = HipDenseMatrix{T}(p[], A.n, A.cols, A.ld, A.ctx)
    finalizer(x -> alive(x.ctx) && ccall((:mik_free, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.handle, x.ptr), m)
    check(ccall((:mik_copy, libmik), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}), A.ctx.handle, dtype_code(T), A.ld * A.cols, A.ptr, m.ptr),
          "mik_copy", A.ctx.handle)
    LinearAlgebra.qr!(m; resident_rows = resident_rows)
end
Base.size(F::HipQR) = size(F.factors)
Base.size(F::HipQR, d::Integer) = size(F.factors, d)
Base.eltype(::HipQR{T}) where {T} = T
Base.getproperty(F::HipQR, s::Symbol) = s === :Q ? HipQRQ(F) : getfield(F, s)
Base.adjoint(Q::HipQRQ) = HipQRQAdjoint(Q.F)
Base.adjoint(Q::HipQRQAdjoint) = HipQRQ(Q.F)
function qr_lmul!(F::HipQR{T}, adjoint::Bool, ptr::Ptr{Cvoid}, rows::Int, ld::Int, cols::Int) where {T}
    rows == F.factors.n || throw(DimensionMismatch("lmul!: $rows rows, a factorisation of $(F.factors.n) x $(F.factors.cols)"))
    check(ccall((:mik_dense_qr_lmul, libmik), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64), F.handle, adjoint ? 1 : 0, ptr, ld, cols), "mik_dense_qr_lmul", F.ctx.handle)
end
LinearAlgebra.lmul!(Q::HipQRQ{T}, y::HipVector{T}) where {T} = (qr_lmul!(Q.F, false, y.ptr, length(y), length(y), 1); y)
LinearAlgebra.lmul!(Q::HipQRQAdjoint{T}, y::HipVector{T}) where {T} = (qr_lmul!(Q.F, true, y.ptr, length(y), length(y), 1); y)
LinearAlgebra.lmul!(Q::HipQRQ{T}, Y::HipDenseMatrix{T}) where {T} = (qr_lmul!(Q.F, false, Y.ptr, Y.n, Y.ld, Y.cols); Y)
LinearAlgebra.lmul!(Q::HipQRQAdjoint{T}, Y::HipDenseMatrix{T}) where {T} = (qr_lmul!(Q.F, true, Y.ptr, Y.n, Y.ld, Y.cols); Y)
function Base.Matrix(Q::HipQRQ{T}) where {T}                    # the thin Q, m x n, on the device
    F = Q.F
    out = HipDenseMatrix(zeros(T, F.factors.n, F.factors.cols), F.ctx)
    check(ccall((:mik_dense_qr_thin_q, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), F.handle, out.ptr, out.ld), "mik_dense_qr_thin_q", F.ctx.handle)
    out
end
function qr_R(F::HipQR{T}) where {T}                            # F.R as a new n x n device matrix
    out = HipDenseMatrix(zeros(T, F.factors.cols, F.factors.cols), F.ctx)
    check(ccall((:mik_dense_qr_r, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), F.handle, out.ptr, out.ld), "mik_dense_qr_r", F.ctx.handle)
    out
end
function LinearAlgebra.ldiv!(x::HipVector{T}, F::HipQR{T}, b::HipVector{T}) where {T}
    (length(b) == F.factors.n && length(x) == (x === b ? F.factors.n : F.factors.cols)) ||
        throw(DimensionMismatch("ldiv!: vectors of $(length(x)) and $(length(b)), a factorisation of $(F.factors.n) x $(F.factors.cols)"))
    F.zero_diag == 0 || throw(LinearAlgebra.SingularException(Int(F.zero_diag)))
    check(ccall((:mik_dense_qr_solve, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), F.handle, x.ptr, b.ptr), "mik_dense_qr_solve", F.ctx.handle)
    x
end
LinearAlgebra.ldiv!(F::HipQR{T}, b::HipVector{T}) where {T} = LinearAlgebra.ldiv!(b, F, b)
Base.:\(F::HipQR{T}, b::HipVector{T}) where {T} = LinearAlgebra.ldiv!(HipVector(zeros(T, F.factors.cols), F.ctx), F, b)
function LinearAlgebra.ldiv!(X::HipDenseMatrix{T}, F::HipQR{T}, B::HipDenseMatrix{T}) where {T}
    (B.n == F.factors.n && X.n == (X === B ? F.factors.n : F.factors.cols) && X.cols >= B.cols >= 1) ||
        throw(DimensionMismatch("ldiv!: blocks of $(X.n) x $(X.cols) and $(B.n) x $(B.cols), a factorisation of $(F.factors.n) x $(F.factors.cols)"))
    F.zero_diag == 0 || throw(LinearAlgebra.SingularException(Int(F.zero_diag)))
    check(ccall((:mik_dense_qr_solve_block, libmik), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64), F.handle, X.ptr, X.ld, B.ptr, B.ld, B.cols),
          "mik_dense_qr_solve_block", F.ctx.handle)
    X
end
LinearAlgebra.ldiv!(F::HipQR{T}, B::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(B, F, B)
Base.:\(F::HipQR{T}, B::HipDenseMatrix{T}) where {T} = LinearAlgebra.ldiv!(HipDenseMatrix(zeros(T, F.factors.cols, B.cols), B.ctx), F, B)
"A \\ b on a dense device matrix: lu for a square one, qr (least squares) for a tall one; a wide one is refused"
function Base.:\(A::HipDenseMatrix{T}, b::Union{HipVector{T}, HipDenseMatrix{T}}) where {T}
    size(A, 1) >= size(A, 2) || throw(DimensionMismatch("A \\ b of a wide matrix ($(size(A, 1)) x $(size(A, 2))): the minimum-norm solution is not offered"))
    size(A, 1) == size(A, 2) ? LinearAlgebra.lu(A) \ b : LinearAlgebra.qr(A) \ b
end
"panel width, accumulators of a reduction, the row limit of the LDS-resident form and whether the handle is within it, launches, device bytes, zero_diag"
function dense_qr_info(F::HipQR)
    w = Ref{Int64}(0); a = Ref{Int64}(0); rr = Ref{Int64}(0); r = Ref{Int64}(0); lf = Ref{Int64}(0); ls = Ref{Int64}(0); b = Ref{Int64}(0); z = Ref{Int64}(0)
    check(ccall((:mik_dense_qr_info, libmik), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ref{Int64}),
                F.handle, w, a, rr, r, lf, ls, b, z), "mik_dense_qr_info", F.ctx.handle)
    (W = w[], accumulators = a[], resident_rows = rr[], resident = r[] != 0, launches_factor = lf[], launches_solve = ls[], bytes = b[], zero_diag = z[])
end
function qr_precond_struct(F::HipQR, ::Type{T}, n::Int) where {T}
    (eltype(F) == T && F.factors.n == n && F.factors.cols == n) ||
        throw(DimensionMismatch("the qr of a $(F.factors.n) x $(F.factors.cols) $(eltype(F)) matrix as a preconditioner of $n-vectors of $T"))
    MikPrecond(C_NULL, cglobal((:mik_dense_qr_ldiv_fn, libmik)), F.handle)
end

end # module
