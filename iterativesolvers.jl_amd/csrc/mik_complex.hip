// mik_complex.hip -- ComplexF64 / ComplexF32 (MIK_C64 / MIK_C32) for cg and gmres on a CSR operator: DESIGN.md section 17.
//
// Storage is interleaved (re, im), so a complex n-vector is also a real 2 n-vector, and the level-1 segment of a complex vector
// (256 * W * L elements, W = 16 B / sizeof(element)) is the same stretch of memory as the level-1 segment of that real vector: thread t
// owns the same 16-byte groups either way.  The kernels below therefore walk a complex vector with the segment toolkit of
// csrc/mik_kernels.h instantiated for the component type R over 2 n reals (seg_load / seg_store, block_tree_256, k_finalize_store,
// launch_segments); register q = 2 p holds the real part and q = 2 p + 1 the imaginary part of the thread's p-th element.
//
// Arithmetic (the reference's Base definitions, nothing contracted -- the library is built -ffp-contract=off):
//   z * w     = (zr wr - zi wi) + (zr wi + zi wr) i
//   dot(x, y) = sum conj(x_i) y_i: per element re = xr yr + xi yi, im = xr yi - xi yr (every product rounded, the two terms added),
//               then one two-level tree for re and one for im
//   norm, copy, sub, the real-scalar forms of scal / axpy / xpby: the real sweeps over 2 n (forwarded in mik_core.hip)
#include "mik_complex.h"
#include "mik_kernels.h"
#include "mik_spmv.h"
#include "mik_dense_cmul.h"

#include <new>
#include <vector>

// =============================================================================================
// element-wise sweeps over complex vectors
// =============================================================================================
// Op interface of k_cvec: which of the three operands are read (x, z: inputs; y: read and/or written), how many sums (NRED: 0, 1, 2) and
//   __device__ void elem(R xr, R xi, R zr, R zi, R &yr, R &yi, R &a0, R &a1) const;     // one complex element
// prepare(): once per thread before the sweep (coefficients that live in device memory).

// The update-then-reduce op: first y is updated from x (UPD), then the updated y is reduced (RED).
//   UPD  CU_NONE; CU_AXPY: y .+= a .* x, a = ar + ai i by value (src/cg.jl:58-59); CU_AXPY_REAL: the same with a real a = ar (real x complex);
//        CU_MGS_SUB: y .-= h .* x with h the complex at *hp (device: the projection the previous pass reduced, src/orthogonalize.jl:69-75)
//   RED  CR_DOT: a0 + a1 i = dot(z, y) (src/cg.jl:55, src/orthogonalize.jl:71); CR_SUMSQ: a0 = the sum of squares of y
// The element operations are those of csrc/mik_complex.h.  An update without a reduction is OpCAxpy below; the instances with CU_NONE
// only read y (STORE is false).
enum { CU_NONE, CU_AXPY, CU_AXPY_REAL, CU_MGS_SUB };
enum { CR_DOT, CR_SUMSQ };
template <typename R, int UPD, int RED> struct OpCUpdRed {
    static constexpr bool LOADX = UPD != CU_NONE, LOADZ = RED == CR_DOT, LOADY = true, STORE = UPD != CU_NONE;
    static constexpr int NRED = RED == CR_DOT ? 2 : 1;
    const R *x, *z; R *y; const R *hp; R ar, ai;
    __device__ __forceinline__ void prepare() { if (UPD == CU_MGS_SUB) { ar = hp[0]; ai = hp[1]; } }
    __device__ __forceinline__ void elem(R xr, R xi, R zr, R zi, R &yr, R &yi, R &a0, R &a1) const
    {
        if (UPD == CU_AXPY) cx_madd(ar, ai, xr, xi, yr, yi);
        if (UPD == CU_AXPY_REAL) cx_madd_real(ar, xr, xi, yr, yi);
        if (UPD == CU_MGS_SUB) cx_msub(ar, ai, xr, xi, yr, yi);
        if (RED == CR_DOT) cx_dot_acc(zr, zi, yr, yi, a0, a1);
        if (RED == CR_SUMSQ) cx_sumsq_acc(yr, yi, a0);
    }
};

// y .+= alpha .* x                                               -- src/cg.jl:58-59
template <typename R> struct OpCAxpy {
    static constexpr bool LOADX = true, LOADZ = false, LOADY = true, STORE = true;
    static constexpr int NRED = 0;
    const R *x, *z; R *y; R ar, ai;
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void elem(R xr, R xi, R, R, R &yr, R &yi, R &, R &) const { cx_madd(ar, ai, xr, xi, yr, yi); }
};

// y .= x .+ beta .* y                                            -- src/cg.jl:51 with a complex beta
template <typename R> struct OpCXpby {
    static constexpr bool LOADX = true, LOADZ = false, LOADY = true, STORE = true;
    static constexpr int NRED = 0;
    const R *x, *z; R *y; R br, bi;
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void elem(R xr, R xi, R, R, R &yr, R &yi, R &, R &) const
    {
        const CxVal<R> p = cx_mul(br, bi, yr, yi);
        yr = xr + p.re;
        yi = xi + p.im;
    }
};

// y .*= alpha
template <typename R> struct OpCScal {
    static constexpr bool LOADX = false, LOADZ = false, LOADY = true, STORE = true;
    static constexpr int NRED = 0;
    const R *x, *z; R *y; R ar, ai;
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void elem(R, R, R, R, R &yr, R &yi, R &, R &) const
    {
        const CxVal<R> p = cx_mul(yr, yi, ar, ai);
        yr = p.re;
        yi = p.im;
    }
};

// y .= value
template <typename R> struct OpCFill {
    static constexpr bool LOADX = false, LOADZ = false, LOADY = false, STORE = true;
    static constexpr int NRED = 0;
    const R *x, *z; R *y; R vr, vi;
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void elem(R, R, R, R, R &yr, R &yi, R &, R &) const { yr = vr; yi = vi; }
};

// n2 = 2 n reals; seg_out: [NRED][nseg]
template <typename R, bool VEC, typename Op>
__global__ __launch_bounds__(MIK_BLOCK) void k_cvec(int64_t n2, int64_t nseg, Op op, R *__restrict__ seg_out)
{
    constexpr int W = VT<R>::W;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    __shared__ R lds4[4];
    op.prepare();
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)W * threadIdx.x;
        R xr[SEG_REGS<R>], zr[SEG_REGS<R>], yr[SEG_REGS<R>];
#pragma unroll
        for (int q = 0; q < SEG_REGS<R>; ++q) { xr[q] = R(0); zr[q] = R(0); yr[q] = R(0); }
        if (Op::LOADX) seg_load<R, VEC>(op.x, base, n2, 0, xr);
        if (Op::LOADZ) seg_load<R, VEC>(op.z, base, n2, 0, zr);
        if (Op::LOADY) seg_load<R, VEC>(op.y, base, n2, 0, yr);
        R a0 = R(0), a1 = R(0);
#pragma unroll
        for (int l = 0; l < MIK_RED_L; ++l) {
#pragma unroll
            for (int p = 0; p < W / 2; ++p) {
                const int q = l * W + 2 * p;
                if (base + (int64_t)l * MIK_BLOCK * W + 2 * p < n2) op.elem(xr[q], xr[q + 1], zr[q], zr[q + 1], yr[q], yr[q + 1], a0, a1);
            }
        }
        if (Op::STORE) seg_store<R, VEC>(op.y, base, n2, yr);
        if (Op::NRED >= 1) {
            const R tot = block_tree_256(a0, lds4);
            if (threadIdx.x == 0) seg_out[s] = tot;
        }
        if (Op::NRED >= 2) {
            const R tot = block_tree_256(a1, lds4);
            if (threadIdx.x == 0) seg_out[nseg + s] = tot;
        }
    }
}

template <typename R, typename Op> static int launch_cvec(mik_ctx *ctx, int64_t n, Op op, bool vec, R *seg_out)
{
    return launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t nseg) {
        hipLaunchKernelGGL((k_cvec<R, decltype(v)::value, Op>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, op, seg_out);
    });
}

// The mik_c_* entries take untyped pointers and a dtype code; c_typed calls f with a value of the component type (double for MIK_C64, float
// for MIK_C32), and the c_* templates below cast their pointers once, where they name them.
template <typename F> static inline int c_typed(int dtype, F &&f) { return dtype == MIK_C64 ? f(double{}) : f(float{}); }

// level 2 of `cols` reductions whose segment sums sit in ctx->partials (c_finalize, csrc/mik_complex.h), through ctx->coef to the host
template <typename R> static int c_sums_to_host(mik_ctx *ctx, int64_t nseg, int cols, R *out)
{
    MIK_TRY(c_finalize<R>(ctx, nseg, cols, (R *)ctx->coef));
    return mik_read_scalars<R>(ctx, (const R *)ctx->coef, cols, out);
}

// y is updated from x (UPD != CU_NONE: alpha, x given), then reduced to *out (host): CR_DOT: dot(z, y), CR_SUMSQ: norm(y)
//                                                                 -- src/cg.jl:55, src/minres.jl:106+109, :111+114
// With CU_NONE alpha and x are not read (NULL is fine) and y is not written: the op's STORE is false.
template <typename R, int UPD, int RED> static int c_update_reduce(mik_ctx *ctx, int64_t n, const void *alpha, const void *x, void *y, const void *z, void *out)
{
    constexpr bool upd = UPD != CU_NONE, dot = RED == CR_DOT;
    const int64_t nseg = mik_nseg<R>(2 * n);
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * 2 * (size_t)std::max<int64_t>(nseg, 1)));
    const R *a = (const R *)alpha;
    OpCUpdRed<R, UPD, RED> op{(const R *)x, (const R *)z, (R *)y, nullptr, upd ? a[0] : R(0), UPD == CU_AXPY ? a[1] : R(0)};
    const bool vec = mik_aligned16(y) && (!upd || mik_aligned16(x)) && (!dot || mik_aligned16(z));
    MIK_TRY((launch_cvec<R>(ctx, n, op, vec, (R *)ctx->partials)));
    if (dot) return c_sums_to_host<R>(ctx, nseg, 2, (R *)out);
    R ss;
    MIK_TRY(c_sums_to_host<R>(ctx, nseg, 1, &ss));
    return mik_norm_from_sumsq<R>(ctx, 2 * n, (const R *)y, ss, (R *)out);      // include/mik.h "Norms"
}

// dot(x, y): the reduction alone, with x as z.  The cast drops const only to fit the op's y member: a CU_NONE instance never stores.
int mik_c_dot(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *y, void *out)
{
    return c_typed(dtype, [&](auto r) { return c_update_reduce<decltype(r), CU_NONE, CR_DOT>(ctx, n, nullptr, nullptr, const_cast<void *>(y), x, out); });
}

// real_alpha needs z; the forms with neither x nor z, or with a real alpha and no z, are the real entry over 2 n and never come here
int mik_c_axpy_dot(mik_ctx *ctx, int dtype, int64_t n, int real_alpha, const void *alpha, const void *x, void *y, const void *z, void *out)
{
    return c_typed(dtype, [&](auto r) {
        using R = decltype(r);
        if (!z) return c_update_reduce<R, CU_AXPY, CR_SUMSQ>(ctx, n, alpha, x, y, z, out);
        if (!x) return c_update_reduce<R, CU_NONE, CR_DOT>(ctx, n, alpha, x, y, z, out);
        return real_alpha ? c_update_reduce<R, CU_AXPY_REAL, CR_DOT>(ctx, n, alpha, x, y, z, out) : c_update_reduce<R, CU_AXPY, CR_DOT>(ctx, n, alpha, x, y, z, out);
    });
}

template <typename R> static int c_fill(mik_ctx *ctx, int64_t n, const void *value, void *x)
{
    const R *v = (const R *)value;
    if (memcmp(v, v + 1, sizeof(R)) == 0) {             // re and im carry the same bits (zero(T) of src/cg.jl:129): the real fill over 2 n
        OpFill<R> op{(R *)x, v[0]};
        return launch_map<R>(ctx, 2 * n, op, mik_aligned16(x), (R *)nullptr, nullptr);
    }
    OpCFill<R> op{nullptr, nullptr, (R *)x, v[0], v[1]};
    return launch_cvec<R>(ctx, n, op, mik_aligned16(x), (R *)nullptr);
}
int mik_c_fill(mik_ctx *ctx, int dtype, int64_t n, const void *value, void *x)
{
    return c_typed(dtype, [&](auto r) { return c_fill<decltype(r)>(ctx, n, value, x); });
}

template <typename R> static int c_axpy(mik_ctx *ctx, int64_t n, const void *alpha, const void *x, void *y)
{
    OpCAxpy<R> op{(const R *)x, nullptr, (R *)y, ((const R *)alpha)[0], ((const R *)alpha)[1]};
    return launch_cvec<R>(ctx, n, op, mik_aligned16(x) && mik_aligned16(y), (R *)nullptr);
}
int mik_c_axpy(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, const void *x, void *y)
{
    return c_typed(dtype, [&](auto r) { return c_axpy<decltype(r)>(ctx, n, alpha, x, y); });
}

template <typename R> static int c_xpby(mik_ctx *ctx, int64_t n, const void *x, const void *beta, void *y)
{
    OpCXpby<R> op{(const R *)x, nullptr, (R *)y, ((const R *)beta)[0], ((const R *)beta)[1]};
    return launch_cvec<R>(ctx, n, op, mik_aligned16(x) && mik_aligned16(y), (R *)nullptr);
}
int mik_c_xpby(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *beta, void *y)
{
    return c_typed(dtype, [&](auto r) { return c_xpby<decltype(r)>(ctx, n, x, beta, y); });
}

template <typename R> static int c_scal(mik_ctx *ctx, int64_t n, const void *alpha, void *x)
{
    OpCScal<R> op{nullptr, nullptr, (R *)x, ((const R *)alpha)[0], ((const R *)alpha)[1]};
    return launch_cvec<R>(ctx, n, op, mik_aligned16(x), (R *)nullptr);
}
int mik_c_scal(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, void *x)
{
    return c_typed(dtype, [&](auto r) { return c_scal<decltype(r)>(ctx, n, alpha, x); });
}

// =============================================================================================
// Modified Gram-Schmidt -- orthogonalize_and_normalize!(V[:, 1:k], w, h, ModifiedGramSchmidt()), src/orthogonalize.jl:67-79
// =============================================================================================
// One sweep over w per basis column: the pass that subtracts column i accumulates the projection on column i + 1 (of the updated w), the
// pass that subtracts the last column carries the sum of squares of the norm; then w .*= inv(nrm) as the real sweep over 2 n.  h, nrm and
// inv(nrm) stay in the context's coefficient area between the passes (reals: [0, 2 k) = h, [2 k] = nrm, [2 k + 1] = inv(nrm)); the host
// waits once, at the end.
template <typename R>
static int c_mgs(mik_ctx *ctx, int64_t n, int k, const void *Vv, int64_t ldv, void *wv, void *hv, void *nrmv)
{
    const R *V = (const R *)Vv;
    R *w = (R *)wv, *h = (R *)hv, *nrm = (R *)nrmv;
    if ((size_t)(2 * k + 2) * sizeof(R) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_orthogonalize: too many columns (k = %d) for a complex basis", k);
    const int64_t nseg = mik_nseg<R>(2 * n);
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * 2 * (size_t)std::max<int64_t>(nseg, 1)));
    R *part = (R *)ctx->partials, *cf = (R *)ctx->coef;
    const bool vec = mik_aligned16(w) && (k == 0 || (mik_aligned16(V) && (2 * ldv) % VT<R>::W == 0));
    auto colp = [&](int j) { return V + 2 * (int64_t)j * ldv; };
    if (k == 0) {
        OpCUpdRed<R, CU_NONE, CR_SUMSQ> op{nullptr, nullptr, w, nullptr, R(0), R(0)};
        MIK_TRY((launch_cvec<R>(ctx, n, op, vec, part)));
    } else {
        OpCUpdRed<R, CU_NONE, CR_DOT> first{nullptr, colp(0), w, nullptr, R(0), R(0)};
        MIK_TRY((launch_cvec<R>(ctx, n, first, vec, part)));
        MIK_TRY(c_finalize<R>(ctx, nseg, 2, cf));
        for (int i = 1; i < k; ++i) {
            OpCUpdRed<R, CU_MGS_SUB, CR_DOT> op{colp(i - 1), colp(i), w, cf + 2 * (i - 1), R(0), R(0)};
            MIK_TRY((launch_cvec<R>(ctx, n, op, vec, part)));
            MIK_TRY(c_finalize<R>(ctx, nseg, 2, cf + 2 * i));
        }
        OpCUpdRed<R, CU_MGS_SUB, CR_SUMSQ> last{colp(k - 1), nullptr, w, cf + 2 * (k - 1), R(0), R(0)};
        MIK_TRY((launch_cvec<R>(ctx, n, last, vec, part)));
    }
    hipLaunchKernelGGL((k_finalize_nrm_inv<R>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const R *)part, nseg, cf + 2 * k);
    MIK_LAUNCH_CHECK(ctx);
    OpScal<R> sc{w, coef_ptr<R>(cf + 2 * k + 1)};                        // inv(nrm), or 1 when the sum of squares left the safe range
    MIK_TRY((launch_map<R>(ctx, 2 * n, sc, mik_aligned16(w), (R *)nullptr, nullptr)));
    std::vector<R> host((size_t)2 * k + 2);
    MIK_TRY(mik_read_scalars<R>(ctx, cf, 2 * k + 2, host.data()));
    if (k) memcpy(h, host.data(), sizeof(R) * 2 * (size_t)k);
    *nrm = host[(size_t)2 * k];
    if (*nrm != *nrm) {                                                   // include/mik.h "Norms": the scaled recomputation, then the scale
        MIK_TRY(mik_safe_norm_slow<R>(ctx, 2 * n, w, nrm));
        OpScal<R> s2{w, coef_val<R>(R(1) / *nrm)};
        MIK_TRY((launch_map<R>(ctx, 2 * n, s2, mik_aligned16(w), (R *)nullptr, nullptr)));
    }
    return MIK_OK;
}

int mik_c_orthogonalize(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *w, void *h, void *nrm, int method)
{
    if (method == MIK_CGS) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_orthogonalize: ClassicalGramSchmidt is not implemented for complex element types");
    if (method == MIK_DGKS) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_orthogonalize: DGKS is not implemented for complex element types");
    return c_typed(dtype, [&](auto r) { return c_mgs<decltype(r)>(ctx, n, k, V, ldv, w, h, nrm); });
}

// =============================================================================================
// y += alpha V[:, 1:k] c -- mul!(y, V, c, alpha, 1), src/gmres.jl:275
// =============================================================================================
// t_j = alpha * c_j on the host; y = y + t_j * V[:, j], columns ascending, y held in registers over the k columns
template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cgemv_n(int64_t n2, int64_t nseg, int k, const R *__restrict__ V, int64_t ldv2, const R *__restrict__ t,
                                                       R *__restrict__ y, int nt)
{
    constexpr int W = VT<R>::W;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)W * threadIdx.x;
        R yr[SEG_REGS<R>];
        seg_load<R, VEC>(y, base, n2, 0, yr);
        for (int j = 0; j < k; ++j) {
            R vr[SEG_REGS<R>];
            seg_load<R, VEC>(V + (int64_t)j * ldv2, base, n2, nt, vr);
            cseg_madd<R>(t[2 * j], t[2 * j + 1], vr, yr);
        }
        seg_store<R, VEC>(y, base, n2, yr);
    }
}

template <typename R>
static int c_gemv_n(mik_ctx *ctx, int64_t n, int k, const void *Vv, int64_t ldv, const void *cv, const void *av, void *yv)
{
    const R *V = (const R *)Vv, *c = (const R *)cv, *alpha = (const R *)av;
    R *y = (R *)yv;
    if (k == 0 || n == 0) return MIK_OK;
    if ((size_t)(2 * k) * sizeof(R) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_gemv_n: too many columns (k = %d) for a complex basis", k);
    MIK_HIP(ctx, mik_wait(ctx));                        // staging buffer must be idle
    R *st = (R *)ctx->coef_host;
    for (int j = 0; j < k; ++j) {
        const CxVal<R> t = cx_mul(alpha[0], alpha[1], c[2 * j], c[2 * j + 1]);
        st[2 * j] = t.re;
        st[2 * j + 1] = t.im;
    }
    MIK_HIP(ctx, hipMemcpyAsync(ctx->coef, st, sizeof(R) * 2 * (size_t)k, hipMemcpyHostToDevice, ctx->stream));
    const bool vec = mik_aligned16(y) && mik_aligned16(V) && (2 * ldv) % VT<R>::W == 0;
    const int nt = (double)n * (double)k * 2.0 * sizeof(R) > 192.0e6 ? 1 : 0;
    return launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t nseg) {
        hipLaunchKernelGGL((k_cgemv_n<R, decltype(v)::value>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, k, V, 2 * ldv, (const R *)ctx->coef, y, nt);
    });
}

int mik_c_gemv_n(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *c, const void *alpha, void *y)
{
    return c_typed(dtype, [&](auto r) { return c_gemv_n<decltype(r)>(ctx, n, k, V, ldv, c, alpha, y); });
}

// =============================================================================================
// SpMV on the CSR arrays
// =============================================================================================
// k_spmv_complex: one workgroup per 256-row block (grid-stride over the blocks).  The block's stretch of val / col is streamed coalesced,
// TILE entries at a time -- 16-byte loads of the values (one ComplexF64, two ComplexF32), each streaming thread gathers x[col] and leaves
// the rounded product in LDS -- and then thread r adds the products of row r from LDS, re and im each, strictly in ascending column order:
// the order in which the reference's CSC scatter reaches the row.  Rows longer than MIK_LONG_ROW entries are left to k_spmv_complex_long.
constexpr int MIK_C_TILE = 1024;
constexpr int MIK_C_WG_PER_CU = 8;                     // grid cap of the row-block kernel: what is resident (16 KB of LDS per workgroup at C64)

template <typename R, bool XV>
__global__ __launch_bounds__(MIK_BLOCK) void k_spmv_complex(int n_rows, int nb, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                            const R *__restrict__ val, const R *__restrict__ x, R *__restrict__ y)
{
    constexpr int W = VT<R>::W / 2;                    // complex values per 16-byte load
    __shared__ R prod[2 * MIK_C_TILE];
    const int tid = (int)threadIdx.x;
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
        const int r0 = b * MIK_BLOCK, r = r0 + tid;
        const int e0 = rowptr[r0], e1 = rowptr[min(r0 + MIK_BLOCK, n_rows)];
        int lo = 0, hi = 0;
        if (r < n_rows) { lo = rowptr[r]; hi = rowptr[r + 1]; }
        const bool mine = r < n_rows && hi - lo <= MIK_LONG_ROW;
        R sr = R(0), si = R(0);
        for (int cb = e0 & ~(W - 1); cb < e1; cb += MIK_C_TILE) {
            for (int j = tid * W; j < MIK_C_TILE && cb + j < e1; j += MIK_BLOCK * W) {
                auto av = vload_nt<R>(val + 2 * (int64_t)(cb + j));       // val is padded by W entries; cb + j is a multiple of W
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const int e = cb + j + q;
                    if (e >= e0 && e < e1) {
                        const int64_t c = col[e];
                        R xr, xi;
                        if (XV) {
                            const auto xv = *reinterpret_cast<const typename std::conditional<sizeof(R) == 8, double2, float2>::type *>(x + 2 * c);
                            xr = xv.x; xi = xv.y;
                        } else { xr = x[2 * c]; xi = x[2 * c + 1]; }
                        const CxVal<R> p = cx_mul(el<R>(av, 2 * q), el<R>(av, 2 * q + 1), xr, xi);
                        prod[2 * (j + q)] = p.re;
                        prod[2 * (j + q) + 1] = p.im;
                    }
                }
            }
            __syncthreads();
            if (mine) {
                const int a = max(lo, cb), z = min(hi, cb + MIK_C_TILE);
                for (int e = a; e < z; ++e) {
                    sr = sr + prod[2 * (e - cb)];
                    si = si + prod[2 * (e - cb) + 1];
                }
            }
            __syncthreads();
        }
        if (mine) { y[2 * (int64_t)r] = sr; y[2 * (int64_t)r + 1] = si; }
    }
}

// Long rows: one wave per segment of at most `segment` consecutive entries (mik_spmv_long_segment), summed with the wave shape of the real
// path (csrc/mik_spmv.h): lane l adds, from +0 and in ascending order, the products of the groups l, l + 64, ... of MIK_LONG_G consecutive
// entries, re and im each, then the wave-64 tree.  seg_sum: [nvirt] (re, im).
template <typename R>
__global__ __launch_bounds__(MIK_BLOCK) void k_spmv_complex_long(int nvirt, const int *__restrict__ vstart, const int *__restrict__ vlen,
                                                                 const int *__restrict__ col, const R *__restrict__ val, const R *__restrict__ x,
                                                                 R *__restrict__ seg_sum)
{
    const int lane = threadIdx.x & 63;
    for (int w = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); w < nvirt; w += (int)gridDim.x * 4) {
        const int k0 = vstart[w], len = vlen[w];
        const int ng = (len + MIK_LONG_G - 1) / MIK_LONG_G;
        R sr = R(0), si = R(0);
        for (int g = lane; g < ng; g += 64) {
#pragma unroll
            for (int q = 0; q < MIK_LONG_G; ++q) {
                const int e = MIK_LONG_G * g + q;
                if (e < len) {
                    const int64_t k = (int64_t)k0 + e, c = col[k];
                    const CxVal<R> p = cx_mul(val[2 * k], val[2 * k + 1], x[2 * c], x[2 * c + 1]);
                    sr = sr + p.re;
                    si = si + p.im;
                }
            }
        }
        sr = wave_tree(sr);
        si = wave_tree(si);
        if (lane == 0) { seg_sum[2 * (int64_t)w] = sr; seg_sum[2 * (int64_t)w + 1] = si; }
    }
}

// ... and the segment sums of a row added left to right
template <typename R>
__global__ __launch_bounds__(MIK_BLOCK) void k_spmv_complex_long_sum(int nlong, const int *__restrict__ lrow, const int *__restrict__ lfirst,
                                                                     const int *__restrict__ lnseg, const R *__restrict__ seg_sum, R *__restrict__ y)
{
    for (int h = (int)(blockIdx.x * blockDim.x + threadIdx.x); h < nlong; h += (int)(gridDim.x * blockDim.x)) {
        const int f = lfirst[h], ns = lnseg[h];
        R tr = seg_sum[2 * (int64_t)f], ti = seg_sum[2 * (int64_t)f + 1];
        for (int q = 1; q < ns; ++q) {
            tr = tr + seg_sum[2 * (int64_t)(f + q)];
            ti = ti + seg_sum[2 * (int64_t)(f + q) + 1];
        }
        const int64_t r = lrow[h];
        y[2 * r] = tr;
        y[2 * r + 1] = ti;
    }
}

template <typename R> static int c_spmv(mik_ctx *ctx, const mik_csr *A, const void *x_, void *y_)
{
    if (A->n_rows == 0) return MIK_OK;
    const R *x = (const R *)x_;
    R *y = (R *)y_;
    const int nb = (int)((A->n_rows + MIK_BLOCK - 1) / MIK_BLOCK);
    const int grid = std::min(nb, mik_cus(ctx) * MIK_C_WG_PER_CU);
    const bool xv = ((uintptr_t)x % (2 * sizeof(R))) == 0;
    if (xv) hipLaunchKernelGGL((k_spmv_complex<R, true>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, (int)A->n_rows, nb, A->rowptr, A->col, (const R *)A->val, x, y);
    else hipLaunchKernelGGL((k_spmv_complex<R, false>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, (int)A->n_rows, nb, A->rowptr, A->col, (const R *)A->val, x, y);
    MIK_LAUNCH_CHECK(ctx);
    if (A->c_nlong > 0) {
        const int *t = A->long_rows;                     // [nvirt] start, [nvirt] length, [nlong] row, [nlong] first segment, [nlong] segments
        const int nv = A->c_nvirt, nl = A->c_nlong;
        const int g1 = std::min((nv + 3) / 4, mik_max_grid(ctx));
        hipLaunchKernelGGL((k_spmv_complex_long<R>), dim3(g1), dim3(MIK_BLOCK), 0, ctx->stream, nv, t, t + nv, A->col, (const R *)A->val, x, (R *)A->seg_sum);
        MIK_LAUNCH_CHECK(ctx);
        const int g2 = std::min((nl + MIK_BLOCK - 1) / MIK_BLOCK, mik_max_grid(ctx));
        hipLaunchKernelGGL((k_spmv_complex_long_sum<R>), dim3(g2), dim3(MIK_BLOCK), 0, ctx->stream, nl, t + 2 * nv, t + 2 * nv + nl, t + 2 * nv + 2 * nl,
                           (const R *)A->seg_sum, y);
        MIK_LAUNCH_CHECK(ctx);
    }
    return MIK_OK;
}

int mik_c_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y)
{
    return c_typed(A->dtype, [&](auto r) { return c_spmv<decltype(r)>(ctx, A, x, y); });
}

const char *mik_c_spmv_kernel_name(const mik_csr *A) { return A->c_nlong > 0 ? "k_spmv_complex+k_spmv_complex_long" : "k_spmv_complex"; }

int64_t mik_c_stored_bytes(const mik_csr *A)
{
    const int64_t es = (int64_t)mik_dtype_size(A->dtype);
    return A->nnz * (es + 4) + (A->n_rows + 1) * 4 + (A->c_nlong ? 8LL * A->c_nvirt + 12LL * A->c_nlong : 0);
}

// ---------------------------------------------------------------------------------------------
// upload (host path: upload is not hot for the complex types)
// ---------------------------------------------------------------------------------------------
int mik_c_csr_create(mik_ctx *ctx, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *ptr, const int64_t *idx,
                     const void *val, int index_base, int is_csc, bool on_device, mik_csr **out)
{
    const size_t es = mik_dtype_size(dtype);
    const int64_t n_major = is_csc ? n_cols : n_rows, n_minor = is_csc ? n_rows : n_cols;
    std::vector<int64_t> hp, hi;
    std::vector<unsigned char> hv, v;
    std::vector<int> rowptr, col, perm;
    try {
        if (on_device) {
            hp.resize((size_t)n_major + 1); hi.resize((size_t)nnz); hv.resize((size_t)nnz * es);
            if (hipMemcpy(hp.data(), ptr, sizeof(int64_t) * hp.size(), hipMemcpyDeviceToHost) != hipSuccess ||
                (nnz && (hipMemcpy(hi.data(), idx, sizeof(int64_t) * hi.size(), hipMemcpyDeviceToHost) != hipSuccess ||
                         hipMemcpy(hv.data(), val, hv.size(), hipMemcpyDeviceToHost) != hipSuccess)))
                return mik_fail(ctx, MIK_ERR_HIP, "mik_csr_create: reading the device arrays failed");
            ptr = hp.data(); idx = hi.data(); val = hv.data();
        }
        if (ptr[0] != index_base || ptr[n_major] - index_base != nnz)
            return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_csr_create: ptr[0]=%lld, ptr[end]=%lld inconsistent with nnz=%lld, base=%d", (long long)ptr[0],
                            (long long)ptr[n_major], (long long)nnz, index_base);
        for (int64_t j = 0; j < n_major; ++j)
            if (ptr[j + 1] < ptr[j]) return mik_fail(ctx, MIK_ERR_INVALID, "mik_csr_create: ptr is not non-decreasing at %lld", (long long)j);
        for (int64_t k = 0; k < nnz; ++k)
            if (idx[k] - index_base < 0 || idx[k] - index_base >= n_minor)
                return mik_fail(ctx, MIK_ERR_INVALID, "mik_csr_create: index %lld at position %lld is out of range", (long long)idx[k], (long long)k);
        // entry k of the upload -> (row, column); CSR position by a stable counting sort on the row, then (CSR uploads with unsorted rows) a
        // stable sort of every row by column: columns ascending within a row, duplicates in upload order
        rowptr.assign((size_t)n_rows + 1, 0);
        col.resize((size_t)nnz);
        perm.resize((size_t)nnz);
        v.resize(((size_t)nnz + 2) * es, 0);
        std::vector<int> rowof((size_t)nnz), colof((size_t)nnz);
        for (int64_t j = 0; j < n_major; ++j)
            for (int64_t k = ptr[j] - index_base; k < ptr[j + 1] - index_base; ++k) {
                const int64_t m = idx[k] - index_base;
                rowof[(size_t)k] = (int)(is_csc ? m : j);
                colof[(size_t)k] = (int)(is_csc ? j : m);
            }
        for (int64_t k = 0; k < nnz; ++k) rowptr[(size_t)rowof[(size_t)k] + 1]++;
        for (int64_t r = 0; r < n_rows; ++r) rowptr[(size_t)r + 1] += rowptr[(size_t)r];
        std::vector<int> next(rowptr.begin(), rowptr.end() - 1);
        for (int64_t k = 0; k < nnz; ++k) perm[(size_t)next[(size_t)rowof[(size_t)k]]++] = (int)k;
        for (int64_t r = 0; r < n_rows; ++r) {
            int *b = perm.data() + rowptr[(size_t)r], *e = perm.data() + rowptr[(size_t)r + 1];
            if (!std::is_sorted(b, e, [&](int p, int q) { return colof[(size_t)p] < colof[(size_t)q]; }))
                std::stable_sort(b, e, [&](int p, int q) { return colof[(size_t)p] < colof[(size_t)q]; });
        }
        for (int64_t k = 0; k < nnz; ++k) {
            col[(size_t)k] = colof[(size_t)perm[(size_t)k]];
            memcpy(&v[(size_t)k * es], (const unsigned char *)val + (size_t)perm[(size_t)k] * es, es);
        }
    } catch (const std::bad_alloc &) {
        return mik_fail(ctx, MIK_ERR_NOMEM, "mik_csr_create: host staging allocation failed");
    }
    // long rows: segments of `seg` entries, one wave each
    const int seg = ((ctx->tuning[MIK_KNOB_LONG_SEGMENT] > 0 ? ctx->tuning[MIK_KNOB_LONG_SEGMENT] : MIK_LONG_SEG) + 3) & ~3;
    std::vector<int> vstart, vlen, lrow, lfirst, lnseg;
    int max_row = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int len = rowptr[(size_t)r + 1] - rowptr[(size_t)r];
        max_row = std::max(max_row, len);
        if (len <= MIK_LONG_ROW) continue;
        lrow.push_back((int)r);
        lfirst.push_back((int)vstart.size());
        lnseg.push_back((len + seg - 1) / seg);
        for (int o = 0; o < len; o += seg) { vstart.push_back(rowptr[(size_t)r] + o); vlen.push_back(std::min(seg, len - o)); }
    }
    mik_csr *A = new (std::nothrow) mik_csr();
    if (!A) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_csr_create: host allocation failed");
    A->ctx = ctx; A->dtype = dtype; A->n_rows = n_rows; A->n_cols = n_cols; A->nnz = nnz; A->max_row_nnz = max_row;
    A->c_nlong = (int)lrow.size(); A->c_nvirt = (int)vstart.size();
    (void)hipSetDevice(ctx->device);
    auto up = [&](void **dst, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up((void **)&A->rowptr, rowptr.data(), sizeof(int) * rowptr.size());
    if (e == hipSuccess) e = up((void **)&A->col, col.data(), sizeof(int) * col.size());
    if (e == hipSuccess) e = up(&A->val, v.data(), v.size());
    if (e == hipSuccess && A->c_nlong) {
        std::vector<int> t;
        t.insert(t.end(), vstart.begin(), vstart.end());
        t.insert(t.end(), vlen.begin(), vlen.end());
        t.insert(t.end(), lrow.begin(), lrow.end());
        t.insert(t.end(), lfirst.begin(), lfirst.end());
        t.insert(t.end(), lnseg.begin(), lnseg.end());
        e = up((void **)&A->long_rows, t.data(), sizeof(int) * t.size());
        if (e == hipSuccess) e = hipMalloc(&A->seg_sum, es * vstart.size());
    }
    if (e != hipSuccess) {
        mik_csr_destroy(A);
        return mik_fail(ctx, e == hipErrorOutOfMemory ? MIK_ERR_NOMEM : MIK_ERR_HIP, "mik_csr_create: device upload failed: %s", hipGetErrorString(e));
    }
    *out = A;
    return MIK_OK;
}

// =============================================================================================
// host: complex Givens rotation and the Hessenberg least squares -- src/hessenberg.jl:15-46
// =============================================================================================
template <typename R> struct HC { R re, im; };
template <typename R> static inline HC<R> hc_mul(HC<R> z, HC<R> w) { const CxVal<R> p = cx_mul(z.re, z.im, w.re, w.im); return HC<R>{p.re, p.im}; }
template <typename R> static inline HC<R> hc_add(HC<R> z, HC<R> w) { return HC<R>{z.re + w.re, z.im + w.im}; }
template <typename R> static inline HC<R> hc_rmul(R a, HC<R> z) { return HC<R>{a * z.re, a * z.im}; }
template <typename R> static inline HC<R> hc_conj(HC<R> z) { return HC<R>{z.re, -z.im}; }
template <typename R> static inline HC<R> hc_neg(HC<R> z) { return HC<R>{-z.re, -z.im}; }
template <typename R> static inline R hc_abs1(HC<R> z) { return std::max(std::fabs(z.re), std::fabs(z.im)); }
template <typename R> static inline R hc_abs2(HC<R> z) { return z.re * z.re + z.im * z.im; }
// z / w by Smith's scaling (host only: back substitution of the small triangular system)
template <typename R> static inline HC<R> hc_div(HC<R> z, HC<R> w)
{
    if (std::fabs(w.re) >= std::fabs(w.im)) {
        const R t = w.im / w.re, d = w.re + w.im * t;
        return HC<R>{(z.re + z.im * t) / d, (z.im - z.re * t) / d};
    }
    const R t = w.re / w.im, d = w.re * t + w.im;
    return HC<R>{(z.re * t + z.im) / d, (z.im * t - z.re) / d};
}

// LinearAlgebra.givensAlgorithm(f::Complex, g::Complex) -> (c real, s complex, r complex): LAPACK's xLARTG convention with power-of-two
// rescaling; [c s; -conj(s) c] * [f; g] = [r; 0].
template <typename R> static void c_givens(HC<R> f, HC<R> g, R &cs, HC<R> &sn, HC<R> &r)
{
    const R eps = std::numeric_limits<R>::epsilon(), safmin = std::numeric_limits<R>::min();
    const R safmn2 = std::pow(R(2), R((int)(std::log(safmin / eps) / std::log(R(2)) / R(2))));
    const R safmx2 = R(1) / safmn2;
    R scale = std::max(hc_abs1(f), hc_abs1(g));
    HC<R> fs = f, gs = g;
    int count = 0;
    if (scale >= safmx2) {
        do { ++count; fs = hc_rmul(safmn2, fs); gs = hc_rmul(safmn2, gs); scale *= safmn2; } while (scale >= safmx2 && count < 20);
    } else if (scale <= safmn2) {
        if (g.re == R(0) && g.im == R(0)) { cs = R(1); sn = HC<R>{R(0), R(0)}; r = f; return; }
        do { --count; fs = hc_rmul(safmx2, fs); gs = hc_rmul(safmx2, gs); scale *= safmx2; } while (scale <= safmn2);
    }
    const R f2 = hc_abs2(fs), g2 = hc_abs2(gs);
    if (f2 <= std::max(g2, R(1)) * safmin) {            // the rare case: f is very small
        if (f.re == R(0) && f.im == R(0)) {
            cs = R(0);
            r = HC<R>{std::hypot(g.re, g.im), R(0)};
            const R d = std::hypot(gs.re, gs.im);
            sn = HC<R>{gs.re / d, -gs.im / d};
            return;
        }
        const R f2s = std::hypot(fs.re, fs.im), g2s = std::sqrt(g2);
        cs = f2s / g2s;
        HC<R> ff;
        if (hc_abs1(f) > R(1)) {
            const R d = std::hypot(f.re, f.im);
            ff = HC<R>{f.re / d, f.im / d};
        } else {
            const R dr = safmx2 * f.re, di = safmx2 * f.im, d = std::hypot(dr, di);
            ff = HC<R>{dr / d, di / d};
        }
        sn = hc_mul(ff, HC<R>{gs.re / g2s, -gs.im / g2s});
        r = hc_add(hc_rmul(cs, f), hc_mul(sn, g));
        return;
    }
    const R f2s = std::sqrt(R(1) + g2 / f2);            // the common case
    r = HC<R>{f2s * fs.re, f2s * fs.im};
    cs = R(1) / f2s;
    const R d = f2 + g2;
    sn = hc_mul(HC<R>{r.re / d, r.im / d}, hc_conj(gs));
    for (int i = 0; i < count; ++i) r = hc_rmul(safmx2, r);
    for (int i = 0; i < -count; ++i) r = hc_rmul(safmn2, r);
}

// out = {c + 0 i, s, r}
int mik_c_givens(int dtype, const void *f, const void *g, void *out)
{
    if (dtype == MIK_C64) {
        double c; HC<double> s, r;
        c_givens<double>(*(const HC<double> *)f, *(const HC<double> *)g, c, s, r);
        HC<double> *o = (HC<double> *)out; o[0] = HC<double>{c, 0.0}; o[1] = s; o[2] = r;
    } else {
        float c; HC<float> s, r;
        c_givens<float>(*(const HC<float> *)f, *(const HC<float> *)g, c, s, r);
        HC<float> *o = (HC<float> *)out; o[0] = HC<float>{c, 0.0f}; o[1] = s; o[2] = r;
    }
    return MIK_OK;
}

template <typename R> static void c_hessenberg_ldiv(HC<R> *H, int64_t ldh, int width, HC<R> *rhs)
{
    auto at = [&](int i, int j) -> HC<R> & { return H[(size_t)j * ldh + i]; };
    for (int i = 0; i < width; ++i) {
        R c; HC<R> s, rr;
        c_givens<R>(at(i, i), at(i + 1, i), c, s, rr);
        const HC<R> ms = hc_neg(hc_conj(s));
        at(i, i) = hc_add(hc_rmul(c, at(i, i)), hc_mul(s, at(i + 1, i)));                 // :27
        for (int j = i + 1; j < width; ++j) {
            const HC<R> tmp = hc_add(hc_mul(ms, at(i, j)), hc_rmul(c, at(i + 1, j)));     // :31
            at(i, j) = hc_add(hc_rmul(c, at(i, j)), hc_mul(s, at(i + 1, j)));             // :32
            at(i + 1, j) = tmp;
        }
        const HC<R> tmp = hc_add(hc_mul(ms, rhs[i]), hc_rmul(c, rhs[i + 1]));             // :37
        rhs[i] = hc_add(hc_rmul(c, rhs[i]), hc_mul(s, rhs[i + 1]));
        rhs[i + 1] = tmp;
    }
    for (int j = width - 1; j >= 0; --j) {                                                // :43-44
        rhs[j] = hc_div(rhs[j], at(j, j));
        const HC<R> t = rhs[j];
        for (int i = 0; i < j; ++i) { const HC<R> p = hc_mul(t, at(i, j)); rhs[i] = HC<R>{rhs[i].re - p.re, rhs[i].im - p.im}; }
    }
}

int mik_c_hessenberg_ldiv(int dtype, void *H, int64_t ldh, int width, void *rhs)
{
    if (dtype == MIK_C64) c_hessenberg_ldiv<double>((HC<double> *)H, ldh, width, (HC<double> *)rhs);
    else c_hessenberg_ldiv<float>((HC<float> *)H, ldh, width, (HC<float> *)rhs);
    return MIK_OK;
}

// =============================================================================================
// what bicgstabl, minres and chebyshev stand on
// =============================================================================================
// ---- mik_gemv_t: h[j] = dot(V[:, j], w) -- mul!(h, adjoint(V), w), one column of src/bicgstabl.jl:121 --------------------------------
// k_cdense_t (csrc/mik_dense_cmul.h) is this sweep: a workgroup holds its segment of w and reads every column against it, each column's
// two sums with the bits of the complex mik_dot.  Launched here on the basis instead of a mik_dense; the segment sums go to ctx->partials.
template <typename R> static int c_gemv_t(mik_ctx *ctx, int64_t n, int k, const void *Vv, int64_t ldv, const void *wv, void *hv)
{
    const R *V = (const R *)Vv, *w = (const R *)wv;
    R *h = (R *)hv;
    if (k == 0) return MIK_OK;
    if ((size_t)(2 * k) * sizeof(R) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_gemv_t: too many columns (k = %d) for a complex basis", k);
    const int64_t nseg = mik_nseg<R>(2 * n);
    if (nseg == 0) { memset(h, 0, sizeof(R) * 2 * (size_t)k); return MIK_OK; }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * 2 * (size_t)k * (size_t)nseg));
    const bool vec = mik_aligned16(V) && (2 * ldv) % VT<R>::W == 0 && mik_aligned16(w);
    const int64_t gx = std::min<int64_t>(nseg, mik_max_grid(ctx));
    const int64_t batches = ((int64_t)k + MIK_CDM_TCOLS - 1) / MIK_CDM_TCOLS;
    const int64_t gy = std::min<int64_t>(batches, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(ctx) / gx)));
    const dim3 grid((unsigned)gx, (unsigned)gy);
    R *part = (R *)ctx->partials;
    if (vec) hipLaunchKernelGGL((k_cdense_t<R, true, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, (int64_t)k, V, ldv, w, part);
    else hipLaunchKernelGGL((k_cdense_t<R, false, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, (int64_t)k, V, ldv, w, part);
    MIK_LAUNCH_CHECK(ctx);
    return c_sums_to_host<R>(ctx, nseg, 2 * k, h);
}

int mik_c_gemv_t(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *w, void *h)
{
    return c_typed(dtype, [&](auto r) { return c_gemv_t<decltype(r)>(ctx, n, k, V, ldv, w, h); });
}

// ---- mik_gram: M = V' V for K <= 5 columns in one pass -- src/bicgstabl.jl:120 --------------------------------------------------------
// The K segments stay in registers (K * SEG_REGS reals a lane); K * K sums a segment: re of the K diagonal pairs (their im is a sum of
// xr xi - xi xr = +0), then re and im of the pairs r < c in row-major order of the upper triangle.  seg_out: [K * K][nseg].
template <typename R, bool VEC, int K>
__global__ __launch_bounds__(MIK_BLOCK) void k_cgram(int64_t n2, int64_t nseg, const R *__restrict__ V, int64_t ldv2, R *__restrict__ seg_out)
{
    constexpr int NS = K * K;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    __shared__ R lds[NS][4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R cr[K][SEG_REGS<R>];
#pragma unroll
        for (int j = 0; j < K; ++j) seg_load<R, VEC>(V + (int64_t)j * ldv2, base, n2, 0, cr[j]);
        int p = K;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            R re, im;
            cseg_dot<R>(cr[r], cr[r], base, n2, re, im);
            pair_put(re, lds[r]);
#pragma unroll
            for (int c = r + 1; c < K; ++c) {
                cseg_dot<R>(cr[r], cr[c], base, n2, re, im);
                pair_put(re, lds[p]);
                pair_put(im, lds[p + 1]);
                p += 2;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < NS) seg_out[(int64_t)threadIdx.x * nseg + s] = pair_total(lds[threadIdx.x]);
        __syncthreads();
    }
}

template <typename R, int K> static int launch_cgram_k(mik_ctx *ctx, int64_t n, const R *V, int64_t ldv)
{
    const bool vec = mik_aligned16(V) && (2 * ldv) % VT<R>::W == 0;
    return launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t nseg) {
        hipLaunchKernelGGL((k_cgram<R, decltype(v)::value, K>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, V, 2 * ldv, (R *)ctx->partials);
    });
}

template <typename R> static int c_gram(mik_ctx *ctx, int64_t n, int k, const void *Vv, int64_t ldv, void *Mv)
{
    const R *V = (const R *)Vv;
    R *M = (R *)Mv;
    const int ns = k * k;
    const int64_t nseg = mik_nseg<R>(2 * n);
    if (nseg == 0) { memset(M, 0, sizeof(R) * 2 * (size_t)ns); return MIK_OK; }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * (size_t)ns * (size_t)nseg));
    switch (k) {
    case 1: MIK_TRY((launch_cgram_k<R, 1>(ctx, n, V, ldv))); break;
    case 2: MIK_TRY((launch_cgram_k<R, 2>(ctx, n, V, ldv))); break;
    case 3: MIK_TRY((launch_cgram_k<R, 3>(ctx, n, V, ldv))); break;
    case 4: MIK_TRY((launch_cgram_k<R, 4>(ctx, n, V, ldv))); break;
    default: MIK_TRY((launch_cgram_k<R, 5>(ctx, n, V, ldv))); break;
    }
    R out[25];
    MIK_TRY(c_sums_to_host<R>(ctx, nseg, ns, out));
    auto at = [&](int r, int c) { return M + 2 * ((size_t)c * k + r); };
    int p = k;
    for (int r = 0; r < k; ++r) {
        at(r, r)[0] = out[r];
        at(r, r)[1] = R(0);
        for (int c = r + 1; c < k; ++c) {
            at(r, c)[0] = out[p]; at(r, c)[1] = out[p + 1];
            at(c, r)[0] = out[p]; at(c, r)[1] = -out[p + 1];                // the lower triangle: the conjugate
            p += 2;
        }
    }
    return MIK_OK;
}

int mik_c_gram(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *M)
{
    return c_typed(dtype, [&](auto r) { return c_gram<decltype(r)>(ctx, n, k, V, ldv, M); });
}

// ---- mik_minres_update with five complex scalars (skew-Hermitian) -- src/minres.jl:115, :138-144 --------------------------------------
// per element, in statement order: v_next *= inv_h3; w = v_curr; w += neg_h1 w_curr; w += neg_h0 w_prev; w *= inv_h2; x += rhs0 w
template <typename R> struct CMinresCoef { R inv_h3[2], neg_h1[2], neg_h0[2], inv_h2[2], rhs0[2]; };

template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cminres_update(int64_t n2, int64_t nseg, R *__restrict__ v_next, const R *__restrict__ v_curr,
                                                              const R *__restrict__ w_curr, const R *__restrict__ w_prev, R *__restrict__ w_next,
                                                              R *__restrict__ x, CMinresCoef<R> cf)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R vn[SEG_REGS<R>], w[SEG_REGS<R>], xx[SEG_REGS<R>], t[SEG_REGS<R>];
        seg_load<R, VEC>(v_next, base, n2, 0, vn);
        seg_load<R, VEC>(v_curr, base, n2, 0, w);
        seg_load<R, VEC>(x, base, n2, 0, xx);
        cseg_scale<R>(vn, cf.inv_h3[0], cf.inv_h3[1]);
        seg_store<R, VEC>(v_next, base, n2, vn);
        if (w_curr) {
            seg_load<R, VEC>(w_curr, base, n2, 0, t);
            cseg_madd<R>(cf.neg_h1[0], cf.neg_h1[1], t, w);
        }
        if (w_prev) {
            seg_load<R, VEC>(w_prev, base, n2, 0, t);
            cseg_madd<R>(cf.neg_h0[0], cf.neg_h0[1], t, w);
        }
        cseg_scale<R>(w, cf.inv_h2[0], cf.inv_h2[1]);
        cseg_madd<R>(cf.rhs0[0], cf.rhs0[1], w, xx);
        seg_store<R, VEC>(w_next, base, n2, w);
        seg_store<R, VEC>(x, base, n2, xx);
    }
}

template <typename R>
static int c_minres_update(mik_ctx *ctx, int64_t n, const void *inv_h3, void *v_next, const void *v_curr, const void *neg_h1, const void *w_curr,
                           const void *neg_h0, const void *w_prev, const void *inv_h2, void *w_next, const void *rhs0, void *x)
{
    CMinresCoef<R> cf{};
    memcpy(cf.inv_h3, inv_h3, sizeof cf.inv_h3);
    if (w_curr) memcpy(cf.neg_h1, neg_h1, sizeof cf.neg_h1);
    if (w_prev) memcpy(cf.neg_h0, neg_h0, sizeof cf.neg_h0);
    memcpy(cf.inv_h2, inv_h2, sizeof cf.inv_h2);
    memcpy(cf.rhs0, rhs0, sizeof cf.rhs0);
    const bool vec = mik_aligned16(v_next) && mik_aligned16(v_curr) && mik_aligned16(w_next) && mik_aligned16(x) && (!w_curr || mik_aligned16(w_curr)) &&
                     (!w_prev || mik_aligned16(w_prev));
    return launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t nseg) {
        hipLaunchKernelGGL((k_cminres_update<R, decltype(v)::value>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, (R *)v_next, (const R *)v_curr,
                           (const R *)w_curr, (const R *)w_prev, (R *)w_next, (R *)x, cf);
    });
}

int mik_c_minres_update(mik_ctx *ctx, int dtype, int64_t n, const void *inv_h3, void *v_next, const void *v_curr, const void *neg_h1, const void *w_curr,
                        const void *neg_h0, const void *w_prev, const void *inv_h2, void *w_next, const void *rhs0, void *x)
{
    return c_typed(dtype, [&](auto r) { return c_minres_update<decltype(r)>(ctx, n, inv_h3, v_next, v_curr, neg_h1, w_curr, neg_h0, w_prev, inv_h2, w_next, rhs0, x); });
}

// ---- mik_bicgstab_mr_update: the complex sibling of k_bicg_mr -- src/bicgstabl.jl:126-131 --------------------------------------------
//   us_0 += sum_{j=1..l} tn_j us_j;  x += sum_{j=0..l-1} tp_{j+1} rs_j;  rs_0 += sum_{j=1..l} tn_j rs_j;  segment sums of |rs_0|^2
// tn_j = (-1 + 0 i) gamma_j and tp_j = (1 + 0 i) gamma_j are formed on the host, as mik_gemv_n forms alpha c_j: the per-element operations
// and their order are those of the three mik_gemv_n calls; x reads rs_0 before its update.
template <typename R> struct CBicgGamma { R tn[16], tp[16]; };           // l <= 8 complex coefficients each

template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cbicg_mr(int64_t n2, int64_t nseg, int l, R *__restrict__ us, int64_t ldu2, R *__restrict__ rs, int64_t ldr2,
                                                        R *__restrict__ x, CBicgGamma<R> gm, R *__restrict__ seg_out)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    __shared__ R lds4[4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R u0[SEG_REGS<R>], r0[SEG_REGS<R>], xx[SEG_REGS<R>];
        seg_load<R, VEC>(us, base, n2, 0, u0);
        seg_load<R, VEC>(rs, base, n2, 0, r0);
        seg_load<R, VEC>(x, base, n2, 0, xx);
        // The multiply-adds are written out here (cx_mul, then one add per component: what cx_madd is): through cseg_madd the ComplexF32
        // instances measured 2 % slower.
#pragma unroll
        for (int q = 0; q < SEG_REGS<R>; q += 2) {                         // x += gamma_1 rs_0 (the not yet updated residual)
            const CxVal<R> p = cx_mul(gm.tp[0], gm.tp[1], r0[q], r0[q + 1]);
            xx[q] = xx[q] + p.re;
            xx[q + 1] = xx[q + 1] + p.im;
        }
        for (int j = 1; j <= l; ++j) {
            R uj[SEG_REGS<R>], rj[SEG_REGS<R>];
            seg_load<R, VEC>(us + (int64_t)j * ldu2, base, n2, 0, uj);
            seg_load<R, VEC>(rs + (int64_t)j * ldr2, base, n2, 0, rj);
            const R nr = gm.tn[2 * (j - 1)], ni = gm.tn[2 * (j - 1) + 1];
#pragma unroll
            for (int q = 0; q < SEG_REGS<R>; q += 2) {
                const CxVal<R> p = cx_mul(nr, ni, uj[q], uj[q + 1]);
                u0[q] = u0[q] + p.re;
                u0[q + 1] = u0[q + 1] + p.im;
                const CxVal<R> t = cx_mul(nr, ni, rj[q], rj[q + 1]);
                r0[q] = r0[q] + t.re;
                r0[q + 1] = r0[q + 1] + t.im;
            }
            if (j < l) {
                const R pr = gm.tp[2 * j], pi = gm.tp[2 * j + 1];
#pragma unroll
                for (int q = 0; q < SEG_REGS<R>; q += 2) {
                    const CxVal<R> p = cx_mul(pr, pi, rj[q], rj[q + 1]);
                    xx[q] = xx[q] + p.re;
                    xx[q + 1] = xx[q + 1] + p.im;
                }
            }
        }
        seg_store<R, VEC>(us, base, n2, u0);
        seg_store<R, VEC>(rs, base, n2, r0);
        seg_store<R, VEC>(x, base, n2, xx);
        const R tot = block_tree_256(cseg_sumsq<R>(r0, base, n2), lds4);
        if (threadIdx.x == 0) seg_out[s] = tot;
    }
}

template <typename R> static int c_bicg_mr(mik_ctx *ctx, int64_t n, int l, void *usv, int64_t ldu, void *rsv, int64_t ldr, void *xv, const void *gv, void *outv)
{
    R *us = (R *)usv, *rs = (R *)rsv, *x = (R *)xv, *out = (R *)outv;
    const R *gamma = (const R *)gv;
    const int64_t nseg = mik_nseg<R>(2 * n);
    if (nseg == 0) { *out = R(0); return MIK_OK; }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * (size_t)nseg));
    CBicgGamma<R> gm{};
    for (int j = 0; j < l; ++j) {
        const CxVal<R> tn = cx_mul(R(-1), R(0), gamma[2 * j], gamma[2 * j + 1]), tp = cx_mul(R(1), R(0), gamma[2 * j], gamma[2 * j + 1]);
        gm.tn[2 * j] = tn.re; gm.tn[2 * j + 1] = tn.im;
        gm.tp[2 * j] = tp.re; gm.tp[2 * j + 1] = tp.im;
    }
    const bool vec = mik_aligned16(us) && mik_aligned16(rs) && mik_aligned16(x) && (2 * ldu) % VT<R>::W == 0 && (2 * ldr) % VT<R>::W == 0;
    MIK_TRY((launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t ns) {
        hipLaunchKernelGGL((k_cbicg_mr<R, decltype(v)::value>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, ns, l, us, 2 * ldu, rs, 2 * ldr, x, gm,
                           (R *)ctx->partials);
    })));
    R ss;
    MIK_TRY(c_sums_to_host<R>(ctx, nseg, 1, &ss));
    return mik_norm_from_sumsq<R>(ctx, 2 * n, rs, ss, out);                 // norm(rs[:, 1])
}

int mik_c_bicgstab_mr_update(mik_ctx *ctx, int dtype, int64_t n, int l, void *us, int64_t ldu, void *rs, int64_t ldr, void *x, const void *gamma, void *out)
{
    return c_typed(dtype, [&](auto r) { return c_bicg_mr<decltype(r)>(ctx, n, l, us, ldu, rs, ldr, x, gamma, out); });
}

// ---- the three QMR sweeps on complex vectors -- src/qmr.jl:70-78, :81, :90-91, :188-197 ---------------------------
// Complex scalars by value as (re, im); with REAL (MIK_SCALAR_REAL and a reduction) a and b are reals that multiply as real x complex.
// The operands are not __restrict__: p_out may be p_prev's storage (a thread reads its elements of a segment before it writes them).
template <typename R> struct CPair { R re, im; };

// y += a x1; y += b x2 (x2 may be NULL); z != NULL: the segment sums of dot(z, y) = sum conj(z_i) y_i, re then im: the bits of mik_dot
template <typename R, bool VEC, bool REAL>
__global__ __launch_bounds__(MIK_BLOCK) void k_caxpy2_dot(int64_t n2, int64_t nseg, const R *x1, const R *x2, R *y, const R *z, CPair<R> a, CPair<R> b,
                                                          R *__restrict__ seg_out)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    __shared__ R lds4[4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R yy[SEG_REGS<R>], t[SEG_REGS<R>];
        seg_load<R, VEC>(y, base, n2, 0, yy);
        seg_load<R, VEC>(x1, base, n2, 0, t);
#pragma unroll
        for (int q = 0; q < SEG_REGS<R>; q += 2) {
            if (REAL) cx_madd_real(a.re, t[q], t[q + 1], yy[q], yy[q + 1]);
            else cx_madd(a.re, a.im, t[q], t[q + 1], yy[q], yy[q + 1]);
        }
        if (x2) {
            seg_load<R, VEC>(x2, base, n2, 0, t);
#pragma unroll
            for (int q = 0; q < SEG_REGS<R>; q += 2) {
                if (REAL) cx_madd_real(b.re, t[q], t[q + 1], yy[q], yy[q + 1]);
                else cx_madd(b.re, b.im, t[q], t[q + 1], yy[q], yy[q + 1]);
            }
        }
        seg_store<R, VEC>(y, base, n2, yy);
        if (z) {
            seg_load<R, VEC>(z, base, n2, 0, t);
            R re, im;
            cseg_dot<R>(t, yy, base, n2, re, im);
            const R tre = block_tree_256(re, lds4);
            if (threadIdx.x == 0) seg_out[s] = tre;
            const R tim = block_tree_256(im, lds4);
            if (threadIdx.x == 0) seg_out[nseg + s] = tim;
        }
    }
}

template <typename R>
static int c_axpy2_dot(mik_ctx *ctx, int64_t n, int real_scalars, const void *av, const void *x1, const void *bv, const void *x2, void *y, const void *z, void *out)
{
    const R *ap = (const R *)av, *bp = (const R *)bv;
    const CPair<R> a{ap[0], real_scalars ? R(0) : ap[1]}, b{x2 ? bp[0] : R(0), (x2 && !real_scalars) ? bp[1] : R(0)};
    const int64_t nseg = mik_nseg<R>(2 * n);
    if (nseg == 0) { if (z) { ((R *)out)[0] = R(0); ((R *)out)[1] = R(0); } return MIK_OK; }
    if (z) MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * 2 * (size_t)nseg));
    const bool vec = mik_aligned16(y) && mik_aligned16(x1) && (!x2 || mik_aligned16(x2)) && (!z || mik_aligned16(z));
    MIK_TRY((launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto v, int grid, int64_t ns) {
        if (real_scalars)
            hipLaunchKernelGGL((k_caxpy2_dot<R, decltype(v)::value, true>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, ns, (const R *)x1, (const R *)x2, (R *)y,
                               (const R *)z, a, b, (R *)ctx->partials);
        else
            hipLaunchKernelGGL((k_caxpy2_dot<R, decltype(v)::value, false>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, ns, (const R *)x1, (const R *)x2, (R *)y,
                               (const R *)z, a, b, (R *)ctx->partials);
    })));
    if (!z) return MIK_OK;
    return c_sums_to_host<R>(ctx, nseg, 2, (R *)out);
}

int mik_c_axpy2_dot(mik_ctx *ctx, int dtype, int64_t n, int real_scalars, const void *a, const void *x1, const void *b, const void *x2, void *y, const void *z,
                    void *out)
{
    return c_typed(dtype, [&](auto r) { return c_axpy2_dot<decltype(r)>(ctx, n, real_scalars, a, x1, b, x2, y, z, out); });
}

// x *= a; y *= b
template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cscal2(int64_t n2, int64_t nseg, R *x, R *y, CPair<R> a, CPair<R> b)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R xx[SEG_REGS<R>], yy[SEG_REGS<R>];
        seg_load<R, VEC>(x, base, n2, 0, xx);
        seg_load<R, VEC>(y, base, n2, 0, yy);
        cseg_scale<R>(xx, a.re, a.im);
        cseg_scale<R>(yy, b.re, b.im);
        seg_store<R, VEC>(x, base, n2, xx);
        seg_store<R, VEC>(y, base, n2, yy);
    }
}

int mik_c_scal2(mik_ctx *ctx, int dtype, int64_t n, const void *a, void *x, const void *b, void *y)
{
    return c_typed(dtype, [&](auto r) {
        using R = decltype(r);
        const CPair<R> ca{((const R *)a)[0], ((const R *)a)[1]}, cb{((const R *)b)[0], ((const R *)b)[1]};
        return launch_segments<R>(ctx, 2 * n, mik_aligned16(x) && mik_aligned16(y), 0, [&](auto v, int grid, int64_t ns) {
            hipLaunchKernelGGL((k_cscal2<R, decltype(v)::value>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, ns, (R *)x, (R *)y, ca, cb);
        });
    });
}

// p = v; p += neg_h1 p_curr (if p_curr); p += neg_h0 p_prev (if p_prev); p *= inv; x += g p; p_out = p
template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cqmr_update(int64_t n2, int64_t nseg, const R *v, const R *p_curr, const R *p_prev, R *p_out, R *x, CPair<R> neg_h1,
                                                           CPair<R> neg_h0, CPair<R> inv, CPair<R> g)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R p[SEG_REGS<R>], xx[SEG_REGS<R>], t[SEG_REGS<R>];
        seg_load<R, VEC>(v, base, n2, 0, p);
        seg_load<R, VEC>(x, base, n2, 0, xx);
        if (p_curr) {
            seg_load<R, VEC>(p_curr, base, n2, 0, t);
            cseg_madd<R>(neg_h1.re, neg_h1.im, t, p);
        }
        if (p_prev) {
            seg_load<R, VEC>(p_prev, base, n2, 0, t);
            cseg_madd<R>(neg_h0.re, neg_h0.im, t, p);
        }
        cseg_scale<R>(p, inv.re, inv.im);
        cseg_madd<R>(g.re, g.im, p, xx);
        seg_store<R, VEC>(p_out, base, n2, p);
        seg_store<R, VEC>(x, base, n2, xx);
    }
}

int mik_c_qmr_update(mik_ctx *ctx, int dtype, int64_t n, const void *v, const void *neg_h1, const void *p_curr, const void *neg_h0, const void *p_prev,
                     const void *inv, const void *g, void *x, void *p_out)
{
    return c_typed(dtype, [&](auto r) {
        using R = decltype(r);
        auto pair = [](const void *p) { return p ? CPair<R>{((const R *)p)[0], ((const R *)p)[1]} : CPair<R>{R(0), R(0)}; };
        const CPair<R> h1 = pair(p_curr ? neg_h1 : nullptr), h0 = pair(p_prev ? neg_h0 : nullptr), ci = pair(inv), cg = pair(g);
        const bool vec = mik_aligned16(v) && mik_aligned16(x) && mik_aligned16(p_out) && (!p_curr || mik_aligned16(p_curr)) && (!p_prev || mik_aligned16(p_prev));
        return launch_segments<R>(ctx, 2 * n, vec, 0, [&](auto vv, int grid, int64_t ns) {
            hipLaunchKernelGGL((k_cqmr_update<R, decltype(vv)::value>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, ns, (const R *)v, (const R *)p_curr,
                               (const R *)p_prev, (R *)p_out, (R *)x, h1, h0, ci, cg);
        });
    });
}

// ---- host: complex LU with partial pivoting -- lu!(view(M, L, L)); ldiv!(gamma, F, view(M, L, 1)), src/bicgstabl.jl:123-125 ------------
// LAPACK getrf's pivot rule (izamax: the first maximum of |re| + |im|); divisions by Smith's scaling (hc_div)
template <typename R> static int c_lu_solve(HC<R> *A, int64_t lda, int n, HC<R> *b)
{
    auto at = [&](int i, int j) -> HC<R> & { return A[(size_t)j * lda + i]; };
    auto cabs1 = [](HC<R> z) { return std::fabs(z.re) + std::fabs(z.im); };
    auto sub = [](HC<R> z, HC<R> w) { return HC<R>{z.re - w.re, z.im - w.im}; };
    for (int j = 0; j < n; ++j) {
        int p = j;
        R best = cabs1(at(j, j));
        for (int i = j + 1; i < n; ++i) { const R a = cabs1(at(i, j)); if (a > best) { best = a; p = i; } }
        if (best == R(0)) return MIK_ERR_SINGULAR;
        if (p != j) {
            for (int c = 0; c < n; ++c) std::swap(at(j, c), at(p, c));
            std::swap(b[j], b[p]);
        }
        const HC<R> piv = at(j, j);
        for (int i = j + 1; i < n; ++i) {
            const HC<R> m = hc_div(at(i, j), piv);
            at(i, j) = m;
            for (int c = j + 1; c < n; ++c) at(i, c) = sub(at(i, c), hc_mul(m, at(j, c)));
            b[i] = sub(b[i], hc_mul(m, b[j]));
        }
    }
    for (int j = n - 1; j >= 0; --j) {
        b[j] = hc_div(b[j], at(j, j));
        const HC<R> t = b[j];
        for (int i = 0; i < j; ++i) b[i] = sub(b[i], hc_mul(t, at(i, j)));
    }
    return MIK_OK;
}

int mik_c_lu_solve(int dtype, void *A, int64_t lda, int n, void *b)
{
    return c_typed(dtype, [&](auto r) { using R = decltype(r); return c_lu_solve<R>((HC<R> *)A, lda, n, (HC<R> *)b); });
}
