// mik_svdl.hip -- the two device entries svdl (src/svdl.jl) needs beyond the Krylov helpers of mik_krylov.hip:
//   mik_basis_rotate   Y = V[:, 1:k] * F[:, 1:l], the basis rotation of thickrestart! / harmonicrestart! and the singular vectors
//   mik_svdl_reorth    the double classical Gram-Schmidt of extend! with its norm test, and the normalisation that follows it
// Kernels: k_basis_rotate (csrc/mik_svdl.h); the two sweeps of mik_svdl_reorth are k_multidot / k_gemv_n themselves (csrc/mik_kernels.h,
// SQ = true: the squared norm rides on the sweep), launched as mik_gemv_t / mik_gemv_n launch them.
#include <algorithm>
#include <cmath>

#include "mik_svdl.h"

namespace {

template <typename T, int LB>
int rotate_launch(mik_ctx *ctx, int64_t n, int k, int l, const T *V, int64_t ldv, const T *Fd, T *Y, int64_t ldy)
{
    constexpr int W = VT<T>::W;
    const int64_t groups = (n + W - 1) / W;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + MIK_BLOCK - 1) / MIK_BLOCK, mik_max_grid(ctx)));
    const dim3 grid(gx, (unsigned)((l + LB - 1) / LB));
    const bool vec = mik_aligned16(V) && mik_aligned16(Y) && ldv % W == 0 && ldy % W == 0;
    if (vec) hipLaunchKernelGGL((k_basis_rotate<T, true, LB>), grid, dim3(MIK_BLOCK), 0, ctx->stream, n, k, l, V, ldv, Fd, Y, ldy);
    else hipLaunchKernelGGL((k_basis_rotate<T, false, LB>), grid, dim3(MIK_BLOCK), 0, ctx->stream, n, k, l, V, ldv, Fd, Y, ldy);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
int rotate_impl(mik_ctx *ctx, int64_t n, int k, int l, const T *V, int64_t ldv, const T *F, int64_t ldf, T *Y, int64_t ldy)
{
    T *Fd = nullptr;
    MIK_TRY(mik_stage_small<T>(ctx, F, k, l, ldf, &Fd));
    if (l <= 8) return rotate_launch<T, 8>(ctx, n, k, l, V, ldv, Fd, Y, ldy);
    if (l <= 16) return rotate_launch<T, 16>(ctx, n, k, l, V, ldv, Fd, Y, ldy);
    return rotate_launch<T, 32>(ctx, n, k, l, V, ldv, Fd, Y, ldy);
}

template <typename T> int sumsq_to_norm(mik_ctx *ctx, int64_t n, const T *x, const T *dev, T *out)
{
    T t;
    MIK_TRY(mik_read_scalars<T>(ctx, dev, 1, &t));
    return mik_norm_from_sumsq<T>(ctx, n, x, t, out);       // include/mik.h "Norms" (may use ctx->partials and the tail of ctx->coef)
}

// Coefficient area (elements of T): [0, k) = h = Q' q, [k] = sum of squares of q before the pass, [k + 1] = after the update.
template <typename T>
int reorth_impl(mik_ctx *ctx, int64_t n, int k, const T *Q, int64_t ldq, T *q, T alpha, T *beta_out, int *passes_out)
{
    if ((size_t)(k + 2) * sizeof(T) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_svdl_reorth: k = %d too large", k);
    *passes_out = 1;
    if (n == 0) { *beta_out = T(0); return MIK_OK; }
    const int64_t nseg = mik_nseg<T>(n);
    const int nt = mik_basis_nt<T>(n, k);
    T *hd = (T *)ctx->coef;
    T old = T(0), nw = T(0);
    int passes = 0;
    for (;;) {
        ++passes;
        // sweep 1: h = Q' q, and on the first pass oldqnorm from the same read of q   -- src/svdl.jl:569-570 (:572)
        MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)nseg * (size_t)(k + 1)));
        MIK_TRY((launch_multidot<T, true>(ctx, n, k, Q, ldq, q, hd, nt)));
        if (passes == 1) MIK_TRY(sumsq_to_norm<T>(ctx, n, q, hd + k, &old));       // q is still the old vector if the scaled recomputation is needed
        if (k == 0) { nw = old; break; }
        // sweep 2: q -= Q h, and norm(q) from the same sweep   -- :570-571 (:572, :576)
        MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)nseg));
        MIK_TRY((launch_gemv_n<T, true>(ctx, n, k, Q, ldq, hd, T(-1), q, nt)));
        hipLaunchKernelGGL((k_finalize_store<T>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)ctx->partials, nseg, (int64_t)0, hd + k + 1, (const int *)nullptr);
        MIK_LAUNCH_CHECK(ctx);
        MIK_TRY(sumsq_to_norm<T>(ctx, n, q, hd + k + 1, &nw));
        if (passes == 2 || !(nw <= alpha * old)) break;                             // :571
    }
    if (k == 0 && nw <= alpha * old) passes = 2;            // (the second pass over an empty basis changes nothing)
    *passes_out = passes;
    *beta_out = nw;                                         // :576
    if (nw == T(0)) return MIK_OK;                          // the caller decides (the reference would fill q with Inf / NaN)
    OpScal<T> sc{q, coef_val<T>(T(1) / nw)};               // :577
    return launch_map<T>(ctx, n, sc, mik_aligned16(q), (T *)nullptr, nullptr);
}

}  // namespace

extern "C" int mik_basis_rotate(mik_ctx *ctx, int dtype, int64_t n, int k, int l, const void *V, int64_t ldv, const void *F, int64_t ldf,
                                void *Y, int64_t ldy)
{
    if (!ctx || n < 0 || (dtype != MIK_F64 && dtype != MIK_F32)) return MIK_ERR_INVALID;
    if (l < 1 || k < l || k > MIK_ROT_MAX)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_basis_rotate: needs 1 <= l <= k <= %d (k = %d, l = %d)", MIK_ROT_MAX, k, l);
    if (!F || ldf < k || ldv < n || ldy < n || (n && (!V || !Y))) return mik_fail(ctx, MIK_ERR_INVALID, "mik_basis_rotate: null pointer or leading dimension too small");
    if (n == 0) return MIK_OK;
    const size_t es = mik_dtype_size(dtype);
    if (mik_overlap(V, mik_block_bytes(es, n, k, ldv), Y, mik_block_bytes(es, n, l, ldy)))
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_basis_rotate: Y overlaps V");
    if (dtype == MIK_F64) return rotate_impl<double>(ctx, n, k, l, (const double *)V, ldv, (const double *)F, ldf, (double *)Y, ldy);
    return rotate_impl<float>(ctx, n, k, l, (const float *)V, ldv, (const float *)F, ldf, (float *)Y, ldy);
}

extern "C" int mik_svdl_reorth(mik_ctx *ctx, int dtype, int64_t n, int k, const void *Q, int64_t ldq, void *q, const void *alpha,
                               void *beta_out, int *passes_out)
{
    if (!ctx || n < 0 || k < 0 || !alpha || !beta_out || !passes_out || (n && !q) || (n && k && (!Q || ldq < n))) return MIK_ERR_INVALID;
    if (dtype == MIK_F64) return reorth_impl<double>(ctx, n, k, (const double *)Q, ldq, (double *)q, *(const double *)alpha, (double *)beta_out, passes_out);
    if (dtype == MIK_F32) return reorth_impl<float>(ctx, n, k, (const float *)Q, ldq, (float *)q, *(const float *)alpha, (float *)beta_out, passes_out);
    return MIK_ERR_INVALID;
}
