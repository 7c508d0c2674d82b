// mik_lobpcg.hip -- the four block entries lobpcg (src/lobpcg.jl) needs beyond the vector entries of mik_core.hip / mik_krylov.hip:
//   mik_spmm           Y = A * X for a block of columns, the operator read once per column block
//   mik_block_gram     G = X' * Y, every entry with the bits of mik_dot
//   mik_block_rdiv     X <- X * inv(R), R upper triangular (CholQR)
//   mik_block_update   the Ritz update of one block triple in one pass
// Kernels: csrc/mik_lobpcg.h; k_block_gram is written in the segment helpers of csrc/mik_kernels.h that k_multidot / k_gram use.
// The complex instances (MIK_C64 / MIK_C32): csrc/mik_lobpcg_complex.h.
#include <algorithm>
#include <vector>

#include "mik_lobpcg.h"
#include "mik_lobpcg_complex.h"

namespace {

unsigned row_grid(mik_ctx *ctx, int64_t n)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + MIK_BLOCK - 1) / MIK_BLOCK, mik_max_grid(ctx)));
}

// ---- mik_spmm ---------------------------------------------------------------------------------
template <typename T, int CB>
int spmm_launch(mik_ctx *ctx, const mik_csr *A, int b, const T *X, int64_t ldx, T *Y, int64_t ldy)
{
    const dim3 grid((unsigned)mik_spmv_nwg(A->n_rows), (unsigned)((b + CB - 1) / CB));
    hipLaunchKernelGGL((k_spmm_rowgather<T, CB>), grid, dim3(MIK_BLOCK), 0, ctx->stream, (int)A->n_rows, b, A->rowptr, A->col, (const T *)A->val, X, ldx,
                       Y, ldy);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
int spmm_impl(mik_ctx *ctx, const mik_csr *A, int b, const T *X, int64_t ldx, T *Y, int64_t ldy)
{
    if (A->n_rows == 0) return MIK_OK;
    if (!A->col || A->n_long) {                             // CSR arrays released, or split-off long rows: column by column
        for (int j = 0; j < b; ++j) MIK_TRY(mik_spmv(ctx, A, X + (int64_t)j * ldx, Y + (int64_t)j * ldy));
        return MIK_OK;
    }
    if (b == 1) return spmm_launch<T, 1>(ctx, A, b, X, ldx, Y, ldy);
    if (b == 2) return spmm_launch<T, 2>(ctx, A, b, X, ldx, Y, ldy);
    if (b <= 4) return spmm_launch<T, 4>(ctx, A, b, X, ldx, Y, ldy);
    return spmm_launch<T, 8>(ctx, A, b, X, ldx, Y, ldy);
}

// ---- mik_block_gram ---------------------------------------------------------------------------
template <typename T>
int gram_impl(mik_ctx *ctx, int64_t n, int p, int q, const T *X, int64_t ldx, const T *Y, int64_t ldy, T *G, int64_t ldg)
{
    const int np = p * q;
    const int64_t nseg = mik_nseg<T>(n);
    if (nseg == 0) {                                        // empty vectors: every dot is +0
        for (int j = 0; j < q; ++j)
            for (int i = 0; i < p; ++i) G[(size_t)j * ldg + i] = T(0);
        return MIK_OK;
    }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * ((size_t)nseg + 1) * (size_t)np));
    T *part = (T *)ctx->partials, *out = part + (size_t)nseg * (size_t)np;
    const int tiles = ((p + MIK_GRAM_TP - 1) / MIK_GRAM_TP) * ((q + MIK_GRAM_TQ - 1) / MIK_GRAM_TQ);
    const dim3 grid((unsigned)std::min<int64_t>(nseg, mik_max_grid(ctx)), (unsigned)tiles);
    const bool vec = mik_aligned16(X) && mik_aligned16(Y) && ldx % VT<T>::W == 0 && ldy % VT<T>::W == 0;
    if (vec) hipLaunchKernelGGL((k_block_gram<T, true>), grid, dim3(MIK_BLOCK), 0, ctx->stream, n, nseg, p, q, X, ldx, Y, ldy, part);
    else hipLaunchKernelGGL((k_block_gram<T, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, n, nseg, p, q, X, ldx, Y, ldy, part);
    MIK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL((k_finalize_store<T>), dim3(np), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)part, nseg, nseg, out, (const int *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    std::vector<T> host((size_t)np);
    const int chunk = (int)(mik_ctx::PUB_BYTES / sizeof(T));
    for (int at = 0; at < np; at += chunk) MIK_TRY(mik_read_scalars<T>(ctx, out + at, std::min(chunk, np - at), host.data() + at));
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < p; ++i) G[(size_t)j * ldg + i] = host[(size_t)j * p + i];
    return MIK_OK;
}

// ---- mik_block_rdiv ---------------------------------------------------------------------------
template <typename T, int S>
int rdiv_launch(mik_ctx *ctx, int64_t n, int s, const T *Rd, T *X, int64_t ldx)
{
    hipLaunchKernelGGL((k_block_rdiv<T, S>), dim3(row_grid(ctx, n)), dim3(MIK_BLOCK), 0, ctx->stream, n, s, Rd, X, ldx);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
int rdiv_impl(mik_ctx *ctx, int64_t n, int s, const T *R, int64_t ldr, T *X, int64_t ldx)
{
    T *Rd = nullptr;
    MIK_TRY(mik_stage_small<T>(ctx, R, s, s, ldr, &Rd));
    if (s <= 4) return rdiv_launch<T, 4>(ctx, n, s, Rd, X, ldx);
    if (s <= 8) return rdiv_launch<T, 8>(ctx, n, s, Rd, X, ldx);
    if (s <= 16) return rdiv_launch<T, 16>(ctx, n, s, Rd, X, ldx);
    return rdiv_launch<T, 32>(ctx, n, s, Rd, X, ldx);
}

// ---- mik_block_update -------------------------------------------------------------------------
template <typename T, int LB>
int update_launch(mik_ctx *ctx, int64_t n, int sx, int b1, int b2, const T *X, int64_t ldx, const T *R, int64_t ldr, const T *P, int64_t ldp,
                  const T *Vd, T *Xout, int64_t ldxo, T *Pout, int64_t ldpo)
{
    hipLaunchKernelGGL((k_block_update<T, LB>), dim3(row_grid(ctx, n)), dim3(MIK_BLOCK), 0, ctx->stream, n, sx, b1, b2, X, ldx, R, ldr, P, ldp, Vd, Xout,
                       ldxo, Pout, ldpo);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
int update_impl(mik_ctx *ctx, int64_t n, int sx, int b1, int b2, const T *X, int64_t ldx, const T *R, int64_t ldr, const T *P, int64_t ldp,
                const T *V, int64_t ldv, T *Xout, int64_t ldxo, T *Pout, int64_t ldpo)
{
    T *Vd = nullptr;
    MIK_TRY(mik_stage_small<T>(ctx, V, sx + b1 + b2, sx, ldv, &Vd));
    if (sx <= 4) return update_launch<T, 4>(ctx, n, sx, b1, b2, X, ldx, R, ldr, P, ldp, Vd, Xout, ldxo, Pout, ldpo);
    if (sx <= 8) return update_launch<T, 8>(ctx, n, sx, b1, b2, X, ldx, R, ldr, P, ldp, Vd, Xout, ldxo, Pout, ldpo);
    if (sx <= 16) return update_launch<T, 16>(ctx, n, sx, b1, b2, X, ldx, R, ldr, P, ldp, Vd, Xout, ldxo, Pout, ldpo);
    return update_launch<T, 32>(ctx, n, sx, b1, b2, X, ldx, R, ldr, P, ldp, Vd, Xout, ldxo, Pout, ldpo);
}

// ---- the complex instances: R = the component type, pointers to interleaved (re, im), leading dimensions in elements ------------
template <typename R, int CB>
int cspmm_launch(mik_ctx *ctx, const mik_csr *A, int b, const R *X, int64_t ldx, R *Y, int64_t ldy)
{
    const int nb = (int)((A->n_rows + MIK_BLOCK - 1) / MIK_BLOCK);
    const dim3 grid((unsigned)std::min(nb, mik_cus(ctx) * MIK_CSPMM_WG_PER_CU), (unsigned)((b + CB - 1) / CB));
    hipLaunchKernelGGL((k_cspmm<R, CB>), grid, dim3(MIK_BLOCK), 0, ctx->stream, (int)A->n_rows, nb, b, A->rowptr, A->col, (const R *)A->val, X, ldx, Y, ldy);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename R>
int cspmm_impl(mik_ctx *ctx, const mik_csr *A, int b, const R *X, int64_t ldx, R *Y, int64_t ldy)
{
    if (A->n_rows == 0) return MIK_OK;
    if (A->c_nlong > 0) {                                   // split-off long rows: column by column
        for (int j = 0; j < b; ++j) MIK_TRY(mik_spmv(ctx, A, X + 2 * (int64_t)j * ldx, Y + 2 * (int64_t)j * ldy));
        return MIK_OK;
    }
    if (b == 1) return cspmm_launch<R, 1>(ctx, A, b, X, ldx, Y, ldy);
    if (b == 2) return cspmm_launch<R, 2>(ctx, A, b, X, ldx, Y, ldy);
    return cspmm_launch<R, MIK_CSPMM_CB>(ctx, A, b, X, ldx, Y, ldy);
}

// G: host, p x q interleaved complex, ldg in elements
template <typename R>
int cgram_impl(mik_ctx *ctx, int64_t n, int p, int q, const R *X, int64_t ldx, const R *Y, int64_t ldy, R *G, int64_t ldg)
{
    const int ns = 2 * p * q;                               // sums: re and im of every pair
    const int64_t nseg = mik_nseg<R>(2 * n);
    if (nseg == 0) {                                        // empty vectors: every dot is (+0, +0)
        for (int j = 0; j < q; ++j)
            for (int i = 0; i < p; ++i) { G[2 * ((size_t)j * ldg + i)] = R(0); G[2 * ((size_t)j * ldg + i) + 1] = R(0); }
        return MIK_OK;
    }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(R) * ((size_t)nseg + 1) * (size_t)ns));
    R *part = (R *)ctx->partials, *out = part + (size_t)nseg * (size_t)ns;
    const int tiles = ((p + MIK_GRAM_TP - 1) / MIK_GRAM_TP) * ((q + MIK_GRAM_TQ - 1) / MIK_GRAM_TQ);
    const dim3 grid((unsigned)std::min<int64_t>(nseg, mik_max_grid(ctx)), (unsigned)tiles);
    const bool vec = mik_aligned16(X) && mik_aligned16(Y) && (2 * ldx) % VT<R>::W == 0 && (2 * ldy) % VT<R>::W == 0;
    if (vec) hipLaunchKernelGGL((k_cblock_gram<R, true>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, p, q, X, 2 * ldx, Y, 2 * ldy, part);
    else hipLaunchKernelGGL((k_cblock_gram<R, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * n, nseg, p, q, X, 2 * ldx, Y, 2 * ldy, part);
    MIK_LAUNCH_CHECK(ctx);
    MIK_TRY(c_finalize<R>(ctx, nseg, ns, out));
    std::vector<R> host((size_t)ns);
    const int chunk = (int)(mik_ctx::PUB_BYTES / sizeof(R));
    for (int at = 0; at < ns; at += chunk) MIK_TRY(mik_read_scalars<R>(ctx, out + at, std::min(chunk, ns - at), host.data() + at));
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < p; ++i) {
            G[2 * ((size_t)j * ldg + i)] = host[2 * ((size_t)j * p + i)];
            G[2 * ((size_t)j * ldg + i) + 1] = host[2 * ((size_t)j * p + i) + 1];
        }
    return MIK_OK;
}

template <typename R, int S, int PW>
int crdiv_launch(mik_ctx *ctx, int64_t n, int s, const R *Rd, R *X, int64_t ldx)
{
    hipLaunchKernelGGL((k_cblock_rdiv<R, S, PW>), dim3(row_grid(ctx, n)), dim3(MIK_BLOCK), 0, ctx->stream, n, s, Rd, X, ldx);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename R>
int crdiv_impl(mik_ctx *ctx, int64_t n, int s, const R *Rh, int64_t ldr, R *X, int64_t ldx)
{
    for (int i = 0; i < s; ++i)                             // the division is by real(R[i, i]): a diagonal that is not real is refused
        if (!(Rh[2 * ((size_t)i * ldr + i) + 1] == R(0)))
            return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_rdiv: R[%d, %d] has a non-zero imaginary part (column %d; the diagonal of the factor must be real)", i, i, i);
    CxVal<R> *Rd = nullptr;
    MIK_TRY(mik_stage_small<CxVal<R>>(ctx, (const CxVal<R> *)Rh, s, s, ldr, &Rd));
    constexpr int PW = CBlk<R>::RDIV_PW;
    if (s <= 4) return crdiv_launch<R, 4, 4>(ctx, n, s, (const R *)Rd, X, ldx);
    if (s <= 8) return crdiv_launch<R, 8, 8>(ctx, n, s, (const R *)Rd, X, ldx);
    if (s <= 16) return crdiv_launch<R, 16, PW>(ctx, n, s, (const R *)Rd, X, ldx);
    return crdiv_launch<R, 32, PW>(ctx, n, s, (const R *)Rd, X, ldx);
}

template <typename R, int LB>
int cupdate_launch(mik_ctx *ctx, int64_t n, int sx, int b1, int b2, const R *X, int64_t ldx, const R *Rm, int64_t ldr, const R *P, int64_t ldp,
                   const R *Vd, R *Xout, int64_t ldxo, R *Pout, int64_t ldpo)
{
    const dim3 grid(row_grid(ctx, n), (unsigned)((sx + LB - 1) / LB));
    hipLaunchKernelGGL((k_cblock_update<R, LB>), grid, dim3(MIK_BLOCK), 0, ctx->stream, n, sx, b1, b2, X, ldx, Rm, ldr, P, ldp, Vd, Xout, ldxo, Pout, ldpo);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename R>
int cupdate_impl(mik_ctx *ctx, int64_t n, int sx, int b1, int b2, const R *X, int64_t ldx, const R *Rm, int64_t ldr, const R *P, int64_t ldp,
                 const R *V, int64_t ldv, R *Xout, int64_t ldxo, R *Pout, int64_t ldpo)
{
    CxVal<R> *Vd = nullptr;
    MIK_TRY(mik_stage_small<CxVal<R>>(ctx, (const CxVal<R> *)V, sx + b1 + b2, sx, ldv, &Vd));
    if (sx <= 4) return cupdate_launch<R, 4>(ctx, n, sx, b1, b2, X, ldx, Rm, ldr, P, ldp, (const R *)Vd, Xout, ldxo, Pout, ldpo);
    if (sx <= 8 || CBlk<R>::UPD_LB == 8) return cupdate_launch<R, 8>(ctx, n, sx, b1, b2, X, ldx, Rm, ldr, P, ldp, (const R *)Vd, Xout, ldxo, Pout, ldpo);
    return cupdate_launch<R, CBlk<R>::UPD_LB>(ctx, n, sx, b1, b2, X, ldx, Rm, ldr, P, ldp, (const R *)Vd, Xout, ldxo, Pout, ldpo);
}

bool block_dtype_ok(int dtype) { return dtype == MIK_F64 || dtype == MIK_F32 || mik_is_complex(dtype); }

}  // namespace

extern "C" int mik_spmm(mik_ctx *ctx, const mik_csr *A, int b, const void *X, int64_t ldx, void *Y, int64_t ldy)
{
    if (!ctx || !A || b < 0) return MIK_ERR_INVALID;
    if (b > MIK_BLK_MAX) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_spmm: b = %d (at most %d columns)", b, MIK_BLK_MAX);
    if (b == 0) return MIK_OK;
    if (!X || !Y || ldx < A->n_cols || ldy < A->n_rows) return mik_fail(ctx, MIK_ERR_INVALID, "mik_spmm: null pointer or leading dimension too small");
    const size_t es = mik_dtype_size(A->dtype);
    if (mik_overlap(X, mik_block_bytes(es, A->n_cols, b, ldx), Y, mik_block_bytes(es, A->n_rows, b, ldy)))
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_spmm: Y overlaps X");
    if (A->dtype == MIK_C64) return cspmm_impl<double>(ctx, A, b, (const double *)X, ldx, (double *)Y, ldy);
    if (A->dtype == MIK_C32) return cspmm_impl<float>(ctx, A, b, (const float *)X, ldx, (float *)Y, ldy);
    if (A->dtype == MIK_F64) return spmm_impl<double>(ctx, A, b, (const double *)X, ldx, (double *)Y, ldy);
    return spmm_impl<float>(ctx, A, b, (const float *)X, ldx, (float *)Y, ldy);
}

extern "C" int mik_block_gram(mik_ctx *ctx, int dtype, int64_t n, int p, int q, const void *X, int64_t ldx, const void *Y, int64_t ldy, void *G,
                              int64_t ldg)
{
    if (!ctx || n < 0 || p < 1 || q < 1 || !block_dtype_ok(dtype)) return MIK_ERR_INVALID;
    if (p > MIK_BLK_MAX || q > MIK_BLK_MAX) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_block_gram: %d x %d (at most %d columns a side)", p, q, MIK_BLK_MAX);
    if (!G || ldg < p || ldx < n || ldy < n || (n && (!X || !Y))) return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_gram: null pointer or leading dimension too small");
    if (dtype == MIK_C64) return cgram_impl<double>(ctx, n, p, q, (const double *)X, ldx, (const double *)Y, ldy, (double *)G, ldg);
    if (dtype == MIK_C32) return cgram_impl<float>(ctx, n, p, q, (const float *)X, ldx, (const float *)Y, ldy, (float *)G, ldg);
    if (dtype == MIK_F64) return gram_impl<double>(ctx, n, p, q, (const double *)X, ldx, (const double *)Y, ldy, (double *)G, ldg);
    return gram_impl<float>(ctx, n, p, q, (const float *)X, ldx, (const float *)Y, ldy, (float *)G, ldg);
}

extern "C" int mik_block_rdiv(mik_ctx *ctx, int dtype, int64_t n, int s, const void *R, int64_t ldr, void *X, int64_t ldx)
{
    if (!ctx || n < 0 || s < 1 || !block_dtype_ok(dtype)) return MIK_ERR_INVALID;
    if (s > MIK_BLK_MAX) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_block_rdiv: s = %d (at most %d columns)", s, MIK_BLK_MAX);
    if (!R || ldr < s || ldx < n || (n && !X)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_rdiv: null pointer or leading dimension too small");
    if (dtype == MIK_C64 && n) return crdiv_impl<double>(ctx, n, s, (const double *)R, ldr, (double *)X, ldx);
    if (dtype == MIK_C32 && n) return crdiv_impl<float>(ctx, n, s, (const float *)R, ldr, (float *)X, ldx);
    if (n == 0) return MIK_OK;
    if (dtype == MIK_F64) return rdiv_impl<double>(ctx, n, s, (const double *)R, ldr, (double *)X, ldx);
    return rdiv_impl<float>(ctx, n, s, (const float *)R, ldr, (float *)X, ldx);
}

extern "C" int mik_block_update(mik_ctx *ctx, int dtype, int64_t n, int sx, int b1, int b2, const void *X, int64_t ldx, const void *R, int64_t ldr,
                                const void *P, int64_t ldp, const void *V, int64_t ldv, void *Xout, int64_t ldxo, void *Pout, int64_t ldpo)
{
    if (!ctx || n < 0 || sx < 1 || b1 < 0 || b2 < 0 || !block_dtype_ok(dtype)) return MIK_ERR_INVALID;
    if (sx > MIK_BLK_MAX || b1 > sx || b2 > sx)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_block_update: needs b1, b2 <= sx <= %d (sx = %d, b1 = %d, b2 = %d)", MIK_BLK_MAX, sx, b1, b2);
    if (b1 == 0 && b2 > 0) return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_update: b2 > 0 needs b1 > 0");
    if (!V || ldv < sx + b1 + b2 || ldx < n || ldxo < n || (n && (!X || !Xout)) || (b1 && (ldr < n || ldpo < n || (n && (!R || !Pout)))) ||
        (b2 && (ldp < n || (n && !P))))
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_update: null pointer or leading dimension too small");
    if (n == 0) return MIK_OK;
    const size_t es = mik_dtype_size(dtype);
    const void *in[3] = {X, R, P};
    const size_t inb[3] = {mik_block_bytes(es, n, sx, ldx), mik_block_bytes(es, n, b1, ldr), mik_block_bytes(es, n, b2, ldp)};
    const size_t xob = mik_block_bytes(es, n, sx, ldxo), pob = mik_block_bytes(es, n, b1 ? sx : 0, ldpo);
    for (int i = 0; i < 3; ++i)
        if (mik_overlap(in[i], inb[i], Xout, xob) || mik_overlap(in[i], inb[i], Pout, pob))
            return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_update: an output overlaps an input");
    if (mik_overlap(Xout, xob, Pout, pob)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_block_update: Xout overlaps Pout");
    if (dtype == MIK_C64)
        return cupdate_impl<double>(ctx, n, sx, b1, b2, (const double *)X, ldx, (const double *)R, ldr, (const double *)P, ldp, (const double *)V, ldv,
                                    (double *)Xout, ldxo, (double *)Pout, ldpo);
    if (dtype == MIK_C32)
        return cupdate_impl<float>(ctx, n, sx, b1, b2, (const float *)X, ldx, (const float *)R, ldr, (const float *)P, ldp, (const float *)V, ldv,
                                   (float *)Xout, ldxo, (float *)Pout, ldpo);
    if (dtype == MIK_F64)
        return update_impl<double>(ctx, n, sx, b1, b2, (const double *)X, ldx, (const double *)R, ldr, (const double *)P, ldp, (const double *)V, ldv,
                                   (double *)Xout, ldxo, (double *)Pout, ldpo);
    return update_impl<float>(ctx, n, sx, b1, b2, (const float *)X, ldx, (const float *)R, ldr, (const float *)P, ldp, (const float *)V, ldv,
                              (float *)Xout, ldxo, (float *)Pout, ldpo);
}
