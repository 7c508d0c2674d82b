// mik_dense_factor.h -- the host side that the dense factorisations (csrc/mik_dense_lu.hip, csrc/mik_dense_chol.hip) share: the handle's
// common fields, its allocation behind create's argument checks, its release, the overlap checks of a solve, the flag a failing column
// is recorded in, and the dispatch on the element type.  `entry` is the exported entry's name, for the message.
#pragma once
#include "mik_internal.h"
#include "mik_dense_elem.h"

#include <new>

struct mik_dense_factor {
    mik_ctx *ctx = nullptr;
    int dtype = MIK_F64;
    int n = 0;
    int64_t ld = 0;
    void *A = nullptr;               // the caller's matrix, now its factors
    void *work = nullptr;            // n elements: the right-hand side, then the accumulators of both substitutions
    int *aux = nullptr;              // device integers of the handle's own (lu: the interchanges as one gather; cholesky: the flag)
    int64_t launches_factor = 0;
    int64_t bytes = 0;
};

inline unsigned dense_grid(int count, int per) { return (unsigned)((count + per - 1) / per); }

template <typename H>
void dense_free(H *F)
{
    if (!F) return;
    if (F->ctx) { (void)hipSetDevice(F->ctx->device); (void)hipStreamSynchronize(F->ctx->stream); }
    for (void *p : {F->work, (void *)F->aux})
        if (p) (void)hipFree(p);
    delete F;
}

// create, after the entry's own dtype check: the shape checks, the handle with its common fields, its work vector and aux (n integers if
// aux_per_row, else one)
template <typename H>
int dense_new(mik_ctx *ctx, const char *entry, void *A, int64_t n, int64_t ld, int dtype, bool aux_per_row, H **out)
{
    if (n < 1 || ld < n) return mik_fail(ctx, MIK_ERR_MISMATCH, "%s: n = %lld, ld = %lld (need 1 <= n <= ld)", entry, (long long)n, (long long)ld);
    if (n > (int64_t)std::numeric_limits<int>::max() - MIK_DS_W) return mik_fail(ctx, MIK_ERR_NOTIMPL, "%s: n >= 2^31 - 64", entry);
    H *F = new (std::nothrow) H();
    if (!F) return mik_fail(ctx, MIK_ERR_NOMEM, "%s: host allocation failed", entry);
    *out = F;
    F->ctx = ctx; F->dtype = dtype; F->n = (int)n; F->ld = ld; F->A = A;
    (void)hipSetDevice(ctx->device);
    const size_t vec = std::max<size_t>((size_t)n * mik_dtype_size(dtype), 16), aux_bytes = std::max<size_t>((aux_per_row ? (size_t)n : 1) * sizeof(int), 16);
    MIK_HIP(ctx, hipMalloc(&F->work, vec));
    MIK_HIP(ctx, hipMalloc((void **)&F->aux, aux_bytes));
    F->bytes = (int64_t)(vec + aux_bytes);
    return MIK_OK;
}

// solve: y may be x, but neither may overlap the other otherwise, nor the factors
inline int dense_check_solve(const mik_dense_factor *F, const char *entry, const void *y, const void *x)
{
    const size_t es = mik_dtype_size(F->dtype), bytes = (size_t)F->n * es, all = (size_t)F->ld * (size_t)F->n * es;
    if (y != x && mik_overlap(y, bytes, x, bytes)) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: y and x overlap without being equal", entry);
    if (mik_overlap(y, bytes, F->A, all) || mik_overlap(x, bytes, F->A, all)) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: a vector overlaps the factors", entry);
    (void)hipSetDevice(F->ctx->device);
    return MIK_OK;
}

// The first failing column: the kernels atomicMin their column into *flag.  Armed with 0x7f7f7f7f, above every column index, before the
// first launch; read once after the last one -- the factorisation's only host synchronisation.
inline int dense_flag_arm(mik_ctx *ctx, int *flag)
{
    MIK_HIP(ctx, hipMemsetAsync(flag, 0x7f, sizeof(int), ctx->stream));
    return MIK_OK;
}
inline int dense_flag_read(mik_ctx *ctx, const int *flag, int *first)
{
    MIK_HIP(ctx, hipMemcpyAsync(first, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIK_OK;
}

// fn(E{}) with the element type of dtype; COMPLEX: the two complex types are offered too
template <bool COMPLEX, typename Fn>
int dense_dispatch(int dtype, Fn &&fn)
{
    if (dtype == MIK_F64) return fn(double{});
    if constexpr (COMPLEX) {
        if (dtype == MIK_C64) return fn(de_cx<double>{});
        if (dtype == MIK_C32) return fn(de_cx<float>{});
    }
    return fn(float{});
}
