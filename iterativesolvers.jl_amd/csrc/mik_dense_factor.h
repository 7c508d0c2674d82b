// mik_dense_factor.h -- the host side that the dense factorisations (csrc/mik_dense_lu.hip, csrc/mik_dense_chol.hip) share: the handle's
// common fields, its allocation behind create's argument checks, its release, the overlap checks of a solve, the flag a failing column
// is recorded in, the dispatch on the element type, and a block solve's plan, refusals, workspace and passes.  `entry` is the exported entry's name, for the message.
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
    void *block = nullptr;           // n x MIK_DS_G elements: the workspace of a block solve, allocated at the first one and kept
    int64_t launches_factor = 0;
    int64_t bytes = 0;
};

inline unsigned dense_grid(int count, int per) { return (unsigned)((count + per - 1) / per); }

template <typename H>
void dense_free(H *F)
{
    if (!F) return;
    if (F->ctx) { (void)hipSetDevice(F->ctx->device); (void)hipStreamSynchronize(F->ctx->stream); }
    for (void *p : {F->work, (void *)F->aux, F->block})
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

// ---- a block solve: Y[:, 0:nrhs) = F \ X[:, 0:nrhs), column-major with the leading dimensions ldy and ldx.  It runs in passes of at most
// MIK_DS_G columns through the handle's block workspace; a pass is the launches of one vector solve, each over the pass's groups of NB
// columns (grid y), NB = de_block<E>::NB right-hand sides per lane.
struct dense_block_plan { int nb = 0, g = MIK_DS_G; int64_t passes = 0, launches = 0, bytes = 0; };

inline int dense_block_nb(int dtype) { return dtype == MIK_C64 ? de_block<de_cx<double>>::NB : dtype == MIK_C32 ? de_block<de_cx<float>>::NB : dtype == MIK_F64 ? de_block<double>::NB : de_block<float>::NB; }

// launches_solve: the launches of one vector solve of this handle.  bytes: the block workspace, whether or not it has been allocated yet.
inline dense_block_plan dense_block_plan_of(const mik_dense_factor *F, int64_t nrhs, int64_t launches_solve)
{
    dense_block_plan p;
    p.nb = dense_block_nb(F->dtype);
    p.passes = nrhs < 1 ? 0 : (nrhs + MIK_DS_G - 1) / MIK_DS_G;
    p.launches = p.passes * launches_solve;
    p.bytes = (int64_t)F->n * MIK_DS_G * (int64_t)mik_dtype_size(F->dtype);
    return p;
}

// the refusals of a block solve, before anything is launched or allocated: Y may be X with the same leading dimension, but the blocks may
// not overlap otherwise, nor the factors.  A block's extent is from its first element to the last row of its last column.
inline int dense_check_block(const mik_dense_factor *F, const char *entry, const void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs)
{
    if (nrhs < 1) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: nrhs = %lld (need nrhs >= 1)", entry, (long long)nrhs);
    if (ldy < F->n || ldx < F->n)
        return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ldy = %lld, ldx = %lld (need both >= n = %d)", entry, (long long)ldy, (long long)ldx, F->n);
    const size_t es = mik_dtype_size(F->dtype), all = (size_t)F->ld * (size_t)F->n * es;
    const size_t ybytes = ((size_t)(nrhs - 1) * (size_t)ldy + (size_t)F->n) * es, xbytes = ((size_t)(nrhs - 1) * (size_t)ldx + (size_t)F->n) * es;
    if (Y == X ? ldy != ldx : mik_overlap(Y, ybytes, X, xbytes))
        return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: Y and X overlap without being the same block (equal pointers and leading dimensions)", entry);
    if (mik_overlap(Y, ybytes, F->A, all) || mik_overlap(X, xbytes, F->A, all)) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: a block overlaps the factors", entry);
    (void)hipSetDevice(F->ctx->device);
    return MIK_OK;
}

inline int dense_block_reserve(mik_dense_factor *F)
{
    if (!F->block) MIK_HIP(F->ctx, hipMalloc(&F->block, (size_t)F->n * MIK_DS_G * mik_dtype_size(F->dtype)));
    return MIK_OK;
}

// the passes: pass(t, y, x, cols), called with pointers of the element type, enqueues the `cols` columns from y / x through the workspace t
template <bool COMPLEX, typename Pass>
int dense_block_passes(mik_dense_factor *F, void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs, Pass &&pass)
{
    MIK_TRY(dense_block_reserve(F));
    return dense_dispatch<COMPLEX>(F->dtype, [&](auto e) {
        using E = decltype(e);
        for (int64_t c = 0; c < nrhs; c += MIK_DS_G)
            MIK_TRY(pass((E *)F->block, (E *)Y + c * ldy, (const E *)X + c * ldx, (int)std::min<int64_t>(MIK_DS_G, nrhs - c)));
        return (int)MIK_OK;
    });
}

inline int dense_block_query(const mik_dense_factor *F, int64_t nrhs, int64_t launches_solve, int64_t *nb, int64_t *g, int64_t *passes, int64_t *launches, int64_t *bytes)
{
    const dense_block_plan p = dense_block_plan_of(F, nrhs, launches_solve);
    if (nb) *nb = p.nb;
    if (g) *g = p.g;
    if (passes) *passes = p.passes;
    if (launches) *launches = p.launches;
    if (bytes) *bytes = p.bytes;
    return MIK_OK;
}
