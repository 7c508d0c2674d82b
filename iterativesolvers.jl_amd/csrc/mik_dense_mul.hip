// mik_dense_mul.hip -- the dense operator: mul!(y, A, x) and mul!(y, adjoint(A), x) on a column-major device matrix, and the
// mik_mul_fn callbacks that put it under the fused iterables (mik_cg_create_op / mik_gmres_create_op) with no host-language frame
// per product.
//
// The handle owns its workspace -- the chunk partials of the N form and the segment sums of the T form share one allocation made in
// create; the partials of the block product Y = A X live in a second allocation made by mik_dense_block_reserve -- and never touches ctx->partials / ctx->coef: the callback runs in the middle of a fused CG / GMRES step that may hold
// state there.  Nothing is allocated per call; every call is asynchronous on the ctx stream; no workgroup waits for another.
#include "mik_internal.h"
#include "mik_dense_mul.h"
#include "mik_dense_cmul.h"

#include <new>

struct mik_dense {
    mik_ctx *ctx = nullptr;
    int dtype = MIK_F64;
    int64_t m = 0, n = 0, lda = 0;
    const void *A = nullptr;
    void *work = nullptr;            // N: [chunks][m_pad] partials;  T: [n][segments of m] segment sums
    int64_t m_pad = 0;               // m rounded up to whole workgroups of the N form (keeps every partial column 16-byte aligned)
                                     // complex dtypes (csrc/mik_dense_cmul.h): the same layouts in complex elements, the segment sums as [n][re, im][segments]
    void *bwork = nullptr;           // block form: [right-hand side of the group][chunk][m_pad] partials of ONE group; never shared with `work`
    size_t bwork_bytes = 0;
    bool breserved = false;          // mik_dense_block_reserve has run (one chunk needs no workspace: bwork stays null)
    int bmin = 0;                    // development override of MIK_DM_GW_MIN (mik_dev_dense_block_min_width); 0 = the default
};

namespace {

inline int64_t dm_chunks(int64_t n) { return (n + MIK_DM_C - 1) / MIK_DM_C; }

// The launch plan of one call: which kernel variant, which grid, how many chunks / column batches and segments its loops walk.  dm_mul_n /
// dm_mul_t launch what it says and mik_dev_dense_plan (include/mik_dev.h) reports it: one computation, so the two cannot drift apart.
// A call with an empty dimension launches no product kernel: its plan is all zero (the T form still reports its segments).
struct dm_plan {
    int vec = 0, streamed = 0;
    int64_t gx = 0, gy = 0, cols = 0, nseg = 0;      // cols: chunks of the N form, column batches of the T form; nseg: segments of the T form
};

// a matrix the caches cannot keep is streamed past them
template <typename T> inline int dm_streamed(int64_t m, int64_t n) { return (double)m * (double)n * sizeof(T) > MIK_DM_STREAM_BYTES ? 1 : 0; }

template <typename T>
dm_plan dm_plan_n(const mik_dense *D, const T *x, const T *y)
{
    (void)x;
    dm_plan p;
    const int64_t m = D->m, n = D->n;
    if (m == 0 || n == 0) return p;
    p.cols = dm_chunks(n);
    const T *out = p.cols == 1 ? y : (const T *)D->work;
    p.vec = mik_aligned16(D->A) && D->lda % VT<T>::W == 0 && mik_aligned16(out);
    p.streamed = dm_streamed<T>(m, n);
    // at most 4 workgroups per compute unit, all resident at once: a workgroup walks its chunks c, c + grid.y, ... in turn (measured neutral
    // against one workgroup per chunk, scripts/micro/dense_chunk.hip; it bounds the launch for very wide matrices)
    p.gx = (m + MIK_DM_R - 1) / MIK_DM_R;
    p.gy = std::min<int64_t>(p.cols, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(D->ctx) / p.gx)));
    return p;
}

template <typename T>
dm_plan dm_plan_t(const mik_dense *D, const T *x, const T *y)
{
    (void)y;
    dm_plan p;
    const int64_t m = D->m, n = D->n;
    p.nseg = mik_nseg<T>(m);
    if (n == 0 || p.nseg == 0) return p;
    p.vec = mik_aligned16(D->A) && D->lda % VT<T>::W == 0 && mik_aligned16(x);
    p.streamed = dm_streamed<T>(m, n);
    p.cols = (n + MIK_DM_TCOLS - 1) / MIK_DM_TCOLS;
    p.gx = std::min<int64_t>(p.nseg, mik_max_grid(D->ctx));
    p.gy = std::min<int64_t>(p.cols, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(D->ctx) / p.gx)));      // as in the N form
    return p;
}

template <typename T>
int dm_mul_n(mik_dense *D, const T *x, T *y)
{
    mik_ctx *ctx = D->ctx;
    const int64_t m = D->m, n = D->n;
    if (m == 0) return MIK_OK;
    if (n == 0) {                                             // the empty sum: +0
        MIK_HIP(ctx, hipMemsetAsync(y, 0, sizeof(T) * (size_t)m, ctx->stream));
        return MIK_OK;
    }
    const dm_plan p = dm_plan_n<T>(D, x, y);
    const int64_t nc = p.cols;
    T *out = nc == 1 ? y : (T *)D->work;
    const bool vec = p.vec != 0;
    const int nt = p.streamed;
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    if (vec && nt) hipLaunchKernelGGL((k_dense_n<T, true, true, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, x, out, D->m_pad);
    else if (vec) hipLaunchKernelGGL((k_dense_n<T, true, false, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, x, out, D->m_pad);
    else hipLaunchKernelGGL((k_dense_n<T, false, false, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, x, out, D->m_pad);
    MIK_LAUNCH_CHECK(ctx);
    if (nc > 1) {
        hipLaunchKernelGGL((k_dense_n_combine<T, MIK_DM_PF>), dim3((unsigned)((m + MIK_DM_CB - 1) / MIK_DM_CB)), dim3(MIK_DM_CB), 0, ctx->stream, m, nc, (const T *)out, D->m_pad, y, (int64_t)0, (int64_t)0);
        MIK_LAUNCH_CHECK(ctx);
    }
    return MIK_OK;
}

// ---- block form: Y[:, j] = A X[:, j], j < b ---------------------------------------------------------------------------------------------
// b right-hand sides run as groups of MIK_DM_GW, one after another on the stream (which makes the reuse of the one-group workspace safe): A is
// read once per group.  A last group narrower than MIK_DM_GW_MIN runs column by column through dm_mul_n instead -- the bits are the same by
// construction (dm_rows is the one body of both kernels), the choice is one of time alone.
constexpr int MIK_DM_GW_MIN = 2;

struct dm_bplan {
    int vec = 0, streamed = 0, groups = 0, last_w = 0, vector_cols = 0;     // groups: launches of the block kernel; vector_cols: columns left to dm_mul_n
    int64_t gx = 0, gy = 0, chunks = 0;
};

template <typename T>
dm_bplan dm_plan_nb(const mik_dense *D, int b, const T *X, int64_t ldx, const T *Y, int64_t ldy)
{
    dm_bplan p;
    const int64_t m = D->m, n = D->n;
    if (m == 0 || n == 0 || b <= 0) return p;
    const int wmin = D->bmin > 0 ? D->bmin : MIK_DM_GW_MIN;
    const int last = b % MIK_DM_GW ? b % MIK_DM_GW : MIK_DM_GW;
    p.groups = (b + MIK_DM_GW - 1) / MIK_DM_GW;
    p.last_w = last;
    if (last < wmin) { p.vector_cols = last; p.groups -= 1; p.last_w = p.groups ? MIK_DM_GW : 0; }
    if (p.groups == 0) {                                       // every column goes through the vector kernels: their plan, for column 0
        const dm_plan v = dm_plan_n<T>(D, X, Y);
        p.vec = v.vec; p.streamed = v.streamed; p.gx = v.gx; p.gy = v.gy; p.chunks = v.cols;
        return p;
    }
    p.chunks = dm_chunks(n);
    // one chunk: the product kernel stores into Y itself, so every column of Y has to start on a 16-byte boundary for the 16-byte variant
    const bool out16 = p.chunks == 1 ? (mik_aligned16(Y) && ldy % VT<T>::W == 0) : true;
    p.vec = mik_aligned16(D->A) && D->lda % VT<T>::W == 0 && out16;
    p.streamed = dm_streamed<T>(m, n);
    p.gx = (m + MIK_DM_R - 1) / MIK_DM_R;                       // the grid of the vector form
    p.gy = std::min<int64_t>(p.chunks, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(D->ctx) / p.gx)));
    return p;
}

int dm_block_reserve(mik_dense *D)
{
    if (D->breserved) return MIK_OK;
    const int64_t nc = dm_chunks(D->n);
    if (nc > 1 && D->m > 0) {
        const size_t bytes = mik_dtype_size(D->dtype) * (size_t)MIK_DM_GW * (size_t)nc * (size_t)D->m_pad;
        (void)hipSetDevice(D->ctx->device);
        const hipError_t e = hipMalloc(&D->bwork, bytes);
        if (e != hipSuccess) {
            D->bwork = nullptr;
            return mik_fail(D->ctx, e == hipErrorOutOfMemory ? MIK_ERR_NOMEM : MIK_ERR_HIP, "mik_dense_block_reserve: hipMalloc of %zu bytes failed: %s", bytes,
                            hipGetErrorString(e));
        }
        D->bwork_bytes = bytes;
    }
    D->breserved = true;
    return MIK_OK;
}

template <typename T>
int dm_mm(mik_dense *D, int b, const T *X, int64_t ldx, T *Y, int64_t ldy)
{
    mik_ctx *ctx = D->ctx;
    const int64_t m = D->m, n = D->n;
    if (n == 0) {                                             // the empty sum: +0 in every column
        MIK_HIP(ctx, hipMemset2DAsync(Y, sizeof(T) * (size_t)ldy, 0, sizeof(T) * (size_t)m, (size_t)b, ctx->stream));
        return MIK_OK;
    }
    const dm_bplan p = dm_plan_nb<T>(D, b, X, ldx, Y, ldy);
    const int64_t nc = p.chunks;
    if (p.groups > 0 && nc > 1) {
        const int rc = dm_block_reserve(D);
        if (rc != MIK_OK) return rc;
    }
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    const dim3 cgrid((unsigned)((m + MIK_DM_CB - 1) / MIK_DM_CB));
    for (int g = 0; g < p.groups; ++g) {
        const int w = g + 1 < p.groups ? MIK_DM_GW : p.last_w;
        const T *Xg = X + (int64_t)g * MIK_DM_GW * ldx;
        T *Yg = Y + (int64_t)g * MIK_DM_GW * ldy;
        T *out = nc == 1 ? Yg : (T *)D->bwork;
        const int64_t col_stride = nc == 1 ? ldy : nc * D->m_pad;
        if (p.vec && p.streamed) hipLaunchKernelGGL((k_dense_nb<T, true, true, MIK_DM_C, MIK_DM_GW>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, Xg, ldx, w, out, col_stride, D->m_pad);
        else if (p.vec) hipLaunchKernelGGL((k_dense_nb<T, true, false, MIK_DM_C, MIK_DM_GW>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, Xg, ldx, w, out, col_stride, D->m_pad);
        else hipLaunchKernelGGL((k_dense_nb<T, false, false, MIK_DM_C, MIK_DM_GW>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const T *)D->A, D->lda, Xg, ldx, w, out, col_stride, D->m_pad);
        MIK_LAUNCH_CHECK(ctx);
        if (nc > 1) {
            hipLaunchKernelGGL((k_dense_n_combine<T, MIK_DM_PF>), dim3(cgrid.x, (unsigned)w), dim3(MIK_DM_CB), 0, ctx->stream, m, nc, (const T *)out, D->m_pad, Yg, col_stride, ldy);
            MIK_LAUNCH_CHECK(ctx);
        }
    }
    for (int j = b - p.vector_cols; j < b; ++j) {
        const int rc = dm_mul_n<T>(D, X + (int64_t)j * ldx, Y + (int64_t)j * ldy);
        if (rc != MIK_OK) return rc;
    }
    return MIK_OK;
}

template <typename T>
int dm_mul_t(mik_dense *D, const T *x, T *y)
{
    mik_ctx *ctx = D->ctx;
    const int64_t m = D->m, n = D->n;
    if (n == 0) return MIK_OK;
    const dm_plan p = dm_plan_t<T>(D, x, y);
    const int64_t nseg = p.nseg;
    if (nseg == 0) {                                          // empty columns: every dot is +0
        MIK_HIP(ctx, hipMemsetAsync(y, 0, sizeof(T) * (size_t)n, ctx->stream));
        return MIK_OK;
    }
    const bool vec = p.vec != 0;
    const int nt = p.streamed;
    T *part = (T *)D->work;
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    if (vec && nt) hipLaunchKernelGGL((k_dense_t<T, true, true>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, nseg, n, (const T *)D->A, D->lda, x, part);
    else if (vec) hipLaunchKernelGGL((k_dense_t<T, true, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, nseg, n, (const T *)D->A, D->lda, x, part);
    else hipLaunchKernelGGL((k_dense_t<T, false, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, nseg, n, (const T *)D->A, D->lda, x, part);
    MIK_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL((k_finalize_store<T>), dim3((unsigned)n), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)part, nseg, nseg, y, (const int *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// ---- complex element types (csrc/mik_dense_cmul.h; R: the component type) -------------------------------------------------------------
// The same plans over the same struct: the N form owns MIK_CDM_R rows per workgroup, the T form walks the 2 m reals of a column.
inline const char *cdm_name(int dtype) { return dtype == MIK_C64 ? "ComplexF64" : "ComplexF32"; }

template <typename R>
dm_plan cdm_plan_n(const mik_dense *D, const R *x, const R *y)
{
    (void)x;
    dm_plan p;
    const int64_t m = D->m, n = D->n;
    if (m == 0 || n == 0) return p;
    p.cols = dm_chunks(n);
    const R *out = p.cols == 1 ? y : (const R *)D->work;
    p.vec = mik_aligned16(D->A) && (2 * D->lda) % VT<R>::W == 0 && mik_aligned16(out);
    p.streamed = (double)m * (double)n * 2.0 * sizeof(R) > MIK_DM_STREAM_BYTES ? 1 : 0;
    p.gx = (m + MIK_CDM_R - 1) / MIK_CDM_R;
    p.gy = std::min<int64_t>(p.cols, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(D->ctx) / p.gx)));      // as in the real N form
    return p;
}

template <typename R>
dm_plan cdm_plan_t(const mik_dense *D, const R *x, const R *y)
{
    (void)y;
    dm_plan p;
    const int64_t m = D->m, n = D->n;
    p.nseg = mik_nseg<R>(2 * m);
    if (n == 0 || p.nseg == 0) return p;
    p.vec = mik_aligned16(D->A) && (2 * D->lda) % VT<R>::W == 0 && mik_aligned16(x);
    p.streamed = (double)m * (double)n * 2.0 * sizeof(R) > MIK_DM_STREAM_BYTES ? 1 : 0;
    p.cols = (n + MIK_CDM_TCOLS - 1) / MIK_CDM_TCOLS;
    p.gx = std::min<int64_t>(p.nseg, mik_max_grid(D->ctx));
    p.gy = std::min<int64_t>(p.cols, std::max<int64_t>(1, std::min<int64_t>(65535, 4 * (int64_t)mik_cus(D->ctx) / p.gx)));
    return p;
}

template <typename R>
int cdm_mul_n(mik_dense *D, const R *x, R *y)
{
    mik_ctx *ctx = D->ctx;
    const int64_t m = D->m, n = D->n;
    if (m == 0) return MIK_OK;
    if (n == 0) {                                             // the empty sum: (+0, +0)
        MIK_HIP(ctx, hipMemsetAsync(y, 0, 2 * sizeof(R) * (size_t)m, ctx->stream));
        return MIK_OK;
    }
    const dm_plan p = cdm_plan_n<R>(D, x, y);
    const int64_t nc = p.cols;
    R *out = nc == 1 ? y : (R *)D->work;
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    if (p.vec && p.streamed) hipLaunchKernelGGL((k_cdense_n<R, MIK_CDM_R, true, true, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const R *)D->A, D->lda, x, out, D->m_pad);
    else if (p.vec) hipLaunchKernelGGL((k_cdense_n<R, MIK_CDM_R, true, false, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const R *)D->A, D->lda, x, out, D->m_pad);
    else hipLaunchKernelGGL((k_cdense_n<R, MIK_CDM_R, false, false, MIK_DM_C>), grid, dim3(MIK_BLOCK), 0, ctx->stream, m, n, (const R *)D->A, D->lda, x, out, D->m_pad);
    MIK_LAUNCH_CHECK(ctx);
    if (nc > 1) {                                             // complex addition is componentwise: the real combine over 2 m reals
        hipLaunchKernelGGL((k_dense_n_combine<R, MIK_DM_PF>), dim3((unsigned)((2 * m + MIK_DM_CB - 1) / MIK_DM_CB)), dim3(MIK_DM_CB), 0, ctx->stream, 2 * m, nc, (const R *)out, 2 * D->m_pad, y, (int64_t)0, (int64_t)0);
        MIK_LAUNCH_CHECK(ctx);
    }
    return MIK_OK;
}

template <typename R>
int cdm_mul_t(mik_dense *D, const R *x, R *y)
{
    mik_ctx *ctx = D->ctx;
    const int64_t m = D->m, n = D->n;
    if (n == 0) return MIK_OK;
    const dm_plan p = cdm_plan_t<R>(D, x, y);
    const int64_t nseg = p.nseg;
    if (nseg == 0) {                                          // empty columns: every dot is (+0, +0)
        MIK_HIP(ctx, hipMemsetAsync(y, 0, 2 * sizeof(R) * (size_t)n, ctx->stream));
        return MIK_OK;
    }
    R *part = (R *)D->work;
    const dim3 grid((unsigned)p.gx, (unsigned)p.gy);
    if (p.vec && p.streamed) hipLaunchKernelGGL((k_cdense_t<R, true, true>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * m, nseg, n, (const R *)D->A, D->lda, x, part);
    else if (p.vec) hipLaunchKernelGGL((k_cdense_t<R, true, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * m, nseg, n, (const R *)D->A, D->lda, x, part);
    else hipLaunchKernelGGL((k_cdense_t<R, false, false>), grid, dim3(MIK_BLOCK), 0, ctx->stream, 2 * m, nseg, n, (const R *)D->A, D->lda, x, part);
    MIK_LAUNCH_CHECK(ctx);
    // two sums per column: workgroup 2 j + c leaves component c of y[j] in real 2 j + c of y
    hipLaunchKernelGGL((k_finalize_store<R>), dim3((unsigned)(2 * n)), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const R *)part, nseg, nseg, y, (const int *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

}  // namespace

extern "C" int mik_dense_mul_shape_for(int dtype, int *chunk, int *rows_per_workgroup)
{
    if (dtype != MIK_F64 && dtype != MIK_F32 && !mik_is_complex(dtype)) return MIK_ERR_INVALID;
    if (chunk) *chunk = MIK_DM_C;
    if (rows_per_workgroup) *rows_per_workgroup = mik_is_complex(dtype) ? MIK_CDM_R : MIK_DM_R;
    return MIK_OK;
}

extern "C" int mik_dense_mul_shape(int *chunk, int *rows_per_workgroup)
{
    if (chunk) *chunk = MIK_DM_C;
    if (rows_per_workgroup) *rows_per_workgroup = MIK_DM_R;
    return MIK_OK;
}

extern "C" int mik_dense_create(mik_ctx *ctx, int dtype, int64_t m, int64_t n, const void *A, int64_t lda, mik_dense **out)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    const bool cplx = mik_is_complex(dtype);
    if (dtype != MIK_F64 && dtype != MIK_F32 && !cplx) return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_create: dtype must be MIK_F64, MIK_F32, MIK_C64 or MIK_C32");
    if (m < 0 || n < 0) return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_create: m = %lld, n = %lld", (long long)m, (long long)n);
    if (lda < m) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_dense_create: lda = %lld < m = %lld", (long long)lda, (long long)m);
    if (!A && m > 0 && n > 0) return MIK_ERR_INVALID;
    if (m > (int64_t)std::numeric_limits<int>::max() - MIK_DM_R || n > (int64_t)std::numeric_limits<int>::max() - MIK_DM_C)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_dense_create: a dimension >= 2^31");
    if (cplx && n >= ((int64_t)1 << 30)) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_dense_create: a %s matrix of 2^30 columns or more", cdm_name(dtype));   // 2 n finalisers
    mik_dense *D = new (std::nothrow) mik_dense();
    if (!D) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_dense_create: host allocation failed");
    D->ctx = ctx; D->dtype = dtype; D->m = m; D->n = n; D->lda = lda; D->A = A;
    const int64_t rw = cplx ? MIK_CDM_R : MIK_DM_R;
    D->m_pad = (m + rw - 1) / rw * rw;
    const size_t es = mik_dtype_size(dtype);
    const int64_t nc = dm_chunks(n);
    const int64_t nseg = dtype == MIK_F64 ? mik_nseg<double>(m) : dtype == MIK_F32 ? mik_nseg<float>(m)
                       : dtype == MIK_C64 ? mik_nseg<double>(2 * m) : mik_nseg<float>(2 * m);     // complex: n x nseg (re, im) pairs = es bytes each
    const size_t bytes = std::max<size_t>(16, es * std::max<size_t>(nc > 1 ? (size_t)nc * (size_t)D->m_pad : 0, (size_t)n * (size_t)nseg));
    (void)hipSetDevice(ctx->device);
    const hipError_t e = hipMalloc(&D->work, bytes);
    if (e != hipSuccess) {
        delete D;
        return mik_fail(ctx, e == hipErrorOutOfMemory ? MIK_ERR_NOMEM : MIK_ERR_HIP, "mik_dense_create: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    *out = D;
    return MIK_OK;
}

extern "C" int mik_dense_destroy(mik_dense *D)
{
    if (!D) return MIK_OK;
    if (D->ctx) { (void)hipSetDevice(D->ctx->device); (void)hipStreamSynchronize(D->ctx->stream); }
    if (D->work) (void)hipFree(D->work);
    if (D->bwork) (void)hipFree(D->bwork);
    delete D;
    return MIK_OK;
}

extern "C" int mik_dense_mul(mik_dense *D, int adjoint, const void *x, void *y)
{
    if (!D) return MIK_ERR_INVALID;
    const size_t es = mik_dtype_size(D->dtype);
    const int64_t nx = adjoint ? D->m : D->n, ny = adjoint ? D->n : D->m;
    if ((nx && !x) || (ny && !y)) return MIK_ERR_INVALID;
    if (mik_overlap(x, es * (size_t)nx, y, es * (size_t)ny)) return mik_fail(D->ctx, MIK_ERR_INVALID, "mik_dense_mul: x and y must not overlap");
    const size_t abytes = (D->m > 0 && D->n > 0) ? es * ((size_t)(D->n - 1) * (size_t)D->lda + (size_t)D->m) : 0;
    if (mik_overlap(y, es * (size_t)ny, D->A, abytes)) return mik_fail(D->ctx, MIK_ERR_INVALID, "mik_dense_mul: y must not overlap A");
    if (D->dtype == MIK_C64)
        return adjoint ? cdm_mul_t<double>(D, (const double *)x, (double *)y) : cdm_mul_n<double>(D, (const double *)x, (double *)y);
    if (D->dtype == MIK_C32)
        return adjoint ? cdm_mul_t<float>(D, (const float *)x, (float *)y) : cdm_mul_n<float>(D, (const float *)x, (float *)y);
    if (D->dtype == MIK_F64)
        return adjoint ? dm_mul_t<double>(D, (const double *)x, (double *)y) : dm_mul_n<double>(D, (const double *)x, (double *)y);
    return adjoint ? dm_mul_t<float>(D, (const float *)x, (float *)y) : dm_mul_n<float>(D, (const float *)x, (float *)y);
}

extern "C" int mik_dense_block_shape(int *group_width)
{
    if (group_width) *group_width = MIK_DM_GW;
    return MIK_OK;
}

extern "C" int mik_dense_block_reserve(mik_dense *D)
{
    if (!D) return MIK_ERR_INVALID;
    if (mik_is_complex(D->dtype)) return mik_fail(D->ctx, MIK_ERR_NOTIMPL, "mik_dense_block_reserve: the block product is not implemented for %s matrices", cdm_name(D->dtype));
    return dm_block_reserve(D);
}

extern "C" int mik_dense_mm(mik_dense *D, int b, const void *X, int64_t ldx, void *Y, int64_t ldy)
{
    if (!D || b < 0) return MIK_ERR_INVALID;
    if (mik_is_complex(D->dtype)) return mik_fail(D->ctx, MIK_ERR_NOTIMPL, "mik_dense_mm: the block product is not implemented for %s matrices", cdm_name(D->dtype));
    if (b > MIK_DM_BMAX) return mik_fail(D->ctx, MIK_ERR_NOTIMPL, "mik_dense_mm: b = %d (at most %d columns)", b, MIK_DM_BMAX);
    if (b == 0) return MIK_OK;
    if (ldx < D->n || ldy < D->m)
        return mik_fail(D->ctx, MIK_ERR_MISMATCH, "mik_dense_mm: ldx = %lld < n = %lld or ldy = %lld < m = %lld", (long long)ldx, (long long)D->n, (long long)ldy, (long long)D->m);
    if (D->m == 0) return MIK_OK;
    if ((D->n && !X) || !Y) return MIK_ERR_INVALID;
    const size_t es = mik_dtype_size(D->dtype);
    const size_t xbytes = mik_block_bytes(es, D->n, b, ldx), ybytes = mik_block_bytes(es, D->m, b, ldy);
    if (mik_overlap(X, xbytes, Y, ybytes)) return mik_fail(D->ctx, MIK_ERR_INVALID, "mik_dense_mm: Y overlaps X");
    const size_t abytes = D->n > 0 ? es * ((size_t)(D->n - 1) * (size_t)D->lda + (size_t)D->m) : 0;
    if (mik_overlap(Y, ybytes, D->A, abytes)) return mik_fail(D->ctx, MIK_ERR_INVALID, "mik_dense_mm: Y overlaps A");
    if (D->dtype == MIK_F64) return dm_mm<double>(D, b, (const double *)X, ldx, (double *)Y, ldy);
    return dm_mm<float>(D, b, (const float *)X, ldx, (float *)Y, ldy);
}

extern "C" int mik_dev_dense_block_plan(const mik_dense *D, int b, const void *X, int64_t ldx, const void *Y, int64_t ldy, int *vec, int *streamed,
                                        int64_t *grid_x, int64_t *grid_y, int64_t *chunks, int *groups, int *last_width, int *vector_cols,
                                        int64_t *workspace_bytes)
{
    if (!D) return MIK_ERR_INVALID;
    if (mik_is_complex(D->dtype)) return mik_fail(D->ctx, MIK_ERR_NOTIMPL, "mik_dev_dense_block_plan: the block product is not implemented for %s matrices", cdm_name(D->dtype));
    const dm_bplan p = D->dtype == MIK_F64 ? dm_plan_nb<double>(D, b, (const double *)X, ldx, (const double *)Y, ldy)
                                           : dm_plan_nb<float>(D, b, (const float *)X, ldx, (const float *)Y, ldy);
    if (vec) *vec = p.vec;
    if (streamed) *streamed = p.streamed;
    if (grid_x) *grid_x = p.gx;
    if (grid_y) *grid_y = p.gy;
    if (chunks) *chunks = p.chunks;
    if (groups) *groups = p.groups;
    if (last_width) *last_width = p.last_w;
    if (vector_cols) *vector_cols = p.vector_cols;
    if (workspace_bytes) *workspace_bytes = (int64_t)D->bwork_bytes;
    return MIK_OK;
}

extern "C" int mik_dev_dense_block_min_width(mik_dense *D, int width)
{
    if (!D || width < 0 || width > MIK_DM_GW) return MIK_ERR_INVALID;
    D->bmin = width;
    return MIK_OK;
}

extern "C" int mik_dev_dense_plan(const mik_dense *D, int adjoint, const void *x, const void *y, int *vec, int *streamed, int64_t *grid_x,
                                  int64_t *grid_y, int64_t *chunks_or_batches, int64_t *segments)
{
    if (!D) return MIK_ERR_INVALID;
    dm_plan p;
    if (D->dtype == MIK_C64) p = adjoint ? cdm_plan_t<double>(D, (const double *)x, (const double *)y) : cdm_plan_n<double>(D, (const double *)x, (const double *)y);
    else if (D->dtype == MIK_C32) p = adjoint ? cdm_plan_t<float>(D, (const float *)x, (const float *)y) : cdm_plan_n<float>(D, (const float *)x, (const float *)y);
    else if (D->dtype == MIK_F64) p = adjoint ? dm_plan_t<double>(D, (const double *)x, (const double *)y) : dm_plan_n<double>(D, (const double *)x, (const double *)y);
    else p = adjoint ? dm_plan_t<float>(D, (const float *)x, (const float *)y) : dm_plan_n<float>(D, (const float *)x, (const float *)y);
    if (vec) *vec = p.vec;
    if (streamed) *streamed = p.streamed;
    if (grid_x) *grid_x = p.gx;
    if (grid_y) *grid_y = p.gy;
    if (chunks_or_batches) *chunks_or_batches = p.cols;
    if (segments) *segments = p.nseg;
    return MIK_OK;
}

extern "C" int mik_dense_mul_fn(void *user, const void *x, void *y) { return mik_dense_mul((mik_dense *)user, 0, x, y); }

extern "C" int mik_dense_mul_adj_fn(void *user, const void *x, void *y) { return mik_dense_mul((mik_dense *)user, 1, x, y); }
