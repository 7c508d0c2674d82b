// mik_dense_qr.hip -- qr!(A) (Householder, no pivoting), lmul!(Q, Y), lmul!(Q', Y), F \ b and Matrix(F.Q) on a column-major m x n device
// matrix, m >= n: A \ b for a tall matrix is what the reference's tests hold lsqr and lsmr to (test/lsqr.jl:15-19, test/lsmr.jl:68-72), and
// Matrix(qr(A).Q) is its orthonormal basis (test/orthogonalize.jl:17-18).
//
// The bit contract and the kernels are in csrc/mik_dense_qr.h.  The plan is right-looking over panels of W columns: one launch per column
// (apply the previous reflector to the panel's remaining columns, form the next one), then one launch of the trailing update, in which a
// workgroup owns a column and applies the panel's W reflectors to it in order.  Every dependency between workgroups is a kernel boundary on
// the context's stream.  R[k,k] == 0 is recorded, not refused (qr! does not throw): create reads the flag once at the end -- the
// factorisation's only host synchronisation -- and a solve on such a handle is SingularException(k).  A solve is a copy of b, one launch of
// Q' on it and the LU's backward substitution on R; a block of right-hand sides runs the same launches per pass of MIK_DS_G columns through a
// workspace of m x MIK_DS_G elements that the handle allocates at the first one.
#include "mik_internal.h"
#include "mik_dense_factor.h"
#include "mik_dense_lu.h"
#include "mik_dense_qr.h"

#include <type_traits>
#include <algorithm>
#include <vector>

struct mik_dense_qr : mik_dense_factor {      // n: the columns; work: m elements; aux: the flag; block: m x MIK_DS_G elements
    int m = 0;
    void *tau = nullptr;             // device, n elements
    std::vector<unsigned char> tau_host;
    int64_t resident_rows = 0;       // the row limit of the LDS-resident form, in use
    bool resident = false;           // m <= resident_rows: a launch that starts at reflector 0 (lmul, solve, thin Q) keeps its column in LDS; a trailing
                                     // update from reflector k0 on keeps the rows [k0, m), so it does as soon as m - k0 <= resident_rows
    int64_t zero_diag = 0;           // 0, or the 1-based index of the first R[k,k] == 0
};

namespace {

void qr_free(mik_dense_qr *F)
{
    if (!F) return;
    void *tau = F->tau;
    const int device = F->ctx ? F->ctx->device : -1;
    dense_free(F);                                             // synchronises the stream first
    if (tau) { if (device >= 0) (void)hipSetDevice(device); (void)hipFree(tau); }
}

template <typename T> qr_cols<T> qr_plain(T *Y, int64_t ldy, int m) { return qr_cols<T>{Y, 1, ldy, ldy, 0, 1, m}; }

// the reflectors [r0, r1) on `ncols` columns: resident while the rows [r0, m) a workgroup has to keep are within the handle's limit
template <bool DESC, typename T>
void qr_apply(const mik_dense_qr *F, int r0, int r1, qr_cols<T> Y, int64_t ncols)
{
    hipStream_t st = F->ctx->stream;
    const T *V = (const T *)F->A, *tau = (const T *)F->tau;
    if (F->m - r0 <= F->resident_rows)
        hipLaunchKernelGGL((k_qr_apply<T, true, DESC>), dim3((unsigned)ncols), dim3(MIK_QR_ACC), (size_t)(F->m - r0) * sizeof(T), st, F->m, r0, r1, V, F->ld, tau, Y);
    else
        hipLaunchKernelGGL((k_qr_apply<T, false, DESC>), dim3((unsigned)ncols), dim3(MIK_QR_ACC), 0, st, F->m, r0, r1, V, F->ld, tau, Y);
}

template <typename T>
int qr_factor(mik_dense_qr *F)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int m = F->m, n = F->n;
    const int64_t ld = F->ld;
    T *A = (T *)F->A;
    MIK_TRY(dense_flag_arm(ctx, F->aux));
    int64_t launches = 0;
    for (int k0 = 0; k0 < n; k0 += MIK_QR_W) {
        const int k1 = std::min(k0 + MIK_QR_W, n);
        for (int j = k0; j < k1; ++j)
            hipLaunchKernelGGL((k_qr_panel<T>), dim3((unsigned)(k1 - j)), dim3(MIK_QR_ACC), 0, st, m, j, k0, A, ld, (T *)F->tau, F->aux);
        launches += k1 - k0;
        if (k1 < n) {
            qr_apply<false>(F, k0, k1, qr_plain(A + (int64_t)k1 * ld, ld, m), n - k1);
            ++launches;
        }
        MIK_LAUNCH_CHECK(ctx);
    }
    F->launches_factor = launches;
    F->tau_host.resize((size_t)n * sizeof(T));
    MIK_HIP(ctx, hipMemcpyAsync(F->tau_host.data(), F->tau, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
    int first = 0;
    MIK_TRY(dense_flag_read(ctx, F->aux, &first));
    F->zero_diag = first < n ? (int64_t)first + 1 : 0;
    return MIK_OK;
}

template <typename T>
void qr_bwd(const mik_dense_qr *F, T *t, T *x)
{
    const int n = F->n;
    for (int k0 = (n - 1) / MIK_LU_W * MIK_LU_W; k0 >= 0; k0 -= MIK_LU_W)
        hipLaunchKernelGGL((k_lu_bwd<T>), dim3((unsigned)(k0 / MIK_DS_R + 1)), dim3(MIK_DS_R), 0, F->ctx->stream, n, k0, std::min(k0 + MIK_LU_W, n), (const T *)F->A, F->ld, t, x);
}

template <typename T>
int qr_solve_dev(mik_dense_qr *F, T *x, const T *b)
{
    mik_ctx *ctx = F->ctx;
    T *t = (T *)F->work;
    MIK_HIP(ctx, hipMemcpyAsync(t, b, (size_t)F->m * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    qr_apply<false>(F, 0, F->n, qr_plain(t, (int64_t)F->m, F->m), 1);
    qr_bwd(F, t, x);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// one pass of a block solve: the `cols` columns from b to x through the block workspace t, NB columns per lane of the substitution
template <int NB, typename T>
int qr_solve_block_dev(mik_dense_qr *F, T *t, T *x, int64_t ldx, const T *b, int64_t ldb, int cols)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int m = F->m, n = F->n;
    const unsigned groups = dense_grid(cols, NB);
    hipLaunchKernelGGL((k_qr_stage_nb<T, NB>), dim3(dense_grid(m, 256), groups), dim3(256), 0, st, m, n, b, ldb, cols, t);
    qr_apply<false>(F, 0, n, qr_cols<T>{t, NB, (int64_t)NB * n, (int64_t)NB * (m - n), (int64_t)n * MIK_DS_G, NB, n}, cols);
    for (int k0 = (n - 1) / MIK_LU_W * MIK_LU_W; k0 >= 0; k0 -= MIK_LU_W)
        hipLaunchKernelGGL((k_lu_bwd_nb<T, NB>), dim3((unsigned)(k0 / MIK_DS_R + 1), groups), dim3(MIK_DS_R), 0, st, n, k0, std::min(k0 + MIK_LU_W, n), (const T *)F->A, F->ld, t, x, ldx, cols);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

int64_t qr_launches_solve(const mik_dense_qr *F) { return 1 + ((int64_t)F->n + MIK_LU_W - 1) / MIK_LU_W; }

size_t qr_factor_bytes(const mik_dense_qr *F) { return (size_t)F->ld * (size_t)F->n * mik_dtype_size(F->dtype); }

int qr_refuse_singular(const mik_dense_qr *F, const char *entry)
{
    if (F->zero_diag) return mik_fail(F->ctx, MIK_ERR_SINGULAR, "%s: SingularException(%lld): R has a zero on its diagonal", entry, (long long)F->zero_diag);
    return MIK_OK;
}

// a block of `rows` rows and `cols` columns with the leading dimension ld: from its first element to the last row of its last column
size_t qr_extent(const mik_dense_qr *F, int64_t rows, int64_t ld, int64_t cols) { return ((size_t)(cols - 1) * (size_t)ld + (size_t)rows) * mik_dtype_size(F->dtype); }

}  // namespace

extern "C" int mik_dense_qr_create(mik_ctx *ctx, void *A, int64_t m, int64_t n, int64_t ld, int dtype, const mik_dense_qr_plan *plan, int64_t *zero_diag, mik_dense_qr **out)
{
    const char *entry = "mik_dense_qr_create";
    if (zero_diag) *zero_diag = 0;
    if (!ctx || !A || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (dtype == MIK_C64 || dtype == MIK_C32)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "%s: qr is not built for %s (it needs complex reflectors: a complex tau and conjugated products)", entry,
                        dtype == MIK_C64 ? "ComplexF64 (MIK_C64)" : "ComplexF32 (MIK_C32)");
    if (dtype != MIK_F64 && dtype != MIK_F32) return mik_fail(ctx, MIK_ERR_INVALID, "%s: dtype must be MIK_F64 or MIK_F32", entry);
    if (n < 1 || m < n) return mik_fail(ctx, MIK_ERR_MISMATCH, "%s: DimensionMismatch: m = %lld, n = %lld (need 1 <= n <= m; a wide matrix is not offered)", entry, (long long)m, (long long)n);
    if (ld < m) return mik_fail(ctx, MIK_ERR_MISMATCH, "%s: m = %lld, ld = %lld (need ld >= m)", entry, (long long)m, (long long)ld);
    if (m > (int64_t)std::numeric_limits<int>::max() - MIK_DS_W) return mik_fail(ctx, MIK_ERR_NOTIMPL, "%s: m >= 2^31 - 64", entry);
    if (plan && plan->resident_rows < 0) return mik_fail(ctx, MIK_ERR_INVALID, "%s: plan->resident_rows = %lld (need >= 0; 0 = default)", entry, (long long)plan->resident_rows);
    mik_dense_qr *F = new (std::nothrow) mik_dense_qr();
    if (!F) return mik_fail(ctx, MIK_ERR_NOMEM, "%s: host allocation failed", entry);
    F->ctx = ctx; F->dtype = dtype; F->m = (int)m; F->n = (int)n; F->ld = ld; F->A = A;
    const size_t es = mik_dtype_size(dtype);
    const int64_t fits = (int64_t)(MIK_QR_LDS_BYTES / es);
    F->resident_rows = plan && plan->resident_rows ? std::min(plan->resident_rows, fits) : fits;
    F->resident = m <= F->resident_rows;
    (void)hipSetDevice(ctx->device);
    const size_t vec = std::max<size_t>((size_t)m * es, 16), taub = std::max<size_t>((size_t)n * es, 16);
    int rc = MIK_OK;
    auto alloc = [&]() {
        MIK_HIP(ctx, hipMalloc(&F->work, vec));
        MIK_HIP(ctx, hipMalloc((void **)&F->aux, 16));
        MIK_HIP(ctx, hipMalloc(&F->tau, taub));
        return (int)MIK_OK;
    };
    rc = alloc();
    F->bytes = (int64_t)(vec + 16 + taub);
    if (rc == MIK_OK) rc = dense_dispatch<false>(dtype, [&](auto e) { return qr_factor<decltype(e)>(F); });
    if (rc != MIK_OK) { qr_free(F); return rc; }
    if (zero_diag) *zero_diag = F->zero_diag;
    *out = F;
    return MIK_OK;
}

extern "C" int mik_dense_qr_destroy(mik_dense_qr *F)
{
    qr_free(F);
    return MIK_OK;
}

extern "C" int mik_dense_qr_tau(const mik_dense_qr *F, void *tau)
{
    if (!F || !tau) return MIK_ERR_INVALID;
    std::copy(F->tau_host.begin(), F->tau_host.end(), (unsigned char *)tau);
    return MIK_OK;
}

extern "C" int mik_dense_qr_lmul(mik_dense_qr *F, int adjoint, void *Y, int64_t ldy, int64_t ncols)
{
    const char *entry = "mik_dense_qr_lmul";
    if (!F || !Y) return MIK_ERR_INVALID;
    if (ncols < 1 || ncols > std::numeric_limits<int>::max()) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ncols = %lld (need 1 <= ncols < 2^31)", entry, (long long)ncols);
    if (ldy < F->m) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ldy = %lld (need ldy >= m = %d)", entry, (long long)ldy, F->m);
    if (mik_overlap(Y, qr_extent(F, F->m, ldy, ncols), F->A, qr_factor_bytes(F))) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: Y overlaps the factors", entry);
    (void)hipSetDevice(F->ctx->device);
    return dense_dispatch<false>(F->dtype, [&](auto e) {
        using T = decltype(e);
        if (adjoint) qr_apply<false>(F, 0, F->n, qr_plain((T *)Y, ldy, F->m), ncols);
        else qr_apply<true>(F, 0, F->n, qr_plain((T *)Y, ldy, F->m), ncols);
        MIK_LAUNCH_CHECK(F->ctx);
        return (int)MIK_OK;
    });
}

extern "C" int mik_dense_qr_solve(mik_dense_qr *F, void *x, const void *b)
{
    const char *entry = "mik_dense_qr_solve";
    if (!F || !x || !b) return MIK_ERR_INVALID;
    MIK_TRY(qr_refuse_singular(F, entry));
    const size_t es = mik_dtype_size(F->dtype), xbytes = (size_t)F->n * es, bbytes = (size_t)F->m * es;
    if (x != b && mik_overlap(x, xbytes, b, bbytes)) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: x and b overlap without starting at the same element", entry);
    if (mik_overlap(x, xbytes, F->A, qr_factor_bytes(F)) || mik_overlap(b, bbytes, F->A, qr_factor_bytes(F))) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: a vector overlaps the factors", entry);
    (void)hipSetDevice(F->ctx->device);
    return dense_dispatch<false>(F->dtype, [&](auto e) { return qr_solve_dev(F, (decltype(e) *)x, (const decltype(e) *)b); });
}

extern "C" int mik_dense_qr_solve_block(mik_dense_qr *F, void *X, int64_t ldx, const void *B, int64_t ldb, int64_t nrhs)
{
    const char *entry = "mik_dense_qr_solve_block";
    if (!F || !X || !B) return MIK_ERR_INVALID;
    MIK_TRY(qr_refuse_singular(F, entry));
    if (nrhs < 1) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: nrhs = %lld (need nrhs >= 1)", entry, (long long)nrhs);
    if (ldx < F->n || ldb < F->m) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ldx = %lld, ldb = %lld (need ldx >= n = %d and ldb >= m = %d)", entry, (long long)ldx, (long long)ldb, F->n, F->m);
    const size_t xbytes = qr_extent(F, F->n, ldx, nrhs), bbytes = qr_extent(F, F->m, ldb, nrhs);
    if (X == B ? ldx != ldb : mik_overlap(X, xbytes, B, bbytes))
        return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: X and B overlap without being the same block (equal pointers and leading dimensions)", entry);
    if (mik_overlap(X, xbytes, F->A, qr_factor_bytes(F)) || mik_overlap(B, bbytes, F->A, qr_factor_bytes(F))) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: a block overlaps the factors", entry);
    (void)hipSetDevice(F->ctx->device);
    if (!F->block) MIK_HIP(F->ctx, hipMalloc(&F->block, (size_t)F->m * MIK_DS_G * mik_dtype_size(F->dtype)));
    return dense_dispatch<false>(F->dtype, [&](auto e) {
        using T = decltype(e);
        for (int64_t c = 0; c < nrhs; c += MIK_DS_G)
            MIK_TRY(qr_solve_block_dev<de_block<T>::NB>(F, (T *)F->block, (T *)X + c * ldx, ldx, (const T *)B + c * ldb, ldb, (int)std::min<int64_t>(MIK_DS_G, nrhs - c)));
        return (int)MIK_OK;
    });
}

extern "C" int mik_dense_qr_thin_q(mik_dense_qr *F, void *Q, int64_t ldq)
{
    const char *entry = "mik_dense_qr_thin_q";
    if (!F || !Q) return MIK_ERR_INVALID;
    if (ldq < F->m) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ldq = %lld (need ldq >= m = %d)", entry, (long long)ldq, F->m);
    if (mik_overlap(Q, qr_extent(F, F->m, ldq, F->n), F->A, qr_factor_bytes(F))) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: Q overlaps the factors", entry);
    const int64_t rb = dense_grid(F->m, 256);
    if (rb * F->n > std::numeric_limits<int>::max()) return mik_fail(F->ctx, MIK_ERR_NOTIMPL, "%s: m n / 256 >= 2^31", entry);
    (void)hipSetDevice(F->ctx->device);
    return dense_dispatch<false>(F->dtype, [&](auto e) {
        using T = decltype(e);
        hipLaunchKernelGGL((k_qr_eye<T>), dim3((unsigned)(rb * F->n)), dim3(256), 0, F->ctx->stream, F->m, (int)rb, (T *)Q, ldq);
        qr_apply<true>(F, 0, F->n, qr_plain((T *)Q, ldq, F->m), F->n);
        MIK_LAUNCH_CHECK(F->ctx);
        return (int)MIK_OK;
    });
}

extern "C" int mik_dense_qr_r(mik_dense_qr *F, void *R, int64_t ldr)
{
    const char *entry = "mik_dense_qr_r";
    if (!F || !R) return MIK_ERR_INVALID;
    if (ldr < F->n) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "%s: ldr = %lld (need ldr >= n = %d)", entry, (long long)ldr, F->n);
    if (mik_overlap(R, qr_extent(F, F->n, ldr, F->n), F->A, qr_factor_bytes(F))) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: R overlaps the factors", entry);
    const int64_t rb = dense_grid(F->n, 256);
    if (rb * F->n > std::numeric_limits<int>::max()) return mik_fail(F->ctx, MIK_ERR_NOTIMPL, "%s: n n / 256 >= 2^31", entry);
    (void)hipSetDevice(F->ctx->device);
    return dense_dispatch<false>(F->dtype, [&](auto e) {
        using T = decltype(e);
        hipLaunchKernelGGL((k_qr_upper<T>), dim3((unsigned)(rb * F->n)), dim3(256), 0, F->ctx->stream, F->n, (int)rb, (const T *)F->A, F->ld, (T *)R, ldr);
        MIK_LAUNCH_CHECK(F->ctx);
        return (int)MIK_OK;
    });
}

extern "C" int mik_dense_qr_ldiv_fn(void *user, void *y, const void *x)
{
    mik_dense_qr *F = (mik_dense_qr *)user;
    if (!F) return MIK_ERR_INVALID;
    if (F->m != F->n) return mik_fail(F->ctx, MIK_ERR_MISMATCH, "mik_dense_qr_ldiv_fn: the factorisation of a %d x %d matrix is no preconditioner (square handles only)", F->m, F->n);
    return mik_dense_qr_solve(F, y, x);
}

extern "C" int mik_dense_qr_info(const mik_dense_qr *F, int64_t *panel_w, int64_t *accumulators, int64_t *resident_rows, int64_t *resident, int64_t *launches_factor,
                                 int64_t *launches_solve, int64_t *bytes, int64_t *zero_diag)
{
    if (!F) return MIK_ERR_INVALID;
    if (panel_w) *panel_w = MIK_QR_W;
    if (accumulators) *accumulators = MIK_QR_ACC;
    if (resident_rows) *resident_rows = F->resident_rows;
    if (resident) *resident = F->resident ? 1 : 0;
    if (launches_factor) *launches_factor = F->launches_factor;
    if (launches_solve) *launches_solve = qr_launches_solve(F);
    if (bytes) *bytes = F->bytes;
    if (zero_diag) *zero_diag = F->zero_diag;
    return MIK_OK;
}
