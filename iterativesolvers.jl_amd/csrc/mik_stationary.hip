// mik_stationary.hip -- Jacobi, Gauss-Seidel, SOR and SSOR building blocks on a device CSR operator (src/stationary_sparse.jl).
//
// mik_stationary_create reads the operator's CSR arrays back once (rows longer than MIK_LONG_ROW from behind the short part, through the
// long-row table of mik_csr_create) and builds, on the host:
//   - the diagonal positions (DiagonalIndices, :6-28) and the first singular column;
//   - a row-major copy of the matrix (+ diagonal positions and values) for the row-parallel sweeps;
//   - for each triangular direction a level schedule of the strict-triangle DAG (level of row i = 1 + the largest level of the rows
//     it reads; rows sorted by level, stable by row index) and a level-ordered copy of the strict triangle, every row's entries in the
//     order the reference's column loop delivers them;
//   - a launch plan: a level with more than MIK_ST_NARROW rows is one launch; a run of consecutive narrow levels is one launch of one
//     workgroup that steps through them with a barrier in between.  No workgroup ever waits for another one.
// The operator's own layouts and upload are untouched.
//
// A ComplexF64 / ComplexF32 operator (MIK_C64 / MIK_C32) goes through the same analysis -- it is written over an element size in bytes, and a
// complex mik_csr keeps every row, long ones included, contiguous in rowptr / col / val (csrc/mik_complex.hip: n_long stays 0), so the
// read-back takes the plain path -- and through the kernels of csrc/mik_stationary_complex.h.
#include "mik_internal.h"
#include "mik_stationary.h"
#include "mik_stationary_complex.h"

#include <chrono>
#include <new>
#include <vector>

namespace {

struct StLaunch { int narrow; int a, b; };     // narrow: levels [a, b); wide: level-order positions [a, b)

struct StTri {                                 // one direction of the triangular sweeps
    int *perm = nullptr, *tp = nullptr, *tc = nullptr, *lev = nullptr;
    void *tv = nullptr;
    int64_t levels = 0;
    std::vector<StLaunch> plan;
};

}  // namespace

struct mik_stationary {
    mik_ctx *ctx = nullptr;
    int dtype = MIK_F64;
    int n = 0;
    int *rp = nullptr, *cl = nullptr, *dg = nullptr;
    void *vl = nullptr, *d = nullptr, *tmp = nullptr;
    StTri lo, up;
    int64_t bytes = 0;
    double analysis_ms = 0.0;
};

namespace {

void st_free(mik_stationary *S)
{
    if (!S) return;
    if (S->ctx) { (void)hipSetDevice(S->ctx->device); (void)hipStreamSynchronize(S->ctx->stream); }
    for (void *p : {(void *)S->rp, (void *)S->cl, (void *)S->dg, S->vl, S->d, S->tmp, (void *)S->lo.perm, (void *)S->lo.tp, (void *)S->lo.tc,
                    (void *)S->lo.lev, S->lo.tv, (void *)S->up.perm, (void *)S->up.tp, (void *)S->up.tc, (void *)S->up.lev, S->up.tv})
        if (p) (void)hipFree(p);
    delete S;
}

template <typename V>
int st_upload(mik_stationary *S, void **dst, const V *src, size_t count, size_t es)
{
    const size_t bytes = std::max<size_t>(count * es, 16);
    MIK_HIP(S->ctx, hipMalloc(dst, bytes));
    if (count) MIK_HIP(S->ctx, hipMemcpyAsync(*dst, src, count * es, hipMemcpyHostToDevice, S->ctx->stream));
    S->bytes += (int64_t)bytes;
    return MIK_OK;
}

// level schedule + level-ordered strict triangle of one direction (lower: entries j < i ascending; upper: j > i descending)
int st_build_tri(mik_stationary *S, StTri &T, bool upper, const std::vector<int> &rp, const std::vector<int> &cl, const std::vector<unsigned char> &vl,
                 const std::vector<int> &dg, size_t es)
{
    const int n = S->n;
    std::vector<int> level((size_t)n, 0);
    int nlev = 0;
    for (int s = 0; s < n; ++s) {
        const int i = upper ? n - 1 - s : s;
        int lv = 0;
        if (upper) { for (int k = dg[(size_t)i] + 1; k < rp[(size_t)i + 1]; ++k) lv = std::max(lv, level[(size_t)cl[(size_t)k]] + 1); }
        else       { for (int k = rp[(size_t)i]; k < dg[(size_t)i]; ++k) lv = std::max(lv, level[(size_t)cl[(size_t)k]] + 1); }
        level[(size_t)i] = lv;
        nlev = std::max(nlev, lv + 1);
    }
    if (n == 0) nlev = 0;
    std::vector<int> lev((size_t)nlev + 1, 0), perm((size_t)n), tp((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) ++lev[(size_t)level[(size_t)i] + 1];
    for (int l = 0; l < nlev; ++l) lev[(size_t)l + 1] += lev[(size_t)l];
    {
        std::vector<int> cur(lev.begin(), lev.end() - (nlev ? 1 : 0));
        for (int i = 0; i < n; ++i) perm[(size_t)cur[(size_t)level[(size_t)i]]++] = i;      // stable by row index
    }
    for (int p = 0; p < n; ++p) {
        const int i = perm[(size_t)p];
        tp[(size_t)p + 1] = tp[(size_t)p] + (upper ? rp[(size_t)i + 1] - dg[(size_t)i] - 1 : dg[(size_t)i] - rp[(size_t)i]);
    }
    std::vector<int> tc((size_t)tp[(size_t)n]);
    std::vector<unsigned char> tv(tc.size() * es);
    for (int p = 0; p < n; ++p) {
        const int i = perm[(size_t)p];
        int q = tp[(size_t)p];
        if (upper) {
            for (int k = rp[(size_t)i + 1] - 1; k > dg[(size_t)i]; --k, ++q) { tc[(size_t)q] = cl[(size_t)k]; memcpy(&tv[(size_t)q * es], &vl[(size_t)k * es], es); }
        } else {
            for (int k = rp[(size_t)i]; k < dg[(size_t)i]; ++k, ++q) { tc[(size_t)q] = cl[(size_t)k]; memcpy(&tv[(size_t)q * es], &vl[(size_t)k * es], es); }
        }
    }
    T.levels = nlev;
    for (int l = 0; l < nlev;) {
        if (lev[(size_t)l + 1] - lev[(size_t)l] > MIK_ST_NARROW) { T.plan.push_back({0, lev[(size_t)l], lev[(size_t)l + 1]}); ++l; continue; }
        int l1 = l + 1;
        while (l1 < nlev && lev[(size_t)l1 + 1] - lev[(size_t)l1] <= MIK_ST_NARROW) ++l1;
        T.plan.push_back({1, l, l1});
        l = l1;
    }
    MIK_TRY(st_upload(S, (void **)&T.perm, perm.data(), perm.size(), sizeof(int)));
    MIK_TRY(st_upload(S, (void **)&T.tp, tp.data(), tp.size(), sizeof(int)));
    MIK_TRY(st_upload(S, (void **)&T.lev, lev.data(), lev.size(), sizeof(int)));
    MIK_TRY(st_upload(S, (void **)&T.tc, tc.data(), tc.size(), sizeof(int)));
    MIK_TRY(st_upload(S, &T.tv, tv.data(), tc.size(), es));
    return MIK_OK;
}

bool st_is_zero(const unsigned char *v, int dtype)
{
    if (dtype == MIK_C64) { double a[2]; memcpy(a, v, 16); return a[0] == 0.0 && a[1] == 0.0; }     // iszero(z): both parts, either sign
    if (dtype == MIK_C32) { float a[2]; memcpy(a, v, 8); return a[0] == 0.0f && a[1] == 0.0f; }
    if (dtype == MIK_F64) { double a; memcpy(&a, v, 8); return a == 0.0; }      // -0.0 == 0.0: iszero(-0.0) is true
    float a; memcpy(&a, v, 4); return a == 0.0f;
}

int st_create(mik_ctx *ctx, const mik_csr *A, int64_t *singular_col, mik_stationary *S)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int n = (int)A->n_rows;
    const size_t es = mik_dtype_size(A->dtype);
    S->ctx = ctx; S->dtype = A->dtype; S->n = n;
    (void)hipSetDevice(ctx->device);

    // ---- the operator's rows, read back: [start, start + len) of the stored arrays -------------------------------------------
    std::vector<int> rowptr((size_t)n + 1);
    MIK_HIP(ctx, hipMemcpyAsync(rowptr.data(), A->rowptr, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<int> tab;
    if (A->n_long) {
        const size_t nl = (size_t)A->n_long;
        tab.resize(3 * nl + (size_t)A->n_seg + (size_t)A->n_cut);
        MIK_HIP(ctx, hipMemcpyAsync(tab.data(), A->long_rows, sizeof(int) * tab.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int> start((size_t)n), len((size_t)n);
    for (int i = 0; i < n; ++i) { start[(size_t)i] = rowptr[(size_t)i]; len[(size_t)i] = rowptr[(size_t)i + 1] - rowptr[(size_t)i]; }
    if (A->n_long) {
        // virtual rows of the long part: a whole row (target >= 0) or one segment of a cut row (target = -(segment + 1)); the segments of
        // a cut row are stored back to back, so the row is [smallest segment start, + total length)
        const size_t nl = (size_t)A->n_long;
        const int *tgt = tab.data(), *vs = tgt + nl, *vlen = vs + nl, *seg_row = vlen + nl, *cut_row = seg_row + A->n_seg;
        std::vector<unsigned char> seen((size_t)n, 0);
        for (size_t q = 0; q < nl; ++q) {
            const int r = tgt[q] >= 0 ? tgt[q] : cut_row[seg_row[-tgt[q] - 1]];
            if (!seen[(size_t)r]) { seen[(size_t)r] = 1; start[(size_t)r] = vs[q]; len[(size_t)r] = 0; }
            start[(size_t)r] = std::min(start[(size_t)r], vs[q]);
            len[(size_t)r] += vlen[q];
        }
    }
    int64_t stored = 0;
    for (int i = 0; i < n; ++i) stored = std::max<int64_t>(stored, (int64_t)start[(size_t)i] + len[(size_t)i]);
    std::vector<int> scol((size_t)stored);
    std::vector<unsigned char> sval((size_t)stored * es);
    if (stored) {
        MIK_HIP(ctx, hipMemcpyAsync(scol.data(), A->col, sizeof(int) * (size_t)stored, hipMemcpyDeviceToHost, ctx->stream));
        MIK_HIP(ctx, hipMemcpyAsync(sval.data(), A->val, es * (size_t)stored, hipMemcpyDeviceToHost, ctx->stream));
        MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }

    // ---- compact row-major copy (columns ascending within a row), diagonal positions: DiagonalIndices (:6-28) --------------------
    std::vector<int> rp((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) rp[(size_t)i + 1] = rp[(size_t)i] + len[(size_t)i];
    std::vector<int> cl((size_t)rp[(size_t)n]), dg((size_t)n, -1);
    std::vector<unsigned char> vl(cl.size() * es), dv((size_t)n * es);
    for (int i = 0; i < n; ++i) {
        if (len[(size_t)i]) {
            memcpy(&cl[(size_t)rp[(size_t)i]], &scol[(size_t)start[(size_t)i]], sizeof(int) * (size_t)len[(size_t)i]);
            memcpy(&vl[(size_t)rp[(size_t)i] * es], &sval[(size_t)start[(size_t)i] * es], es * (size_t)len[(size_t)i]);
        }
        for (int k = rp[(size_t)i]; k < rp[(size_t)i + 1]; ++k)
            if (cl[(size_t)k] >= i) { if (cl[(size_t)k] == i) dg[(size_t)i] = k; break; }       // searchsortedfirst: the first entry >= i
    }
    for (int i = 0; i < n; ++i) {                                                                   // columns 1..n in order: the first one throws
        if (dg[(size_t)i] < 0 || st_is_zero(&vl[(size_t)dg[(size_t)i] * es], A->dtype)) {
            if (singular_col) *singular_col = (int64_t)i + 1;
            return mik_fail(ctx, MIK_ERR_SINGULAR, "mik_stationary_create: SingularException(%d): zero or missing diagonal entry", i + 1);
        }
        memcpy(&dv[(size_t)i * es], &vl[(size_t)dg[(size_t)i] * es], es);
    }
    MIK_TRY(st_upload(S, (void **)&S->rp, rp.data(), rp.size(), sizeof(int)));
    MIK_TRY(st_upload(S, (void **)&S->cl, cl.data(), cl.size(), sizeof(int)));
    MIK_TRY(st_upload(S, &S->vl, vl.data(), cl.size(), es));
    MIK_TRY(st_upload(S, (void **)&S->dg, dg.data(), dg.size(), sizeof(int)));
    MIK_TRY(st_upload(S, &S->d, dv.data(), (size_t)n, es));
    MIK_HIP(ctx, hipMalloc(&S->tmp, std::max<size_t>((size_t)n * es, 16)));      // the old x of mik_gs_multiply when z aliases x
    S->bytes += (int64_t)std::max<size_t>((size_t)n * es, 16);

    // ---- level schedules: forward (strict lower) and backward (strict upper) ----------------------------------------------------
    MIK_TRY(st_build_tri(S, S->lo, false, rp, cl, vl, dg, es));
    MIK_TRY(st_build_tri(S, S->up, true, rp, cl, vl, dg, es));
    MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));     // the host vectors above die with this frame
    S->analysis_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MIK_OK;
}

inline unsigned st_grid(int64_t rows) { return (unsigned)((rows + MIK_ST_BLOCK - 1) / MIK_ST_BLOCK); }

template <typename T, typename S, bool RELAX>
int st_tri(mik_stationary *St, const StTri &T_, S alpha, T *x, S beta, const T *y)
{
    mik_ctx *ctx = St->ctx;
    for (const StLaunch &L : T_.plan) {
        if (L.narrow)
            hipLaunchKernelGGL((k_st_tri_run<T, S, RELAX>), dim3(1), dim3(MIK_ST_BLOCK), 0, ctx->stream, L.a, L.b, T_.lev, T_.perm, T_.tp, T_.tc,
                               (const T *)T_.tv, (const T *)St->d, alpha, x, beta, y);
        else
            hipLaunchKernelGGL((k_st_tri_level<T, S, RELAX>), dim3(st_grid(L.b - L.a)), dim3(MIK_ST_BLOCK), 0, ctx->stream, L.a, L.b, T_.perm, T_.tp,
                               T_.tc, (const T *)T_.tv, (const T *)St->d, alpha, x, beta, y);
    }
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
T st_scalar(const void *p) { T v; memcpy(&v, p, sizeof(T)); return v; }

int cst_sub(mik_stationary *St, const StTri &T_, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype);      // complex, below

int st_sub(mik_stationary *St, bool upper, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype, const char *who)
{
    if (!St || !x) return MIK_ERR_INVALID;
    if (y && (!alpha || !beta || (scalar_dtype != MIK_F64 && scalar_dtype != MIK_F32)))
        return mik_fail(St->ctx, MIK_ERR_INVALID, "%s: the relaxed form needs alpha, beta and scalar_dtype MIK_F64 / MIK_F32", who);
    if (y == x) return mik_fail(St->ctx, MIK_ERR_INVALID, "%s: x and y must not alias", who);
    if (St->n == 0) return MIK_OK;
    const StTri &T_ = upper ? St->up : St->lo;
    if (mik_is_complex(St->dtype)) return cst_sub(St, T_, alpha, x, beta, y, scalar_dtype);
    if (St->dtype == MIK_F64) {
        double *xd = (double *)x;
        if (!y) return st_tri<double, double, false>(St, T_, 0.0, xd, 0.0, nullptr);
        const double a = scalar_dtype == MIK_F64 ? st_scalar<double>(alpha) : (double)st_scalar<float>(alpha);
        const double b = scalar_dtype == MIK_F64 ? st_scalar<double>(beta) : (double)st_scalar<float>(beta);
        return st_tri<double, double, true>(St, T_, a, xd, b, (const double *)y);
    }
    float *xf = (float *)x;
    if (!y) return st_tri<float, float, false>(St, T_, 0.0f, xf, 0.0f, nullptr);
    if (scalar_dtype == MIK_F64)       // Float32 data, Float64 omega: alpha*x/d + beta*y in Float64, one rounding at the store
        return st_tri<float, double, true>(St, T_, st_scalar<double>(alpha), xf, st_scalar<double>(beta), (const float *)y);
    return st_tri<float, float, true>(St, T_, st_scalar<float>(alpha), xf, st_scalar<float>(beta), (const float *)y);
}

template <typename T>
int st_offdiag(mik_stationary *St, const void *alpha, const void *x, const void *beta, void *y)
{
    const T a = st_scalar<T>(alpha), b = st_scalar<T>(beta);
    const int bmode = b == T(1) ? 1 : (b == T(0) ? 0 : 2);
    hipLaunchKernelGGL((k_st_offdiag<T>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const T *)St->vl, St->dg,
                       a, (const T *)x, b, bmode, (T *)y);
    MIK_LAUNCH_CHECK(St->ctx);
    return MIK_OK;
}

template <typename T>
int st_gs(mik_stationary *St, bool upper, const void *alpha, const void *x, const void *beta, const void *y, void *z)
{
    const T a = st_scalar<T>(alpha), b = st_scalar<T>(beta);
    const T *xs = (const T *)x;
    if (z == x) {       // GaussSeidelIterable passes z === x: every row reads the OLD x (:178-208), so the sweep reads a copy
        MIK_HIP(St->ctx, hipMemcpyAsync(St->tmp, x, sizeof(T) * (size_t)St->n, hipMemcpyDeviceToDevice, St->ctx->stream));
        xs = (const T *)St->tmp;
    }
    if (upper)
        hipLaunchKernelGGL((k_st_gs_mul<T, true>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const T *)St->vl,
                           St->dg, a, xs, b, (const T *)y, (T *)z);
    else
        hipLaunchKernelGGL((k_st_gs_mul<T, false>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const T *)St->vl,
                           St->dg, a, xs, b, (const T *)y, (T *)z);
    MIK_LAUNCH_CHECK(St->ctx);
    return MIK_OK;
}

// ---- complex operators: R = the component type, scalars are (re, im) pairs -----------------------------------------------------------
template <typename R>
bool cst_aligned(std::initializer_list<const void *> ps)
{
    for (const void *p : ps)
        if (p && (uintptr_t)p % (2 * sizeof(R)) != 0) return false;
    return true;
}

template <typename R, typename E, bool RELAX>
int cst_tri(mik_stationary *St, const StTri &T_, E alpha, R *x, E ber, E bei, const R *y)
{
    mik_ctx *ctx = St->ctx;
    const int vec = cst_aligned<R>({x, y}) ? 1 : 0;
    for (const StLaunch &L : T_.plan) {
        if (L.narrow)
            hipLaunchKernelGGL((k_cst_tri_run<R, E, RELAX>), dim3(1), dim3(MIK_ST_BLOCK), 0, ctx->stream, L.a, L.b, T_.lev, T_.perm, T_.tp, T_.tc,
                               (const R *)T_.tv, (const R *)St->d, alpha, x, ber, bei, y, vec);
        else
            hipLaunchKernelGGL((k_cst_tri_level<R, E, RELAX>), dim3(st_grid(L.b - L.a)), dim3(MIK_ST_BLOCK), 0, ctx->stream, L.a, L.b, T_.perm, T_.tp,
                               T_.tc, (const R *)T_.tv, (const R *)St->d, alpha, x, ber, bei, y, vec);
    }
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// alpha: a host REAL of scalar_dtype (omega is Real in the reference); beta: a host COMPLEX pair of scalar_dtype (one(T) - omega)
template <typename E>
void cst_relax_scalars(const void *alpha, const void *beta, int scalar_dtype, E &a, E &br, E &bi)
{
    if (scalar_dtype == MIK_F64) {
        double b[2]; memcpy(b, beta, sizeof b);
        a = (E)st_scalar<double>(alpha); br = (E)b[0]; bi = (E)b[1];
    } else {
        float b[2]; memcpy(b, beta, sizeof b);
        a = (E)st_scalar<float>(alpha); br = (E)b[0]; bi = (E)b[1];
    }
}

int cst_sub(mik_stationary *St, const StTri &T_, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype)
{
    if (St->dtype == MIK_C64) {       // ComplexF64 data: every omega type evaluates in Float64
        double *xd = (double *)x;
        if (!y) return cst_tri<double, double, false>(St, T_, 0.0, xd, 0.0, 0.0, nullptr);
        double a, br, bi;
        cst_relax_scalars(alpha, beta, scalar_dtype, a, br, bi);
        return cst_tri<double, double, true>(St, T_, a, xd, br, bi, (const double *)y);
    }
    float *xf = (float *)x;
    if (!y) return cst_tri<float, float, false>(St, T_, 0.0f, xf, 0.0f, 0.0f, nullptr);
    if (scalar_dtype == MIK_F64) {    // ComplexF32 data, Float64 omega: the 64-bit division, one rounding per component at the store
        double a, br, bi;
        cst_relax_scalars(alpha, beta, scalar_dtype, a, br, bi);
        return cst_tri<float, double, true>(St, T_, a, xf, br, bi, (const float *)y);
    }
    float a, br, bi;
    cst_relax_scalars(alpha, beta, scalar_dtype, a, br, bi);
    return cst_tri<float, float, true>(St, T_, a, xf, br, bi, (const float *)y);
}

template <typename R>
int cst_diag_ldiv(mik_stationary *St, void *y, const void *x)
{
    hipLaunchKernelGGL((k_cst_diag_ldiv<R>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, (const R *)St->d, (const R *)x, (R *)y,
                       cst_aligned<R>({x, y}) ? 1 : 0);
    MIK_LAUNCH_CHECK(St->ctx);
    return MIK_OK;
}

template <typename R>
int cst_offdiag(mik_stationary *St, const void *alpha, const void *x, const void *beta, void *y)
{
    R a[2], b[2];
    memcpy(a, alpha, sizeof a);
    memcpy(b, beta, sizeof b);
    const int bmode = (b[0] == R(1) && b[1] == R(0)) ? 1 : ((b[0] == R(0) && b[1] == R(0)) ? 0 : 2);      // beta != one(T); iszero(beta)
    hipLaunchKernelGGL((k_cst_offdiag<R>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const R *)St->vl, St->dg,
                       a[0], a[1], (const R *)x, b[0], b[1], bmode, (R *)y, cst_aligned<R>({x, y}) ? 1 : 0);
    MIK_LAUNCH_CHECK(St->ctx);
    return MIK_OK;
}

template <typename R>
int cst_gs(mik_stationary *St, bool upper, const void *alpha, const void *x, const void *beta, const void *y, void *z)
{
    R a[2], b[2];
    memcpy(a, alpha, sizeof a);
    memcpy(b, beta, sizeof b);
    const R *xs = (const R *)x;
    if (z == x) {       // as st_gs: every row reads the OLD x
        MIK_HIP(St->ctx, hipMemcpyAsync(St->tmp, x, 2 * sizeof(R) * (size_t)St->n, hipMemcpyDeviceToDevice, St->ctx->stream));
        xs = (const R *)St->tmp;
    }
    const int vec = cst_aligned<R>({xs, y, z}) ? 1 : 0;
    if (upper)
        hipLaunchKernelGGL((k_cst_gs_mul<R, true>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const R *)St->vl,
                           St->dg, a[0], a[1], xs, b[0], b[1], (const R *)y, (R *)z, vec);
    else
        hipLaunchKernelGGL((k_cst_gs_mul<R, false>), dim3(st_grid(St->n)), dim3(MIK_ST_BLOCK), 0, St->ctx->stream, St->n, St->rp, St->cl, (const R *)St->vl,
                           St->dg, a[0], a[1], xs, b[0], b[1], (const R *)y, (R *)z, vec);
    MIK_LAUNCH_CHECK(St->ctx);
    return MIK_OK;
}

}  // namespace

extern "C" int mik_stationary_create(mik_ctx *ctx, const mik_csr *A, int64_t *singular_col, mik_stationary **out)
{
    if (singular_col) *singular_col = 0;
    if (!ctx || !A || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (A->n_rows != A->n_cols)
        return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_stationary_create: the operator is %lld x %lld, not square", (long long)A->n_rows, (long long)A->n_cols);
    if (!A->col || !A->rowptr || !A->val)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_stationary_create: the CSR arrays of this operator were released (mik_csr_compact)");
    mik_stationary *S = new (std::nothrow) mik_stationary();
    if (!S) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_stationary_create: host allocation failed");
    int rc;
    try {
        rc = st_create(ctx, A, singular_col, S);
    } catch (const std::bad_alloc &) {
        rc = mik_fail(ctx, MIK_ERR_NOMEM, "mik_stationary_create: host allocation failed");
    }
    if (rc != MIK_OK) { st_free(S); return rc; }
    *out = S;
    return MIK_OK;
}

extern "C" int mik_stationary_destroy(mik_stationary *S)
{
    st_free(S);
    return MIK_OK;
}

extern "C" int mik_stationary_info(const mik_stationary *S, int64_t *levels, int64_t *launches, int64_t *bytes, double *analysis_ms)
{
    if (!S) return MIK_ERR_INVALID;
    if (levels) { levels[0] = S->lo.levels; levels[1] = S->up.levels; }
    if (launches) { launches[0] = (int64_t)S->lo.plan.size(); launches[1] = (int64_t)S->up.plan.size(); }
    if (bytes) *bytes = S->bytes;
    if (analysis_ms) *analysis_ms = S->analysis_ms;
    return MIK_OK;
}

extern "C" int mik_diag_ldiv(mik_stationary *S, void *y, const void *x)
{
    if (!S || !x || !y) return MIK_ERR_INVALID;
    if (S->n == 0) return MIK_OK;
    if (mik_is_complex(S->dtype)) return S->dtype == MIK_C64 ? cst_diag_ldiv<double>(S, y, x) : cst_diag_ldiv<float>(S, y, x);
    if (S->dtype == MIK_F64)
        hipLaunchKernelGGL((k_st_diag_ldiv<double>), dim3(st_grid(S->n)), dim3(MIK_ST_BLOCK), 0, S->ctx->stream, S->n, (const double *)S->d, (const double *)x, (double *)y);
    else
        hipLaunchKernelGGL((k_st_diag_ldiv<float>), dim3(st_grid(S->n)), dim3(MIK_ST_BLOCK), 0, S->ctx->stream, S->n, (const float *)S->d, (const float *)x, (float *)y);
    MIK_LAUNCH_CHECK(S->ctx);
    return MIK_OK;
}

extern "C" int mik_offdiag_mul(mik_stationary *S, const void *alpha, const void *x, const void *beta, void *y)
{
    if (!S || !alpha || !beta || !x || !y) return MIK_ERR_INVALID;
    if (x == y) return mik_fail(S->ctx, MIK_ERR_INVALID, "mik_offdiag_mul: x and y must not alias");
    if (S->n == 0) return MIK_OK;
    if (mik_is_complex(S->dtype)) return S->dtype == MIK_C64 ? cst_offdiag<double>(S, alpha, x, beta, y) : cst_offdiag<float>(S, alpha, x, beta, y);
    return S->dtype == MIK_F64 ? st_offdiag<double>(S, alpha, x, beta, y) : st_offdiag<float>(S, alpha, x, beta, y);
}

extern "C" int mik_gs_multiply(mik_stationary *S, int upper, const void *alpha, const void *x, const void *beta, const void *y, void *z)
{
    if (!S || !alpha || !beta || !x || !y || !z) return MIK_ERR_INVALID;
    if (S->n == 0) return MIK_OK;
    if (mik_is_complex(S->dtype))
        return S->dtype == MIK_C64 ? cst_gs<double>(S, upper != 0, alpha, x, beta, y, z) : cst_gs<float>(S, upper != 0, alpha, x, beta, y, z);
    return S->dtype == MIK_F64 ? st_gs<double>(S, upper != 0, alpha, x, beta, y, z) : st_gs<float>(S, upper != 0, alpha, x, beta, y, z);
}

extern "C" int mik_forward_sub(mik_stationary *S, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype)
{
    return st_sub(S, false, alpha, x, beta, y, scalar_dtype, "mik_forward_sub");
}

extern "C" int mik_backward_sub(mik_stationary *S, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype)
{
    return st_sub(S, true, alpha, x, beta, y, scalar_dtype, "mik_backward_sub");
}
