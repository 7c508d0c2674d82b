// mik_dense_stationary.hip -- Jacobi, Gauss-Seidel, SOR and SSOR on a dense column-major device matrix (src/stationary.jl:31-263):
// one C entry per whole iteration.
//
// An iteration is a row-owned sweep (csrc/mik_dense_stationary.h) and, for the three methods with a triangular half, the forward
// substitution in its PANEL form: ceil(n / W) launches that follow each other on the stream, launch K subtracting panel K - 1 from the
// rows at or below panel K and then solving the diagonal block of panel K in the one workgroup that owns it.  No workgroup waits for
// another one.  The chained (single-launch, workgroups handing x on to each other) form the plan struct names is not built; a plan that asks
// for it is refused.
// The handle holds a copy of the old x (read by the sweeps that store into x: Jacobi and the backward half of SSOR) and the
// accumulators of Gauss-Seidel, which has no tmp of its own.  Nothing is allocated per step.
#include "mik_internal.h"
#include "mik_dense_stationary.h"

#include <new>

struct mik_dense_stationary {
    mik_ctx *ctx = nullptr;
    int dtype = MIK_F64;
    int n = 0;
    int64_t ld = 0;
    const void *A = nullptr;
    void *xold = nullptr, *acc = nullptr;
    int *first = nullptr;
    int form = MIK_DENSE_PANEL;
    int gave_up = 0;
    int64_t bytes = 0;
};

namespace {

void ds_free(mik_dense_stationary *S)
{
    if (!S) return;
    if (S->ctx) { (void)hipSetDevice(S->ctx->device); (void)hipStreamSynchronize(S->ctx->stream); }
    for (void *p : {S->xold, S->acc, (void *)S->first})
        if (p) (void)hipFree(p);
    delete S;
}

inline unsigned ds_grid(int rows) { return (unsigned)((rows + MIK_DS_R - 1) / MIK_DS_R); }

template <typename T>
int ds_check_diag(mik_dense_stationary *S, int64_t *singular_col)
{
    mik_ctx *ctx = S->ctx;
    int first = S->n;
    MIK_HIP(ctx, hipMemcpyAsync(S->first, &first, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL((k_ds_check_diag<T>), dim3((unsigned)((S->n + 255) / 256)), dim3(256), 0, ctx->stream, S->n, (const T *)S->A, S->ld, S->first);
    MIK_LAUNCH_CHECK(ctx);
    MIK_HIP(ctx, hipMemcpyAsync(&first, S->first, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (first < S->n) {
        if (singular_col) *singular_col = (int64_t)first + 1;
        return mik_fail(ctx, MIK_ERR_SINGULAR, "mik_dense_stationary_create: SingularException(%d): zero diagonal entry", first + 1);
    }
    return MIK_OK;
}

int ds_create(mik_dense_stationary *S, int64_t *singular_col)
{
    mik_ctx *ctx = S->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t vec = std::max<size_t>((size_t)S->n * mik_dtype_size(S->dtype), 16);
    MIK_HIP(ctx, hipMalloc(&S->xold, vec));
    MIK_HIP(ctx, hipMalloc(&S->acc, vec));
    MIK_HIP(ctx, hipMalloc((void **)&S->first, 16));
    S->bytes = (int64_t)(2 * vec + 16);
    return S->dtype == MIK_F64 ? ds_check_diag<double>(S, singular_col) : ds_check_diag<float>(S, singular_col);
}

template <typename T, typename W, int MODE>
void ds_row(mik_dense_stationary *S, const T *x, const T *b, T *acc_out, T *out, W omega)
{
    hipLaunchKernelGGL((k_ds_row<T, W, MODE>), dim3(ds_grid(S->n)), dim3(MIK_DS_R), 0, S->ctx->stream, S->n, (const T *)S->A, S->ld, x, b, acc_out, out, omega);
}

// the strict-lower phase of one sweep (:121-126, :180-185, :240-245): panel after panel
template <typename T, typename W, bool RELAX>
void ds_forward(mik_dense_stationary *S, T *t, T *x, W omega)
{
    for (int k0 = 0; k0 < S->n; k0 += MIK_DS_W)
        hipLaunchKernelGGL((k_ds_panel<T, W, RELAX>), dim3(ds_grid(S->n - k0)), dim3(MIK_DS_R), 0, S->ctx->stream, S->n, k0, (const T *)S->A, S->ld, t, x, omega);
}

template <typename T>
int ds_keep_old(mik_dense_stationary *S, const T *x)
{
    MIK_HIP(S->ctx, hipMemcpyAsync(S->xold, x, sizeof(T) * (size_t)S->n, hipMemcpyDeviceToDevice, S->ctx->stream));
    return MIK_OK;
}

template <typename T>
int ds_jacobi(mik_dense_stationary *S, T *x, T *next, const T *b)
{
    MIK_TRY(ds_keep_old<T>(S, x));
    ds_row<T, T, MIK_DS_JACOBI>(S, (const T *)S->xold, b, next, x, T(0));
    MIK_LAUNCH_CHECK(S->ctx);
    return MIK_OK;
}

template <typename T>
int ds_gs(mik_dense_stationary *S, T *x, const T *b)
{
    ds_row<T, T, MIK_DS_UPPER>(S, x, b, (T *)S->acc, (T *)nullptr, T(0));      // x is only read until the first panel stores into it
    ds_forward<T, T, false>(S, (T *)S->acc, x, T(0));
    MIK_LAUNCH_CHECK(S->ctx);
    return MIK_OK;
}

template <typename T, typename W>
int ds_sor(mik_dense_stationary *S, T *x, T *tmp, const T *b, W omega, bool symmetric)
{
    ds_row<T, W, MIK_DS_UPPER>(S, x, b, tmp, (T *)nullptr, omega);
    ds_forward<T, W, true>(S, tmp, x, omega);
    if (symmetric) {                                                           // :247-260: every product reads the forward half's x
        MIK_TRY(ds_keep_old<T>(S, x));
        ds_row<T, W, MIK_DS_BACKWARD>(S, (const T *)S->xold, b, tmp, x, omega);
    }
    MIK_LAUNCH_CHECK(S->ctx);
    return MIK_OK;
}

bool ds_disjoint(const mik_dense_stationary *S, std::initializer_list<const void *> v)
{
    const size_t bytes = (size_t)S->n * mik_dtype_size(S->dtype);
    for (auto p = v.begin(); p != v.end(); ++p)
        for (auto q = p + 1; q != v.end(); ++q)
            if (mik_overlap(*p, bytes, *q, bytes)) return false;
    return true;
}

int ds_relaxed(mik_dense_stationary *S, void *x, void *tmp, const void *b, const void *omega, int scalar_dtype, bool symmetric, const char *who)
{
    if (!S || !x || !tmp || !b || !omega) return MIK_ERR_INVALID;
    if (scalar_dtype != MIK_F64 && scalar_dtype != MIK_F32) return mik_fail(S->ctx, MIK_ERR_INVALID, "%s: scalar_dtype must be MIK_F64 or MIK_F32", who);
    if (!ds_disjoint(S, {x, tmp, b})) return mik_fail(S->ctx, MIK_ERR_INVALID, "%s: x, tmp and b must not overlap", who);
    double w64 = 0.0;
    float w32 = 0.0f;
    if (scalar_dtype == MIK_F64) memcpy(&w64, omega, 8); else memcpy(&w32, omega, 4);
    if (S->dtype == MIK_F64)
        return ds_sor<double, double>(S, (double *)x, (double *)tmp, (const double *)b, scalar_dtype == MIK_F64 ? w64 : (double)w32, symmetric);
    if (scalar_dtype == MIK_F64)       // Float32 data, Float64 omega: x + omega * (tmp / d - x) in Float64, one rounding at the store
        return ds_sor<float, double>(S, (float *)x, (float *)tmp, (const float *)b, w64, symmetric);
    return ds_sor<float, float>(S, (float *)x, (float *)tmp, (const float *)b, w32, symmetric);
}

}  // namespace

extern "C" int mik_dense_stationary_create(mik_ctx *ctx, const void *A, int64_t n, int64_t ld, int dtype, const mik_dense_plan *plan,
                                           int64_t *singular_col, mik_dense_stationary **out)
{
    if (singular_col) *singular_col = 0;
    if (!ctx || !A || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (dtype != MIK_F64 && dtype != MIK_F32) return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_stationary_create: dtype must be MIK_F64 or MIK_F32");
    if (n < 1 || ld < n) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_dense_stationary_create: n = %lld, ld = %lld (need 1 <= n <= ld)", (long long)n, (long long)ld);
    if (n > (int64_t)std::numeric_limits<int>::max() - MIK_DS_R) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_dense_stationary_create: n >= 2^31");
    const int form = plan ? plan->form : MIK_DENSE_AUTO;
    if (form != MIK_DENSE_AUTO && form != MIK_DENSE_PANEL && form != MIK_DENSE_CHAINED)
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_stationary_create: unknown form %d", form);
    if (plan && plan->spin_limit < 0) return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_stationary_create: negative spin limit");
    if (form == MIK_DENSE_CHAINED)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_dense_stationary_create: the chained form of the forward substitution is not built; use the panel form");
    mik_dense_stationary *S = new (std::nothrow) mik_dense_stationary();
    if (!S) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_dense_stationary_create: host allocation failed");
    S->ctx = ctx; S->dtype = dtype; S->n = (int)n; S->ld = ld; S->A = A;
    const int rc = ds_create(S, singular_col);
    if (rc != MIK_OK) { ds_free(S); return rc; }
    *out = S;
    return MIK_OK;
}

extern "C" int mik_dense_stationary_destroy(mik_dense_stationary *S)
{
    ds_free(S);
    return MIK_OK;
}

extern "C" int mik_dense_stationary_info(const mik_dense_stationary *S, int64_t *panel_w, int64_t *rows_per_workgroup, int64_t *launches_forward,
                                         int *form, int *gave_up, int64_t *bytes)
{
    if (!S) return MIK_ERR_INVALID;
    if (panel_w) *panel_w = MIK_DS_W;
    if (rows_per_workgroup) *rows_per_workgroup = MIK_DS_R;
    if (launches_forward) *launches_forward = ((int64_t)S->n + MIK_DS_W - 1) / MIK_DS_W;
    if (form) *form = S->form;
    if (gave_up) *gave_up = S->gave_up;
    if (bytes) *bytes = S->bytes;
    return MIK_OK;
}

extern "C" int mik_dense_jacobi_step(mik_dense_stationary *S, void *x, void *next, const void *b)
{
    if (!S || !x || !next || !b) return MIK_ERR_INVALID;
    if (!ds_disjoint(S, {x, next, b})) return mik_fail(S->ctx, MIK_ERR_INVALID, "mik_dense_jacobi_step: x, next and b must not overlap");
    return S->dtype == MIK_F64 ? ds_jacobi<double>(S, (double *)x, (double *)next, (const double *)b)
                               : ds_jacobi<float>(S, (float *)x, (float *)next, (const float *)b);
}

extern "C" int mik_dense_gs_step(mik_dense_stationary *S, void *x, const void *b)
{
    if (!S || !x || !b) return MIK_ERR_INVALID;
    if (!ds_disjoint(S, {x, b})) return mik_fail(S->ctx, MIK_ERR_INVALID, "mik_dense_gs_step: x and b must not overlap");
    return S->dtype == MIK_F64 ? ds_gs<double>(S, (double *)x, (const double *)b) : ds_gs<float>(S, (float *)x, (const float *)b);
}

extern "C" int mik_dense_sor_step(mik_dense_stationary *S, void *x, void *tmp, const void *b, const void *omega, int scalar_dtype)
{
    return ds_relaxed(S, x, tmp, b, omega, scalar_dtype, false, "mik_dense_sor_step");
}

extern "C" int mik_dense_ssor_step(mik_dense_stationary *S, void *x, void *tmp, const void *b, const void *omega, int scalar_dtype)
{
    return ds_relaxed(S, x, tmp, b, omega, scalar_dtype, true, "mik_dense_ssor_step");
}
