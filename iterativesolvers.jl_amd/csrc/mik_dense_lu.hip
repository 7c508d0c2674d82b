// mik_dense_lu.hip -- lu!(A) with partial pivoting and ldiv!(y, F, x) on a square column-major device matrix: what the reference's
// tests pass as Pl / Pr (test/gmres.jl:28-35, test/bicgstabl.jl:40-42) and as the operator of invpowm.
//
// The bit contract is stated in csrc/mik_dense_lu.h: the factors, the pivots and the solution are those of the unblocked loops of
// lu_solve<T> (csrc/mik_krylov.hip).  The plan is right-looking over panels of W columns:
//   panel     per column j: pick (one workgroup: combine the search partials, interchange inside the panel) and update (divide the
//             column, subtract it from the panel columns to its right, search column j + 1); the first column of a panel is searched
//             by a launch of its own
//   outside   the panel's interchanges on the columns left and right of it, the strip solve U12 = L11^-1 A12, the trailing update
// Every dependency between workgroups is a kernel boundary on the context's stream.  A zero pivot column records its index and the
// remaining launches still run; create reads the flag (and the pivots) once at the end -- the factorisation's only host synchronisation.
// ldiv! is a gather into the handle's work vector and ceil(n / W) launches each way; nothing is allocated per solve.  A block of right-hand
// sides runs the same launches per pass of MIK_DS_G columns, NB columns per lane, through a workspace the handle allocates at the first one.
#include "mik_internal.h"
#include "mik_dense_factor.h"
#include "mik_dense_lu.h"

#include <type_traits>
#include <vector>

struct mik_dense_lu : mik_dense_factor {      // aux: the interchanges as one gather, n integers
    std::vector<int> ipiv;           // host, 0-based
    std::vector<int> perm_host;
};

namespace {

struct lu_scratch {                  // device memory of the factorisation only
    void *pval = nullptr;
    int *prow = nullptr, *ipiv = nullptr, *flag = nullptr;
    ~lu_scratch()
    {
        for (void *p : {pval, (void *)prow, (void *)ipiv, (void *)flag})
            if (p) (void)hipFree(p);
    }
};

template <typename T>
int lu_factor(mik_dense_lu *F, int64_t *singular_col)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const int64_t ld = F->ld;
    T *A = (T *)F->A;
    lu_scratch s;
    const size_t nparts = dense_grid(n, MIK_LU_R);
    MIK_HIP(ctx, hipMalloc(&s.pval, std::max<size_t>(nparts * sizeof(T), 16)));
    MIK_HIP(ctx, hipMalloc((void **)&s.prow, std::max<size_t>(nparts * sizeof(int), 16)));
    MIK_HIP(ctx, hipMalloc((void **)&s.ipiv, std::max<size_t>((size_t)n * sizeof(int), 16)));
    MIK_HIP(ctx, hipMalloc((void **)&s.flag, 16));
    MIK_TRY(dense_flag_arm(ctx, s.flag));
    T *pval = (T *)s.pval;
    int64_t launches = 0;
    for (int k0 = 0; k0 < n; k0 += MIK_LU_W) {
        const int k1 = std::min(k0 + MIK_LU_W, n);
        hipLaunchKernelGGL((k_lu_search<T>), dim3(dense_grid(n - k0, MIK_LU_R)), dim3(MIK_LU_R), 0, st, n, k0, (const T *)A, ld, pval, s.prow);
        ++launches;
        for (int j = k0; j < k1; ++j) {
            hipLaunchKernelGGL((k_lu_pick<T>), dim3(1), dim3(64), 0, st, n, j, k0, k1, A, ld, (int)dense_grid(n - j, MIK_LU_R), (const T *)pval,
                               (const int *)s.prow, s.ipiv, s.flag);
            ++launches;
            if (j + 1 < n) {
                hipLaunchKernelGGL((k_lu_update<T>), dim3(dense_grid(n - j - 1, MIK_LU_R)), dim3(MIK_LU_R), 0, st, n, j, k1, A, ld, pval, s.prow);
                ++launches;
            }
        }
        if (n > k1 - k0) {
            hipLaunchKernelGGL((k_lu_swap<T>), dim3(dense_grid(n - (k1 - k0), 64)), dim3(64), 0, st, n, k0, k1, A, ld, (const int *)s.ipiv);
            ++launches;
        }
        if (k1 < n) {
            hipLaunchKernelGGL((k_lu_strip<T>), dim3(dense_grid(n - k1, 64)), dim3(64), 0, st, n, k0, A, ld);
            const unsigned tr = dense_grid(n - k1, MIK_LU_TR), tc = dense_grid(n - k1, MIK_LU_TC);
            hipLaunchKernelGGL((k_dense_trail<T, false>), dim3(tr, tc), dim3(MIK_DS_THREADS), 0, st, n, k0, A, ld);
            launches += 2;
        }
        MIK_LAUNCH_CHECK(ctx);
    }
    F->launches_factor = launches;
    int first = 0;
    F->ipiv.resize((size_t)n);
    MIK_HIP(ctx, hipMemcpyAsync(F->ipiv.data(), s.ipiv, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    MIK_TRY(dense_flag_read(ctx, s.flag, &first));
    if (first < n) {
        if (singular_col) *singular_col = (int64_t)first + 1;
        return mik_fail(ctx, MIK_ERR_SINGULAR, "mik_dense_lu_create: SingularException(%d): zero pivot column", first + 1);
    }
    F->perm_host.resize((size_t)n);
    for (int i = 0; i < n; ++i) F->perm_host[(size_t)i] = i;
    for (int j = 0; j < n; ++j) std::swap(F->perm_host[(size_t)j], F->perm_host[(size_t)F->ipiv[(size_t)j]]);
    MIK_HIP(ctx, hipMemcpyAsync(F->aux, F->perm_host.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    return MIK_OK;
}

template <typename T>
int lu_solve_dev(mik_dense_lu *F, T *y, const T *x)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const T *A = (const T *)F->A;
    T *t = (T *)F->work;
    hipLaunchKernelGGL((k_lu_gather<T>), dim3(dense_grid(n, 256)), dim3(256), 0, st, n, (const int *)F->aux, x, t);
    for (int k0 = 0; k0 < n; k0 += MIK_LU_W)
        hipLaunchKernelGGL((k_dense_fwd<T, true>), dim3(dense_grid(n - k0, MIK_DS_R)), dim3(MIK_DS_R), 0, st, n, k0, A, F->ld, (const T *)t, t);
    for (int k0 = (n - 1) / MIK_LU_W * MIK_LU_W; k0 >= 0; k0 -= MIK_LU_W)
        hipLaunchKernelGGL((k_lu_bwd<T>), dim3((unsigned)(k0 / MIK_DS_R + 1)), dim3(MIK_DS_R), 0, st, n, k0, std::min(k0 + MIK_LU_W, n), A, F->ld, t, y);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// one pass of a block solve: the `cols` columns from x to y through the groups of the block workspace t, NB columns per lane
template <int NB, typename T>
int lu_solve_block_dev(mik_dense_lu *F, T *t, T *y, int64_t ldy, const T *x, int64_t ldx, int cols)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const T *A = (const T *)F->A;
    const unsigned groups = dense_grid(cols, NB);
    hipLaunchKernelGGL((k_lu_gather_nb<T, NB>), dim3(dense_grid(n, 256), groups), dim3(256), 0, st, n, (const int *)F->aux, x, ldx, cols, t);
    for (int k0 = 0; k0 < n; k0 += MIK_LU_W)
        hipLaunchKernelGGL((k_dense_fwd_nb<T, true, NB>), dim3(dense_grid(n - k0, MIK_DS_R), groups), dim3(MIK_DS_R), 0, st, n, k0, A, F->ld, (const T *)nullptr, (int64_t)0, cols, t);
    for (int k0 = (n - 1) / MIK_LU_W * MIK_LU_W; k0 >= 0; k0 -= MIK_LU_W)
        hipLaunchKernelGGL((k_lu_bwd_nb<T, NB>), dim3((unsigned)(k0 / MIK_DS_R + 1), groups), dim3(MIK_DS_R), 0, st, n, k0, std::min(k0 + MIK_LU_W, n), A, F->ld, t, y, ldy, cols);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

int64_t lu_launches_solve(const mik_dense_lu *F) { return 1 + 2 * (((int64_t)F->n + MIK_LU_W - 1) / MIK_LU_W); }

}  // namespace

extern "C" int mik_dense_lu_create(mik_ctx *ctx, void *A, int64_t n, int64_t ld, int dtype, int64_t *singular_col, mik_dense_lu **out)
{
    if (singular_col) *singular_col = 0;
    if (!ctx || !A || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (dtype == MIK_C64 || dtype == MIK_C32)
        return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_dense_lu_create: lu is not built for %s (it needs |re| + |im| pivots and a complex division on the device)",
                        dtype == MIK_C64 ? "ComplexF64 (MIK_C64)" : "ComplexF32 (MIK_C32)");
    if (dtype != MIK_F64 && dtype != MIK_F32) return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_lu_create: dtype must be MIK_F64 or MIK_F32");
    mik_dense_lu *F = nullptr;
    int rc = dense_new(ctx, "mik_dense_lu_create", A, n, ld, dtype, true, &F);
    if (rc == MIK_OK) rc = dense_dispatch<false>(dtype, [&](auto e) { return lu_factor<decltype(e)>(F, singular_col); });
    if (rc != MIK_OK) { dense_free(F); return rc; }
    *out = F;
    return MIK_OK;
}

extern "C" int mik_dense_lu_destroy(mik_dense_lu *F)
{
    dense_free(F);
    return MIK_OK;
}

extern "C" int mik_dense_lu_ipiv(const mik_dense_lu *F, int64_t *ipiv)
{
    if (!F || !ipiv) return MIK_ERR_INVALID;
    for (int i = 0; i < F->n; ++i) ipiv[i] = (int64_t)F->ipiv[(size_t)i] + 1;
    return MIK_OK;
}

extern "C" int mik_dense_lu_solve(mik_dense_lu *F, void *y, const void *x)
{
    if (!F || !y || !x) return MIK_ERR_INVALID;
    MIK_TRY(dense_check_solve(F, "mik_dense_lu_solve", y, x));
    return dense_dispatch<false>(F->dtype, [&](auto e) { return lu_solve_dev(F, (decltype(e) *)y, (const decltype(e) *)x); });
}

extern "C" int mik_dense_lu_solve_block(mik_dense_lu *F, void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs)
{
    if (!F || !Y || !X) return MIK_ERR_INVALID;
    MIK_TRY(dense_check_block(F, "mik_dense_lu_solve_block", Y, ldy, X, ldx, nrhs));
    return dense_block_passes<false>(F, Y, ldy, X, ldx, nrhs, [&](auto *t, auto *y, auto *x, int cols) {
        return lu_solve_block_dev<de_block<std::remove_pointer_t<decltype(t)>>::NB>(F, t, y, ldy, x, ldx, cols);
    });
}

extern "C" int mik_dev_dense_lu_block_plan(const mik_dense_lu *F, int64_t nrhs, int64_t *nb, int64_t *g, int64_t *passes, int64_t *launches, int64_t *workspace_bytes)
{
    if (!F) return MIK_ERR_INVALID;
    return dense_block_query(F, nrhs, lu_launches_solve(F), nb, g, passes, launches, workspace_bytes);
}

extern "C" int mik_dense_lu_ldiv_fn(void *user, void *y, const void *x) { return mik_dense_lu_solve((mik_dense_lu *)user, y, x); }

extern "C" int mik_dense_lu_info(const mik_dense_lu *F, int64_t *panel_w, int64_t *search_rows, int64_t *tile_rows, int64_t *tile_cols,
                                 int64_t *one_launch_rows, int64_t *launches_factor, int64_t *launches_solve, int64_t *bytes)
{
    if (!F) return MIK_ERR_INVALID;
    if (panel_w) *panel_w = MIK_LU_W;
    if (search_rows) *search_rows = MIK_LU_R;
    if (tile_rows) *tile_rows = MIK_LU_TR;
    if (tile_cols) *tile_cols = MIK_LU_TC;
    if (one_launch_rows) *one_launch_rows = 0;                 // the one-launch panel is not built
    if (launches_factor) *launches_factor = F->launches_factor;
    if (launches_solve) *launches_solve = lu_launches_solve(F);
    if (bytes) *bytes = F->bytes;
    return MIK_OK;
}
