// mik_dense_chol.hip -- cholesky!(Hermitian(A, :L)) and ldiv!(y, F, x) on a square column-major device matrix, real and complex: what the
// reference's tests pass as Pl to cg (test/cg.jl:44-47) and to chebyshev (test/chebyshev.jl:59-66) in all four element types.
//
// The bit contract and the kernels are in csrc/mik_dense_chol.h.  The plan is right-looking over panels of W columns, three launches per
// panel -- the diagonal block in one workgroup, the rows below it, the lower tiles of the trailing update -- where the pivoted LU needs
// 2 W + 4; the last panel has no rows below it and is one launch.  Every dependency between workgroups is a kernel boundary on the context's
// stream.  A column whose pivot is not positive records its index and the remaining launches still run; create reads the flag once at the
// end -- the factorisation's only host synchronisation.  ldiv! is ceil(n / W) launches each way; nothing is allocated per solve.  A block of
// right-hand sides runs the same launches per pass of MIK_DS_G columns, NB columns per lane, through a workspace the handle allocates at the
// first one.
#include "mik_internal.h"
#include "mik_dense_factor.h"
#include "mik_dense_chol.h"

#include <type_traits>

struct mik_dense_chol : mik_dense_factor {    // aux: the flag -- the first failing column, or a value above every column index
    int64_t info = 0;                // 0, or the 1-based index of the first column whose pivot was not positive
};

namespace {

template <typename E>
int chol_factor(mik_dense_chol *F)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const int64_t ld = F->ld;
    E *A = (E *)F->A;
    MIK_TRY(dense_flag_arm(ctx, F->aux));
    int64_t launches = 0;
    for (int k0 = 0; k0 < n; k0 += MIK_CH_W) {
        const int k1 = std::min(k0 + MIK_CH_W, n);
        hipLaunchKernelGGL((k_chol_diag<E>), dim3(1), dim3(MIK_CH_THREADS), 0, st, k0, k1 - k0, A, ld, F->aux);
        ++launches;
        if (k1 < n) {
            const unsigned tiles = dense_grid(n - k1, MIK_CH_T);
            hipLaunchKernelGGL((k_chol_panel<E>), dim3(dense_grid(n - k1, MIK_CH_R)), dim3(MIK_CH_THREADS), 0, st, n, k0, k1 - k0, A, ld);
            hipLaunchKernelGGL((k_dense_trail<E, true>), dim3(tiles, tiles), dim3(MIK_DS_THREADS), 0, st, n, k0, A, ld);
            launches += 2;
        }
        MIK_LAUNCH_CHECK(ctx);
    }
    F->launches_factor = launches;
    int first = 0;
    MIK_TRY(dense_flag_read(ctx, F->aux, &first));
    F->info = first < n ? (int64_t)first + 1 : 0;
    return MIK_OK;
}

template <typename E>
int chol_solve_dev(mik_dense_chol *F, E *y, const E *x)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const E *A = (const E *)F->A;
    E *t = (E *)F->work;
    for (int k0 = 0; k0 < n; k0 += MIK_CH_W)
        hipLaunchKernelGGL((k_dense_fwd<E, false>), dim3(dense_grid(n - k0, MIK_DS_R)), dim3(MIK_DS_R), 0, st, n, k0, A, F->ld, k0 ? (const E *)t : x, t);
    for (int k0 = (n - 1) / MIK_CH_W * MIK_CH_W; k0 >= 0; k0 -= MIK_CH_W)
        hipLaunchKernelGGL((k_chol_bwd<E>), dim3((unsigned)(k0 / MIK_DS_R + 1)), dim3(MIK_DS_R), 0, st, n, k0, std::min(k0 + MIK_CH_W, n), A, F->ld, t, y);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// one pass of a block solve: the `cols` columns from x to y through the groups of the block workspace t, NB columns per lane
template <int NB, typename E>
int chol_solve_block_dev(mik_dense_chol *F, E *t, E *y, int64_t ldy, const E *x, int64_t ldx, int cols)
{
    mik_ctx *ctx = F->ctx;
    hipStream_t st = ctx->stream;
    const int n = F->n;
    const E *A = (const E *)F->A;
    const unsigned groups = dense_grid(cols, NB);
    for (int k0 = 0; k0 < n; k0 += MIK_CH_W)
        hipLaunchKernelGGL((k_dense_fwd_nb<E, false, NB>), dim3(dense_grid(n - k0, MIK_DS_R), groups), dim3(MIK_DS_R), 0, st, n, k0, A, F->ld, k0 ? (const E *)nullptr : x, ldx, cols, t);
    for (int k0 = (n - 1) / MIK_CH_W * MIK_CH_W; k0 >= 0; k0 -= MIK_CH_W)
        hipLaunchKernelGGL((k_chol_bwd_nb<E, NB>), dim3((unsigned)(k0 / MIK_DS_R + 1), groups), dim3(MIK_DS_R), 0, st, n, k0, std::min(k0 + MIK_CH_W, n), A, F->ld, t, y, ldy, cols);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

int64_t chol_launches_solve(const mik_dense_chol *F) { return 2 * (((int64_t)F->n + MIK_CH_W - 1) / MIK_CH_W); }

int chol_refuse_failed(const mik_dense_chol *F, const char *entry)
{
    if (F->info) return mik_fail(F->ctx, MIK_ERR_INVALID, "%s: the factorisation failed at column %lld (PosDefException)", entry, (long long)F->info);
    return MIK_OK;
}

}  // namespace

extern "C" int mik_dense_chol_create(mik_ctx *ctx, void *A, int64_t n, int64_t ld, int dtype, int check, int64_t *failed_col, mik_dense_chol **out)
{
    if (failed_col) *failed_col = 0;
    if (!ctx || !A || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (dtype != MIK_F64 && dtype != MIK_F32 && dtype != MIK_C64 && dtype != MIK_C32)
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_dense_chol_create: dtype must be MIK_F64, MIK_F32, MIK_C64 or MIK_C32");
    mik_dense_chol *F = nullptr;
    int rc = dense_new(ctx, "mik_dense_chol_create", A, n, ld, dtype, false, &F);
    if (rc == MIK_OK) rc = dense_dispatch<true>(dtype, [&](auto e) { return chol_factor<decltype(e)>(F); });
    if (rc == MIK_OK && F->info && check) {
        if (failed_col) *failed_col = F->info;
        rc = mik_fail(ctx, MIK_ERR_SINGULAR, "mik_dense_chol_create: PosDefException(%lld): the matrix is not positive definite, the pivot of that column is not positive",
                      (long long)F->info);
    }
    if (rc != MIK_OK) { dense_free(F); return rc; }
    if (failed_col) *failed_col = F->info;
    *out = F;
    return MIK_OK;
}

extern "C" int mik_dense_chol_destroy(mik_dense_chol *F)
{
    dense_free(F);
    return MIK_OK;
}

extern "C" int mik_dense_chol_solve(mik_dense_chol *F, void *y, const void *x)
{
    if (!F || !y || !x) return MIK_ERR_INVALID;
    MIK_TRY(chol_refuse_failed(F, "mik_dense_chol_solve"));
    MIK_TRY(dense_check_solve(F, "mik_dense_chol_solve", y, x));
    return dense_dispatch<true>(F->dtype, [&](auto e) { return chol_solve_dev(F, (decltype(e) *)y, (const decltype(e) *)x); });
}

extern "C" int mik_dense_chol_solve_block(mik_dense_chol *F, void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs)
{
    if (!F || !Y || !X) return MIK_ERR_INVALID;
    MIK_TRY(chol_refuse_failed(F, "mik_dense_chol_solve_block"));
    MIK_TRY(dense_check_block(F, "mik_dense_chol_solve_block", Y, ldy, X, ldx, nrhs));
    return dense_block_passes<true>(F, Y, ldy, X, ldx, nrhs, [&](auto *t, auto *y, auto *x, int cols) {
        return chol_solve_block_dev<de_block<std::remove_pointer_t<decltype(t)>>::NB>(F, t, y, ldy, x, ldx, cols);
    });
}

extern "C" int mik_dev_dense_chol_block_plan(const mik_dense_chol *F, int64_t nrhs, int64_t *nb, int64_t *g, int64_t *passes, int64_t *launches, int64_t *workspace_bytes)
{
    if (!F) return MIK_ERR_INVALID;
    return dense_block_query(F, nrhs, chol_launches_solve(F), nb, g, passes, launches, workspace_bytes);
}

extern "C" int mik_dense_chol_ldiv_fn(void *user, void *y, const void *x) { return mik_dense_chol_solve((mik_dense_chol *)user, y, x); }

extern "C" int mik_dense_chol_info(const mik_dense_chol *F, int64_t *panel_w, int64_t *rows_per_group, int64_t *tile_rows, int64_t *tile_cols,
                                   int64_t *launches_factor, int64_t *launches_solve, int64_t *bytes, int64_t *info)
{
    if (!F) return MIK_ERR_INVALID;
    if (panel_w) *panel_w = MIK_CH_W;
    if (rows_per_group) *rows_per_group = MIK_CH_R;
    if (tile_rows) *tile_rows = MIK_CH_T;
    if (tile_cols) *tile_cols = MIK_CH_T;
    if (launches_factor) *launches_factor = F->launches_factor;
    if (launches_solve) *launches_solve = chol_launches_solve(F);
    if (bytes) *bytes = F->bytes;
    if (info) *info = F->info;
    return MIK_OK;
}
