/*
 * mik_dev.h -- DEVELOPMENT interface of libmik.so.  Not part of the drop-in boundary (include/mik.h): nothing a host of the
 * reference needs is declared here.  The knobs pin kernel variants and fall-back paths for the tests that check every one of them
 * against the oracle (tests/test_gpu_layouts.py, test_gpu_lookahead.py, test_gpu_irregular.py, test_dist.py, ...); results never
 * depend on them.  Every mik_ctx carries its OWN table (a copy of the defaults when it is created); launches and object creation
 * read only the table of their context.  mik_ctx_set_tuning changes one context; mik_set_tuning is the process-wide convenience
 * of the test suite: it writes the defaults and every live context, and must not race with calls on those contexts.  A host that
 * wants an operator on its plain CSR arrays uses mik_csr_set_layout (include/mik.h), not a knob.
 *
 * Round 5: 12 knobs, every one referenced by a test (round 6: + MIK_KNOB_MACHINE, the machine-shape override of VERDICT r5 #4).  Knobs whose two settings had been measured and decided are
 * gone with the losing variant (operator-stream cache policy, narrow CSR loads, workgroup-map override, long-row threshold, the
 * hint masks of the vector sweeps and of the Krylov basis, slices per workgroup, hipGraph replay of a GMRES column, DGKS rounds in
 * the single-launch kernel, sweep direction, hipStreamSynchronize vs event spin as a knob of its own); what remains selects between
 * code paths that all ship because each is the fall-back of another.
 */
#include "mik.h"
#ifndef MIK_DEV_H
#define MIK_DEV_H
#ifdef __cplusplus
extern "C" {
#endif
enum {
    /* which operator layouts mik_csr_create builds / mik_spmv uses (bits).  1: the CSR arrays only.  2: no slice-constant values (the per-slice-
     * offset form keeps one value per row and slot: layout 4).  4: no per-slice-offset and no wide slice-constant layout.  8: no jagged slices.
     * 16: jagged slices whenever the operator has no structured layout.  32: no x windows / row permutation for the product-tile kernel (read at
     * mik_csr_create).  64: windows built but not used at launch. */
    MIK_KNOB_LAYOUTS = 0,
    MIK_KNOB_CSR_KERNEL = 1,     /* CSR kernel: 0 = by operator, 1 = register-staged product tile (k_spmv_rowblock), 2 = LDS-DMA tile + per-row gather (k_spmv_rowgather) */
    MIK_KNOB_SDIA_KERNEL = 2,    /* slice-constant layouts: 0 = by operator, 1 = flat loads (k_spmv_sdiac: the path of non-finite coefficients / 64-bit offsets),
                                  * 2 = k_spmv_sdiab slot by slot (operators outside the compiled-in slot classes), 3 = one row per lane (odd n; layout 6: k_spmv_sdiaw) */
    MIK_KNOB_LONG_SEGMENT = 3,   /* long-row segment length (> 0; read at mik_csr_create): lets a small test matrix exercise cut rows */
    MIK_KNOB_UPLOAD = 4,         /* 1 = mik_csr_create on the host path only (rows beyond 256 entries, duplicates), 2 = device transpose but the host builders of layouts 6 / 1 */
    MIK_KNOB_GS = 5,             /* Gram-Schmidt of GMRES: 0 = by size, 1 = unfused multi-launch chain (what n > 2048 segments and row partitions run), 2 = launch-lean chain
                                  * (every pass finalises the previous reduction itself), 3 = single launch, but DGKS hands back to the host loop after ONE round (read at
                                  * mik_gmres_create; default 3 rounds), 4 = single launch on all XCDs (not the XCD-local form), 5 = XCD-local form also beyond 512 KB columns,
                                  * 6 = no resident-w form beyond 8 segments per compute unit (read at mik_gmres_create): the multi-launch chain there, as until round 5 */
    MIK_KNOB_TRANSPORT = 6,      /* row-partitioned CG (bits): 1 = the side stream ordered by events instead of mailbox flags (the path without a mailbox), 2 = the two scalars of a
                                  * step over RCCL although a mailbox is connected, 4 = ... through the mailbox even in a world of one, 8 = ... through the one-wave gather launches
                                  * (k_mail_gather) instead of inside the finalising kernels */
    MIK_KNOB_NO_LOOKAHEAD = 7,   /* 1 = nothing enqueued ahead of the host (GMRES: the next Arnoldi column; CG: the head of the next step) -- what callback operators run */
    MIK_KNOB_SOLVER_FORM = 8,    /* mik_bicgstab_step / mik_minres_step: 1 = separate finaliser launches at every size (the form beyond 1,024 reduction segments), 2 = no SpMV
                                  * epilogues (operators whose kernel takes none: sigma / rho / the Lanczos projection as sweeps of their own, vector tree shape) */
    MIK_KNOB_GS_TIMEOUT = 9,     /* 1 = treat the next single-launch Gram-Schmidt column as timed out (exercises the fall-back to the chains) */
    MIK_KNOB_CG_STEP = 10,       /* CG step (bits; read at create / set_halo_plan): 1 = x updated in the step's own sweep (the classic step of callback operators), 2 = PCG with a
                                  * diagonal Pl as three vector sweeps, 4 = the halo of a row-partitioned step after the whole sweep over u (send rows that are not two runs),
                                  * 8 = row-partitioned step with the separate alpha launch (k_cgd_alpha: the classic step's form) */
    MIK_KNOB_HOST_WAIT = 11,     /* host-visible scalars (bits): 1 = hipMemcpyAsync + wait instead of the publish kernel + mailbox spin (more scalars than the mailbox holds),
                                  * 2 = hipStreamSynchronize instead of the event spin (a context without its event) */
    MIK_KNOB_MACHINE = 12,       /* the machine shape the selection paths plan for instead of the queried one (mik_ctx_info): compute units | XCDs << 16; 0 = as queried.
                                  * Read at mik_csr_create (workgroup map), mik_gmres_create (single-launch Gram-Schmidt) and at launch.  32 | 1 << 16 = a CPX partition */
    MIK_KNOB_COUNT = 13
};
int mik_set_tuning(int key, int value);
int mik_ctx_set_tuning(mik_ctx *ctx, int key, int value);
/* Which form orthogonalize_and_normalize! (src/orthogonalize.jl:13-79) of this handle runs in: *single_launch = 1 the whole column as one
 * kernel (0: the multi-launch chains), *segments_per_workgroup = its G (0: buffers never allocated -- too many segments for this machine),
 * *xcd_local_last = the column last enqueued used the XCD-local form, *timeouts = columns that came back timed out so far.  Any pointer may be NULL. */
int mik_dev_gmres_form(const mik_gmres *it, int *single_launch, int *segments_per_workgroup, int *xcd_local_last, int *timeouts);
/* The launch plan mik_dense_mul(D, adjoint, x, y) takes for these pointers on this context (csrc/mik_dense_mul.hip computes it for the launch and
 * for this query through one helper): *vec = 1 the 16-byte-load variant (0: scalar loads -- a matrix, leading dimension, x of the adjoint or
 * directly written y that is not 16-byte aligned), *streamed = 1 non-temporal loads (a matrix beyond what the caches keep), the grid of the product
 * kernel, *chunks_or_batches = column chunks of y = A x / 32-column batches of y = A' x that grid y strides over, *segments = reduction segments
 * of y = A' x that grid x strides over (0 for y = A x).  Variant, grid and chunks / batches are zero for a call that launches no product kernel
 * (an empty dimension).  Nothing is launched or read on the device.  Any out pointer may be NULL. */
int mik_dev_dense_plan(const mik_dense *D, int adjoint, const void *x, const void *y, int *vec, int *streamed, int64_t *grid_x, int64_t *grid_y,
                       int64_t *chunks_or_batches, int64_t *segments);
/* The launch plan mik_dense_mm(D, b, X, ldx, Y, ldy) takes (computed by the helper the launch runs): *groups = launches of the block kernel,
 * *last_width = columns of the last of them, *vector_cols = trailing columns that run one by one through the kernels of mik_dense_mul (a last group
 * narrower than the threshold); *vec / *streamed / grid / *chunks describe the block kernel -- 16-byte loads need an aligned matrix and leading
 * dimension and, when n <= C (the product kernel stores into Y itself), Y and ldy aligned too; X never matters -- or, with *groups = 0, the vector
 * call of column 0.  *workspace_bytes = the block workspace the handle holds now (0 before mik_dense_block_reserve, or when n <= C).  All zero
 * for an empty dimension or b <= 0.  Nothing is launched or read on the device.  Any out pointer may be NULL. */
int mik_dev_dense_block_plan(const mik_dense *D, int b, const void *X, int64_t ldx, const void *Y, int64_t ldy, int *vec, int *streamed,
                             int64_t *grid_x, int64_t *grid_y, int64_t *chunks, int *groups, int *last_width, int *vector_cols, int64_t *workspace_bytes);
/* The narrowest last group this handle gives to the block kernel: 1 .. group width; 0 = the library's threshold.  For measurements and for
 * tests that want the block kernel at every width; results never depend on it. */
int mik_dev_dense_block_min_width(mik_dense *D, int width);
/* The plan mik_dense_lu_solve_block / mik_dense_chol_solve_block take for nrhs columns on this handle (the helper the entries run):
 * *nb = columns a lane of the substitution kernels carries (by element type), *g = columns per pass, *passes = ceil(nrhs / g) (0 for
 * nrhs < 1), *launches = passes x the launches of one vector solve, *workspace_bytes = the block workspace (n x g elements), whether or
 * not a block solve has allocated it yet.  Nothing is launched or read on the device.  Any out pointer may be NULL. */
int mik_dev_dense_lu_block_plan(const mik_dense_lu *F, int64_t nrhs, int64_t *nb, int64_t *g, int64_t *passes, int64_t *launches, int64_t *workspace_bytes);
int mik_dev_dense_chol_block_plan(const mik_dense_chol *F, int64_t nrhs, int64_t *nb, int64_t *g, int64_t *passes, int64_t *launches, int64_t *workspace_bytes);
/* Shape of the resident-w Modified Gram-Schmidt kernel (csrc/mik_mgs_res.h): threads per workgroup (threads / 256 segments per round), rounds of a
 * workgroup's segments kept in registers and in LDS; the rest of w is streamed in every pass.  For byte accounting (bench.py). */
int mik_dev_mgs_resident_shape(int *threads, int *register_rounds, int *lds_rounds);
/* The launch plan of y = A x for these arguments on the operator's context as it is now (csrc/mik_core.hip: the plan the launcher itself computes and
 * executes; mik_spmv_kernel is this query for a whole launch with an aligned x and no fused dot).  skip_begin < 0: the request is row-blocks
 * [rb_begin, rb_begin + rb_count) (rb_count < 0: all), as the solvers and the interior sweep of the row-partitioned CG ask for; else it is every
 * row-block OUTSIDE [skip_begin, skip_end), the boundary sweep of that CG (rb_begin / rb_count are not read), which is one launch where the kernel leaves
 * a range out itself and two ranges elsewhere.  x only matters through its 16-byte alignment; fuse_dot: the dot(x, y) segment sums are asked for.
 * kernel_name (len bytes): the name mik_spmv_kernel uses, *grid = its workgroups, *pre_longrows = 1 when k_spmv_longrows goes first, *post_rowdot = 1
 * when k_rowdot follows -- all of the first launching range of the request -- and *launches = kernel launches of the whole request (0: nothing to do).
 * Returns the launcher's refusal (code, and the same text as the context's error) where the launcher would refuse.  Nothing is launched or read on the
 * device.  Any out pointer may be NULL. */
int mik_dev_spmv_plan(const mik_csr *A, const void *x, int fuse_dot, int rb_begin, int rb_count, int skip_begin, int skip_end, char *kernel_name, int len,
                      int64_t *grid, int *launches, int *pre_longrows, int *post_rowdot);
/* Runs the request mik_dev_spmv_plan describes (same rb_begin / rb_count / skip_begin / skip_end) on the context's stream: the rows of y of the
 * request's row-blocks are written, nothing else of y.  fuse_dot: seg_out (device, one element of the operator's dtype per 256-row block of A) takes
 * the dot(x, y) segment sum of every row-block of the request; else seg_out is not read.  For tests of the row-range launches, which otherwise only
 * the row-partitioned CG issues. */
int mik_dev_spmv_run(mik_ctx *ctx, const mik_csr *A, const void *x, void *y, int fuse_dot, void *seg_out, int rb_begin, int rb_count, int skip_begin,
                     int skip_end);
/* The exclusive scan of the device-side upload (csrc/mik_upload.hip: row pointer, slot pointer and slice pointer all come from it) on its own.
 * data (device, n + 1 ints): data[0..n) -> exclusive prefix sums in place, data[n] = total.  Allocates its own scratch, by the rule the
 * upload sizes its own with; returns when the result is in place.  For tests. */
int mik_dev_exclusive_scan(mik_ctx *ctx, int *data, int64_t n);
/* Host-only: the rule that places a 256-row block's window of x in LDS (k_spmv_rowblock XWIN) on caller-supplied per-block statistics
 * (first / last referenced column, entry count).  win_lo[b] = first column of block b's window (16-byte aligned) or -1 (the block gathers from
 * memory); *span = common window length in elements, 0 = no window table.  Guarantee the tests check: win_lo[b] >= 0 implies
 * win_lo[b] <= first_col[b], last_col[b] < win_lo[b] + span <= n_cols. */
int mik_dev_xwin_plan(int64_t n_blocks, const int *first_col, const int *last_col, const int *entries, int elem_size, int64_t n_cols,
                      int64_t total_entries, int *win_lo, int *span);
#ifdef __cplusplus
}
#endif
#endif /* MIK_DEV_H */
