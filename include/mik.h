/*
 * mik.h -- C ABI of libmik.so: the MI355X (gfx950) Krylov inner loop behind IterativeSolvers.jl's
 *          cg! / gmres! iteration path.
 *
 * This is the drop-in boundary.  IterativeSolvers.jl (v0.9.4, pure Julia) has no FFI of its own;
 * its "plugin mechanism" is multiple dispatch on the operator/vector types
 * (docs/src/getting_started.md:25-30).  A Julia host binds these entry points with `ccall` behind
 * `mul!`, `dot`, `norm`, broadcast and `iterate` methods for a device vector / CSR operator type
 * (INTEGRATION.md shows the binding); the Python harness in this repo binds the same symbols with
 * ctypes.  Each entry point cites the reference call it replaces (file:line relative to the
 * reference checkout).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Every function returns an int status
 *    (MIK_OK = 0); no C++ exception crosses the boundary; mik_last_error() gives the text.
 *  - `dtype` is MIK_F64 or MIK_F32 (the arithmetic type of the whole path; indices are Int32 on
 *    the device).  Scalars cross the boundary as `const void*` / `void*` to a host value of that
 *    dtype, or as double where stated.
 *  - Vector arguments are raw DEVICE pointers (from mik_malloc, or from any HIP allocator of the
 *    same device -- e.g. a torch tensor's data_ptr or an AMDGPU.jl ROCArray).  16-byte aligned
 *    pointers take the vectorised kernels, others a scalar-load variant with identical results.
 *  - Host pointers are borrowed for the duration of the call.  Calls that return a scalar to the
 *    host synchronise the context's stream; everything else is asynchronous on that stream.
 *  - One mik_ctx = one device + one HIP stream; calls on a ctx are not re-entrant (the reference
 *    is single-threaded).  Multi-GPU = one process (and one ctx) per GPU.
 *
 * Reduction semantics (what makes results reproducible and checkable bit-for-bit)
 *  Every dot / norm on the device is a fixed-shape two-level tree that depends only on (n, dtype):
 *   level 1: the vector is cut into segments of 256*W*L elements (mik_reduce_shape()); virtual
 *            thread t of a segment sums its elements e -> (e/W)*(256*W) + W*t + e%W in ascending
 *            e, then a wave-64 shuffle-down tree (offsets 32..1), then the 4 wave sums left to
 *            right;  the dot fused into the SpMV (CG's dot(u, c)) uses W = 1 (one row per
 *            thread) and L = mik_spmv_dot_shape() consecutive 256-row blocks per segment;
 *   level 2: 1024 virtual threads; thread t sums segment sums t, t+1024, ... ascending, wave tree
 *            per 64, then the 16 wave sums left to right.
 *  Multiply and add are never contracted into an FMA (the library is built -ffp-contract=off) and
 *  the SpMV sums each row serially in ascending column order, exactly like the reference's CSC
 *  column scatter (rows longer than mik_spmv_long_row() entries: one wave per row segment, lane l sums the
 *  products of the groups l, l+64, ... of 4 consecutive entries in order, then the wave tree: mik_spmv_long_row below).  oracle/mik_oracle.c (mode ORC_TREE) restates the same tree on the CPU.
 *
 * Norms (the reference's norm() is BLAS nrm2 / generic_norm2: over- and underflow-safe)
 *  norm(x) = sqrt(t), t = tree sum of x_i^2, whenever t lies in [2^-900, 2^900] (fp32: [2^-70, 2^100]) -- then no
 *  square that matters has underflowed and nothing has overflowed.  Outside that range (t = 0, denormal, Inf or NaN
 *  although x may be finite and non-zero: a badly scaled system) the norm is recomputed with scaling: amax = max |x_i|
 *  (0, Inf, NaN are returned as they are); s = 2^-e with amax = f * 2^e, f in [0.5, 1), e clamped to +-1022 (+-126);
 *  t' = the same tree over (x_i * s)^2; norm = sqrt(t') / s.  mik_nrm2, the fused sweeps and the single-GPU iterables
 *  (CG residual, GMRES beta and the Gram-Schmidt norms) all do this, so a solve on a system scaled by 1e-200 takes
 *  the iterations of the unscaled one instead of "converging" on a residual that underflowed to 0.  The row-partitioned
 *  iterables do the same ACROSS the ranks: every rank sees the same out-of-range total, the ranks exchange their local max |x_i|
 *  (mik_cgd_init / mik_cgd_iterate_many / the group calls: one more scalar gather; mik_gmres_create_partitioned: through the
 *  reduce() callback, every rank contributing its value in its own slot of a zero vector), scale by the common power of two,
 *  add the local tree sums in rank order and divide -- so switching to N GPUs does not change what converges.  Only the legacy
 *  host-driven phases (mik_cgd_phase + mik_cgd_wait) still report MIK_ERR_RANGE.  The oracle mirrors it.
 */
#ifndef MIK_H
#define MIK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIK_ABI_VERSION 6   /* 6 (round 6): mik_ctx_info / mik_device_info (the machine is queried, not assumed); mik_plink_exchange;
                             *   mik_comm_allgather_sum also over a mailbox-only communicator.  Added later, without a version bump (additive):
                             *   the stationary methods (mik_stationary_*, mik_diag_ldiv, mik_offdiag_mul, mik_gs_multiply, mik_forward_sub,
                             *   mik_backward_sub).
                             *   5 (round 5): mik_partition gained `link`; the pushed halo lands in library-owned buffers (mik_plink_*, mik_cgd_ghost_export;
                             *   mik_cgd_connect_ghosts takes ghost counts instead of byte offsets; mik_mem_export is gone); mik_cgd_profile.
                             *   4 (round 4): MIK_ERR_SINGULAR replaces MIK_ERR_INVALID for an exactly singular pivot (mik_lu_solve, mik_bicgstab_step);
                             *   the scalar mailbox transport (mik_mailbox_*).  3 (round 3): mik_csr_pack and the knob setters left this header
                             *   (include/mik_dev.h) */

/* status codes */
enum {
    MIK_OK = 0,
    MIK_ERR_INVALID = 1,     /* invalid argument */
    MIK_ERR_HIP = 2,         /* HIP runtime error (text in mik_last_error) */
    MIK_ERR_MISMATCH = 3,    /* dimension / dtype mismatch */
    MIK_ERR_NOMEM = 4,       /* out of (device or host) memory */
    MIK_ERR_NOTIMPL = 5,     /* not implemented (e.g. nnz >= 2^31) */
    MIK_ERR_CALLBACK = 6,    /* a mik_partition / operator / preconditioner callback returned non-zero */
    MIK_ERR_RANGE = 7,       /* a norm left the safe range while the HOST drives the phases of a row-partitioned step itself (see "Norms") */
    MIK_ERR_SINGULAR = 8     /* lu! met an exactly singular pivot (the reference throws SingularException, src/bicgstabl.jl:124): mik_lu_solve,
                              * mik_bicgstab_step -- a code of its own, so that an invalid handle is never reported as a singular matrix;
                              * mik_stationary_create: a zero or missing diagonal entry (src/stationary_sparse.jl:19) */
};

enum { MIK_F64 = 0, MIK_F32 = 1,
       /* ComplexF64 / ComplexF32, stored interleaved (re, im) like Julia and numpy -- the element types test/cg.jl:27,99 and
        * test/gmres.jl:16,38,76 run next to the real ones.  Accepted by the entries marked "complex:" below and by no other: everywhere
        * else a complex code is answered like any unknown code.  Arithmetic (Base's definitions, nothing contracted):
        *   z * w = (zr wr - zi wi) + (zr wi + zi wr) i;   a * z = (a zr) + (a zi) i for a real a;
        *   dot(x, y) = sum conj(x_i) y_i: per element re = xr yr + xi yi and im = xr yi - xi yr (every product rounded, the two terms
        *   added), then the two-level tree of "Reduction semantics", one for re and one for im, with W = 16 B / sizeof(element);
        *   norm(x) = mik_nrm2 over the 2 n interleaved reals (same bits, the same safe second pass).
        * No complex division runs on the device. */
       MIK_C64 = 2, MIK_C32 = 3 };
/* Or-ed into the `dtype` of mik_axpy / mik_xpby / mik_scal with a complex code: the scalar is a HOST REAL of the component type and the
 * product is real * complex -- what Julia's broadcast does with the real beta of src/cg.jl:51 and with inv(nrm) of
 * src/orthogonalize.jl:76, src/gmres.jl:253.  (The sweep is then the real one over the 2 n interleaved reals.) */
#define MIK_SCALAR_REAL 0x100

/* orthogonalisation methods -- src/orthogonalize.jl:4-7 */
enum { MIK_MGS = 0, MIK_CGS = 1, MIK_DGKS = 2 };

typedef struct mik_ctx mik_ctx;       /* device + stream + reduction workspace */
typedef struct mik_csr mik_csr;       /* device CSR operator (the `A` of mul!(y, A, x)) */
typedef struct mik_cg mik_cg;         /* CGIterable            -- src/cg.jl:5-16 */
typedef struct mik_gmres mik_gmres;   /* GMRESIterable + ArnoldiDecomp + Residual -- src/gmres.jl:5-49 */

/* ---- library / context ------------------------------------------------------------------ */
int mik_abi_version(void);
int mik_device_count(int *count);
int mik_ctx_create(int device, mik_ctx **out);
int mik_ctx_destroy(mik_ctx *ctx);
/* The machine behind a context, as hipDeviceGetAttribute reported it in mik_ctx_create, and what the library's selection paths derive
 * from it: nothing assumes "256 compute units in 8 XCDs".  The workgroup -> XCD maps of the banded SpMV kernels and the XCD-local
 * Gram-Schmidt are written for the 8-XCD round-robin dispatch of an unpartitioned MI355X; on any other shape (xcd_maps = 0) the
 * identity map and the device-wide forms run -- same bits (src/orthogonalize.jl:67-79 has one result whatever the form). */
typedef struct mik_device_info {
    int device;                          /* HIP ordinal */
    int compute_units;                   /* hipDeviceAttributeMultiprocessorCount */
    int xcds;                            /* hipDeviceAttributeNumberOfXccs (1 if the runtime does not know the attribute) */
    int wavefront_size;                  /* 64 (mik_ctx_create refuses anything else) */
    int64_t lds_bytes_per_cu, l2_bytes, hbm_bytes;
    char arch[64];                       /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    /* derived (what launch and selection code reads): */
    int planned_compute_units, planned_xcds;   /* = the two above unless a development override is set (include/mik_dev.h MIK_KNOB_MACHINE) */
    int xcd_maps;                        /* 1: XCD-aware workgroup maps in use (planned_xcds == 8) */
    int resident_workgroup_cap;          /* workgroups of a launch whose workgroups wait for each other: one per compute unit */
    int gs_single_launch_max_segments;   /* orthogonalize_and_normalize! as ONE launch up to this many reduction segments (8 per workgroup) */
    int gs_xcd_local_max_workgroups;     /* ... in its XCD-local form up to this many workgroups (0: form not available on this shape) */
    int sweep_grid_cap;                  /* grid cap of the grid-stride vector sweeps */
    int mgs_resident_max_segments;       /* ... and ModifiedGramSchmidt beyond that, with w resident in registers / LDS, up to this many (86 per workgroup: while at
                                          * least 0.6 of w fits on the chip; 0: the device reports less than 160 KB of LDS per compute unit) */
    int reserved[7];
} mik_device_info;
int mik_ctx_info(const mik_ctx *ctx, mik_device_info *out);
/* Adopt an external hipStream_t (e.g. torch's current stream); NULL restores the ctx's own. */
int mik_ctx_set_stream(mik_ctx *ctx, void *hip_stream);
int mik_ctx_synchronize(mik_ctx *ctx);
const char *mik_last_error(mik_ctx *ctx);   /* ctx may be NULL: last error of a failed create */
/* (W, L) of the level-1 reduction tree for `dtype` (see "Reduction semantics").  complex: W = 16 B / sizeof(element) = 1 (MIK_C64), 2 (MIK_C32). */
int mik_reduce_shape(int dtype, int *W, int *L);
/* (W, L) of the dot(u, c) fused into the SpMV of the CG step: one row per thread (W = 1), L
 * consecutive 256-row blocks per workgroup. */
int mik_spmv_dot_shape(int *W, int *L);
/* Rows with more than *threshold stored entries are summed with the wave shape: the row's entries are taken in GROUPS of *group
 * (= 4) consecutive entries; lane l of a wave adds, from +0 and in ascending order, the products of the groups l, l + 64, ...
 * (entry e belongs to lane (e / 4) % 64 -- the shape of one 64-thread segment of a dot product read with 16-byte loads), then the
 * wave-64 tree; shorter rows strictly in column order like the reference.  None of the reference's fixtures has such rows. */
int mik_spmv_long_row(int *threshold);
int mik_spmv_long_group(int *group);
/* Rows with more than *segment entries (a multiple of the group) are cut into segments of that many consecutive entries; every
 * segment is summed with the wave shape above and the segment sums are added left to right (one wave per row left a
 * 20,000-entry row to a single wave). */
int mik_spmv_long_segment(int *segment);

/* ---- device memory (similar / zero / copyto! / fill! of the vector interface) ----------- */
int mik_malloc(mik_ctx *ctx, size_t bytes, void **dptr);            /* similar(x)             */
int mik_free(mik_ctx *ctx, void *dptr);
int mik_memcpy_h2d(mik_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous  */
int mik_memcpy_d2h(mik_ctx *ctx, void *dst, const void *src, size_t bytes);   /* synchronous  */
int mik_copy(mik_ctx *ctx, int dtype, int64_t n, const void *x, void *y);     /* copyto!(y, x) src/cg.jl:130, src/gmres.jl:241; complex: yes */
int mik_fill(mik_ctx *ctx, int dtype, int64_t n, const void *value, void *x); /* x .= value    src/cg.jl:129; complex: value is a host complex */

/* ---- operator ---------------------------------------------------------------------------- */
/* Upload a SparseMatrixCSC (is_csc = 1: ptr = colptr, idx = rowval -- the layout of
 * test/laplace_matrix.jl:12) or a CSR matrix (is_csc = 0).  Host arrays, Int64 indices with
 * `index_base` (1 for Julia).  The arrays are copied to the device as they are; validation, the conversion to 0-based
 * Int32 CSR (CSC -> CSR transpose, columns ascending within a row = the order Julia's column scatter reaches a row), the
 * operator statistics and the layout analysis run there as kernels (csrc/mik_upload.hip; 0.06 s for the 256^3 Laplacian).
 * Matrices with rows longer than mik_spmv_long_row() or with duplicate (row, column) entries take the host path
 * (single-threaded counting-sort transpose + builders), as does everything when the development knob MIK_KNOB_UPLOAD is set.
 * complex (SparseMatrixCSC{ComplexF64} of test/cg.jl:99-121, test/gmres.jl:38-57): CSC or CSR, any index base, rectangular; always the
 * host path, and the operator always runs on its CSR arrays: mik_csr_layout reports 0, mik_csr_set_layout changes nothing,
 * mik_csr_compact answers MIK_ERR_NOTIMPL, mik_csr_info / mik_csr_stored_bytes work.  Only mik_spmv takes such an operator: the fused
 * iterables and every other entry with a mik_csr argument answer MIK_ERR_NOTIMPL. */
int mik_csr_create(mik_ctx *ctx, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz,
                   const int64_t *ptr, const int64_t *idx, const void *val, int index_base,
                   int is_csc, mik_csr **out);
/* The same for SparseMatrixCSC{T, Int32} (the reference's tests run Ti in (Int64, Int32): test/gmres.jl:38, test/cg.jl:57): ptr / idx
 * are 32-bit.  Host or device arrays. */
int mik_csr_create_i32(mik_ctx *ctx, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *ptr, const int32_t *idx,
                       const void *val, int index_base, int is_csc, mik_csr **out);
int mik_csr_destroy(mik_csr *A);
/* Release the CSR arrays (rowptr / col / val: 12 B per entry at fp64) of an operator whose active layout is one of the sliced
 * forms (1, 2, 4, 5) -- mik_spmv never reads them then; they are only what mik_csr_set_layout(A, 0) and the development knobs
 * (csrc/mik_dev.h) fall back to, which have no effect on this operator afterwards.  MIK_ERR_NOTIMPL (nothing released) for an
 * operator that runs on its CSR arrays or has split-off long rows. */
int mik_csr_compact(mik_csr *A);
/* Device layout mik_spmv uses for this operator (chosen at upload from the sparsity pattern; results are
 * bit-identical across layouts): 0 = CSR row-blocks (LDS tile filled by LDS-DMA; product tile for uneven rows; any matrix),
 * 1 = jagged slices (one row per lane, groups of 16 B / sizeof(T) consecutive entries stored lane-interleaved per 64-row
 * slice: long near-uniform rows -- finite-element matrices, variable-coefficient stencils), (2, 3: retired), 4 = sliced-ELL values with per-slice offsets and one presence-mask byte per row (every
 * 256-row slice uses <= 8 distinct offsets: stencils on structured grids), 5 = the same with slice-CONSTANT slot values
 * (within a slice every row that has a slot carries the same value there -- constant-coefficient stencils): the slice
 * stores its <= 8 values once and a row is one mask byte, 6 = the same idea for up to 32 offsets per slice with one 32-bit mask per
 * row (9-point 2-D, 13 / 19 / 27-point 3-D constant-coefficient stencils). */
int mik_csr_layout(const mik_csr *A, int *layout);
/* Choose the layout mik_spmv and the iterables created AFTERWARDS use for this operator: layout = 0 runs it on its plain CSR
 * arrays (k_spmv_rowgather / k_spmv_rowblock -- what any matrix can run on; bench.py measures the north star's CSR figure this
 * way on the same operator), layout = -1 returns to the automatic choice.  MIK_ERR_NOTIMPL for any other value or after
 * mik_csr_compact released the CSR arrays.  Results are bit-identical either way. */
int mik_csr_set_layout(mik_csr *A, int layout);
/* Name of the kernel mik_spmv launches for this operator now (layout, operator properties, development knobs): for
 * profiles and the bench line.  Layout 5 runs k_spmv_sdiab (x through buffer loads: a slot a row does not have reads 0.0 by
 * the descriptor's range check) when every slice value is finite and the offsets fit 32 bits, else k_spmv_sdiac. */
int mik_spmv_kernel(const mik_csr *A, char *name, int len);
/* Bytes of operator data (values, indices / codes, pointers) one mik_spmv launch streams in that layout. */
int mik_csr_stored_bytes(const mik_csr *A, int64_t *bytes);
/* size(A, d), nnz, eltype(A) */
int mik_csr_info(const mik_csr *A, int64_t *n_rows, int64_t *n_cols, int64_t *nnz, int *dtype);

/* ---- L1 operator / vector interface ------------------------------------------------------ */
/* mul!(y, A, x) -- SparseArrays mul!, called at src/cg.jl:54,137; src/gmres.jl:245,287
 * complex: a row is summed serially in ascending column order, re and im each (rows beyond mik_spmv_long_row() / mik_spmv_long_segment()
 * entries: the wave shape and the left-to-right segments of the real path); mik_spmv_kernel names the kernel (k_spmv_complex). */
int mik_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y);
/* dot(x, y) -- src/cg.jl:55, src/orthogonalize.jl:71.  *out is a host scalar of `dtype`.  complex: sum conj(x_i) y_i, *out one host complex. */
int mik_dot(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *y, void *out);
/* norm(x) -- src/cg.jl:62,140; src/orthogonalize.jl:75; src/gmres.jl:252.  complex: *out is a host REAL of the component type. */
int mik_nrm2(mik_ctx *ctx, int dtype, int64_t n, const void *x, void *out);
/* y .+= alpha .* x  -- src/cg.jl:58 (alpha) / :59 (-alpha).  complex: alpha is a host complex (a host real with dtype | MIK_SCALAR_REAL). */
int mik_axpy(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, const void *x, void *y);
/* y .= x .+ beta .* y -- src/cg.jl:51 (u .= r .+ beta .* u).  complex: beta is a host complex; the REAL beta of src/cg.jl:50-51 is
 * passed as a host real with dtype | MIK_SCALAR_REAL and multiplies as real * complex, like Julia's promotion in beta .* u. */
int mik_xpby(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *beta, void *y);
/* y .-= x -- src/cg.jl:138, src/gmres.jl:246.  complex: yes */
int mik_sub(mik_ctx *ctx, int dtype, int64_t n, const void *x, void *y);
/* x .*= alpha -- src/orthogonalize.jl:76, src/gmres.jl:253.  complex: a host complex, or (both reference lines: inv of a norm) a host
 * real with dtype | MIK_SCALAR_REAL. */
int mik_scal(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, void *x);
/* y .= x ./ d -- ldiv!(y, P::JacobiPrec, x) of test/cg.jl:18 (diagonal left preconditioner) */
int mik_divide(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *d, void *y);

/* ---- L2 Krylov helpers ------------------------------------------------------------------- */
/* orthogonalize_and_normalize!(V[:, 1:k], w, h, method) -> nrm -- src/orthogonalize.jl:13-79.
 * V: device, column-major, leading dimension ldv (elements); w: device n-vector (updated in
 * place, normalised); h: HOST array of k scalars (written); nrm: HOST scalar (written).
 * complex: MIK_MGS only (src/orthogonalize.jl:67-79; MIK_CGS / MIK_DGKS answer MIK_ERR_NOTIMPL): h[i] = dot(V[:, i], w), w -= h[i] V[:, i],
 * nrm = norm(w) (a host REAL), w *= inv(nrm) with inv(nrm) real; one sweep over w per column, h on the device between the sweeps. */
int mik_orthogonalize(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv,
                      void *w, void *h, void *nrm, int method);
/* orthogonalize_and_normalize!(V::Vector{Vector}, w, h, ModifiedGramSchmidt()) -> nrm -- src/orthogonalize.jl:53-65: the basis as
 * k separate device n-vectors (V: HOST array of k device pointers).  Same arithmetic and bits as mik_orthogonalize with MIK_MGS
 * on a matrix holding those columns.  (The reference defines this method for ModifiedGramSchmidt only.) */
int mik_orthogonalize_vectors(mik_ctx *ctx, int dtype, int64_t n, int k, const void *const *V, void *w, void *h, void *nrm);
/* mul!(y, V[:, 1:k], c, alpha, 1) -- src/gmres.jl:275 (alpha = 1), src/orthogonalize.jl:16 (-1).
 * c: HOST array of k scalars.  complex (src/gmres.jl:275): t_j = alpha * c[j], then y = y + t_j * V[:, j], columns ascending. */
int mik_gemv_n(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv,
               const void *c, const void *alpha, void *y);

/* h = V[:, 1:k]' * w -- mul!(h, adjoint(V), w): src/orthogonalize.jl:15,43 and (column by column) the
 * Gram matrix of src/bicgstabl.jl:121.  One sweep reads w once and every column once.  h: HOST.
 * complex: h[j] has the bits of the complex mik_dot(V[:, j], w); h is k host complex scalars. */
int mik_gemv_t(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *w,
               void *h);
/* Host: solve the small dense system A x = b (column-major n x n) by LU with partial pivoting --
 * lu! + ldiv! at src/bicgstabl.jl:124-125.  A is overwritten by its factors, b by x; MIK_ERR_SINGULAR if A is
 * exactly singular.
 * complex: the pivot of a column is the FIRST row with the largest |re| + |im| (LAPACK getrf's izamax, what lu! reaches for a complex
 * matrix); quotients by Smith's scaling; MIK_ERR_SINGULAR on an exactly zero pivot column. */
int mik_lu_solve(int dtype, void *A, int64_t lda, int n, void *b);

/* ---- L3 iterables ------------------------------------------------------------------------ */
/* cg_iterator!(x, A, b, Pl; abstol, reltol, maxiter, statevars, initially_zero)
 *   -- src/cg.jl:120-155.  x, b and the CGStateVariables u, r, c (src/cg.jl:114-118) are device
 * n-vectors owned by the caller.  `jacobi_diag` (device n-vector or NULL) selects the
 * PCGIterable with a diagonal left preconditioner (src/cg.jl:18-30,72-100); NULL = Identity(). */
int mik_cg_create(mik_ctx *ctx, const mik_csr *A, void *x, const void *b, void *u, void *r,
                  void *c, const void *jacobi_diag, double abstol, double reltol,
                  int64_t maxiter, int initially_zero, mik_cg **out);
int mik_cg_destroy(mik_cg *it);
/* iterate(it, iteration) -- src/cg.jl:43-66 / :72-100.  *done = 1 and nothing is computed when
 * done(it, iteration) (src/cg.jl:36); otherwise one step runs and *residual = it.residual.
 * r and the residual are those of the step just returned, and so is x for every reader ordered after the
 * ctx stream (mik_memcpy_d2h, kernels on that stream, or after mik_synchronize): with a CSR operator the
 * update x .+= alpha .* u of a step is carried out by the sweep over u that opens the next step (same
 * operands, same rounding), which is on the stream before this call returns.  The search direction u and c = A u are
 * the iterable's scratch: with a CSR operator and no host callbacks the library enqueues the first half of
 * the NEXT step (u = r + beta u, c = A u, alpha) before it waits for this step's residual, so on return
 * u and c may already belong to step iteration + 1 (results of any call sequence are unchanged; the
 * device-side stopping flag turns that half into a no-op once the iteration has stopped). */
int mik_cg_iterate(mik_cg *it, int64_t iteration, double *residual, int *done);
/* 1 if this iterable applies x .+= alpha .* u in the sweep over u that opens the next step (CSR operator, no
 * preconditioner callback; see mik_cg_iterate), 0 if in the step's own update sweep.  Results are bit-identical either way. */
int mik_cg_fused_x(const mik_cg *it, int *fused);
/* Up to max_steps consecutive iterate() calls with ONE host synchronisation: the stopping test
 * of src/cg.jl:36 is evaluated on the device after every step and later steps become no-ops.
 * residuals[0..*steps_done-1] receive it.residual after each executed step. */
int mik_cg_iterate_many(mik_cg *it, int64_t iteration, int64_t max_steps, double *residuals,
                        int64_t *steps_done);
/* fields of CGIterable read by cg! (src/cg.jl:227,232,238): mv_products, residual, tol,
 * converged(it) */
int mik_cg_state(const mik_cg *it, double *residual, double *prev_residual, double *tol,
                 int64_t *maxiter, int64_t *mv_products, int *converged);

/* gmres_iterable!(x, A, b; Pl, Pr, abstol, reltol, restart, maxiter, initially_zero, orth_meth)
 * -- src/gmres.jl:108-136.  x, b: device n-vectors owned by the caller.  pl_diag / pr_diag: NULL =
 * Identity(), or a device n-vector d making the preconditioner ldiv!(y, P, x) = y .= x ./ d (the three
 * expand! methods src/gmres.jl:285-304, init! :249 and update_solution! :278-283 are followed).  The Krylov basis V (n x (restart+1), src/gmres.jl:13) lives on the device and
 * the Hessenberg matrix, Givens least squares and null-vector residual recurrence
 * (src/gmres.jl:224-233,262-271; src/hessenberg.jl:15-46) on the host, inside the handle. */
int mik_gmres_create(mik_ctx *ctx, const mik_csr *A, void *x, const void *b, const void *pl_diag,
                     const void *pr_diag, double abstol, double reltol, int restart, int64_t maxiter,
                     int initially_zero, int orth_method, mik_gmres **out);
int mik_gmres_destroy(mik_gmres *it);
/* iterate(g, iteration) -- src/gmres.jl:57-106 */
int mik_gmres_iterate(mik_gmres *it, int64_t iteration, double *residual, int *done);
/* Up to max_steps consecutive iterate() calls in one entry (the loop of gmres!, src/gmres.jl:207-214): residuals[j] =
 * residual.current after step j; *steps_done < max_steps iff done(g, iteration + *steps_done). */
int mik_gmres_iterate_many(mik_gmres *it, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done);
/* fields read by gmres! (src/gmres.jl:210,218): mv_products, residual.current, tol, k, beta */
int mik_gmres_state(const mik_gmres *it, double *residual, double *tol, double *beta, int *k,
                    int64_t *mv_products, int *converged);

/* ---- any operator, any preconditioner on the fused iterables -------------------------------------------- */
/* The reference asks of A only mul!(y, A, v) and of Pl / Pr only ldiv!(y, P, x) (docs/src/getting_started.md:25-30,
 * docs/src/preconditioning.md:5-14; exercised with a LinearMap at test/gmres.jl:59-66 and with lu(A) as Pl at
 * test/gmres.jl:28-35, test/cg.jl:71-77).  The callbacks below carry that contract across the C ABI: x and y are DEVICE
 * n-vectors of the handle's dtype; the callback must leave its work ordered on the context's stream (enqueue kernels on
 * it -- mik_ctx_set_stream adopts a host framework's stream -- or finish before returning) and return 0.  A non-zero
 * return surfaces as MIK_ERR_CALLBACK.  With a callback operator the CG step keeps its fused vector sweeps and reduces
 * dot(u, c) with the (W, L) shape of mik_reduce_shape instead of inside the SpMV epilogue. */
typedef int (*mik_mul_fn)(void *user, const void *x, void *y);      /* y = A * x      -- mul!(y, A, x)   */
typedef int (*mik_ldiv_fn)(void *user, void *y, const void *x);     /* y = P \ x      -- ldiv!(y, P, x); y may alias x */
typedef struct mik_operator {
    int dtype;                  /* MIK_F64 / MIK_F32 (ignored when csr is given) */
    int64_t n;                  /* size(A, 1) = size(A, 2) (ignored when csr is given) */
    const mik_csr *csr;         /* a device CSR operator: the fully fused path ...                            */
    mik_mul_fn mul;             /* ... or any operator as a callback (csr == NULL)                           */
    void *user;
} mik_operator;
typedef struct mik_precond {    /* all NULL = Identity() (src/common.jl:28-32) */
    const void *diag;           /* device n-vector d: ldiv!(y, P, x) = y .= x ./ d, fused into the sweeps       */
    mik_ldiv_fn ldiv;           /* or any preconditioner as a callback                                        */
    void *user;
} mik_precond;
/* cg_iterator!(x, A, b, Pl; ...) -- src/cg.jl:120-155 with any A / Pl; mik_cg_iterate* and mik_cg_state work as usual. */
int mik_cg_create_op(mik_ctx *ctx, const mik_operator *A, const mik_precond *Pl, void *x, const void *b, void *u, void *r,
                     void *c, double abstol, double reltol, int64_t maxiter, int initially_zero, mik_cg **out);
/* gmres_iterable!(x, A, b; Pl, Pr, ...) -- src/gmres.jl:108-136 with any A / Pl / Pr (all three expand! methods,
 * src/gmres.jl:285-304). */
int mik_gmres_create_op(mik_ctx *ctx, const mik_operator *A, const mik_precond *Pl, const mik_precond *Pr, void *x, const void *b,
                        double abstol, double reltol, int restart, int64_t maxiter, int initially_zero, int orth_method,
                        mik_gmres **out);

/* ---- fused sweeps for the other solvers of the package ------------------------------------------- */
/* Each call is several consecutive reference statements executed as ONE pass over the vectors, with the
 * same per-element operations in the same order (bit-identical to issuing the L1 calls one by one).  `hints` is a
 * bit mask of operands the caller will not touch again soon: they are streamed past the caches (non-temporal
 * loads / stores) so that the operands that ARE re-read stay resident; results never depend on it (0 = none). */
/* y .+= alpha .* x (x NULL: no update); then *out = dot(z, y), or norm(y) when z is NULL
 *   -- src/minres.jl:104+107 and :109+112
 * complex: alpha is a host complex, or, with MIK_SCALAR_REAL or-ed into dtype, a host real that multiplies as real x complex; *out is one
 * host complex (dot(z, y) = sum conj(z_i) y_i, the bits of mik_dot) or, z NULL, a host REAL (norm(y), the bits and the safe second pass
 * of mik_nrm2).  The flag on a fused entry means that EVERY scalar argument of the call is a real of the component type. */
int mik_axpy_dot(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, const void *x, void *y, const void *z, void *out,
                 int hints /* 1: x */);
/* x .+= alpha .* u; r .-= alpha .* c; *out = norm(r)   -- src/chebyshev.jl:51-54 (same shape as src/cg.jl:58-62)
 * complex: alpha is real in src/chebyshev.jl, so MIK_SCALAR_REAL is required (without it: MIK_ERR_INVALID); the sweep and the norm are
 * the real ones over the 2 n interleaved reals. */
int mik_axpy2_nrm2(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, const void *u, void *x, const void *c, void *r, void *out,
                   int hints /* 1: x, 2: c, 4: u */);
/* c = Pl \ r (pl_diag NULL = Identity); u .= c when `first`, else u .= c .+ beta .* c   -- src/chebyshev.jl:35-45
 * complex: beta is real, MIK_SCALAR_REAL is required (without it: MIK_ERR_INVALID); pl_diag != NULL is MIK_ERR_NOTIMPL (no complex
 * division on the device). */
int mik_cheb_direction(mik_ctx *ctx, int dtype, int64_t n, const void *r, const void *pl_diag, const void *beta, int first, void *u);
/* LSQR / LSMR (src/lsqr.jl, src/lsmr.jl), groups of consecutive statements as single sweeps with the same per-element operations:
 *   mik_xpby_nrm2     y .= x .+ beta .* y; *out = norm(y)           u .= -alpha .* u .+ tmpm; beta = norm(u)  (src/lsqr.jl:151-152, :159-160;
 *                                                                   src/lsmr.jl:161-162, :167-168)
 *   mik_lsqr_update   x .+= t1*w; w = t2 .* w .+ v; wrho .= w .* inv_rho (never stored); *out = norm(wrho)              (src/lsqr.jl:189-192)
 *   mik_lsmr_update   hbar .= hbar .* c1 .+ h; x .+= c2 * hbar; h .= h .* c3 .+ v; *out = norm(x)                        (src/lsmr.jl:199-201, :242)
 * Scalars: HOST values of `dtype`. */
int mik_xpby_nrm2(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *beta, void *y, void *out);
int mik_lsqr_update(mik_ctx *ctx, int dtype, int64_t n, const void *t1, const void *t2, const void *inv_rho, void *x, void *w, const void *v, void *out);
int mik_lsmr_update(mik_ctx *ctx, int dtype, int64_t n, const void *c1, const void *c2, const void *c3, void *hbar, void *h, void *x, const void *v, void *out);
/* QMR (src/qmr.jl), groups of consecutive statements as single sweeps with the same per-element operations:
 *   mik_axpy2_dot    y .+= a .* x1; y .+= b .* x2 (x2 may be NULL); *out = dot(z, y) = sum conj(z[i]) y[i] (z may be NULL: no reduction,
 *                    out untouched).  z is the conjugated argument: what both callers need -- QMR passes y = w_next, z = v_next for
 *                    vw = dot(v_next, w_next), IDR(s) y = G[k], z = P[i + 1] for dot(P[i + 1], G[k]); for the real types the order is immaterial
 *                    -- the two axpy! of a Lanczos vector (:70-72 / :76-78) and, for the second vector, vw = dot(v_next, w_next) (:81)
 *   mik_scal2        x .*= a; y .*= b                                                                             (:90-91)
 *   mik_qmr_update   p = v; p .+= neg_h1 .* p_curr; p .+= neg_h0 .* p_prev (either vector may be NULL), p .*= inv, x .+= g .* p; p is stored at
 *                    p_out, the next p_curr (p_out may be p_prev's storage: the caller rotates names instead of the two copies of :196-197;
 *                    p_out == v or p_out == p_curr is MIK_ERR_INVALID)                                             (:188-197)
 * Scalars: HOST values of `dtype` (neg_h1 = -H[2], neg_h0 = -H[1]).
 * complex (MIK_C64 / MIK_C32): every scalar is a host complex (re, im) of `dtype`; each axpy is the rounded complex product (zr wr - zi wi,
 * zr wi + zi wr) followed by one rounded add per component, each scaling the product x * a, in the statement order above, nothing
 * contracted; *out is one host complex with the bits of the complex mik_dot(z, y) (one tree for re, one for im).  With MIK_SCALAR_REAL
 * or-ed into dtype EVERY scalar of the call is a host real of the component type that multiplies as real x complex: mik_scal2,
 * mik_qmr_update and mik_axpy2_dot with z NULL are then the real sweeps over the 2 n interleaved reals (the same bits by construction);
 * mik_axpy2_dot with z keeps the complex dot.  The 16-byte variant runs when every vector is 16-byte aligned, the element-wise one
 * otherwise; both give the same bits.  The NULL and aliasing rules are those of the real codes. */
int mik_axpy2_dot(mik_ctx *ctx, int dtype, int64_t n, const void *a, const void *x1, const void *b, const void *x2, void *y, const void *z, void *out);
int mik_scal2(mik_ctx *ctx, int dtype, int64_t n, const void *a, void *x, const void *b, void *y);
int mik_qmr_update(mik_ctx *ctx, int dtype, int64_t n, const void *v, const void *neg_h1, const void *p_curr, const void *neg_h0, const void *p_prev,
                   const void *inv, const void *g, void *x, void *p_out);
/* v_next .*= inv_h3; w_next .= v_curr .+ neg_h1 .* w_curr .+ neg_h0 .* w_prev (each term skipped when its vector
 * is NULL); w_next .*= inv_h2; x .+= rhs0 .* w_next   -- src/minres.jl:113, :136-142
 * complex: with MIK_SCALAR_REAL the five scalars are host reals (Hermitian: H and rhs are real(T)) and the sweep is the real one over
 * 2 n; without it the five are host complex (skew-Hermitian) and every product is the complex one, in the statement order above. */
int mik_minres_update(mik_ctx *ctx, int dtype, int64_t n, const void *inv_h3, void *v_next, const void *v_curr, const void *neg_h1,
                      const void *w_curr, const void *neg_h0, const void *w_prev, const void *inv_h2, void *w_next,
                      const void *rhs0, void *x, int hints /* 1: x, 2: w_prev */);

/* M = V' * V for k <= 5 columns in ONE pass over V (all pairwise dots; M is k x k, column-major, host) -- the
 * Gram matrix of src/bicgstabl.jl:120; entry (r, c) equals mik_dot(V[:, r], V[:, c]) bit for bit.
 * complex: for r <= c, M[r, c] has the bits of the complex mik_dot(V[:, r], V[:, c]); the lower triangle is the conjugate of the upper
 * (equal real parts, negated imaginary parts: mik_dot as numbers, the sign of a zero aside); the diagonal's imaginary part is +0. */
int mik_gram(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *M);
/* BiCGStab(l) minimal-residual update, src/bicgstabl.jl:127-132, as one sweep: us[:, 1] -= us[:, 2:l+1] * gamma;
 * x += rs[:, 1:l] * gamma; rs[:, 1] -= rs[:, 2:l+1] * gamma; *out = norm(rs[:, 1]).  l <= 8; gamma: l host scalars.
 * complex: gamma is l host complex scalars, *out a host real; the per-element operations are those of three complex mik_gemv_n calls
 * with alpha = -/+(1 + 0 i) (t_j = alpha * gamma_j on the host, columns ascending); l <= 8 as for the real types. */
int mik_bicgstab_mr_update(mik_ctx *ctx, int dtype, int64_t n, int l, void *us, int64_t ldu, void *rs, int64_t ldr, void *x,
                           const void *gamma, void *out);

/* One whole outer iteration of BiCGStab(l) -- iterate(::BiCGStabIterable), src/bicgstabl.jl:79-134 -- per call, with rho, beta,
 * sigma, alpha, the Gram matrix, gamma and omega kept on the device: the host waits once, for the residual norm it returns
 * (the statement-by-statement form through mik_dot / mik_xpby / mik_spmv / mik_axpy / mik_gram / mik_lu_solve /
 * mik_bicgstab_mr_update waits 2 l + 3 times; the same bits wherever mik_bicgstab_dot_shape reports the vector shape).  The caller owns x, the residual block rs and the
 * search block us (n x (l + 1), column-major, leading dimensions ldr / ldu) as set up by bicgstabl_iterator!
 * (src/bicgstabl.jl:25-73: rs[:, 1] = Pl \ (b - A x), us = 0) and the shadow residual r_shadow (:38); pl_diag: the diagonal
 * of a Jacobi Pl (ldiv! = elementwise division, :98, :108) or NULL for Identity.  omega = sigma = 1 at creation (:59).
 * l = 1 ... 4.  Between two steps of a handle the blocks are the handle's state (as the fields of the reference's iterable are): the MR sweep of a
 * step leaves the segment sums of dot(r_shadow, rs[:, 1]) -- rho of the next step's first column (:89) -- with the handle.
 * MIK_ERR_SINGULAR when lu! meets an exactly singular pivot (the reference throws SingularException); the handle is
 * then latched: every later mik_bicgstab_step reports MIK_ERR_SINGULAR again (its device scalars are not steppable).  Handles a host
 * never destroys are freed by mik_ctx_destroy of their context (a finalizer that finds the context closed must skip the destroy call). */
typedef struct mik_bicgstab mik_bicgstab;
int mik_bicgstab_create(mik_ctx *ctx, const mik_csr *A, int l, void *x, void *rs, int64_t ldr, void *us, int64_t ldu,
                        const void *r_shadow, const void *pl_diag, mik_bicgstab **out);
int mik_bicgstab_step(mik_bicgstab *it, void *residual);          /* residual: one scalar of A's element type */
/* (W, L) of the reduction tree of sigma = dot(r_shadow, A u) (src/bicgstabl.jl:100) and of rho = dot(r_shadow, rs[:, j]) for j >= 2 (:89)
 * inside mik_bicgstab_step: where the operator's SpMV kernel takes a dot epilogue and Pl = Identity, both are formed in the SpMV launch
 * that produces the vector, one partial per 256-row block (mik_spmv_dot_shape); else the vector shape (mik_reduce_shape), which rho of
 * the first column and the Gram matrix always have.  The oracle takes it. */
int mik_bicgstab_dot_shape(const mik_bicgstab *it, int *W, int *L);
int mik_bicgstab_destroy(mik_bicgstab *it);

/* One whole iteration of MINRES -- iterate(::MINRESIterable), src/minres.jl:95-159 -- per call: mul!, the Lanczos step with its
 * projection (:104-107), the orthogonalisation with its norm (:109-112), both Givens rotations and the right-hand side (:116-133),
 * and the tail sweep (:113, :136-142), the scalars on the device; the host waits once, for the residual norm |rhs[2]| (:154) it
 * returns (the statement-by-statement form through mik_spmv / mik_axpy_dot / mik_givens / mik_minres_update waits twice inside
 * the iteration; same bits).  The caller owns x and the six work vectors as minres_iterable! sets them up (:38-87:
 * v_curr = (b - A x) / resnorm0, w's = 0); the handle rotates its three v and three w pointers after every step exactly as
 * :145-146 do, and the caller rotates its own names with it.  iteration counts from 1 (:91). */
typedef struct mik_minres mik_minres;
int mik_minres_create(mik_ctx *ctx, const mik_csr *A, void *x, void *v_prev, void *v_curr, void *v_next, void *w_prev, void *w_curr,
                      void *w_next, double resnorm0, int skew_hermitian, mik_minres **out);
int mik_minres_step(mik_minres *it, int64_t iteration, void *resnorm);   /* resnorm: one scalar of A's element type */
/* (W, L) of the reduction tree of proj = dot(v_curr, v_next) (src/minres.jl:107) inside mik_minres_step: where the operator's SpMV
 * kernel takes the Lanczos step as its epilogue (y = A x - H[2] v_prev stored once, the dot formed in the same launch) it is the
 * shape of the dot fused into the CG SpMV (mik_spmv_dot_shape), else the vector shape (mik_reduce_shape).  The oracle takes it. */
int mik_minres_proj_shape(const mik_minres *it, int *W, int *L);
int mik_minres_destroy(mik_minres *it);

/* One step of IDR(s) -- iterate(::IDRSIterable, (iter, step)), src/idrs.jl:164-272 -- per call.  step = 1..s: the small triangular solve (:187,
 * host), V / Q / ldiv!(Pl, V) / U[k] in ONE sweep (:188-202), mul! (:203), the bi-orthogonalisation against P[1..k-1] as a chain of sweeps whose
 * coefficients never leave the device (:207-211), M[k..s, k] as one batched dot (:215-217), and beta / R / X / norm(R) in one sweep (:221-225);
 * step = s + 1: the polynomial step with omega(Q, R) (:242-256).  Residual smoothing (:226-235) when X_s / R_s are given.  The host waits once per
 * step (twice in steps 1 and s + 1).  The caller owns the vectors as idrs_iterable! sets them up (:116-147): R = C - A X, U = G = 0 (n x s,
 * column-major), X_s = copy(X) and R_s = copy(R) for smoothing (both NULL otherwise), and P: the s shadow vectors (the reference fills them
 * with rand!, :136).  pl_diag: diagonal of a Jacobi Pl or NULL (Identity).  M (= I), f, c and omega (= 1) live in the handle.  s <= 32.
 * normR0 = norm(R).  mik_idrs_step returns it.normR of the reference after the step (norm(R), or norm(R_s) with smoothing); the caller copies
 * X_s into X on termination as :171-173 do. */
typedef struct mik_idrs mik_idrs;
int mik_idrs_create(mik_ctx *ctx, const mik_csr *A, int s, void *x, void *r, const void *P, int64_t ldp, void *U, int64_t ldu, void *G,
                    int64_t ldg, const void *pl_diag, void *x_s, void *r_s, double normR0, mik_idrs **out);
int mik_idrs_step(mik_idrs *it, int step, void *normR);            /* normR: one scalar of A's element type */
int mik_idrs_state(const mik_idrs *it, void *omega, void *M, void *f);   /* host copies (any may be NULL): omega, M (s x s column-major), f (s) */
int mik_idrs_destroy(mik_idrs *it);

/* ---- row-partitioned GMRESIterable: one process per GPU ---------------------------------------- */
/* The same iterable (src/gmres.jl:57-106) over a contiguous row block.  The Arnoldi basis, x, b and
 * the diagonal preconditioners are this rank's n_loc rows; A_loc is the block as an n_loc x n_ext
 * operator whose columns [n_loc, n_ext) are halo entries (same layout as mik_cgd_create).  The two
 * places where ranks couple are handed to the caller:
 *   halo(user):   called with send_buf[i] = v[send_idx[i]] packed (enqueued on the ctx stream) for the
 *                 vector v about to be multiplied; must leave x_ext[n_loc .. n_ext) filled with the
 *                 neighbours' entries, ordered after that packing on the ctx stream (RCCL send/recv on
 *                 the same stream, or a host-staged copy after a stream synchronisation);
 *   reduce(user, dtype, count, values):  values[0..count) are this rank's partial sums (host scalars of
 *                 `dtype`); on return they must hold  ((p_0 + p_1) + p_2) + ...  over ranks 0..P-1 in rank
 *                 order, identically on every rank (dot / norm^2 of src/orthogonalize.jl:71,75,
 *                 src/gmres.jl:252; CGS / DGKS pass all k projections in one call).
 * Either callback returns 0 on success.  Every rank must make the same sequence of calls.  Hessenberg
 * matrix, Givens solve and stopping test are replicated on every rank from identical scalars. */
typedef int (*mik_halo_fn)(void *user);
typedef int (*mik_reduce_fn)(void *user, int dtype, int count, void *values);
typedef struct mik_partition {
    int rank, nranks;
    int64_t n_ext;              /* n_loc + number of halo columns of A_loc */
    void *x_ext;                /* device n_ext-vector: SpMV input; the library writes [0, n_loc) */
    const int32_t *send_idx;    /* device: local indices packed for the neighbours */
    int64_t n_send;
    void *send_buf;             /* device: n_send packed entries */
    mik_halo_fn halo;
    mik_reduce_fn reduce;
    void *user;
    struct mik_plink *link;     /* NULL: the two callbacks above couple the ranks.  A connected link ("Transport 3" below; created on a communicator
                                 * of THIS ctx): the library exchanges by itself, on the device -- halo pushed into the neighbours' landing buffers,
                                 * every projection / norm summed over the ranks inside the kernel that finalises it (rank order, same bits) -- and
                                 * never calls halo / reduce: no host round trip between the k + 1 reductions of an Arnoldi column
                                 * (src/orthogonalize.jl:69-76), one wait per inner iteration as on a single GPU. */
} mik_partition;
int mik_gmres_create_partitioned(mik_ctx *ctx, const mik_csr *A_loc, void *x, const void *b, const void *pl_diag,
                                 const void *pr_diag, double abstol, double reltol, int restart, int64_t maxiter,
                                 int initially_zero, int orth_method, const mik_partition *part, mik_gmres **out);

/* ---- row-partitioned CGIterable: one process per GPU (new design; the reference is serial) --- */
/* out[i] = x[idx[i]], i < m (idx: device Int32) -- packs halo entries for the neighbour ranks. */
int mik_gather(mik_ctx *ctx, int dtype, int64_t m, const int32_t *idx, const void *x, void *out);
/* Rank `rank` of `nranks` owns a contiguous block of n_loc rows.  A_loc is that block as an
 * n_loc x (n_loc + n_ghost) operator: columns [0, n_loc) are the owned entries of a vector, columns
 * [n_loc, n_loc + n_ghost) the halo entries the host receives from the neighbours into the tail of
 * u_ext before STEP_B / INIT_B.  x, b, r, c: device n_loc-vectors; u_ext: device (n_loc + n_ghost)-
 * vector; send_idx / send_buf: local indices to pack and the packed buffer (n_send entries);
 * dot_all / rr_all: device arrays of nranks scalars -- every rank writes slot [rank], the host
 * all-gathers them between phases (RCCL over xGMI via torch.distributed, gloo in CPU tests).
 * Sums over ranks run in rank order on every rank, so all ranks hold identical scalars. */
typedef struct mik_cgd mik_cgd;
int mik_cgd_create(mik_ctx *ctx, const mik_csr *A_loc, void *x, const void *b, void *u_ext, void *r,
                   void *c, const int32_t *send_idx, int64_t n_send, void *send_buf, void *dot_all,
                   void *rr_all, int rank, int nranks, double abstol, double reltol, int64_t maxiter,
                   int initially_zero, mik_cgd **out);
int mik_cgd_destroy(mik_cgd *it);
/* The phases a host may drive itself; [..] is the exchange the host runs between two of them.
 * cg_iterator! (src/cg.jl:120-155): INIT_A, [halo of x], INIT_B, [all-gather rr], INIT_C.
 * iterate (src/cg.jl:43-66): STEP_A, [halo of u], STEP_B, [all-gather dot], STEP_C, [all-gather rr], STEP_D. */
enum mik_cgd_phase_id {
    MIK_CGD_STEP_A = 0,            /* u = r + beta u; pack the halo of u */
    MIK_CGD_STEP_B = 1,            /* c = A u with the local dot(u, c) */
    MIK_CGD_STEP_C = 2,            /* alpha; x += alpha u; r -= alpha c; local |r|^2 */
    MIK_CGD_STEP_D = 3,            /* residual, beta, stopping test of src/cg.jl:36 for iteration + 1 (later steps become no-ops) */
    MIK_CGD_STEP_B_INTERIOR = 4,   /* STEP_B on the row-blocks of mik_cgd_set_interior only */
    MIK_CGD_STEP_B_REST = 5,       /* ... on all other row-blocks, then the local dot(u, c) */
    MIK_CGD_INIT_A = 10,           /* pack the halo of x (nothing if x is zero) */
    MIK_CGD_INIT_B = 11,           /* r = b - A x; local |r|^2; u = 0 */
    MIK_CGD_INIT_C = 12            /* residual, tolerance */
};
/* Enqueue one phase (no host synchronisation). */
int mik_cgd_phase(mik_cgd *it, int phase, int64_t iteration);
/* Overlap of the halo exchange with the SpMV: row-blocks (256 rows each) [rb_begin, rb_end) of this rank contain no
 * row that references a halo column.  Step B may then be issued as STEP_B_INTERIOR (those row-blocks; needs no halo, so
 * it runs while the exchange is in flight) followed by STEP_B_REST (the remaining row-blocks + the local dot) -- same
 * results as STEP_B.  MIK_ERR_NOTIMPL if the operator's layout cannot be launched over a range. */
int mik_cgd_set_interior(mik_cgd *it, int64_t rb_begin, int64_t rb_end);
/* Wait for everything enqueued; residual / tol / done of the last step and the residuals of the
 * steps executed since the previous wait (at most 1024 steps may be enqueued between waits). */
int mik_cgd_wait(mik_cgd *it, double *residual, double *tol, int *done, double *history, int64_t cap,
                 int64_t *steps);

/* ---- the exchanges of the row-partitioned CGIterable inside the library ----------------------------------- */
/* With the calls below the host no longer drives phases and collectives itself: after mik_cgd_create it registers the
 * halo plan and a transport once, and every batch of iterate() calls is ONE entry (a Julia host: one ccall).
 * Halo plan: rank `rank` receives recv_cnt[i] entries from rank recv_peer[i] into the ghost tail of u_ext at element
 * offset recv_off[i] (relative to n_loc), and sends send_cnt[i] entries of send_buf starting at send_off[i] to rank
 * send_peer[i] (the packing order of send_idx).  Arrays are copied. */
int mik_cgd_set_halo_plan(mik_cgd *it, int n_recv, const int *recv_peer, const int64_t *recv_off, const int64_t *recv_cnt,
                          int n_send, const int *send_peer, const int64_t *send_off, const int64_t *send_cnt);
/* What the plan made of the step: *runs = number of contiguous row runs (0, 1 or 2) that are updated, packed and put on the
 * wire before the bulk of the u = r + beta u sweep (0: the halo follows the whole sweep), *rows = their total length,
 * *merged = 1 if update and pack of those rows are one kernel.  Any pointer may be NULL. */
int mik_cgd_halo_early(const mik_cgd *it, int *runs, int64_t *rows, int *merged);

/* Transport 1 -- RCCL over xGMI, one process per GPU.  librccl is bound at run time (dlopen; a process that already
 * carries RCCL, e.g. PyTorch-ROCm, shares that copy); MIK_ERR_NOTIMPL if it cannot be loaded.  Rank 0 obtains the
 * 128-byte ncclUniqueId with mik_comm_unique_id and hands it to the other ranks by whatever channel the host has (MPI.jl
 * bcast, a file, torch.distributed); every rank then calls mik_comm_create (collective).  id128 = NULL gives a communicator
 * without RCCL: a world of one needs nothing else, more ranks connect mailboxes and landing buffers (transport 3 below). */
typedef struct mik_comm mik_comm;
int mik_comm_unique_id(void *id128);
int mik_comm_create(mik_ctx *ctx, const void *id128, int rank, int nranks, mik_comm **out);
int mik_comm_destroy(mik_comm *comm);
int mik_comm_info(const mik_comm *comm, int *rank, int *nranks, int *uses_rccl);
/* values[0..count) (host scalars of dtype, count <= 256): this rank's partial sums in, ((p_0 + p_1) + p_2) + ... over the
 * ranks out, identical on every rank -- exactly the mik_reduce_fn contract, so a row-partitioned GMRES host passes a
 * two-line callback around it.  Blocks (ncclAllGather on the ctx stream + one read-back; a communicator without RCCL sends the
 * values through the vector slots of its connected mailboxes -- same bits, bounded wait). */
int mik_comm_allgather_sum(mik_comm *comm, int dtype, int count, void *values);
/* The mik_halo_fn of a row-partitioned GMRES over RCCL: ncclSend / ncclRecv of the packed buffer into the ghost region
 * on the ctx stream; segments as in mik_cgd_set_halo_plan. */
int mik_comm_halo(mik_comm *comm, int dtype, const void *send_buf, void *ghost, int n_recv, const int *recv_peer,
                  const int64_t *recv_off, const int64_t *recv_cnt, int n_send, const int *send_peer, const int64_t *send_off,
                  const int64_t *send_cnt);
int mik_cgd_set_comm(mik_cgd *it, mik_comm *comm);
/* cg_iterator! (src/cg.jl:120-155) over the partition: init phases + exchanges + one wait. */
int mik_cgd_init(mik_cgd *it, double *residual, double *tol);
/* Up to max_steps iterate() calls (src/cg.jl:43-66) with ONE host wait; collective: every rank makes the same call.
 * Per step: pack, halo (ncclSend / ncclRecv on a side stream -- the interior row-blocks of the SpMV run meanwhile when
 * mik_cgd_set_interior was called), c = A u with the local dot, ncclAllGather of one scalar per rank, update,
 * ncclAllGather, stopping test; the P partial sums are added in rank order on every device.  At most 1024 steps. */
int mik_cgd_iterate_many(mik_cgd *it, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done);

/* Transport 2 -- in-process group: ONE host thread drives all P ranks (its[p] = rank p, each created on its own ctx;
 * the contexts may sit on different GPUs -- halos and scalars then move by peer copies over xGMI -- or share one, which
 * is how the step routine is verified on a single-GPU box).  Same steps, same bits as transport 1. */
int mik_cgd_group_init(mik_cgd **its, int P, double *residual, double *tol);
int mik_cgd_group_iterate_many(mik_cgd **its, int P, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done);
int mik_cgd_group_release(mik_cgd **its, int P);    /* frees the group's events / side streams (also done by mik_cgd_destroy) */

/* Transport 3 -- peer-mapped mailbox over xGMI (SURVEY.md section 5 "backend B", section 8e): no collective launch in the step.
 * Every communicator owns a mailbox in fine-grained device memory.  mik_comm_mailbox_export gives its 64-byte HIP IPC handle; the
 * host gathers the handles of all ranks (rank order) over whatever channel it has and every rank calls mik_comm_mailbox_connect
 * (ranks may even share one GPU: HIP IPC has no one-rank-per-device rule).  From then on the two scalars of a step travel as
 * {value, sequence number} stores into every peer's mailbox, issued by the kernel that finalised the reduction; every rank adds the
 * P values in rank order -- the bits of transports 1 and 2.
 * The halo travels through LANDING BUFFERS: fine-grained device memory owned by the library (one per link, two halves used
 * alternately).  A push kernel stores the packed send buffer straight into the neighbours' landing buffers over xGMI and posts the
 * exchange number in their mailboxes; on the receiving side one kernel waits for the flags and copies the landed entries into the
 * ghost tail of the extended vector with system-scope loads.  The SpMV that follows therefore reads halo data its OWN device wrote --
 * no memory of the host (a tensor of a pooling allocator) is ever mapped into a peer, and nothing depends on which peer-written
 * lines a cache of the receiving device still holds.
 * A communicator created with id128 = NULL and nranks > 1 has no RCCL at all and needs both mailboxes and links; one created with a
 * ncclUniqueId may connect mailboxes only (scalars by mailbox, halo by ncclSend / ncclRecv).
 * Waits are bounded (MIK_MAILBOX_TIMEOUT_MS, default 10000): MIK_ERR_HIP instead of a hung queue. */
int mik_comm_mailbox_export(mik_comm *comm, void *handle64);
int mik_comm_mailbox_connect(mik_comm *comm, const void *handles /* nranks x 64 bytes, rank order; this rank's entry is ignored */);
int mik_comm_mailbox_info(const mik_comm *comm, int *connected, int *finegrained);

/* The links of ONE row partition on a communicator: its halo plan (segments as in mik_cgd_set_halo_plan: offsets into the ghost region
 * of n_ghost entries / into the packed send buffer, at most 8 per direction), its landing buffer and the mappings of the neighbours'.
 *   mik_plink_export   64-byte HIP IPC handle of this rank's landing buffer;
 *   mik_plink_connect  collective, after the host gathered handle and n_ghost of every rank: handles / ghost_counts per RANK (this
 *                      rank's entries are ignored; a rank may be its own neighbour), dst_elem per SEND segment = the element of the
 *                      receiver's ghost region at which the segment lands (the offset of its matching receive segment).
 * A row-partitioned GMRES iterable takes a connected link in mik_partition.link; the row-partitioned CG iterable builds its own from the
 * plan it was given (mik_cgd_ghost_export = create + export, mik_cgd_connect_ghosts = connect). */
typedef struct mik_plink mik_plink;
int mik_plink_create(mik_comm *comm, int dtype, int64_t n_ghost, int n_recv, const int *recv_peer, const int64_t *recv_off, const int64_t *recv_cnt,
                     int n_send, const int *send_peer, const int64_t *send_off, const int64_t *send_cnt, mik_plink **out);
int mik_plink_export(mik_plink *link, void *handle64);
int mik_plink_connect(mik_plink *link, const void *handles, const int64_t *ghost_counts, const int64_t *dst_elem);
int mik_plink_info(const mik_plink *link, int *connected, int *finegrained, int64_t *n_ghost);
/* One halo exchange through a connected link, blocking (collective: every rank of the plan calls it): send_buf (device, packed as the
 * plan's send segments say) is stored into the neighbours' landing buffers, the entries that landed here are copied into ghost (device,
 * n_ghost entries).  What a host that drives a row-partitioned operator itself passes as its mik_halo_fn, and what the transport
 * self-test of bench.py --gpus N times.  A peer that never arrives: MIK_ERR_HIP after MIK_MAILBOX_TIMEOUT_MS.
 * Invariants of the landing buffers (two halves used alternately, no consumed-acknowledgement; one push ticket per communicator):
 *   - ONE exchange in flight per communicator: links of one communicator are used from its context's stream, one after the other;
 *   - a rank must not run two exchanges ahead of a neighbour.  A plan whose send peers equal its receive peers guarantees that by itself;
 *     any other plan only when a sum over all ranks separates two exchanges -- true for cg! / gmres! (a dot or norm follows every
 *     product), so the iterables accept such plans; mik_plink_exchange refuses them (MIK_ERR_NOTIMPL). */
int mik_plink_exchange(mik_plink *link, const void *send_buf, void *ghost);
int mik_plink_destroy(mik_plink *link);
/* After mik_cgd_set_halo_plan and mik_cgd_set_comm (transport "mailbox"): */
int mik_cgd_ghost_export(mik_cgd *it, void *handle64);
int mik_cgd_connect_ghosts(mik_cgd *it, const void *handles, const int64_t *ghost_counts, const int64_t *dst_elem);

/* ---- Hessenberg least squares (host) ------------------------------------------------------ */
/* ldiv!(FastHessenberg(H), rhs) -- src/hessenberg.jl:15-46.  Host arrays of `dtype`; H is
 * (width+1) x width column-major with leading dimension ldh, overwritten by R; rhs has width+1
 * entries, overwritten by [y; residual].  complex (src/hessenberg.jl:24-39 with c real and s complex: -conj(s) in :31, :37; pinned on
 * H2 of test/hessenberg.jl:20-26): host arrays of complex; the back substitution divides on the host. */
int mik_hessenberg_ldiv(int dtype, void *H, int64_t ldh, int width, void *rhs);

/* Host: LinearAlgebra.givensAlgorithm(f, g) -> out = {c, s, r} with [c s; -s c] [f; g] = [r; 0]
 * (src/hessenberg.jl:24, src/minres.jl:129).  f, g, out: host scalars / 3-array of dtype.  complex: givensAlgorithm(f::Complex, g::Complex),
 * LAPACK's lartg convention: out = {c + 0 i, s, r} (three complex) with c real and [c s; -conj(s) c] [f; g] = [r; 0]. */
int mik_givens(int dtype, const void *f, const void *g, void *out);

/* ---- stationary methods: jacobi / gauss_seidel / sor / ssor on a SparseMatrixCSC (src/stationary_sparse.jl) ------------------
 * The building blocks of the four iterables, one entry each.  Every row is summed by one lane, serially, in the order the
 * reference's CSC column loop delivers its terms (no wave tree, no FMA), so the results are bit-identical to the reference's:
 *   mik_offdiag_mul      row i: y[i] = 0 | y[i] | beta*y[i], then y[i] += A[i,j] * (alpha*x[j]) for j != i ascending
 *   mik_gs_multiply  U:  z[i] = beta*y[i], then += A[i,j] * (alpha*x[j]) for j > i ascending (x: the OLD vector)
 *                    L:  the same for j < i DESCENDING
 *   mik_forward_sub      x[i] -= A[i,j]*x[j] for j < i ascending (x[j] already new), then x[i] /= A[i,i]
 *                        (relaxed form: x[i] = alpha*x[i]/A[i,i] + beta*y[i])
 *   mik_backward_sub     the same for j > i DESCENDING
 * The triangular sweeps run a level schedule of the strict triangle built in mik_stationary_create: one launch per level with more
 * than 256 rows, one one-workgroup launch per run of narrower levels (a barrier between its levels).  Their cost is the number of
 * levels: a tridiagonal matrix (one row per level) stays latency-bound.  Asynchronous on the ctx stream.
 *
 * ComplexF64 / ComplexF32 operators (MIK_C64 / MIK_C32, interleaved re, im; added without a version bump, additive): the same entries, the
 * same row orders, the same level schedules and launch plans as the real operator of the same pattern.  Element operations, in Julia's
 * promotion order: every product is (zr wr - zi wi) + (zr wi + zi wr) i with four rounded products, one difference and one sum; every
 * add / subtract is componentwise; every division is Base's -- 64-bit components: the robust division of Baudin and Smith; 32-bit
 * components: evaluated in double with mag = 1 / fma(c, c, d d), re = fma(a, c, b d) mag, im = fma(b, c, -(a d)) mag and rounded to float once
 * per component (the only two FMAs of the library).  Base's branches for infinite divisors are not restated: operators are finite with
 * non-zero diagonals.  Vectors need alignment to their component only; vectors aligned to their element take one 16- / 8-byte access an
 * element, with identical results.
 *   mik_diag_ldiv        y[i] = x[i] / A[i,i] in the data type
 *   mik_offdiag_mul, mik_gs_multiply   alpha, beta: host COMPLEX scalars of the operator's type; acc += A[i,j] * (alpha * x[j]), two complex
 *                        products a term; beta == one(T) and iszero(beta) compare both components (either sign of zero), else beta * y[i]
 *   mik_forward_sub, mik_backward_sub   plain: x[i] -= A[i,j] * x[j] ..., x[i] = x[i] / A[i,i], all in the data type.  Relaxed:
 *                        scalar_dtype (MIK_F64 / MIK_F32) names the REAL component type E of the evaluation; alpha is a host REAL of E
 *                        (omega is Real in the reference), beta a host COMPLEX pair (re, im) of E (one(T) - omega, imaginary part +0.0).
 *                        a = (alpha re(x[i]), alpha im(x[i])) in E; x[i] = T(a / E(A[i,i]) + beta * E(y[i])), one rounding per component at
 *                        the store: ComplexF32 data with MIK_F64 scalars divides with the 64-bit algorithm, with MIK_F32 scalars with the
 *                        widened 32-bit one; ComplexF64 data always evaluates in double.  The subtractions stay in the data type.
 *   mik_stationary_create   a diagonal entry is zero when both components are (either sign). */
typedef struct mik_stationary mik_stationary;    /* DiagonalIndices + the triangular views of one square operator -- :6-64 */
/* DiagonalIndices(A) (:6-28) + both level schedules.  Reads A's CSR arrays once (A's layouts are untouched; A must outlive *out).
 * MIK_ERR_SINGULAR with *singular_col = the first 1-based column whose diagonal entry is missing or zero (-0.0 included);
 * MIK_ERR_MISMATCH for a non-square operator; MIK_ERR_NOTIMPL after mik_csr_compact released the CSR arrays.  Synchronises. */
int mik_stationary_create(mik_ctx *ctx, const mik_csr *A, int64_t *singular_col, mik_stationary **out);
int mik_stationary_destroy(mik_stationary *S);
/* levels[2] / launches[2]: per direction ([0] forward = strict lower, [1] backward = strict upper); bytes: device memory held;
 * analysis_ms: host time of mik_stationary_create.  Any pointer may be NULL. */
int mik_stationary_info(const mik_stationary *S, int64_t *levels, int64_t *launches, int64_t *bytes, double *analysis_ms);
/* ldiv!(y, D, x): y[i] = x[i] / A[i,i] -- :30-35.  y may alias x. */
int mik_diag_ldiv(mik_stationary *S, void *y, const void *x);
/* mul!(alpha, O::OffDiagonal, x, beta, y) -- :148-171 (beta == 0: fill!, beta == 1: untouched, else lmul!).  Host scalars of the
 * operator's dtype; x and y must not alias. */
int mik_offdiag_mul(mik_stationary *S, const void *alpha, const void *x, const void *beta, void *y);
/* gauss_seidel_multiply!(alpha, U (upper = 1) | L (upper = 0), x, beta, y, z) -- :178-191 / :196-208.  z may alias x (GaussSeidelIterable
 * does this, :284): the library then reads a copy of the old x.  Host scalars of the operator's dtype. */
int mik_gs_multiply(mik_stationary *S, int upper, const void *alpha, const void *x, const void *beta, const void *y, void *z);
/* forward_sub!(F, x) (y == NULL: alpha / beta ignored) -- :67-82; forward_sub!(alpha, F, x, beta, y) -- :87-103.  alpha / beta are host
 * scalars of scalar_dtype (MIK_F64 / MIK_F32): Float32 data with MIK_F64 scalars evaluates alpha*x[i]/d + beta*y[i] in Float64 and
 * rounds once at the store (Julia's promotion for sor!(x::Vector{Float32}, A, b, 1.2)); the subtractions stay in the data type. */
int mik_forward_sub(mik_stationary *S, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype);
/* backward_sub!(F, x) -- :109-124; backward_sub!(alpha, F, x, beta, y) -- :126-142.  As mik_forward_sub. */
int mik_backward_sub(mik_stationary *S, const void *alpha, void *x, const void *beta, const void *y, int scalar_dtype);

/* ---- dense stationary methods: jacobi / gauss_seidel / sor / ssor on an AbstractMatrix (src/stationary.jl:31-263) ----------------
 * One entry per whole iteration of the four dense iterables (added without a version bump, additive); real MIK_F64 / MIK_F32.  A is a
 * DEVICE n x n column-major matrix with leading dimension ld >= n, read at every step (the handle keeps no copy of it; A must outlive
 * the handle).  The reference's column loops give every row one serial order of subtractions; with d = A[r,r] and every
 * `acc = acc - (A[r,c] * x[c])` rounded twice (no FMA) they are, row by row:
 *   jacobi        next[r] = b[r] - sum over c != r ascending (old x);  x[r] = next[r] / d                                 -- :48-72
 *   gauss_seidel  t = b[r] - sum over c > r ascending (old x) - sum over c < r ascending (new x);  x[r] = t / d          -- :108-129
 *   sor           tmp[r] = that t;  x[r] = x[r] + omega * (tmp[r] / d - x[r])                                            -- :167-188
 *   ssor          the sor sweep, giving x'; then tmp[r] = b[r] - sum over c < r DESCENDING - sum over c > r DESCENDING, every product
 *                 with x' (:254-260 subtracts column col before it updates x[col]);  x[r] = x'[r] + omega * (tmp[r] / d - x'[r])  -- :227-263
 * A lane owns a row and walks its columns in that order; a row's chain is never split, so a sweep is n-fold parallel and no more.
 * The strict-lower phase is a blocked forward substitution in the PANEL form: ceil(n / W) launches following each other on the
 * stream, launch K subtracting panel K - 1's W columns from the rows at or below panel K and then solving panel K's diagonal block
 * (W serial steps: divide or relax, broadcast, subtract below) in the one workgroup that owns it.  No workgroup waits for another.
 * omega is a HOST scalar of scalar_dtype, as for mik_forward_sub: Float32 data with a MIK_F64 omega evaluates the inner difference in
 * Float32, the product and the sum in Float64, and rounds once at the store; an Int omega is passed in the element type.
 * x, next / tmp and b are DEVICE n-vectors that must not overlap (MIK_ERR_INVALID).  The steps are asynchronous on the ctx stream;
 * the handle owns the copy of the old x and the Gauss-Seidel accumulators, nothing is allocated per step. */
typedef struct mik_dense_stationary mik_dense_stationary;
enum { MIK_DENSE_AUTO = 0, MIK_DENSE_PANEL = 1, MIK_DENSE_CHAINED = 2 };
typedef struct mik_dense_plan {
    int form;         /* MIK_DENSE_AUTO (= the panel form) / MIK_DENSE_PANEL / MIK_DENSE_CHAINED (a single-launch forward substitution whose
                       * workgroups hand x on to each other: not built, MIK_ERR_NOTIMPL) */
    int spin_limit;   /* bound of a chained launch's waits, 0 = default; unused by the panel form */
} mik_dense_plan;
/* check_diag(A) (:6-12) on the device + the handle's two n-vectors.  plan may be NULL (= MIK_DENSE_AUTO).  MIK_ERR_SINGULAR with
 * *singular_col = the first 1-based i with iszero(A[i,i]) (-0.0 included); MIK_ERR_MISMATCH for ld < n or n < 1.  Synchronises. */
int mik_dense_stationary_create(mik_ctx *ctx, const void *A, int64_t n, int64_t ld, int dtype, const mik_dense_plan *plan,
                                int64_t *singular_col, mik_dense_stationary **out);
int mik_dense_stationary_destroy(mik_dense_stationary *S);
/* panel_w: W; rows_per_workgroup: rows a workgroup of the row-owned sweep and of a panel launch owns; launches_forward: launches of one
 * forward substitution; form: the form in use (MIK_DENSE_PANEL); gave_up: 1 once a chained launch gave up (always 0: there is none);
 * bytes: device memory held.  Any pointer may be NULL. */
int mik_dense_stationary_info(const mik_dense_stationary *S, int64_t *panel_w, int64_t *rows_per_workgroup, int64_t *launches_forward,
                              int *form, int *gave_up, int64_t *bytes);
/* One iteration of DenseJacobiIterable -- :48-72.  next keeps the undivided values. */
int mik_dense_jacobi_step(mik_dense_stationary *S, void *x, void *next, const void *b);
/* One iteration of DenseGaussSeidelIterable -- :108-129, in place in x. */
int mik_dense_gs_step(mik_dense_stationary *S, void *x, const void *b);
/* One iteration of DenseSORIterable -- :167-188.  tmp keeps the accumulators the divisions read. */
int mik_dense_sor_step(mik_dense_stationary *S, void *x, void *tmp, const void *b, const void *omega, int scalar_dtype);
/* One iteration of DenseSSORIterable -- :227-263.  tmp keeps the accumulators of the backward half. */
int mik_dense_ssor_step(mik_dense_stationary *S, void *x, void *tmp, const void *b, const void *omega, int scalar_dtype);

/* ---- dense LU: lu!(A) with partial pivoting and ldiv!(y, F, x) on a square device matrix ------------------------------------------
 * What the reference's tests pass as Pl / Pr (test/gmres.jl:28-35, test/bicgstabl.jl:40-42, test/idrs.jl:55) and as the
 * operator of invpowm (test/simple_eigensolvers.jl:40).  Added without a version bump, additive; real MIK_F64 / MIK_F32 (MIK_C64 / MIK_C32:
 * MIK_ERR_NOTIMPL with a message that names the element type).
 * THE BIT CONTRACT: the factors, the pivots and the solution are those of the unblocked loops of mik_lu_solve.
 *   - the pivot of column j is the FIRST row i >= j with the largest |A[i,j]| (strict >, LAPACK's idamax);
 *   - the multiplier is A[i,j] / pivot, a division;
 *   - every element (i,c) receives a = a - m * u for k = 0, 1, ..., min(i,c) - 1 in ascending k, the product and the difference rounded
 *     on their own (no fma, no matrix cores);
 *   - ldiv! applies the row interchanges to x, then runs the unit-lower chain of every row in ascending column order, then the upper chain
 *     of every row in DESCENDING column order with the division by U[i,i] last.
 * Non-finite data follow the same loops: a NaN in A[j,j] keeps the pivot of column j in row j and is not a zero pivot, a NaN in any row
 * below is never the pivot and hides no other row, equal infinities are a tie like any other, and NaN / Inf in A or x propagate as those
 * operations propagate them (where a NaN stands is part of the contract, its sign and payload are not).
 * The device plan is blocked (panels of W columns, a tiled trailing update); blocking keeps k ascending per element and so keeps the bits.
 * Every dependency between workgroups is a kernel boundary on the ctx stream; nothing is allocated per solve. */
typedef struct mik_dense_lu mik_dense_lu;
/* lu!(A): A (column-major n x n, leading dimension ld, device) is overwritten by L\U and must outlive the handle.  MIK_ERR_SINGULAR and
 * *singular_col = k (1-based) for the first exactly zero pivot column (-0.0 included) -- SingularException(k); no handle is returned then.
 * MIK_ERR_MISMATCH for ld < n or n < 1; MIK_ERR_NOTIMPL for n >= 2^31 - 64.  Synchronises once, at the end. */
int mik_dense_lu_create(mik_ctx *ctx, void *A, int64_t n, int64_t ld, int dtype, int64_t *singular_col, mik_dense_lu **out);
int mik_dense_lu_destroy(mik_dense_lu *F);
/* host, n entries, 1-based: LAPACK's ipiv / F.ipiv (row j was interchanged with row ipiv[j]).  No device access. */
int mik_dense_lu_ipiv(const mik_dense_lu *F, int64_t *ipiv);
/* ldiv!(y, F, x) on DEVICE n-vectors, asynchronous on the ctx stream.  y may equal x (ldiv!(F, x)); a partial overlap, or a vector that
 * overlaps the factors, is MIK_ERR_INVALID. */
int mik_dense_lu_solve(mik_dense_lu *F, void *y, const void *x);
/* ldiv!(Y, F, X) on DEVICE column-major blocks: Y[:, 0:nrhs) = F \ X[:, 0:nrhs), n rows each, leading dimensions ldy and ldx; asynchronous
 * on the ctx stream.  Column j of Y has exactly the bits mik_dense_lu_solve gives for column j of X (non-finite data included): the same
 * operations on the same operands in the same order; a lane of the substitution kernels carries NB columns (2 of a real type, 1 of a
 * complex one), and the groups of NB columns run side by side in every launch.  The block runs in passes of at most 32 columns, each pass the launches of one vector solve, through a workspace of
 * n x 32 elements that the handle allocates at the first block solve, keeps, and frees in destroy (mik_dense_lu_info's bytes does not count
 * it); nothing is allocated afterwards.  Y may be X with ldy == ldx (the pass is gathered into the workspace first).  MIK_ERR_MISMATCH for
 * nrhs < 1, ldy < n or ldx < n; MIK_ERR_INVALID for any other overlap of the two blocks, or of a block with the factors.  A refused call
 * launches nothing.  The rows [n, ld) of Y and its columns from nrhs on are never written.  Added without a version bump, additive. */
int mik_dense_lu_solve_block(mik_dense_lu *F, void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs);
/* The same as a mik_ldiv_fn (user = the handle): a host fills mik_precond{NULL, mik_dense_lu_ldiv_fn, handle} and the fused iterables
 * apply Pl / Pr with no host frame of the caller's. */
int mik_dense_lu_ldiv_fn(void *user, void *y, const void *x);
/* Every size at which the code switches.  panel_w: W; search_rows: rows per workgroup of the pivot search and of the panel update;
 * tile_rows / tile_cols: the tile of the trailing update; one_launch_rows: the row limit of a one-launch panel (0: not built);
 * launches_factor: kernel launches the factorisation made; launches_solve: launches of one solve (1 + 2 ceil(n / W)); bytes: device memory
 * held besides A.  Any pointer may be NULL. */
int mik_dense_lu_info(const mik_dense_lu *F, int64_t *panel_w, int64_t *search_rows, int64_t *tile_rows, int64_t *tile_cols,
                      int64_t *one_launch_rows, int64_t *launches_factor, int64_t *launches_solve, int64_t *bytes);

/* ---- dense Cholesky: cholesky!(Hermitian(A, :L)) and ldiv!(y, F, x) on a square device matrix, real and complex ---------------------
 * What the reference's tests pass as Pl to cg (test/cg.jl:44-47: F = cholesky(A, Val(false)); cg(A, b; Pl=F)) and to chebyshev
 * (test/chebyshev.jl:59-66), in Float32, Float64, ComplexF32 and ComplexF64.  Added without a version bump, additive; MIK_F64 / MIK_F32 /
 * MIK_C64 / MIK_C32.
 * THE BIT CONTRACT (restated as unblocked C99 loops in tests/dense_ref/dense_chol_ref.c).  Complex products are four rounded products, one
 * rounded difference and one rounded sum; every subtraction is componentwise; no fma, no matrix cores, no reciprocal.  For j = 0 ... n - 1:
 *   - diagonal: d = re(A[j,j]); for k = 0 ... j - 1 ascending d = d - (lr lr + li li) of L[j,k] (real types: d - L[j,k] L[j,k]); that sum is
 *     exactly the real part of L[j,k] conj(L[j,k]).  !(d > 0), which a NaN satisfies too, fails column j and the FIRST such j is reported,
 *     1-based; otherwise L[j,j] = sqrt(d), correctly rounded, stored with imaginary part +0;
 *   - below the diagonal, i > j: a = A[i,j]; for k = 0 ... j - 1 ascending a = a - L[i,k] conj(L[j,k]); L[i,j] = a / L[j,j], a true division
 *     per component;
 *   - ldiv!: forward, acc = x[i], for k < i ascending acc -= L[i,k] w[k], w[i] = acc / L[i,i]; backward, acc = w[i], for k > i DESCENDING
 *     acc -= conj(L[k,i]) y[k], y[i] = acc / L[i,i].
 * Only the lower triangle of A and the real parts of its diagonal are read (LAPACK's rule); the strict upper triangle is never read and
 * never written.  After a failure at column k the contents of the columns >= k are unspecified.  Whether A is Hermitian is not checked.
 * The device plan is blocked (panels of W columns, three launches each: the diagonal block, the rows below it, the lower tiles of the
 * trailing update); blocking keeps k ascending per element and so keeps the bits.  Nothing indexes memory through a data value: an
 * indefinite or non-finite matrix cannot fault.  Every dependency between workgroups is a kernel boundary on the ctx stream. */
typedef struct mik_dense_chol mik_dense_chol;
/* cholesky!(Hermitian(A, :L)): the lower triangle of A (column-major n x n, leading dimension ld, device) is overwritten by L; A must
 * outlive the handle.  A column whose pivot is not positive: with check != 0, MIK_ERR_SINGULAR, *failed_col = k (1-based), the message names
 * PosDefException(k) and no handle is returned; with check == 0, MIK_OK and a handle whose info is k (cholesky(A; check = false)).
 * MIK_ERR_MISMATCH for ld < n or n < 1; MIK_ERR_NOTIMPL for n >= 2^31 - 64.  Synchronises once, at the end. */
int mik_dense_chol_create(mik_ctx *ctx, void *A, int64_t n, int64_t ld, int dtype, int check, int64_t *failed_col, mik_dense_chol **out);
int mik_dense_chol_destroy(mik_dense_chol *F);
/* ldiv!(y, F, x) on DEVICE n-vectors, asynchronous on the ctx stream; nothing is allocated.  y may equal x (ldiv!(F, x)); a partial overlap,
 * a vector that overlaps the factors, or a handle whose info is not 0 is MIK_ERR_INVALID. */
int mik_dense_chol_solve(mik_dense_chol *F, void *y, const void *x);
/* ldiv!(Y, F, X) on DEVICE column-major blocks, as mik_dense_lu_solve_block: column j of Y has exactly the bits mik_dense_chol_solve gives
 * for column j of X; passes of at most 32 columns, each the launches of one vector solve, through a workspace of n x 32 elements allocated
 * at the first block solve and kept (mik_dense_chol_info's bytes does not count it).  Y may be X with ldy == ldx.  MIK_ERR_MISMATCH for
 * nrhs < 1, ldy < n or ldx < n; MIK_ERR_INVALID for any other overlap of the two blocks, an overlap with the factors, or a handle whose info
 * is not 0.  A refused call launches nothing.  The rows [n, ld) of Y and its columns from nrhs on are never written. */
int mik_dense_chol_solve_block(mik_dense_chol *F, void *Y, int64_t ldy, const void *X, int64_t ldx, int64_t nrhs);
/* The same as a mik_ldiv_fn (user = the handle): a host fills mik_precond{NULL, mik_dense_chol_ldiv_fn, handle} and the fused iterables
 * apply Pl / Pr with no host frame of the caller's. */
int mik_dense_chol_ldiv_fn(void *user, void *y, const void *x);
/* Every size at which the code switches, for the handle's element type.  panel_w: W; rows_per_group: rows per workgroup of the panel
 * kernel; tile_rows / tile_cols: the tile of the trailing update; launches_factor: kernel launches the factorisation made (3 per panel, 1
 * for the last); launches_solve: launches of one solve (2 ceil(n / W)); bytes: device memory held besides A; info: 0, or the 1-based index
 * of the first failing column.  Any pointer may be NULL. */
int mik_dense_chol_info(const mik_dense_chol *F, int64_t *panel_w, int64_t *rows_per_group, int64_t *tile_rows, int64_t *tile_cols,
                        int64_t *launches_factor, int64_t *launches_solve, int64_t *bytes, int64_t *info);

/* ---- dense QR: qr!(A) (Householder, no pivoting), lmul!(Q, Y), lmul!(Q', Y), F \ b and Matrix(F.Q) on an m x n device matrix, m >= n -----
 * A \ b for a tall matrix is what the reference's tests hold lsqr and lsmr to (test/lsqr.jl:15-19, test/lsmr.jl:68-72), and Matrix(qr(A).Q) is
 * how they build an orthonormal basis (test/orthogonalize.jl:17-18).  Added without a version bump, additive; real MIK_F64 / MIK_F32
 * (MIK_C64 / MIK_C32: MIK_ERR_NOTIMPL with a message that names the element type).
 * THE BIT CONTRACT (stated in csrc/mik_dense_qr.h, restated as unblocked C99 loops in tests/dense_ref/dense_qr_ref.c).  No fma, no matrix
 * cores, no reciprocal; `/` and sqrt correctly rounded; a product and the sum or difference that takes it rounded on their own.
 *   - the reduction T over a range of ABSOLUTE rows i: 256 accumulators starting at +0, accumulator i mod 256 takes acc = acc + p_i in
 *     ascending i; each group of 64 accumulators is folded by a[l] += a[l + s], s = 32, 16, 8, 4, 2, 1; the four sums are added left to right;
 *   - column j: alpha = A[j,j], s = T(A[i,j] A[i,j]; j < i < m).  s == 0: tau[j] = 0, nothing stored.  Otherwise nrm = sqrt(alpha alpha + s),
 *     beta = -copysign(nrm, alpha), tau[j] = (beta - alpha) / beta, A[i,j] = A[i,j] / (alpha - beta) for i > j, A[j,j] = beta;
 *   - reflector j on a column a: skipped if tau[j] == 0; else w = T(v_i a_i; j <= i < m) with v_j = 1, v_i = A[i,j]; t = tau[j] w;
 *     a_i = a_i - v_i t.  Ascending j in the factorisation and in Q' y, descending j in Q y;
 *   - F \ b: t = Q' b on a copy of b, then R x = t[0:n] by the upper chain of mik_dense_lu_solve (per row, descending columns, the division
 *     by R[i,i] last); Matrix(F.Q) is Q applied to the first n columns of the m x m identity.
 * RANGE: the sums of squares are not rescaled: a column whose alpha^2 + s overflows, or underflows to a subnormal, follows the loops into
 * Inf / 0 / reduced accuracy.  Non-finite data follow the loops; nothing indexes memory through a data value.
 * The device plan is blocked (panels of W columns, one launch per column, one trailing update per panel in which a workgroup owns a column);
 * an element still meets its reflectors in ascending order, so the bits are the unblocked loop's.  Rows are NOT split across workgroups: a
 * column is worked on by one compute unit, so a tall matrix of very few columns uses few of them.  Every dependency between workgroups is
 * a kernel boundary on the ctx stream. */
typedef struct mik_dense_qr mik_dense_qr;
/* resident_rows: a launch that applies the reflectors from k0 on keeps the rows [k0, m) of the column a workgroup owns in LDS while
 * m - k0 <= resident_rows, and streams them through memory otherwise (same bits): lmul, the solve and the thin Q start at 0, the trailing
 * update of a panel at the panel's first column.  0 = the default, the rows that fit; a larger value is cut to that. */
typedef struct mik_dense_qr_plan { int64_t resident_rows; } mik_dense_qr_plan;
/* qr!(A): A (column-major m x n, leading dimension ld, device) is overwritten by R on and above the diagonal and the reflectors' v below
 * it, and must outlive the handle.  plan may be NULL.  *zero_diag = the 1-based index of the first R[k,k] == 0, or 0: not an error (qr! does
 * not throw); such a handle multiplies, but refuses to solve.  MIK_ERR_MISMATCH for m < n (DimensionMismatch: a wide matrix is not
 * offered), n < 1 or ld < m; MIK_ERR_NOTIMPL for m >= 2^31 - 64 (so also n) or a complex dtype.  Synchronises once, at the end. */
int mik_dense_qr_create(mik_ctx *ctx, void *A, int64_t m, int64_t n, int64_t ld, int dtype, const mik_dense_qr_plan *plan, int64_t *zero_diag,
                        mik_dense_qr **out);
int mik_dense_qr_destroy(mik_dense_qr *F);
/* F.τ: host, n entries of the element type.  No device access. */
int mik_dense_qr_tau(const mik_dense_qr *F, void *tau);
/* lmul!(F.Q, Y) (adjoint == 0) or lmul!(F.Q', Y) (adjoint != 0) in place on `ncols` DEVICE columns of m rows, leading dimension ldy;
 * asynchronous on the ctx stream, one launch.  MIK_ERR_MISMATCH for ldy < m or ncols < 1; MIK_ERR_INVALID when Y overlaps the factors. */
int mik_dense_qr_lmul(mik_dense_qr *F, int adjoint, void *Y, int64_t ldy, int64_t ncols);
/* ldiv!(x, F, b) / F \ b: x a DEVICE vector of n, b of m, not modified -- unless x == b, where the first n entries of b become x
 * (ldiv!(F, b)).  Asynchronous on the ctx stream; nothing is allocated.  MIK_ERR_SINGULAR naming SingularException(k) on a handle whose
 * zero_diag is k; MIK_ERR_INVALID for any other overlap of x and b or an overlap with the factors. */
int mik_dense_qr_solve(mik_dense_qr *F, void *x, const void *b);
/* ldiv!(X, F, B) on DEVICE column-major blocks: X n rows (ldx), B m rows (ldb), nrhs columns.  Column j of X has exactly the bits
 * mik_dense_qr_solve gives for column j of B.  Passes of at most 32 columns, each the launches of one vector solve, through a workspace of
 * m x 32 elements allocated at the first block solve and kept (mik_dense_qr_info's bytes does not count it).  X may be B with ldx == ldb.
 * MIK_ERR_MISMATCH for nrhs < 1, ldx < n or ldb < m; MIK_ERR_INVALID for any other overlap; MIK_ERR_SINGULAR as above. */
int mik_dense_qr_solve_block(mik_dense_qr *F, void *X, int64_t ldx, const void *B, int64_t ldb, int64_t nrhs);
/* Matrix(F.Q): Q (DEVICE, m x n, leading dimension ldq) = Q applied to the first n columns of the identity.  Two launches. */
int mik_dense_qr_thin_q(mik_dense_qr *F, void *Q, int64_t ldq);
/* F.R: R (DEVICE, n x n, leading dimension ldr) = the upper triangle of the factors, +0 below the diagonal.  One launch. */
int mik_dense_qr_r(mik_dense_qr *F, void *R, int64_t ldr);
/* mik_dense_qr_solve as a mik_ldiv_fn (user = the handle), for SQUARE handles only (else MIK_ERR_MISMATCH): Pl / Pr of the fused iterables. */
int mik_dense_qr_ldiv_fn(void *user, void *y, const void *x);
/* panel_w: W; accumulators: those of T (256); resident_rows: the row limit in use; resident: 1 if the launches that start at reflector 0 (lmul,
 * solve, thin Q) keep their column in LDS (m <= resident_rows), 0 if they stream; launches_factor: kernel launches the factorisation made (n, plus one per panel that has
 * columns to its right); launches_solve: launches of one solve (1 + ceil(n / 64)); bytes: device memory held besides A; zero_diag as in
 * create.  Any pointer may be NULL. */
int mik_dense_qr_info(const mik_dense_qr *F, int64_t *panel_w, int64_t *accumulators, int64_t *resident_rows, int64_t *resident,
                      int64_t *launches_factor, int64_t *launches_solve, int64_t *bytes, int64_t *zero_diag);

/* ---- svdl: Golub-Kahan-Lanczos bidiagonalisation with thick restart (src/svdl.jl) ------------------------------------------
 * The Lanczos loop of extend! (:542-609) runs on mik_spmv (A and its adjoint as two operators), mik_gemv_t / mik_gemv_n and the fused
 * sweeps above; the k x k SVD of a restart stays on the host.  Two things no entry above does in one pass (added without a version bump,
 * additive): */
/* Y[:, 0:l] = V[:, 0:k] * F[0:k, 0:l] -- the basis rotations of the restarts, view(L.Q, :, 1:k) * view(F.V, :, 1:l) and
 * view(L.P, :, 1:k) * view(F.U, :, 1:l) (src/svdl.jl:384, :392), L.Q * view(Q, :, 1:k+1) and L.P * view(U, :, 1:k) (:470, :471), and the
 * singular vectors (:231, :237).  V, Y: DEVICE, column-major, leading dimensions ldv / ldy in elements; F: HOST, column-major k x l with
 * leading dimension ldf, of `dtype` (read before the call returns).  Exactly
 *   Y[i, j] = (...((V[i, 0] * F[0, j]) + V[i, 1] * F[1, j]) + ...) + V[i, k-1] * F[k-1, j],
 * columns ascending, every product and every sum rounded on its own (no FMA, no matrix cores): an element depends on its own row
 * only, so the result is independent of the launch shape and equal to the loop `acc = V[:, 0] * F[0, j]; acc = acc + V[:, c] * F[c, j]`
 * bit for bit.  One pass: every element of V is read once (twice when l > 32) and every element of Y written once.
 * 1 <= l <= k <= 64, else MIK_ERR_NOTIMPL; Y must not overlap V (MIK_ERR_INVALID).  Asynchronous on the ctx stream. */
int mik_basis_rotate(mik_ctx *ctx, int dtype, int64_t n, int k, int l, const void *V, int64_t ldv, const void *F, int64_t ldf,
                     void *Y, int64_t ldy);
/* The re-orthogonalisation of a new Lanczos vector and its normalisation -- src/svdl.jl:567-577 (right vectors; :587-597 for the left ones):
 *   old = norm(q); q -= Q * (Q' q); if norm(q) <= alpha * old: q -= Q * (Q' q); beta = norm(q); q .*= inv(beta)
 * Q: DEVICE n x k basis (leading dimension ldq); q: DEVICE n-vector, updated in place; alpha, beta_out: HOST scalars of `dtype`;
 * *passes_out: 1 or 2, the Gram-Schmidt passes that ran.  Bit-identical to issuing mik_nrm2, mik_gemv_t, mik_gemv_n (alpha = -1), mik_nrm2, the
 * comparison on the host in `dtype`, (mik_gemv_t, mik_gemv_n, mik_nrm2), mik_scal by 1 / beta one after another, the scaled recomputation
 * of "Norms" included -- but a pass is two sweeps: the squared norm of q rides on the projection sweep (before) and on the update
 * sweep (after), through the same fixed tree, so Q is read twice per pass and q is not swept for its norms; the closing scaling is one
 * more sweep over q (the norm it divides by is only complete when the update sweep has ended).  k = 0: norm and scaling only.
 * beta == 0 is returned as it is and q is then left unscaled (the reference divides by zero).  Synchronises. */
int mik_svdl_reorth(mik_ctx *ctx, int dtype, int64_t n, int k, const void *Q, int64_t ldq, void *q, const void *alpha, void *beta_out,
                    int *passes_out);

/* ---- lobpcg: the block sweeps of the Locally Optimal Block Preconditioned Conjugate Gradient method (src/lobpcg.jl) ---------
 * Every sweep of LOBPCG works on a block of vectors.  Four entries (added without a version bump, additive): MIK_F64 / MIK_F32 and, added
 * later in the same way, MIK_C64 / MIK_C32 (interleaved re, im; the complex definitions follow each entry and the paragraph below).
 * Blocks: DEVICE, column-major, leading dimension in elements; small matrices: HOST, column-major, of `dtype`, read before the call
 * returns.  A block is at most 32 columns wide, else MIK_ERR_NOTIMPL.  No FMA, no matrix cores: every product and every sum is rounded
 * on its own.  The residual columns and their norms, the gather of the active columns, the constraint and the preconditioner are
 * composed from the vector entries above (mik_axpy_dot, mik_nrm2, mik_copy, mik_gemv_n, mik_divide).
 * Complex blocks: leading dimensions count ELEMENTS, element alignment (8 bytes) suffices, small host matrices are interleaved complex.
 * z * w = (zr wr - zi wi) + (zr wi + zi wr) i with every product and every sum rounded on its own, sums componentwise, re and im each
 * their own chain, nothing contracted; there is no complex division on the device. */
/* Y[:, j] = A * X[:, j] for j < b -- mul!(AX, A, X), :124-139.  Column j of Y equals mik_spmv(A, X[:, j]) bit for bit, whatever layout
 * the operator runs on.  An operator that still holds its CSR arrays and has no row longer than mik_spmv_long_row is swept by one kernel
 * on those arrays, one lane per row: the operator's tile is read once per block of 8 columns instead of once per column, each column's
 * row sum serial in ascending column order from +0.  An operator with long rows, or one whose CSR arrays were released by
 * mik_csr_compact, runs mik_spmv column by column.  ldx >= columns of A, ldy >= rows of A; Y must not overlap X (MIK_ERR_INVALID).
 * A complex operator (MIK_C64 / MIK_C32): column j of Y equals the complex mik_spmv(A, X[:, j]) bit for bit -- a row's products
 * val * x[col] added from (+0, +0) in ascending entry order, re and im separately; the operator's values and columns are read once per
 * block of 4 columns; an operator with a row longer than mik_spmv_long_row runs mik_spmv column by column.
 * Asynchronous on the ctx stream. */
int mik_spmm(mik_ctx *ctx, const mik_csr *A, int b, const void *X, int64_t ldx, void *Y, int64_t ldy);
/* G = X[:, 0:p]' * Y[:, 0:q], a p x q HOST matrix with leading dimension ldg -- every mul!(G, adjoint(X), Y) of :262-270, :217, :375.
 * G[i, j] equals mik_dot(X[:, i], Y[:, j]) bit for bit: the fixed tree of mik_reduce_shape ("Reduction semantics"), the segment sums
 * through the same finaliser.  One launch sweeps both blocks, 4 columns of X against 4 columns of Y per workgroup (a column is read
 * ceil(q / 4) resp. ceil(p / 4) times instead of q resp. p times).  X == Y is allowed.  Synchronises.
 * Complex: G[i, j] equals the complex mik_dot(X[:, i], Y[:, j]) = sum conj(x) y bit for bit (per element re = xr yr + xi yi,
 * im = xr yi - xi yr, one tree of mik_reduce_shape(dtype) for re and one for im); no symmetry is assumed; ldg counts elements. */
int mik_block_gram(mik_ctx *ctx, int dtype, int64_t n, int p, int q, const void *X, int64_t ldx, const void *Y, int64_t ldy, void *G,
                   int64_t ldg);
/* X <- X * inv(R) in place, R: HOST s x s, upper triangular (the strict lower triangle is not read) -- rdiv!, :345-355.  Exactly
 *   for i = 0 .. s-1:  for j = 0 .. i-1:  X[:, i] = X[:, i] - X[:, j] * R[j, i];   then  X[:, i] = X[:, i] / R[i, i]
 * every operation rounded on its own.  A row depends on itself only: a lane keeps its row's s values in registers and makes one pass.
 * Complex: X[:, i] = X[:, i] - X[:, j] * R[j, i] with the complex product above and a componentwise subtraction, then
 * X[:, i] = (re / d, im / d) with d = real(R[i, i]) -- two real divisions.  This differs from Julia's rdiv!, which divides complex by
 * complex (CholQR's factor has a real diagonal, src/lobpcg.jl:357-363,379): a diagonal entry whose imaginary part is not +-0 is
 * MIK_ERR_INVALID with a message naming the column, checked before anything is launched.  A lane works through its row in panels of 8
 * columns and re-reads the finished columns before each later panel; the result does not depend on the panel width.
 * Asynchronous on the ctx stream. */
int mik_block_rdiv(mik_ctx *ctx, int dtype, int64_t n, int s, const void *R, int64_t ldr, void *X, int64_t ldx);
/* The Ritz update of one block triple -- the body of update_X_P!, :629-690.  X: n x sx, R: n x b1, P: n x b2, V: HOST (sx + b1 + b2) x sx,
 * the eigenvector rows [Vx; Vr; Vp].  With rot(W, F) exactly the definition of mik_basis_rotate:
 *   b1 > 0:  Pout = rot(R, Vr);   b2 > 0:  Pout = Pout + rot(P, Vp);   Xout = rot(X, Vx) + Pout   (b1 == 0: Xout = rot(X, Vx))
 * With b1 == 0 Pout is not written (and b2 must be 0).  0 <= b1, b2 <= sx <= 32, else MIK_ERR_NOTIMPL.  One pass: X, R and P are read
 * once, Xout (n x sx) and Pout (n x sx) written once.  No output may overlap an input or the other output (MIK_ERR_INVALID).
 * Complex: rot opens a sum with the complex product W[row, 0] * F[0, jj] and adds W[row, c] * F[c, jj] componentwise, c ascending; V is a
 * host complex matrix.  The output columns run in panels (8 at ComplexF64, 16 at ComplexF32) and X, R and P are read once per panel.
 * Asynchronous on the ctx stream. */
int mik_block_update(mik_ctx *ctx, int dtype, int64_t n, int sx, int b1, int b2, const void *X, int64_t ldx, const void *R, int64_t ldr,
                     const void *P, int64_t ldp, const void *V, int64_t ldv, void *Xout, int64_t ldxo, void *Pout, int64_t ldpo);

/* ---- dense operator: mul!(y, A, x) and mul!(y, adjoint(A), x) for A::Matrix ---------------------------------------------------
 * The first operator of every solver testset of the reference (test/cg.jl:24-29, test/gmres.jl:16-17, ...).  Added without a version
 * bump (additive); real MIK_F64 / MIK_F32.  A is a DEVICE m x n column-major matrix with leading dimension lda >= m, read at every
 * product (the handle keeps no copy of it; A must outlive the handle).  No FMA, no matrix cores, no floating-point atomics: every
 * product and every sum is rounded on its own.
 *   y = A x    The columns are cut into chunks of C consecutive columns (mik_dense_mul_shape).  For row i and chunk c, p_c[i] is the
 *              serial sum from +0, over the chunk's columns ascending, of A[i,j] * x[j]; then y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ...,
 *              left to right.  With n <= C this is exactly the order of Julia's generic column-oriented mul!; with
 *              n <= min(C, mik_spmv_long_row()) it is also the order of mik_spmv on the same matrix stored fully.  The result depends on
 *              (m, n, dtype, C) only -- never on the machine, the launch shape, lda or pointer alignment.  n = 0 gives y = +0 (a row of
 *              -0.0 products therefore gives +0.0); NaN and Inf propagate as IEEE has them.
 *   y = A' x   y[j] equals mik_dot(A[:, j], x) bit for bit: the fixed two-level tree of mik_reduce_shape over m elements ("Reduction
 *              semantics"), through the same finaliser.  The scaled-norm machinery is not involved.
 * N form: rows across lanes (a lane owns 2 fp64 / 4 fp32 consecutive rows per 16-byte load; a scalar-load variant with identical
 * results when a column start is not 16-byte aligned), x[j] broadcast through a scalar load, chunks of the same rows in different
 * workgroups, the chunk partials combined in chunk order by a second small kernel.  T form: one sweep that reads every column once and
 * x once per workgroup pass, the segment sums through the segment toolkit and k_finalize_store.  No workgroup waits for another.
 * The handle owns the workspace of the chunk partials / segment sums (allocated once in create; nothing is allocated per call) and never
 * touches the context's reduction workspace, so the callbacks below may run in the middle of a fused CG / GMRES step.
 *
 * Complex matrices (MIK_C64 / MIK_C32; added without a version bump, additive) -- Matrix{ComplexF64 / ComplexF32} of test/cg.jl:27,
 * test/gmres.jl:16.  A is a DEVICE m x n column-major matrix of interleaved (re, im) elements; lda counts ELEMENTS; A, x and y need
 * element alignment only (8 bytes for ComplexF32 and likewise 8 bytes for a ComplexF64 base).  mik_dense_mul, mik_dense_mul_fn and
 * mik_dense_mul_adj_fn work on such a handle with the element arithmetic of the complex L1 entries; nothing is contracted.
 *   y = A x    The same chunks of C ELEMENTS (one constant for all four element types).  p_c[i] is the serial sum from (+0, +0), over the
 *              chunk's columns ascending, of the rounded product A[i,j] * x[j] = (ar xr - ai xi) + (ar xi + ai xr) i -- re and im each
 *              their own chain -- then y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ... componentwise.  With n <= C this is Julia's generic
 *              column-oriented mul!; with n <= min(C, mik_spmv_long_row()) it is mik_spmv on the same matrix stored fully, bit for bit.
 *              The result depends on (m, n, dtype, C) only.
 *   y = A' x   The conjugate transpose: y[j] equals the complex mik_dot(A[:, j], x) bit for bit -- per element re = ar xr + ai xi,
 *              im = ar xi - ai xr, then one two-level tree of mik_reduce_shape(dtype) for re and one for im, through the same finaliser.
 * Overlap, NULL and empty-dimension rules are those of the real codes (an empty sum is (+0, +0)).  mik_dense_mm and
 * mik_dense_block_reserve answer a complex handle with MIK_ERR_NOTIMPL and a message that names the element type; a complex matrix of
 * 2^30 columns or more is refused by mik_dense_create (MIK_ERR_NOTIMPL). */
typedef struct mik_dense mik_dense;     /* opaque: (ctx, dtype, m, n, A, lda) + its own workspace */
/* C (one compile-time constant for both dtypes, a power of two in [32, 256]) and the rows a workgroup of the N form owns. */
int mik_dense_mul_shape(int *chunk, int *rows_per_workgroup);
/* The same for any of the four element types: C is the same constant for all of them; the complex N form owns its own number of rows per
 * workgroup.  MIK_F64 / MIK_F32 give what mik_dense_mul_shape gives.  MIK_ERR_INVALID for another code. */
int mik_dense_mul_shape_for(int dtype, int *chunk, int *rows_per_workgroup);
/* MIK_ERR_MISMATCH for lda < m; MIK_ERR_INVALID for a NULL argument; m = 0 or n = 0 is MIK_OK. */
int mik_dense_create(mik_ctx *ctx, int dtype, int64_t m, int64_t n, const void *A, int64_t lda, mik_dense **out);
int mik_dense_destroy(mik_dense *D);
/* adjoint = 0: mul!(y, A, x) -- LinearAlgebra's generic mul! for a Matrix, called at src/cg.jl:54,137; src/gmres.jl:245,287.
 * adjoint = 1: mul!(y, adjoint(A), x) -- src/lsqr.jl:132,172; src/lsmr.jl:118,172; src/qmr.jl:76; src/svdl.jl:565.
 * x, y: DEVICE vectors of n and m (adjoint: m and n) elements.  MIK_ERR_INVALID when x and y overlap or y overlaps A.
 * Asynchronous on the ctx stream. */
int mik_dense_mul(mik_dense *D, int adjoint, const void *x, void *y);
/* The same as mik_mul_fn callbacks (user = the mik_dense handle): a host fills mik_operator{dtype, n, NULL, mik_dense_mul_fn, handle} and
 * calls mik_cg_create_op / mik_gmres_create_op -- the whole solve then runs inside the library, no host-language frame per product. */
int mik_dense_mul_fn(void *user, const void *x, void *y);         /* y = A x  -- src/cg.jl:54,137; src/gmres.jl:245,287 */
int mik_dense_mul_adj_fn(void *user, const void *x, void *y);     /* y = A' x -- src/lsqr.jl:132,172; src/lsmr.jl:118,172; src/qmr.jl:76; src/svdl.jl:565 */
/* Block product: Y[:, j] = A * X[:, j] for j < b -- mul!(AX, A, X) of src/lobpcg.jl:124-139 for A::Matrix.  X: DEVICE n x b, column-major,
 * ldx >= n; Y: DEVICE m x b, column-major, ldy >= m.  Column j of Y equals mik_dense_mul(D, 0, X[:, j], Y[:, j]) bit for bit: the chunked
 * order above, no FMA, no matrix cores, no atomics; the result depends on (m, n, dtype, C) only -- never on b, the group width, ldx / ldy,
 * alignment or the launch shape.  n = 0 gives +0 in every column.  The b columns run in groups of mik_dense_block_shape() columns, one
 * after another on the stream: A is read once per group, every loaded element multiplied into the accumulators of all columns of the group;
 * the chunk partials of ONE group go to the handle's block workspace, laid out [column of the group][chunk][m rounded up to whole
 * workgroups], and one combine launch per group sums them in chunk order.  With n <= C the product kernel writes Y itself.  A last group
 * narrower than the library's threshold runs column by column through the kernels of mik_dense_mul.
 * MIK_ERR_INVALID for b < 0, a NULL block with a non-empty extent, Y overlapping X or A; MIK_ERR_NOTIMPL for b > 32; MIK_ERR_MISMATCH for
 * ldx < n or ldy < m; b = 0 or m = 0 is MIK_OK and launches nothing.  Asynchronous on the ctx stream; no workgroup waits for another. */
int mik_dense_mm(mik_dense *D, int b, const void *X, int64_t ldx, void *Y, int64_t ldy);
/* Allocate the block workspace of mik_dense_mm (group width x chunks x padded rows elements; nothing when n <= C).  Idempotent.
 * mik_dense_mm calls it on first use; a host calls it when it builds an iterator, so that nothing is allocated inside an iteration loop.
 * A second allocation: it never replaces or frees the workspace of mik_dense_mul.  mik_dense_destroy frees it. */
int mik_dense_block_reserve(mik_dense *D);
/* The group width: the right-hand sides that share one read of A. */
int mik_dense_block_shape(int *group_width);

/* ---- measurement -------------------------------------------------------------------------- */
/* Time `reps` back-to-back launches of the SpMV (optionally with the fused dot epilogue used by
 * the CG step) with HIP events on the ctx stream; returns average milliseconds per launch. */
int mik_time_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y, int fused_dot, int reps,
                  double *avg_ms);
/* In-loop timing of the SpMV launch inside mik_cg_iterate / mik_cg_iterate_many: a HIP event pair
 * on the ctx stream brackets every SpMV launch of the CG step.  First reports the totals gathered
 * so far (either pointer may be NULL), then: enable = 1 (or 2, see below) resets the totals and switches timing on,
 * 0 switches it off, -1 leaves the mode unchanged. */
int mik_cg_profile(mik_cg *it, int enable, double *spmv_ms_total, int64_t *spmv_launches);
/* enable = 2 in mik_cg_profile brackets all three streaming launches of the step; totals per kernel:
 * [0] the SpMV (src/cg.jl:54), [1] u .= r .+ beta .* u (:51), [2] x / r update + |r|^2 (:58-62).  ms_total / launches: 3 entries each. */
int mik_cg_profile_kernels(const mik_cg *it, double *ms_total, int64_t *launches);
/* The same bracket around every SpMV launch of the row-partitioned iterable's steps (mik_cgd_iterate_many, mik_cgd_phase): the in-loop
 * SpMV time of a rank of BASELINE.json configs[3] (bench.py --gpus N: `roofline`).  Same protocol as mik_cg_profile (enable 1 / 0 / -1). */
int mik_cgd_profile(mik_cgd *it, int enable, double *spmv_ms_total, int64_t *spmv_launches);

#ifdef __cplusplus
}
#endif
#endif /* MIK_H */
