// mik_complex.h -- the complex element types (MIK_C64 / MIK_C32: interleaved re, im) behind the L1 / L2 entries that cg and gmres
// on a CSR operator need.  The entries of include/mik.h forward here when they see a complex code; everything
// else of the library keeps refusing it.  Kernels: csrc/mik_complex.hip.
#pragma once
#include "mik_internal.h"

// z * w = (zr wr - zi wi) + (zr wi + zi wr) i: four rounded products, one rounded difference, one rounded sum (Base's definition)
template <typename R> struct CxVal { R re, im; };

template <typename R> __host__ __device__ __forceinline__ CxVal<R> cx_mul(R zr, R zi, R wr, R wi)
{
    const R a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
    return CxVal<R>{a - b, c + d};
}

// mik_csr_create with a complex dtype: host transpose + validation, the operator runs on its CSR arrays (rows longer than
// MIK_LONG_ROW entries are listed as wave segments).  on_device: the three arrays are device memory and are staged on the host.
int mik_c_csr_create(mik_ctx *ctx, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *ptr, const int64_t *idx,
                     const void *val, int index_base, int is_csc, bool on_device, mik_csr **out);
int mik_c_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y);
const char *mik_c_spmv_kernel_name(const mik_csr *A);
int64_t mik_c_stored_bytes(const mik_csr *A);
int mik_c_time_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y, int reps, double *avg_ms);

int mik_c_dot(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *y, void *out);
int mik_c_fill(mik_ctx *ctx, int dtype, int64_t n, const void *value, void *x);
// scalar: a host complex of `dtype` (the real-scalar forms are the real sweeps over 2 n and never come here)
int mik_c_axpy(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, const void *x, void *y);
int mik_c_xpby(mik_ctx *ctx, int dtype, int64_t n, const void *x, const void *beta, void *y);
int mik_c_scal(mik_ctx *ctx, int dtype, int64_t n, const void *alpha, void *x);
int mik_c_orthogonalize(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *w, void *h, void *nrm, int method);
int mik_c_gemv_n(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *c, const void *alpha, void *y);
// what bicgstabl, minres and chebyshev stand on; h, M, gamma, out: host memory
int mik_c_gemv_t(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *w, void *h);
int mik_c_gram(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *M);
// x != NULL or z != NULL; real_alpha needs z != NULL (the other forms are the real entry over 2 n and never come here)
int mik_c_axpy_dot(mik_ctx *ctx, int dtype, int64_t n, int real_alpha, const void *alpha, const void *x, void *y, const void *z, void *out);
int mik_c_minres_update(mik_ctx *ctx, int dtype, int64_t n, const void *inv_h3, void *v_next, const void *v_curr, const void *neg_h1, const void *w_curr,
                        const void *neg_h0, const void *w_prev, const void *inv_h2, void *w_next, const void *rhs0, void *x);
int mik_c_bicgstab_mr_update(mik_ctx *ctx, int dtype, int64_t n, int l, void *us, int64_t ldu, void *rs, int64_t ldr, void *x, const void *gamma, void *out);
// host
int mik_c_lu_solve(int dtype, void *A, int64_t lda, int n, void *b);
int mik_c_givens(int dtype, const void *f, const void *g, void *out);
int mik_c_hessenberg_ldiv(int dtype, void *H, int64_t ldh, int width, void *rhs);

#ifdef __HIPCC__
#include "mik_kernels.h"

// What the complex kernels of csrc/mik_complex.hip and the complex block kernels of csrc/mik_lobpcg_complex.h share.
// The thread's share of dot(a, b) = sum conj(a_i) b_i over one segment held in registers: the products, the order (l ascending, then the
// elements of a 16-byte group) and the two accumulators of OpCDot.
template <typename R>
__device__ __forceinline__ void cseg_dot(const R (&a)[SEG_REGS<R>], const R (&b)[SEG_REGS<R>], int64_t base, int64_t n2, R &re, R &im)
{
    constexpr int W = VT<R>::W;
    R a0 = R(0), a1 = R(0);
#pragma unroll
    for (int l = 0; l < MIK_RED_L; ++l)
#pragma unroll
        for (int e = 0; e < W; e += 2) {
            const int q = l * W + e;
            if (base + (int64_t)l * MIK_BLOCK * W + e < n2) {
                const R p = a[q] * b[q], r = a[q + 1] * b[q + 1], s = a[q] * b[q + 1], t = a[q + 1] * b[q];
                const R vr = p + r, vi = s - t;
                a0 = a0 + vr;
                a1 = a1 + vi;
            }
        }
    re = a0;
    im = a1;
}

// level 2 of `cols` reductions whose segment sums sit in ctx->partials as [cols][nseg] -> out_dev[0 .. cols)
template <typename R> static inline int c_finalize(mik_ctx *ctx, int64_t nseg, int cols, R *out_dev)
{
    hipLaunchKernelGGL((k_finalize_store<R>), dim3(cols), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const R *)ctx->partials, nseg, nseg, out_dev,
                       (const int *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}
#endif  // __HIPCC__
