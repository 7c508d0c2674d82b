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

// z / w for finite operands and w != 0: Base's two methods, restated.  No contraction except the two fma of the
// widened form, which are explicit calls; tests/complex_ref/complex_stationary_ref.c restates exactly this.
//   64-bit components: the robust division of Baudin and Smith (Base's /(::ComplexF64, ::ComplexF64))
//   32-bit components: evaluated in double -- mag = 1 / fma(c, c, d d), re = fma(a, c, b d) mag, im = fma(b, c, -(a d)) mag -- and
//                      rounded to float once per component (Base's widened method)
__host__ __device__ __forceinline__ double cx_div2(double a, double b, double c, double d, double r, double t)
{
    if (r != 0.0) {
        const double br = b * r;
        if (br != 0.0) return (a + br) * t;
        const double at = a * t, bt = b * t;
        return at + bt * r;
    }
    const double bc = b / c;
    return (a + d * bc) * t;
}
__host__ __device__ __forceinline__ void cx_div1(double a, double b, double c, double d, double &p, double &q)
{
    const double r = d / c;
    const double t = 1.0 / (c + d * r);
    p = cx_div2(a, b, c, d, r, t);
    q = cx_div2(b, -a, c, d, r, t);
}
__host__ __device__ __forceinline__ CxVal<double> cx_div(double a, double b, double c, double d)
{
    constexpr double HALF_OV = 0x1.fffffffffffffp+1022;      // floatmax / 2
    constexpr double TWO_UN_EPS = 0x1p-969;                  // floatmin * 2 / eps
    constexpr double BS = 0x1p+105;                          // 2 / eps^2
    const double absa = a < 0.0 ? -a : a, absb = b < 0.0 ? -b : b, absc = c < 0.0 ? -c : c, absd = d < 0.0 ? -d : d;
    const double ab = absa >= absb ? absa : absb, cd = absc >= absd ? absc : absd;
    double s = 1.0;
    if (ab >= HALF_OV) { a = a * 0.5; b = b * 0.5; s = s * 2.0; }
    if (cd >= HALF_OV) { c = c * 0.5; d = d * 0.5; s = s * 0.5; }
    if (ab <= TWO_UN_EPS) { a = a * BS; b = b * BS; s = s / BS; }
    if (cd <= TWO_UN_EPS) { c = c * BS; d = d * BS; s = s * BS; }
    double p, q;
    if (absd <= absc) cx_div1(a, b, c, d, p, q);
    else { cx_div1(b, a, d, c, p, q); q = -q; }
    return CxVal<double>{p * s, q * s};
}
__host__ __device__ __forceinline__ CxVal<float> cx_div(float af, float bf, float cf, float df)
{
    const double a = (double)af, b = (double)bf, c = (double)cf, d = (double)df;
    const double dd = d * d, bd = b * d, ad = a * d;
    const double mag = 1.0 / __builtin_fma(c, c, dd);
    const double re = __builtin_fma(a, c, bd) * mag, im = __builtin_fma(b, c, -ad) * mag;
    return CxVal<float>{(float)re, (float)im};
}

// mik_csr_create with a complex dtype: host transpose + validation, the operator runs on its CSR arrays (rows longer than
// MIK_LONG_ROW entries are listed as wave segments).  on_device: the three arrays are device memory and are staged on the host.
int mik_c_csr_create(mik_ctx *ctx, int dtype, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *ptr, const int64_t *idx,
                     const void *val, int index_base, int is_csc, bool on_device, mik_csr **out);
int mik_c_spmv(mik_ctx *ctx, const mik_csr *A, const void *x, void *y);
const char *mik_c_spmv_kernel_name(const mik_csr *A);
int64_t mik_c_stored_bytes(const mik_csr *A);

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
// the QMR sweeps; scalars: host complex (real_scalars: host reals, only with z != NULL -- the other real-scalar forms
// are the real entries over 2 n and never come here).  out: one host complex, dot(z, y)
int mik_c_axpy2_dot(mik_ctx *ctx, int dtype, int64_t n, int real_scalars, const void *a, const void *x1, const void *b, const void *x2, void *y, const void *z,
                    void *out);
int mik_c_scal2(mik_ctx *ctx, int dtype, int64_t n, const void *a, void *x, const void *b, void *y);
int mik_c_qmr_update(mik_ctx *ctx, int dtype, int64_t n, const void *v, const void *neg_h1, const void *p_curr, const void *neg_h0, const void *p_prev,
                     const void *inv, const void *g, void *x, void *p_out);
// host
int mik_c_lu_solve(int dtype, void *A, int64_t lda, int n, void *b);
int mik_c_givens(int dtype, const void *f, const void *g, void *out);
int mik_c_hessenberg_ldiv(int dtype, void *H, int64_t ldh, int width, void *rhs);

#ifdef __HIPCC__
#include "mik_kernels.h"

// ---- the complex segment toolkit: what the kernels of csrc/mik_complex.hip, csrc/mik_dense_cmul.h and csrc/mik_lobpcg_complex.h share ----
// Element operations.  Each rounding sequence is written here once; the C checkers under tests/complex_ref/ restate exactly these.
// (a0 + a1 i) += conj(a) b: re = ar br + ai bi, im = ar bi - ai br, every product rounded, the two terms added, one accumulator each
template <typename R> __device__ __forceinline__ void cx_dot_acc(R ar, R ai, R br, R bi, R &a0, R &a1)
{
    const R p = ar * br, q = ai * bi, s = ar * bi, t = ai * br;
    const R re = p + q, im = s - t;
    a0 = a0 + re;
    a1 = a1 + im;
}
// a0 += v^2 for one real: the rounded square, then the rounded add
template <typename R> __device__ __forceinline__ void cx_sq_acc(R v, R &a0)
{
    const R p = v * v;
    a0 = a0 + p;
}
// a0 += yr^2, then yi^2: memory order into one accumulator -- the bits mik_nrm2 squares over the 2 n reals
template <typename R> __device__ __forceinline__ void cx_sumsq_acc(R yr, R yi, R &a0)
{
    cx_sq_acc(yr, a0);
    cx_sq_acc(yi, a0);
}
// y += t x and y -= h x: the rounded product (cx_mul), then one rounded add / subtract per component
template <typename R> __device__ __forceinline__ void cx_madd(R tr, R ti, R xr, R xi, R &yr, R &yi)
{
    const CxVal<R> p = cx_mul(tr, ti, xr, xi);
    yr = yr + p.re;
    yi = yi + p.im;
}
template <typename R> __device__ __forceinline__ void cx_msub(R hr, R hi, R xr, R xi, R &yr, R &yi)
{
    const CxVal<R> p = cx_mul(hr, hi, xr, xi);
    yr = yr - p.re;
    yi = yi - p.im;
}
// y += a x with a real a (real x complex: a xr, a xi)
template <typename R> __device__ __forceinline__ void cx_madd_real(R a, R xr, R xi, R &yr, R &yi)
{
    const R p = a * xr, q = a * xi;
    yr = yr + p;
    yi = yi + q;
}

// Operations on one segment held in registers (register q = 2 p: re, q = 2 p + 1: im of the thread's p-th element); the order is l
// ascending, then the elements of a 16-byte group.  The reducing forms skip the elements at or past n2; the others run over every register:
// lanes past n hold the zeros seg_load left and are never stored.
// the thread's share of dot(a, b) = sum conj(a_i) b_i
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
            if (base + (int64_t)l * MIK_BLOCK * W + e < n2) cx_dot_acc(a[q], a[q + 1], b[q], b[q + 1], a0, a1);
        }
    re = a0;
    im = a1;
}
// the thread's share of the sum of squares of a (every real guarded on its own)
template <typename R> __device__ __forceinline__ R cseg_sumsq(const R (&a)[SEG_REGS<R>], int64_t base, int64_t n2)
{
    constexpr int W = VT<R>::W;
    R acc = R(0);
#pragma unroll
    for (int l = 0; l < MIK_RED_L; ++l)
#pragma unroll
        for (int e = 0; e < W; ++e)
            if (base + (int64_t)l * MIK_BLOCK * W + e < n2) cx_sq_acc(a[l * W + e], acc);
    return acc;
}
// y += (tr + ti i) v
template <typename R> __device__ __forceinline__ void cseg_madd(R tr, R ti, const R (&v)[SEG_REGS<R>], R (&y)[SEG_REGS<R>])
{
#pragma unroll
    for (int q = 0; q < SEG_REGS<R>; q += 2) cx_madd(tr, ti, v[q], v[q + 1], y[q], y[q + 1]);
}
// w = w (cr + ci i)
template <typename R> __device__ __forceinline__ void cseg_scale(R (&w)[SEG_REGS<R>], R cr, R ci)
{
#pragma unroll
    for (int q = 0; q < SEG_REGS<R>; q += 2) {
        const CxVal<R> p = cx_mul(w[q], w[q + 1], cr, ci);
        w[q] = p.re;
        w[q + 1] = p.im;
    }
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
