// mik_stationary_complex.h -- the kernels of csrc/mik_stationary.h for ComplexF64 / ComplexF32 operators (interleaved re, im; R is the
// component type).  The shape is the real kernels': ONE lane owns ONE row and sums it serially in the reference's order, 256 lanes per
// workgroup, a wide level is one launch, a run of narrow levels one workgroup with a fence and a barrier between levels.
//
// Element operations, in Julia's promotion order: every product is cx_mul (four rounded products, one difference,
// one sum), every add / subtract is componentwise, every division is cx_div (csrc/mik_complex.h); no FMA apart from the two inside the
// widened 32-bit division.  The relaxed substitutions evaluate in E = the real type of promote(real(T), typeof(omega)): alpha is a REAL
// of E (a real x complex product: alpha re, alpha im), beta = one(T) - omega a COMPLEX of E.
//
// An element is loaded and stored as one 16-byte (ComplexF64) or 8-byte (ComplexF32) access: always for the handle's own arrays, and for
// the caller's vectors when every one of them is aligned to its element (vec != 0; the rule k_spmv_complex has for x), else per component.
#pragma once
#include "mik_complex.h"
#include "mik_stationary.h"

template <typename R> struct CstPair { using type = float2; };
template <> struct CstPair<double> { using type = double2; };

template <typename R> __device__ __forceinline__ CxVal<R> cst_ldv(const R *p, int64_t i)
{
    const typename CstPair<R>::type v = *reinterpret_cast<const typename CstPair<R>::type *>(p + 2 * i);
    return CxVal<R>{v.x, v.y};
}
template <typename R> __device__ __forceinline__ CxVal<R> cst_ld(const R *p, int64_t i, int vec)
{
    if (vec) return cst_ldv(p, i);
    return CxVal<R>{p[2 * i], p[2 * i + 1]};
}
template <typename R> __device__ __forceinline__ void cst_st(R *p, int64_t i, int vec, CxVal<R> v)
{
    if (vec) {
        typename CstPair<R>::type w;
        w.x = v.re; w.y = v.im;
        *reinterpret_cast<typename CstPair<R>::type *>(p + 2 * i) = w;
    } else { p[2 * i] = v.re; p[2 * i + 1] = v.im; }
}
// acc += A[i,j] * (alpha * x[j]): the two products of the reference's column loop, then one rounded add per component
template <typename R> __device__ __forceinline__ void cst_term(CxVal<R> a, R alr, R ali, CxVal<R> xj, CxVal<R> &acc)
{
    const CxVal<R> ax = cx_mul(alr, ali, xj.re, xj.im);
    const CxVal<R> t = cx_mul(a.re, a.im, ax.re, ax.im);
    acc.re = acc.re + t.re;
    acc.im = acc.im + t.im;
}

// ldiv!(y, D, x): y[i] = x[i] / A[i,i]                                                                  -- src/stationary_sparse.jl:30-35
template <typename R>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_cst_diag_ldiv(int n, const R *__restrict__ d, const R *x, R *y, int vec)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const CxVal<R> xi = cst_ld(x, i, vec), di = cst_ldv(d, i);
    cst_st(y, i, vec, cx_div(xi.re, xi.im, di.re, di.im));
}

// mul!(alpha, O, x, beta, y), bmode as k_st_offdiag (0: fill!, 1: untouched, 2: lmul!(beta, y))                              -- :148-171
template <typename R>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_cst_offdiag(int n, const int *__restrict__ rp, const int *__restrict__ cl, const R *__restrict__ vl,
                                                              const int *__restrict__ dg, R alr, R ali, const R *__restrict__ x, R ber, R bei, int bmode,
                                                              R *y, int vec)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    CxVal<R> acc{R(0), R(0)};
    if (bmode) {
        acc = cst_ld(y, i, vec);
        if (bmode == 2) acc = cx_mul(ber, bei, acc.re, acc.im);
    }
    const int dk = dg[i], k1 = rp[i + 1];
    for (int k = rp[i]; k < k1; ++k) {
        if (k == dk) continue;
        cst_term(cst_ldv(vl, k), alr, ali, cst_ld(x, cl[k], vec), acc);
    }
    cst_st(y, i, vec, acc);
}

// gauss_seidel_multiply!(alpha, U|L, x, beta, y, z): j > i ascending (U, :178-191) or j < i DESCENDING (L, :196-208); x is the OLD vector
template <typename R, bool UPPER>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_cst_gs_mul(int n, const int *__restrict__ rp, const int *__restrict__ cl, const R *__restrict__ vl,
                                                             const int *__restrict__ dg, R alr, R ali, const R *__restrict__ x, R ber, R bei,
                                                             const R *__restrict__ y, R *__restrict__ z, int vec)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const CxVal<R> yi = cst_ld(y, i, vec);
    CxVal<R> acc = cx_mul(ber, bei, yi.re, yi.im);
    if (UPPER) {
        for (int k = dg[i] + 1, k1 = rp[i + 1]; k < k1; ++k) cst_term(cst_ldv(vl, k), alr, ali, cst_ld(x, cl[k], vec), acc);
    } else {
        for (int k = dg[i] - 1, k0 = rp[i]; k >= k0; --k) cst_term(cst_ldv(vl, k), alr, ali, cst_ld(x, cl[k], vec), acc);
    }
    cst_st(z, i, vec, acc);
}

// One row of a triangular sweep, as st_tri_row:
//   plain:   x[i] -= A[i,j] * x[j] ...;  x[i] = x[i] / d                                       (all in R)
//   relaxed: the subtractions in R, then x[i] = R((alpha * E(x[i])) / E(d) + beta * E(y[i])), one rounding per component at the store
template <typename R, typename E, bool RELAX>
__device__ __forceinline__ void cst_tri_row(int p, const int *__restrict__ perm, const int *__restrict__ tp, const int *__restrict__ tc,
                                            const R *__restrict__ tv, const R *__restrict__ d, E alpha, R *x, E ber, E bei, const R *__restrict__ y, int vec)
{
    const int i = perm[p];
    CxVal<R> acc = cst_ld(x, i, vec);
    for (int k = tp[p], k1 = tp[p + 1]; k < k1; ++k) {
        const CxVal<R> a = cst_ldv(tv, k), xj = cst_ld(x, tc[k], vec);
        const CxVal<R> t = cx_mul(a.re, a.im, xj.re, xj.im);
        acc.re = acc.re - t.re;
        acc.im = acc.im - t.im;
    }
    const CxVal<R> di = cst_ldv(d, i);
    if (RELAX) {
        const E ar = alpha * (E)acc.re, ai = alpha * (E)acc.im;
        const CxVal<E> q = cx_div(ar, ai, (E)di.re, (E)di.im);
        const CxVal<R> yi = cst_ld(y, i, vec);
        const CxVal<E> r = cx_mul(ber, bei, (E)yi.re, (E)yi.im);
        cst_st(x, i, vec, CxVal<R>{(R)(q.re + r.re), (R)(q.im + r.im)});
    } else {
        cst_st(x, i, vec, cx_div(acc.re, acc.im, di.re, di.im));
    }
}

// one wide level: level-order positions [p0, p1), one row per lane
template <typename R, typename E, bool RELAX>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_cst_tri_level(int p0, int p1, const int *__restrict__ perm, const int *__restrict__ tp,
                                                                const int *__restrict__ tc, const R *__restrict__ tv, const R *__restrict__ d,
                                                                E alpha, R *x, E ber, E bei, const R *__restrict__ y, int vec)
{
    const int p = p0 + blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (p < p1) cst_tri_row<R, E, RELAX>(p, perm, tp, tc, tv, d, alpha, x, ber, bei, y, vec);
}

// a run of narrow levels [l0, l1) in ONE workgroup, as k_st_tri_run: an agent-scope fence and a workgroup barrier between levels
template <typename R, typename E, bool RELAX>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_cst_tri_run(int l0, int l1, const int *__restrict__ lev, const int *__restrict__ perm,
                                                              const int *__restrict__ tp, const int *__restrict__ tc, const R *__restrict__ tv,
                                                              const R *__restrict__ d, E alpha, R *x, E ber, E bei, const R *__restrict__ y, int vec)
{
    for (int l = l0; l < l1; ++l) {
        const int p1 = lev[l + 1];
        for (int p = lev[l] + (int)threadIdx.x; p < p1; p += MIK_ST_BLOCK) cst_tri_row<R, E, RELAX>(p, perm, tp, tc, tv, d, alpha, x, ber, bei, y, vec);
        __threadfence();
        __syncthreads();
    }
}
