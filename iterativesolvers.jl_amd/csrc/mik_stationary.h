// mik_stationary.h -- device kernels of the stationary methods (src/stationary_sparse.jl): the row-parallel sweeps and the
// level-scheduled triangular sweeps behind mik_diag_ldiv / mik_offdiag_mul / mik_gs_multiply / mik_forward_sub / mik_backward_sub.
//
// Every kernel gives ONE lane ONE row and sums that row serially, term by term, in the order in which the reference's CSC column
// loop reaches the row (include/mik.h, "Stationary methods"); no wave tree, no FMA (the library is built -ffp-contract=off).
#pragma once
#include "mik_internal.h"

constexpr int MIK_ST_BLOCK = 256;          // lanes per workgroup of every stationary kernel
constexpr int MIK_ST_NARROW = 256;         // a level with at most this many rows is "narrow": runs of them share one one-workgroup launch

// ldiv!(y, D, x): y[i] = x[i] / A[i,i]                                                                  -- src/stationary_sparse.jl:30-35
template <typename T>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_st_diag_ldiv(int n, const T *__restrict__ d, const T *x, T *y)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i < n) y[i] = x[i] / d[i];
}

// mul!(alpha, O, x, beta, y): y[i] = {0 | y[i] | beta*y[i]}, then += A[i,j] * (alpha*x[j]) over j != i ascending    -- :148-171
// bmode 0: beta == 0 (fill!), 1: beta == 1 (untouched), 2: lmul!(beta, y)
template <typename T>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_st_offdiag(int n, const int *__restrict__ rp, const int *__restrict__ cl, const T *__restrict__ vl,
                                                             const int *__restrict__ dg, T alpha, const T *__restrict__ x, T beta, int bmode, T *y)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    T acc = bmode == 0 ? T(0) : (bmode == 1 ? y[i] : beta * y[i]);
    const int dk = dg[i], k1 = rp[i + 1];
    for (int k = rp[i]; k < k1; ++k) {
        if (k == dk) continue;
        const T ax = alpha * x[cl[k]];
        const T t = vl[k] * ax;
        acc = acc + t;
    }
    y[i] = acc;
}

// gauss_seidel_multiply!(alpha, U|L, x, beta, y, z): z[i] = beta*y[i], then += A[i,j] * (alpha*x[j]) over j > i ascending (U, :178-191)
// or over j < i DESCENDING (L, :196-208).  x is the OLD vector throughout (the caller passes a copy when z aliases x).
template <typename T, bool UPPER>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_st_gs_mul(int n, const int *__restrict__ rp, const int *__restrict__ cl, const T *__restrict__ vl,
                                                            const int *__restrict__ dg, T alpha, const T *__restrict__ x, T beta,
                                                            const T *__restrict__ y, T *__restrict__ z)
{
    const int i = blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (i >= n) return;
    T acc = beta * y[i];
    if (UPPER) {
        for (int k = dg[i] + 1, k1 = rp[i + 1]; k < k1; ++k) { const T ax = alpha * x[cl[k]]; const T t = vl[k] * ax; acc = acc + t; }
    } else {
        for (int k = dg[i] - 1, k0 = rp[i]; k >= k0; --k) { const T ax = alpha * x[cl[k]]; const T t = vl[k] * ax; acc = acc + t; }
    }
    z[i] = acc;
}

// One row of a triangular sweep (forward_sub! :67-103 / backward_sub! :109-142): the row's strict-triangle entries are stored in
// the order the row receives them (ascending j forward, descending j backward); every x[j] read was finalised at an earlier level.
//   plain:   x[i] -= A[i,j] * x[j] ...;  x[i] = x[i] / d
//   relaxed: the same, then x[i] = alpha * x[i] / d + beta * y[i], evaluated in S (double for Float32 data with a Float64 omega)
template <typename T, typename S, bool RELAX>
__device__ __forceinline__ void st_tri_row(int p, const int *__restrict__ perm, const int *__restrict__ tp, const int *__restrict__ tc,
                                           const T *__restrict__ tv, const T *__restrict__ d, S alpha, T *x, S beta, const T *__restrict__ y)
{
    const int i = perm[p];
    T acc = x[i];
    for (int k = tp[p], k1 = tp[p + 1]; k < k1; ++k) { const T t = tv[k] * x[tc[k]]; acc = acc - t; }
    if (RELAX) {
        const S a = alpha * (S)acc;
        const S q = a / (S)d[i];
        const S r = beta * (S)y[i];
        x[i] = (T)(q + r);
    } else {
        x[i] = acc / d[i];
    }
}

// one wide level: level-order positions [p0, p1), one row per lane
template <typename T, typename S, bool RELAX>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_st_tri_level(int p0, int p1, const int *__restrict__ perm, const int *__restrict__ tp,
                                                               const int *__restrict__ tc, const T *__restrict__ tv, const T *__restrict__ d,
                                                               S alpha, T *x, S beta, const T *__restrict__ y)
{
    const int p = p0 + blockIdx.x * MIK_ST_BLOCK + threadIdx.x;
    if (p < p1) st_tri_row<T, S, RELAX>(p, perm, tp, tc, tv, d, alpha, x, beta, y);
}

// a run of narrow levels [l0, l1) in ONE workgroup: level by level, an agent-scope fence and a workgroup barrier between levels (the
// rows of level l + 1 read what level l stored).  Only this one workgroup exists, so nothing waits on another workgroup.
template <typename T, typename S, bool RELAX>
__global__ void __launch_bounds__(MIK_ST_BLOCK) k_st_tri_run(int l0, int l1, const int *__restrict__ lev, const int *__restrict__ perm,
                                                             const int *__restrict__ tp, const int *__restrict__ tc, const T *__restrict__ tv,
                                                             const T *__restrict__ d, S alpha, T *x, S beta, const T *__restrict__ y)
{
    for (int l = l0; l < l1; ++l) {
        const int p1 = lev[l + 1];
        for (int p = lev[l] + (int)threadIdx.x; p < p1; p += MIK_ST_BLOCK) st_tri_row<T, S, RELAX>(p, perm, tp, tc, tv, d, alpha, x, beta, y);
        __threadfence();
        __syncthreads();
    }
}
