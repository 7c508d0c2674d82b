// mik_dense_stationary.h -- device kernels of the dense stationary methods (src/stationary.jl:31-263) on a column-major device matrix.
//
// The reference's column loops give every row ONE serial order of subtractions, acc = acc - (A[r,c] * x[c]) with the product and the
// difference rounded on their own (the library is built -ffp-contract=off).  A lane therefore owns a row and walks its columns in that
// order; a row's chain is never split, so a sweep has n-fold parallelism and no more.  The 64 lanes of a wave read 64 consecutive rows
// of one column (one coalesced line), x[c] is wave-uniform, and two batches of MIK_DS_U column loads are in flight per lane.  The walk
// (de_walk), the broadcast (ds_bcast) and the panel shape (MIK_DS_W, MIK_DS_R, MIK_DS_U) are those of csrc/mik_dense_elem.h, shared with
// the dense LU and Cholesky.
//   k_ds_row    row-owned sweep: Jacobi (:53-69), the upper phase of Gauss-Seidel / SOR / SSOR (:113-119, :172-178, :232-238), the
//               backward half of SSOR (:247-260)
//   k_ds_panel  one panel of the forward substitution (:121-126, :180-185, :240-245): subtract the previous panel's columns from the
//               rows at or below this panel, then solve this panel's diagonal block in the workgroup that owns it
//   k_ds_check_diag  check_diag (:6-12)
#pragma once
#include "mik_internal.h"
#include "mik_dense_elem.h"

// x + omega * (q - x) with Julia's types (:181, :241, :259): the inner difference in T, the product and the sum in S, one rounding at
// the store.  S is double for Float32 data with a Float64 omega, else T.
template <typename T, typename S>
__device__ __forceinline__ T ds_relax(T xo, T q, S omega)
{
    const T dq = q - xo;
    const S w = omega * (S)dq;
    return (T)((S)xo + w);
}

enum { MIK_DS_JACOBI = 0, MIK_DS_UPPER = 1, MIK_DS_BACKWARD = 2 };

// Row-owned sweep.  x is the vector every product reads and is not written here (the handle's copy of the old x where out aliases it).
//   JACOBI    acc = b[r] - sum over c != r ascending;                       acc_out[r] = acc; out[r] = acc / A[r,r]
//   UPPER     acc = b[r] - sum over c > r ascending;                        acc_out[r] = acc
//   BACKWARD  acc = b[r] - sum over c < r DESCENDING - sum over c > r DESCENDING;  acc_out[r] = acc; out[r] = relax(x[r], acc / A[r,r])
template <typename T, typename S, int MODE>
__global__ void __launch_bounds__(MIK_DS_R) k_ds_row(int n, const T *__restrict__ A, int64_t ld, const T *__restrict__ x, const T *__restrict__ b,
                                                     T *__restrict__ acc_out, T *__restrict__ out, S omega)
{
    const int r0 = (int)blockIdx.x * MIK_DS_R;
    const int r = r0 + (int)threadIdx.x;
    if (r >= n) return;
    const int r1 = min(r0 + MIK_DS_R, n);           // the columns [r0, r1) hold this wave's diagonal entries
    const T *Ar = A + r;
    T acc = b[r];
    if (MODE == MIK_DS_JACOBI) {
        acc = de_walk<T, true, MIK_DS_ALL>(acc, Ar, ld, x, 0, r0, r);
        acc = de_walk<T, true, MIK_DS_OFFDIAG>(acc, Ar, ld, x, r0, r1, r);
        acc = de_walk<T, true, MIK_DS_ALL>(acc, Ar, ld, x, r1, n, r);
        acc_out[r] = acc;
        out[r] = acc / Ar[(int64_t)r * ld];
    } else if (MODE == MIK_DS_UPPER) {
        acc = de_walk<T, true, MIK_DS_ABOVE>(acc, Ar, ld, x, r0, r1, r);
        acc = de_walk<T, true, MIK_DS_ALL>(acc, Ar, ld, x, r1, n, r);
        acc_out[r] = acc;
    } else {
        acc = de_walk<T, false, MIK_DS_BELOW>(acc, Ar, ld, x, r0, r1, r);
        acc = de_walk<T, false, MIK_DS_ALL>(acc, Ar, ld, x, 0, r0, r);
        acc = de_walk<T, false, MIK_DS_ALL>(acc, Ar, ld, x, r1, n, r);
        acc = de_walk<T, false, MIK_DS_ABOVE>(acc, Ar, ld, x, r0, r1, r);
        acc_out[r] = acc;
        out[r] = ds_relax<T, S>(x[r], acc / Ar[(int64_t)r * ld], omega);
    }
}

// Panel k0 / W of the forward substitution, launched over the rows [k0, n) in workgroups of R = W rows.  t holds every row's accumulator
// (after the upper phase: b[r] - sum over c > r); x holds the new values of the columns < k0 and the old values from k0 on.
//   every workgroup:   t-chain of its rows -= A[r, c] * x[c] over the previous panel's columns c in [k0 - W, k0), ascending
//   workgroup 0 only:  its rows are the diagonal block.  W serial steps j: x[k0 + j] = t / d (RELAX: relax(x_old, t / d)), broadcast,
//                      the rows below subtract A[r, k0 + j] * x[k0 + j].  t[r] keeps the accumulator the division read (the reference's tmp).
// No workgroup waits for another one; the launches of a sweep follow each other on the stream.
// The serial loop is de_step's with two additions -- the quotient is relaxed before it is broadcast, and t keeps the accumulator the
// division read -- which de_step could only take as a functor or a further template parameter, so the loop is written out here.
template <typename T, typename S, bool RELAX>
__global__ void __launch_bounds__(MIK_DS_R) k_ds_panel(int n, int k0, const T *__restrict__ A, int64_t ld, T *t, T *x, S omega)
{
    const int lane = (int)threadIdx.x;
    const int r = k0 + (int)blockIdx.x * MIK_DS_R + lane;
    const bool live = r < n;
    const T *Ar = A + (live ? r : k0);              // a dead lane reads row k0 (in bounds) and stores nothing
    T acc = live ? t[r] : T(0);
    if (k0 > 0) acc = de_walk<T, true, MIK_DS_ALL>(acc, Ar, ld, x, k0 - MIK_DS_W, k0, r);
    if (blockIdx.x != 0) {
        if (live) t[r] = acc;
        return;
    }
    const int m = min(MIK_DS_W, n - k0);            // steps of this diagonal block
    const T xo = live ? x[r] : T(0);
    const T d = live ? Ar[(int64_t)r * ld] : T(1);
    T mine = xo, tmine = acc;
    for (int j0 = 0; j0 < m; j0 += MIK_DS_U) {
        T a[MIK_DS_U];
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) a[q] = j0 + q < m ? Ar[(int64_t)(k0 + j0 + q) * ld] : T(0);
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) {
            const int j = j0 + q;
            if (j < m) {                            // wave-uniform
                const T quo = acc / d;
                const T xn = RELAX ? ds_relax<T, S>(xo, quo, omega) : quo;
                const T xj = ds_bcast(xn, j);
                if (lane == j) { mine = xn; tmine = acc; }
                const T p = a[q] * xj;
                const T s = acc - p;
                acc = lane > j ? s : acc;
            }
        }
    }
    if (live) { x[r] = mine; t[r] = tmine; }
}

// check_diag (:6-12): *first = the smallest i with iszero(A[i,i]) (-0.0 counts), left at its initial value n when there is none
template <typename T>
__global__ void __launch_bounds__(256) k_ds_check_diag(int n, const T *__restrict__ A, int64_t ld, int *first)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n && A[(int64_t)i * ld + i] == T(0)) atomicMin(first, i);
}
