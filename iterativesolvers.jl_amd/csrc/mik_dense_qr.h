// mik_dense_qr.h -- device kernels of qr!(A) (Householder, no pivoting), lmul!(Q, Y) / lmul!(Q', Y), F \ b and Matrix(F.Q) on a column-major
// m x n device matrix, m >= n, Float64 / Float32.
//
// THE BIT CONTRACT (restated as unblocked C99 loops in tests/dense_ref/dense_qr_ref.c).  No fma, no matrix cores, no reciprocal (the
// library is built -ffp-contract=off); `/` and sqrt are correctly rounded; a product and the sum or difference that takes it are rounded
// on their own.
//   reduction T  over a range of ABSOLUTE rows i: 256 accumulators, each starting at +0; accumulator i mod 256 takes acc = acc + p_i in
//                ascending i; each group of 64 accumulators is folded by the wave tree a[l] += a[l + s], s = 32, 16, 8, 4, 2, 1; the four
//                sums are added left to right.  The shape depends on the absolute row indices only -- never on n, the column, the panel
//                width, the number of right-hand sides or the launch geometry.
//   column j     alpha = A[j,j], s = T(A[i,j] * A[i,j]; j < i < m) (no row below j: s = 0).  s == 0: tau[j] = 0 and nothing is stored.
//                Otherwise nrm = sqrt(alpha * alpha + s), beta = -copysign(nrm, alpha), tau[j] = (beta - alpha) / beta, d = alpha - beta,
//                A[i,j] = A[i,j] / d for i > j (a true division per element), A[j,j] = beta.
//   reflector j  on a column a (a matrix column c > j, or a column of Y): skipped if tau[j] == 0 (H = I, as LAPACK does).  Otherwise, with
//                v_j = 1 and v_i = A[i,j]: w = T(v_i * a_i; j <= i < m), t = tau[j] * w, a_i = a_i - v_i * t for j <= i < m.  An element
//                meets its reflectors in ascending j in the factorisation and in Q' y, in descending j in Q y.
//   F \ b        t = Q' b on a copy of b, then R x = t[0:n] by the LU's upper chain: per row, descending columns, the division by R[i,i]
//                last (k_lu_bwd / k_lu_bwd_nb of csrc/mik_dense_lu.h, unchanged).  Column k of a block solve has the bits of the vector solve.
//   Matrix(F.Q)  Q applied to the first n columns of the m x m identity.
// RANGE: the sums of squares are not rescaled.  A column whose alpha^2 + s overflows, or underflows to a subnormal, follows the loops into
// Inf / 0 / reduced accuracy; safe scaling is not built.  Nothing indexes memory through a data value: non-finite input follows the loops
// and cannot fault.
//
// THE PLAN.  A workgroup is 256 lanes and lane t owns the rows i with i mod 256 == t of the column it works on, in every kernel: lane t's
// running sum IS accumulator t of T, a wave's shuffle tree is the fold of its 64 accumulators, and a lane only ever reads back elements of
// the column that it stored itself -- so a column needs no barrier between reflectors, only the one inside each reduction.  Rows are not
// split across workgroups: a column runs on one compute unit, and a tall matrix of very few columns therefore uses few of them.
//   k_qr_panel   launch j of a panel [k0, k1): workgroup b owns column j + b.  It applies reflector j - 1 (j > k0) to its column; workgroup
//                0 then forms reflector j from the column it has just updated.  One launch per column.
//   k_qr_apply   a workgroup owns one column and applies the reflectors [r0, r1) to it, ascending or descending.  The trailing update of
//                a panel (reflectors k0 ... k1 - 1, columns >= k1), lmul!(Q', Y) (0 ... n - 1), lmul!(Q, Y) (n - 1 ... 0), the solve and the
//                thin Q are this one kernel.  RESIDENT: the rows [r0, m) of the column stay in LDS from the first reflector to the last
//                (one load, one store); else they stream through global memory (a load and a store per reflector).  Same operations on
//                the same operands in the same order: same bits.
// A right-looking blocked plan gives the unblocked loop's bits because only the order in which ONE element meets its reflectors matters,
// and that stays ascending.  A compact-WY update would not: it changes the rounding.
#pragma once
#include "mik_internal.h"
#include "mik_dense_elem.h"

constexpr int MIK_QR_W = 32;                    // columns per panel
constexpr int MIK_QR_ACC = 256;                 // accumulators of T = lanes of a workgroup
constexpr int MIK_QR_LDS_BYTES = 63 * 1024;     // of a resident column: with the reduction's slots, within the 64 KB a launch gets without opting in
static_assert(MIK_QR_ACC == 256, "the four-wave fold is written for this size");

__device__ __forceinline__ double qr_copysign(double a, double b) { return __builtin_copysign(a, b); }
__device__ __forceinline__ float qr_copysign(float a, float b) { return __builtin_copysignf(a, b); }

// the first row >= lo that lane t owns
__device__ __forceinline__ int qr_first(int lo, int t) { return lo + ((t - lo) & (MIK_QR_ACC - 1)); }

// The fold of T: acc is this lane's accumulator; every lane receives the sum.  `red` is 2 x 4 slots and `par` alternates between them, so
// that one barrier per reduction is enough: a lane that still reads the slots of reduction k has passed the barrier of k, and the slots of
// k are not written again before reduction k + 2, behind the barrier of k + 1.
template <typename T>
__device__ __forceinline__ T qr_fold(T acc, T *red, int &par)
{
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) acc = acc + __shfl_down(acc, s, 64);       // lane l < s: a[l] + a[l + s]; lane 0 holds the wave's sum
    T *slot = red + 4 * par;
    par ^= 1;
    if ((t & 63) == 0) slot[t >> 6] = acc;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

// a column in global memory: row i at lo[i * rs] below `split`, at hi[(i - split) * rs] from there on (a plain column: split = m, rs = 1)
template <typename T> struct qr_col_global {
    T *lo, *hi;
    int split;
    int64_t rs;
    __device__ __forceinline__ T *at(int i) const { return i < split ? lo + (int64_t)i * rs : hi + (int64_t)(i - split) * rs; }
    __device__ __forceinline__ T get(int i) const { return *at(i); }
    __device__ __forceinline__ void set(int i, T v) const { *at(i) = v; }
};
// the rows [base, m) of a column in LDS
template <typename T> struct qr_col_lds {
    T *s;
    int base;
    __device__ __forceinline__ T get(int i) const { return s[i - base]; }
    __device__ __forceinline__ void set(int i, T v) const { s[i - base] = v; }
};

// reflector j (tau != 0) on the column a: v = its column of the factors, v[j] read as 1
template <typename T, typename Col>
__device__ __forceinline__ void qr_reflect(int m, int j, const T *__restrict__ v, T tau, const Col &a, T *red, int &par)
{
    const int i0 = qr_first(j, (int)threadIdx.x);
    T acc = T(0);
#pragma unroll 4
    for (int i = i0; i < m; i += MIK_QR_ACC) {
        const T vi = i == j ? T(1) : v[i];
        const T p = vi * a.get(i);
        acc = acc + p;
    }
    const T w = qr_fold(acc, red, par);
    const T t = tau * w;
#pragma unroll 4
    for (int i = i0; i < m; i += MIK_QR_ACC) {
        const T vi = i == j ? T(1) : v[i];
        const T p = vi * t;
        a.set(i, a.get(i) - p);
    }
}

// ---- launch j of the panel [k0, k1): grid k1 - j, workgroup b owns column j + b of A.  *zero_diag takes the smallest j with R[j,j] == 0.
template <typename T>
__global__ void __launch_bounds__(MIK_QR_ACC) k_qr_panel(int m, int j, int k0, T *A, int64_t ld, T *tau, int *zero_diag)
{
    __shared__ T red[8];
    __shared__ T salpha;
    int par = 0;
    const int t = (int)threadIdx.x;
    T *a = A + (int64_t)(j + (int)blockIdx.x) * ld;
    if (j > k0) {
        const T tp = tau[j - 1];
        if (tp != T(0)) qr_reflect(m, j - 1, (const T *)(A + (int64_t)(j - 1) * ld), tp, qr_col_global<T>{a, a, m, 1}, red, par);     // workgroup-uniform
    }
    if (blockIdx.x != 0) return;
    const int i0 = qr_first(j + 1, t);
    T acc = T(0);
#pragma unroll 4
    for (int i = i0; i < m; i += MIK_QR_ACC) {
        const T x = a[i];
        const T p = x * x;
        acc = acc + p;
    }
    if (t == (j & (MIK_QR_ACC - 1))) salpha = a[j];            // the lane that owns row j stored it, if anyone did
    const T s = qr_fold(acc, red, par);
    const T alpha = salpha;
    if (s == T(0)) {                                           // workgroup-uniform
        if (t == 0) {
            tau[j] = T(0);
            if (alpha == T(0)) atomicMin(zero_diag, j);
        }
        return;
    }
    const T pa = alpha * alpha;
    const T nrm = mik_sqrt(pa + s);
    const T beta = -qr_copysign(nrm, alpha);
    const T d = alpha - beta;
#pragma unroll 4
    for (int i = i0; i < m; i += MIK_QR_ACC) a[i] = a[i] / d;
    if (t == (j & (MIK_QR_ACC - 1))) a[j] = beta;
    if (t == 0) {
        tau[j] = (beta - alpha) / beta;
        if (beta == T(0)) atomicMin(zero_diag, j);
    }
}

// ---- the columns a launch of k_qr_apply works on: column c is member c % nb of group c / nb.  A plain column-major block: nb = 1,
// group = ld, split = m, rs = 1.  The workspace of a block solve (k_qr_stage_nb): the rows below n interleaved as k_lu_bwd_nb reads them.
template <typename T> struct qr_cols {
    T *base;
    int nb;
    int64_t group_lo, group_hi, hi_off, rs;
    int split;
    __device__ __forceinline__ qr_col_global<T> col(int c) const
    {
        const int g = c / nb, b = c - g * nb;
        return qr_col_global<T>{base + g * group_lo + b, base + hi_off + g * group_hi + b, split, rs};
    }
};

// ---- the reflectors [r0, r1) of the factors V on column blockIdx.x of Y, ascending or (DESC) descending.  RESIDENT: dynamic LDS of
// (m - r0) elements.
template <typename T, bool RESIDENT, bool DESC>
__global__ void __launch_bounds__(MIK_QR_ACC) k_qr_apply(int m, int r0, int r1, const T *__restrict__ V, int64_t ldv, const T *__restrict__ tau, qr_cols<T> Y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qr_lds[];
    __shared__ T red[8];
    int par = 0;
    const qr_col_global<T> g = Y.col((int)blockIdx.x);
    const qr_col_lds<T> l{(T *)qr_lds, r0};
    const int i0 = qr_first(r0, (int)threadIdx.x);
    if (RESIDENT) {
#pragma unroll 4
        for (int i = i0; i < m; i += MIK_QR_ACC) l.set(i, g.get(i));
    }
    for (int q = r0; q < r1; ++q) {
        const int j = DESC ? r1 - 1 - (q - r0) : q;
        const T tj = tau[j];
        if (tj == T(0)) continue;                              // workgroup-uniform
        if (RESIDENT) qr_reflect(m, j, V + (int64_t)j * ldv, tj, l, red, par);
        else qr_reflect(m, j, V + (int64_t)j * ldv, tj, g, red, par);
    }
    if (RESIDENT) {
#pragma unroll 4
        for (int i = i0; i < m; i += MIK_QR_ACC) g.set(i, l.get(i));
    }
}

// ---- a pass of a block solve into its workspace t (m x G elements): group blockIdx.y holds the columns [c0, c0 + NB) of B; the rows below n
// as k_lu_bwd_nb reads them (group c0 * n, row r at r * NB + b), the rows from n on behind them (at n * G: group c0 * (m - n), row r at
// (r - n) * NB + b).  A dead column carries a copy of the group's first column.
template <typename T, int NB>
__global__ void __launch_bounds__(256) k_qr_stage_nb(int m, int n, const T *__restrict__ B, int64_t ldb, int cols, T *__restrict__ t)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int c0 = de_group_first<NB>();
    if (i >= m) return;
    T *dst = i < n ? t + (int64_t)c0 * n + (int64_t)i * NB : t + (int64_t)n * MIK_DS_G + (int64_t)c0 * (m - n) + (int64_t)(i - n) * NB;
#pragma unroll
    for (int b = 0; b < NB; ++b) dst[b] = B[(int64_t)(de_col_live<NB>(c0, b, cols) ? c0 + b : c0) * ldb + i];
}

// Q[:, c] = column c of the m x m identity: workgroup blockIdx.x covers 256 rows of column blockIdx.x / rb, rb = ceil(m / 256)
template <typename T>
__global__ void __launch_bounds__(256) k_qr_eye(int m, int rb, T *__restrict__ Q, int64_t ldq)
{
    const int c = (int)(blockIdx.x / (unsigned)rb);
    const int i = (int)(blockIdx.x % (unsigned)rb) * 256 + (int)threadIdx.x;
    if (i < m) Q[(int64_t)c * ldq + i] = i == c ? T(1) : T(0);
}

// R[:, c] = the upper triangle's part of column c of the factors, +0 below the diagonal; the same grid over n rows
template <typename T>
__global__ void __launch_bounds__(256) k_qr_upper(int n, int rb, const T *__restrict__ A, int64_t ld, T *__restrict__ R, int64_t ldr)
{
    const int c = (int)(blockIdx.x / (unsigned)rb);
    const int i = (int)(blockIdx.x % (unsigned)rb) * 256 + (int)threadIdx.x;
    if (i < n) R[(int64_t)c * ldr + i] = i <= c ? A[(int64_t)c * ld + i] : T(0);
}
