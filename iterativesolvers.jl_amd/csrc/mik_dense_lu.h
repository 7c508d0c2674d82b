// mik_dense_lu.h -- device kernels of lu!(A) and ldiv!(y, F, x) on a square column-major device matrix.
//
// THE BIT CONTRACT.  The factors, the pivots and the solution are those of the loops of lu_solve<T> in csrc/mik_krylov.hip:
//   pivot       of column j: the FIRST row i >= j with the largest |A[i,j]| (strict >, LAPACK's idamax)
//   multiplier  A[i,j] / pivot -- a division, not a product with a reciprocal
//   element     (i,c) receives a = a - m * u for k = 0, 1, ..., min(i,c) - 1 in ASCENDING k; the product and the difference are
//               rounded on their own (the library is built -ffp-contract=off; no fma, no matrix cores)
//   ldiv!       the row interchanges go to x first; then per row the unit-lower chain in ascending column order; then per row the
//               upper chain in DESCENDING column order with the division by U[i,i] last
// Only the order within one element's (one row's) chain matters, so the blocked right-looking plan below -- panels of W columns, each
// element's k ascending inside a panel and panel after panel -- gives the same bits as the unblocked loop.
//
//   k_lu_search  per-workgroup (key, row) partials of max |A[r,j]| over the rows [j, n); lu_key  (first column of a panel only)
//   k_lu_pick    ONE workgroup: combine the partials (larger value, else smaller row), record ipiv[j] and a zero pivot, interchange
//                the rows j and p inside the panel
//   k_lu_update  a lane owns a row r > j: m = A[r,j] / pivot, A[r,c] -= m * A[j,c] for the panel columns c > j, and the partials of
//                the search of column j + 1 from the values it has just stored
//   k_lu_swap    the panel's interchanges on the columns left and right of it: a lane owns a column and applies them in order, in LDS
//   k_lu_strip   U12 = L11^-1 A12: a lane owns a column, its W values in registers, L11 in LDS, k ascending
//   k_lu_gather  w[i] = x[perm[i]]: the interchanges of ldiv!
//   k_lu_bwd     one panel of the backward substitution
//   k_lu_gather_nb, k_lu_bwd_nb   the two for a block of right-hand sides, NB per lane (ldiv!(Y, F, X)): per column the same operations
//                on the same operands in the same order, so column j has the bits of the vector solve of column j
// and, from csrc/mik_dense_elem.h, where the pieces the dense kernels share are written once (the walk de_walk, the serial step de_step):
//   k_dense_trail<T, false>  A22[i,c] -= L21[i,k] * U12[k,c], k ascending: TR x TC tiles, L21 and U12 tiles in LDS, a 4 x 4 register block per lane
//   k_dense_fwd<T, true>     one panel of the forward substitution with the unit-lower factor (k_dense_fwd_nb<T, true, NB>: for a block)
// Every dependency between workgroups is a kernel boundary; nothing indexes memory through a DATA value (ipiv is clamped to [j, n)
// where it is produced), so a singular or non-finite matrix cannot fault.  Non-finite data follow the loop too: the pivot search treats a
// NaN as the loop's comparisons do (lu_key), and everything else is the same operations on the same operands in the same order.
#pragma once
#include "mik_internal.h"
#include "mik_dense_elem.h"

#include <climits>

constexpr int MIK_LU_W = MIK_DS_W;      // panel width: the substitution panels are the factorisation's
constexpr int MIK_LU_R = 256;           // rows per workgroup of the pivot search and of the panel update
constexpr int MIK_LU_TR = MIK_DS_T;     // tile rows of the trailing update
constexpr int MIK_LU_TC = MIK_DS_T;     // tile columns of the trailing update
static_assert(MIK_LU_W == 64, "k_lu_swap and k_lu_strip are written for this size");

// What the row of the value a = |A[r,j]| offers to the search of column j.  The loop starts with best = |A[j,j]| and replaces it only by a
// strictly larger value, so a NaN in the FIRST searched row is never replaced (the pivot stays in row j, and best, a NaN, is not zero),
// while a NaN in any other row never replaces anything.  A compare-and-keep tree cannot hold a NaN for that: the lane that holds it would
// also refuse every candidate folded into it and hide them from the lanes above.  So no NaN enters the tree.  The first row's becomes
// +Inf -- it wins, also against a real Inf further down (same value, smaller row), and is not zero; any other becomes -1, below every
// magnitude, like a dead lane.  The keys only choose the row and raise the zero-pivot flag; no key is ever stored into the matrix.
template <typename T> __device__ __forceinline__ T lu_key(T a, bool first) { return a != a ? (first ? T(INFINITY) : T(-1)) : a; }

// b replaces a: a larger key, else the same key in a smaller row -- the loop's "first of the largest".  Keys are never NaN (lu_key).
template <typename T> __device__ __forceinline__ bool lu_better(T vb, int rb, T va, int ra) { return vb > va || (vb == va && rb < ra); }

// (key, row) of the workgroup's best candidate, valid in thread 0.  A dead lane offers (-1, INT_MAX): it loses to every live lane, since a
// live lane's key is >= 0 or, at -1, comes with a smaller row.
template <typename T>
__device__ __forceinline__ void lu_block_best(T &v, int &row, T *sval, int *srow)
{
    const int t = (int)threadIdx.x;
    sval[t] = v;
    srow[t] = row;
    __syncthreads();
    for (int s = MIK_LU_R / 2; s > 0; s >>= 1) {
        if (t < s && lu_better(sval[t + s], srow[t + s], sval[t], srow[t])) { sval[t] = sval[t + s]; srow[t] = srow[t + s]; }
        __syncthreads();
    }
    v = sval[0];
    row = srow[0];
}

template <typename T>
__global__ void __launch_bounds__(MIK_LU_R) k_lu_search(int n, int j, const T *__restrict__ A, int64_t ld, T *__restrict__ pval, int *__restrict__ prow)
{
    __shared__ T sval[MIK_LU_R];
    __shared__ int srow[MIK_LU_R];
    const int r = j + (int)blockIdx.x * MIK_LU_R + (int)threadIdx.x;
    T v = r < n ? lu_key((T)fabs(A[(int64_t)j * ld + r]), r == j) : T(-1);
    int row = r < n ? r : INT_MAX;
    lu_block_best(v, row, sval, srow);
    if (threadIdx.x == 0) { pval[blockIdx.x] = v; prow[blockIdx.x] = row; }
}

// One wave.  nparts >= 1 partials of the rows [j, n); partial 0 always names a live row, and its key is >= 0: it holds the first searched
// row, whose key is never -1.  No partial is a NaN (lu_key), so the combine below is the loop's rule across workgroups, and v == 0 is the
// loop's best == 0.
template <typename T>
__global__ void __launch_bounds__(64) k_lu_pick(int n, int j, int k0, int k1, T *A, int64_t ld, int nparts, const T *__restrict__ pval,
                                                const int *__restrict__ prow, int *__restrict__ ipiv, int *first_zero)
{
    const int lane = (int)threadIdx.x;
    T v = T(-1);
    int row = INT_MAX;
    for (int q = lane; q < nparts; q += 64) {                  // ascending per lane: an equal value in a later partial has a larger row
        const T vq = pval[q];
        const int rq = prow[q];
        if (q == lane || lu_better(vq, rq, v, row)) { v = vq; row = rq; }
    }
    for (int s = 32; s > 0; s >>= 1) {
        const T vo = __shfl_down(v, s, 64);
        const int ro = __shfl_down(row, s, 64);
        if (lu_better(vo, ro, v, row)) { v = vo; row = ro; }
    }
    v = __shfl(v, 0, 64);
    row = __shfl(row, 0, 64);
    const int p = min(max(row, j), n - 1);                     // a row of [j, n) whatever the data were
    if (lane == 0) {
        ipiv[j] = p;
        if (v == T(0)) atomicMin(first_zero, j);
    }
    if (p != j)
        for (int c = k0 + lane; c < k1; c += 64) {
            const T a = A[(int64_t)c * ld + p], b = A[(int64_t)c * ld + j];
            A[(int64_t)c * ld + j] = a;
            A[(int64_t)c * ld + p] = b;
        }
}

// Rows (j, n).  The pivot row j is read, never written, by this launch.  A launch is short and latency-bound, so every load of a lane's
// row (at most W - 1 columns) is issued before the first value is used: one memory round trip instead of one per batch.  The pivot row
// goes through LDS (its entries are workgroup-uniform).
template <typename T>
__global__ void __launch_bounds__(MIK_LU_R) k_lu_update(int n, int j, int k1, T *A, int64_t ld, T *__restrict__ pval, int *__restrict__ prow)
{
    constexpr int C = MIK_LU_W - 1;                            // columns right of j inside a panel, at most
    __shared__ T sval[MIK_LU_R];
    __shared__ int srow[MIK_LU_R];
    __shared__ T su[MIK_LU_W];
    const int t = (int)threadIdx.x;
    const int r = j + 1 + (int)blockIdx.x * MIK_LU_R + t;
    const bool live = r < n;
    const int cnt = k1 - j - 1;                                // uniform
    T *Ar = A + (live ? r : j);                                // a dead lane reads the pivot row (in bounds) and stores nothing
    if (t <= cnt) su[t] = A[(int64_t)(j + t) * ld + j];        // su[0] the pivot, su[1 + q] the pivot row's entry in column j + 1 + q
    const T mine = Ar[(int64_t)j * ld];
    T a[C];
#pragma unroll
    for (int q = 0; q < C; ++q)
        if (q < cnt) a[q] = Ar[(int64_t)(j + 1 + q) * ld];
    __syncthreads();
    const T m = mine / su[0];
    if (live) Ar[(int64_t)j * ld] = m;
#pragma unroll
    for (int q = 0; q < C; ++q)
        if (q < cnt) {
            const T p = m * su[1 + q];
            a[q] = a[q] - p;
            if (live) Ar[(int64_t)(j + 1 + q) * ld] = a[q];
        }
    if (cnt > 0) {                                             // the search of column j + 1 over the rows [j + 1, n): this launch's rows
        T v = live ? lu_key((T)fabs(a[0]), r == j + 1) : T(-1);
        int row = live ? r : INT_MAX;
        lu_block_best(v, row, sval, srow);
        if (t == 0) { pval[blockIdx.x] = v; prow[blockIdx.x] = row; }
    }
}

// The interchanges of the panel [k0, k1) on the n - (k1 - k0) columns outside it, in order.  One wave; a lane owns a column.  Walking the
// interchanges through memory would be a chain of W dependent round trips, so the rows they touch -- the panel's own rows (slots
// 0 .. W - 1) and the pivot rows below the panel (slot W + q for the FIRST interchange q that names the row) -- are loaded into LDS in one
// round trip, interchanged there in order, and stored back.
template <typename T>
__global__ void __launch_bounds__(64) k_lu_swap(int n, int k0, int k1, T *A, int64_t ld, const int *__restrict__ ipiv)
{
    constexpr int W = MIK_LU_W;
    __shared__ T S[2 * W * 64];                                // S[slot * 64 + lane]
    __shared__ int sp[W], sslot[W];
    const int lane = (int)threadIdx.x;
    const int w = k1 - k0;
    if (lane < w) sp[lane] = ipiv[k0 + lane];
    __syncthreads();
    if (lane < w) {
        const int p = sp[lane];
        int slot = p - k0;                                     // a row of the panel
        if (p >= k1) {
            int first = lane;
            for (int q = lane - 1; q >= 0; --q)
                if (sp[q] == p) first = q;
            slot = W + first;
        }
        sslot[lane] = slot;
    }
    __syncthreads();
    const int idx = (int)blockIdx.x * 64 + lane;
    const bool live = idx < n - w;
    T *Ac = A + (int64_t)(live ? (idx < k0 ? idx : idx + w) : 0) * ld;      // a dead lane reads column 0 (in bounds) and stores nothing
#pragma unroll 16
    for (int q = 0; q < W; ++q)
        if (q < w) S[q * 64 + lane] = Ac[k0 + q];
#pragma unroll 16
    for (int q = 0; q < W; ++q)
        if (q < w && sslot[q] == W + q) S[(W + q) * 64 + lane] = Ac[sp[q]];
    for (int q = 0; q < w; ++q) {                              // a lane touches its own column of S only: no barrier
        const int b = sslot[q];
        if (b != q) {
            const T u = S[q * 64 + lane], v = S[b * 64 + lane];
            S[q * 64 + lane] = v;
            S[b * 64 + lane] = u;
        }
    }
    if (!live) return;
#pragma unroll 16
    for (int q = 0; q < W; ++q)
        if (q < w) Ac[k0 + q] = S[q * 64 + lane];
#pragma unroll 16
    for (int q = 0; q < W; ++q)
        if (q < w && sslot[q] == W + q) Ac[sp[q]] = S[(W + q) * 64 + lane];
}

// U12 = L11^-1 A12 for the full panel [k0, k0 + W) and the columns [k0 + W, n).  One wave; lane = column.
template <typename T>
__global__ void __launch_bounds__(64) k_lu_strip(int n, int k0, T *A, int64_t ld)
{
    constexpr int W = MIK_LU_W;
    __shared__ T Ls[W * W];                                    // Ls[k * W + i] = L11[i, k]
    const int lane = (int)threadIdx.x;
    for (int k = 0; k < W; ++k) Ls[k * W + lane] = A[(int64_t)(k0 + k) * ld + k0 + lane];
    __syncthreads();
    const int c = k0 + W + (int)blockIdx.x * 64 + lane;
    const bool live = c < n;
    T *Ac = A + (int64_t)(live ? c : k0 + W) * ld + k0;
    T v[W];
#pragma unroll
    for (int i = 0; i < W; ++i) v[i] = Ac[i];
#pragma unroll
    for (int k = 0; k < W - 1; ++k) {
#pragma unroll
        for (int i = k + 1; i < W; ++i) {
            const T p = Ls[k * W + i] * v[k];
            v[i] = v[i] - p;
        }
    }
    if (live) {
#pragma unroll
        for (int i = 1; i < W; ++i) Ac[i] = v[i];
    }
}

// w[i, b] = x[perm[i], c0 + b] for the NB columns of group blockIdx.y (de_group_first): perm[i] is loaded once for them.  x is column-major
// with the leading dimension ldx, w the group's workspace.  x may be the caller's Y: the whole pass is gathered before anything is stored there.
template <typename T>
__global__ void __launch_bounds__(256) k_lu_gather(int n, const int *__restrict__ perm, const T *__restrict__ x, T *__restrict__ w)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i < n) w[i] = x[perm[i]];
}

// the gather of a block solve
template <typename T, int NB>
__global__ void __launch_bounds__(256) k_lu_gather_nb(int n, const int *__restrict__ perm, const T *__restrict__ x, int64_t ldx, int cols, T *__restrict__ w)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int c0 = de_group_first<NB>();
    if (i >= n) return;
    const int p = perm[i];
    w += (int64_t)c0 * n;
#pragma unroll
    for (int b = 0; b < NB; ++b) w[(int64_t)i * NB + b] = x[(int64_t)(de_col_live<NB>(c0, b, cols) ? c0 + b : c0) * ldx + p];
}

// Panel [k0, k1) of the backward substitution with the upper factor, launched over the rows [0, k1) in workgroups of W rows.
//   every workgroup:     t-chain of its rows -= U[r, c] * t[c] over the columns c of the panel ABOVE, [k1, min(k1 + W, n)), DESCENDING
//   the last workgroup:  its rows are the diagonal block: steps j = m - 1 ... 0, t[k0 + j] = acc / U[k0 + j, k0 + j], the rows above
//                        subtract U[r, k0 + j] * t[k0 + j].  The solution goes to t (read by the later launches) and to y.
template <typename T>
__global__ void __launch_bounds__(MIK_DS_R) k_lu_bwd(int n, int k0, int k1, const T *__restrict__ A, int64_t ld, T *t, T *y)
{
    const int lane = (int)threadIdx.x;
    const int r = (int)blockIdx.x * MIK_DS_R + lane;
    const bool live = r < k1;
    const T *Ar = A + (live ? r : 0);
    T acc = live ? t[r] : T(0);
    if (k1 < n) acc = de_walk<T, false, MIK_DS_ALL>(acc, Ar, ld, t, k1, min(k1 + MIK_LU_W, n), r);
    if ((int)blockIdx.x * MIK_DS_R != k0) {
        if (live) t[r] = acc;
        return;
    }
    const int m = k1 - k0;
    const T d = live ? Ar[(int64_t)r * ld] : T(1);
    T mine = acc;
    for (int j0 = 0; j0 < m; j0 += MIK_DS_U) {
        T a[MIK_DS_U];
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) a[q] = j0 + q < m ? Ar[(int64_t)(k1 - 1 - j0 - q) * ld] : T(0);
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) {
            const int j = m - 1 - j0 - q;                  // tested as j >= 0: shared with the loads' bound the test becomes a lane mask
            if (j >= 0) de_step<false, false>(acc, mine, d, a[q], j, lane);                       // wave-uniform
        }
    }
    if (live) { t[r] = mine; y[r] = mine; }
}
// k_lu_bwd for a block of right-hand sides.  A lane carries the NB right-hand sides of group blockIdx.y (csrc/mik_dense_elem.h): t is the
// group's workspace, y column-major with the leading dimension ldy, and only the live columns are stored there.
template <typename T, int NB>
__global__ void __launch_bounds__(MIK_DS_R) k_lu_bwd_nb(int n, int k0, int k1, const T *__restrict__ A, int64_t ld, T *t, T *y, int64_t ldy, int cols)
{
    const int lane = (int)threadIdx.x;
    const int r = (int)blockIdx.x * MIK_DS_R + lane;
    const bool live = r < k1;
    const T *Ar = A + (live ? r : 0);
    const int c0 = de_group_first<NB>();
    t += (int64_t)c0 * n;
    T acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = live ? t[(int64_t)r * NB + b] : T(0);
    if (k1 < n) de_walk_nb<T, NB, false>(acc, Ar, ld, t, k1, min(k1 + MIK_LU_W, n));
    if ((int)blockIdx.x * MIK_DS_R != k0) {
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) t[(int64_t)r * NB + b] = acc[b];
        }
        return;
    }
    const int m = k1 - k0;
    const T d = live ? Ar[(int64_t)r * ld] : T(1);
    T mine[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) mine[b] = acc[b];
    for (int j0 = 0; j0 < m; j0 += MIK_DS_U) {
        T a[MIK_DS_U];
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) a[q] = j0 + q < m ? Ar[(int64_t)(k1 - 1 - j0 - q) * ld] : T(0);
#pragma unroll
        for (int q = 0; q < MIK_DS_U; ++q) {
            const int j = m - 1 - j0 - q;                  // tested as j >= 0: shared with the loads' bound the test becomes a lane mask
            if (j >= 0) de_step<false, false>(acc, mine, d, a[q], j, lane);                       // wave-uniform
        }
    }
    if (!live) return;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        t[(int64_t)r * NB + b] = mine[b];
        if (de_col_live<NB>(c0, b, cols)) y[(int64_t)(c0 + b) * ldy + r] = mine[b];
    }
}
