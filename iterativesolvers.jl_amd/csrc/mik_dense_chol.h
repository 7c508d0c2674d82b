// mik_dense_chol.h -- device kernels of cholesky!(Hermitian(A, :L)) and ldiv!(y, F, x) on a square column-major device matrix, for
// Float64, Float32, ComplexF64 and ComplexF32.
//
// THE BIT CONTRACT (restated as unblocked C99 loops in tests/dense_ref/dense_chol_ref.c).  Complex products are cx_mul of
// csrc/mik_complex.h (four rounded products, one rounded difference, one rounded sum); every subtraction is componentwise; no fma, no
// matrix cores, no reciprocal.  For j = 0 ... n - 1:
//   diagonal   d = re(A[j,j]); for k = 0 ... j - 1 ascending d = d - (lr lr + li li) of L[j,k] (real types: d - L[j,k] L[j,k]).  That sum
//              is exactly the real part of cx_mul(L[j,k], conj(L[j,k])), so a trailing update that treats the diagonal like any other
//              element gives the same bits.  !(d > 0) -- a NaN too -- fails column j; the FIRST such j is reported, 1-based.  Otherwise
//              L[j,j] = sqrt(d), correctly rounded, stored with imaginary part +0.
//   below      a = A[i,j]; for k = 0 ... j - 1 ascending a = a - cx_mul(L[i,k], conj(L[j,k])); L[i,j] = a / L[j,j], a true division per
//              component.
//   ldiv!      forward: acc = x[i]; for k < i ascending acc -= L[i,k] w[k]; w[i] = acc / L[i,i].
//              backward: acc = w[i]; for k > i DESCENDING acc -= conj(L[k,i]) y[k]; y[i] = acc / L[i,i].
// Only the lower triangle of A and the real parts of its diagonal are read (LAPACK's rule); the strict upper triangle is never read and
// never written.  After a failure at column k the contents of the columns >= k are unspecified.
// Only the order within one element's chain matters, so the blocked right-looking plan below -- panels of W columns, each element's k
// ascending inside a panel and panel after panel -- gives the same bits as the unblocked loop.  Per panel [k0, k1), three launches:
//   k_chol_diag   ONE workgroup factors the w x w diagonal block, columns serially with a barrier between them (the block in registers, the
//                 current column in LDS), records a failing column (atomicMin) and stores the block's L
//   k_chol_panel  L21 = A21 L11^-H: four lanes own a row below the block, its W values in their registers, L11 in LDS, k ascending, the
//                 division last
//   k_dense_trail<E, true>  A22[i,c] -= sum_k L21[i,k] conj(L21[c,k]), k ascending: T x T tiles with blockIdx.x >= blockIdx.y, the diagonal
//                 tiles masked to r >= c, both LDS tiles loaded from L21 along contiguous rows
// and per panel of a solve one launch each way:
//   k_dense_fwd<E, false>   one panel of the forward substitution, with the division by the diagonal
//   k_chol_bwd    one panel of the backward substitution: row r needs conj(L[c,r]), element c of COLUMN r, so the block is loaded along
//                 its columns (coalesced), turned in LDS (padded pitch) and walked from there, c descending
//   k_dense_fwd_nb<E, false, NB>, k_chol_bwd_nb<E, NB>   the two for a block of right-hand sides, NB per lane (ldiv!(Y, F, X)): per column the
//                 same operations on the same operands in the same order, so column j has the bits of the vector solve of column j
// The element (de_cx and the de_* operations), the serial step of a diagonal block (de_step) and the two k_dense_* kernels are those of
// csrc/mik_dense_elem.h, written once for the dense stationary methods, the LU and this file.
// Nothing indexes memory through a data value, so an indefinite or non-finite matrix cannot fault: after the first failing column the
// remaining launches run on whatever values there are.
#pragma once
#include "mik_internal.h"
#include "mik_dense_elem.h"

#include <utility>

constexpr int MIK_CH_W = MIK_DS_W;      // panel width; the substitution panels are the factorisation's
constexpr int MIK_CH_R = 64;            // rows per workgroup of k_chol_panel (four waves; wave g owns the columns g, g + 4, ... of the 64 rows)
constexpr int MIK_CH_T = MIK_DS_T;      // tile edge of the trailing update (rows and columns)
constexpr int MIK_CH_THREADS = 256;     // workgroup of k_chol_diag and of k_chol_panel
constexpr int MIK_CH_BC = 32;           // columns per transposed chunk of the backward substitution
static_assert(MIK_CH_W == 64 && MIK_CH_R == 64 && MIK_CH_THREADS == 256 && MIK_CH_W % MIK_CH_BC == 0 && MIK_DS_R == 64, "the loaders are written for these sizes");

// ---- the diagonal block [k0, k0 + w), w <= W.  ONE workgroup of four waves.  Thread (i, g) keeps the elements (i, c) of the columns
// c = g, g + 4, ... in registers, so wave g owns every fourth column.  Column j: its wave reads the pivot from lane j, divides, and puts
// the column into LDS; after ONE barrier every thread subtracts it from its own columns c > j.  The column buffer is doubled: the wave of
// column j + 1 writes the other half while the rest still read column j.  The columns are unrolled (chol_diag_col<J>) so that every register index is
// a constant.  2 KB of LDS for ComplexF64; the block itself never is in LDS.
template <typename E, int J>
__device__ __forceinline__ void chol_diag_col(E (&a)[MIK_CH_W / (MIK_CH_THREADS / 64)], E (*Cb)[MIK_CH_W], int i, int g, int w, int k0, int *first_bad)
{
    using R = typename de_real<E>::type;
    constexpr int G = MIK_CH_THREADS / 64, Q = MIK_CH_W / G, QJ = J / G;
    if (J >= w) return;                                        // workgroup-uniform
    if (g == J % G) {
        const R d = ds_bcast(de_re(a[QJ]), J);
        const R ljj = mik_sqrt(d);
        if (i == 0 && !(d > R(0))) atomicMin(first_bad, k0 + J);
        if (i == J) de_set_real(a[QJ], ljj);
        else if (i > J) a[QJ] = de_div(a[QJ], ljj);
        Cb[J & 1][i] = a[QJ];
    }
    __syncthreads();
    const E lij = Cb[J & 1][i];
#pragma unroll
    for (int q = QJ; q < Q; ++q)
        if (q > QJ || g > J % G) de_msub_cj(a[q], lij, Cb[J & 1][g + G * q]);      // the columns c > J of this thread
}
template <typename E, int... J>
__device__ __forceinline__ void chol_diag_cols(std::integer_sequence<int, J...>, E (&a)[MIK_CH_W / (MIK_CH_THREADS / 64)], E (*Cb)[MIK_CH_W], int i, int g, int w,
                                               int k0, int *first_bad)
{
    (chol_diag_col<E, J>(a, Cb, i, g, w, k0, first_bad), ...);
}

template <typename E>
__global__ void __launch_bounds__(MIK_CH_THREADS) k_chol_diag(int k0, int w, E *A, int64_t ld, int *first_bad)
{
    constexpr int W = MIK_CH_W, G = MIK_CH_THREADS / 64, Q = W / G;
    __shared__ E Cb[2][W];
    const int t = (int)threadIdx.x;
    const int i = t & 63, g = t >> 6;                          // g is wave-uniform
    E *Ab = A + (int64_t)k0 * ld + k0;
    E a[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = g + G * q;
        a[q] = (i >= c && i < w) ? Ab[(int64_t)c * ld + i] : de_zero<E>();      // i < w and i >= c: c < w
    }
    chol_diag_cols<E>(std::make_integer_sequence<int, W>{}, a, Cb, i, g, w, k0, first_bad);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = g + G * q;
        if (i >= c && i < w) Ab[(int64_t)c * ld + i] = a[q];
    }
}

// ---- L21 = A21 L11^-H for the full panel [k0, k0 + W) and the rows [k0 + W, n): k_chol_diag's shape without the square root.  One
// workgroup of four waves per 64 rows.  Thread (i, g) keeps the elements (row i, column c) of the columns c = g, g + 4, ... in registers,
// all loaded before the first use.  Column k: its wave divides by L11[k,k] and puts the 64 quotients into the doubled LDS buffer; after
// ONE barrier every thread subtracts them, times conj(L11[c,k]), from its own columns c > k -- k ascending per element, the division
// last.  L11's lower triangle is in LDS, packed: column k starts at k W - k (k - 1) / 2 (33 KB for ComplexF64).  w is the panel's width and
// always W here (only full panels have rows below them); passing it at run time keeps every column's code a block of its own -- as straight-line
// code the compiler hoists the later columns' reads of L11 into registers and spills 3.3 KB per lane in ComplexF64.
template <typename E, int K>
__device__ __forceinline__ void chol_panel_col(E (&a)[MIK_CH_W / (MIK_CH_THREADS / 64)], const E *Lt, E (*Cb)[MIK_CH_W], int i, int g, int w)
{
    constexpr int W = MIK_CH_W, G = MIK_CH_THREADS / 64, Q = W / G, QK = K / G, OFF = K * W - K * (K - 1) / 2;
    if (K >= w) return;                                        // workgroup-uniform and never taken (w = W), see k_chol_panel
    if (g == K % G) {
        a[QK] = de_div(a[QK], de_re(Lt[OFF]));
        Cb[K & 1][i] = a[QK];
    }
    __syncthreads();
    const E vk = Cb[K & 1][i];
#pragma unroll
    for (int q = QK; q < Q; ++q)
        if (q > QK || g > K % G) de_msub_cj(a[q], vk, Lt[OFF + g + G * q - K]);      // the columns c > K of this thread
}
template <typename E, int... K>
__device__ __forceinline__ void chol_panel_cols(std::integer_sequence<int, K...>, E (&a)[MIK_CH_W / (MIK_CH_THREADS / 64)], const E *Lt, E (*Cb)[MIK_CH_W], int i, int g,
                                                int w)
{
    (chol_panel_col<E, K>(a, Lt, Cb, i, g, w), ...);
}

template <typename E>
__global__ void __launch_bounds__(MIK_CH_THREADS) k_chol_panel(int n, int k0, int w, E *A, int64_t ld)
{
    constexpr int W = MIK_CH_W, G = MIK_CH_THREADS / 64, Q = W / G;
    __shared__ E Lt[W * (W + 1) / 2];
    __shared__ E Cb[2][W];
    const int t = (int)threadIdx.x;
    const int i = t & 63, g = t >> 6;                          // g is wave-uniform
    const int k1 = k0 + W;
    const int r = k1 + (int)blockIdx.x * MIK_CH_R + i;
    const bool live = r < n;
    E *Ar = A + (int64_t)k0 * ld + (live ? r : k1);           // a dead lane reads row k1 (in bounds) and stores nothing
    E a[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) a[q] = Ar[(int64_t)(g + G * q) * ld];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = g + G * q;
        if (i >= k) Lt[k * W - k * (k - 1) / 2 + i - k] = A[(int64_t)(k0 + k) * ld + k0 + i];
    }
    __syncthreads();
    chol_panel_cols<E>(std::make_integer_sequence<int, W>{}, a, Lt, Cb, i, g, w);
    if (live) {
#pragma unroll
        for (int q = 0; q < Q; ++q) Ar[(int64_t)(g + G * q) * ld] = a[q];
    }
}

// ---- panel [k0, k1) of the backward substitution, launched over the rows [0, k1) in workgroups of W rows.
//   every workgroup:     its rows' chains -= conj(L[c, r]) t[c] over the columns c of the panel ABOVE, [k1, min(k1 + W, n)), DESCENDING
//   the last workgroup:  the diagonal block: steps j = m - 1 ... 0, t[k0 + j] = acc / L[k0 + j, k0 + j], the rows above subtract
//                        conj(L[k0 + j, r]) t[k0 + j].  The solution goes to t (read by the later launches) and to y.
// L[c, r] for the 64 rows r of a workgroup lies along the columns r: chunks of BC rows c are loaded along those columns (a lane pair per
// column, BC consecutive elements each), stored transposed as Ts[row * (BC + 1) + c] -- the odd pitch spreads the 64 rows over the banks --
// and walked from there.  Only elements strictly below the diagonal are loaded.  A launch is short and latency-bound: all loads of a chunk
// are issued at once, and those of the next chunk before the current one is walked, so a launch waits for memory about once.
template <typename E>
__device__ __forceinline__ void ch_turn_load(E (&reg)[MIK_CH_BC], const E *__restrict__ A, int64_t ld, int r0, int rows_end, int c_lo, int c_hi, int lane)
{
    constexpr int BC = MIK_CH_BC, PER = 64 / BC;              // rows per pass of the wave
    const int c = c_lo + (lane & (BC - 1)), h = lane / BC;
#pragma unroll
    for (int it = 0; it < BC; ++it) {
        const int row = r0 + h + PER * it;
        reg[it] = (row < rows_end && c < c_hi && c > row) ? A[(int64_t)row * ld + c] : de_zero<E>();
    }
}
template <typename E>
__device__ __forceinline__ void ch_turn_store(E *Ts, const E (&reg)[MIK_CH_BC], int lane)
{
    constexpr int BC = MIK_CH_BC, PER = 64 / BC;
    const int cc = lane & (BC - 1), h = lane / BC;
    __syncthreads();                                           // the previous chunk has been read
#pragma unroll
    for (int it = 0; it < BC; ++it) Ts[(h + PER * it) * (BC + 1) + cc] = reg[it];
    __syncthreads();
}

template <typename E>
__global__ void __launch_bounds__(MIK_DS_R) k_chol_bwd(int n, int k0, int k1, const E *__restrict__ A, int64_t ld, E *t, E *y)
{
    using R = typename de_real<E>::type;
    constexpr int BC = MIK_CH_BC;
    static_assert(64 % BC == 0 && 64 / BC * BC == 64 && BC == 32, "a wave loads 64 / BC columns of BC elements per pass, BC passes per chunk");
    __shared__ E Ts[64 * (BC + 1)];
    const int lane = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * MIK_DS_R;
    const int r = r0 + lane;
    const bool live = r < k1;
    const bool diag = r0 == k0;                                // workgroup-uniform: this workgroup owns the diagonal block
    const int hi = min(k1 + MIK_CH_W, n);
    // the chunks of the columns [lo, hi) in descending order, lo = k0 for the workgroup of the diagonal block and k1 for the others;
    // k1 - k0 = W whenever there are columns above k1, so every chunk lies on one side of k1
    const int lo = diag ? k0 : k1;
    E acc = live ? t[r] : de_zero<E>();
    const R d = (diag && live) ? de_re(A[(int64_t)r * ld + r]) : R(1);
    E mine = acc;
    E reg[BC];
    int c_lo = lo + (hi - lo - 1) / BC * BC;
    if (hi > lo) ch_turn_load<E>(reg, A, ld, r0, k1, c_lo, hi, lane);
    for (; c_lo >= lo && hi > lo; c_lo -= BC) {                // uniform
        ch_turn_store<E>(Ts, reg, lane);
        if (c_lo - BC >= lo) ch_turn_load<E>(reg, A, ld, r0, k1, c_lo - BC, hi, lane);
        const int cnt = min(BC, hi - c_lo);
        if (c_lo >= k1) {                                      // the panel above: its solution is in t
            for (int c = cnt - 1; c >= 0; --c) de_msub_lc(acc, Ts[lane * (BC + 1) + c], t[c_lo + c]);
        } else {                                               // the diagonal block: steps j descending
            for (int c = cnt - 1; c >= 0; --c) de_step<false, false>(acc, mine, d, de_conj(Ts[lane * (BC + 1) + c]), c_lo + c - k0, lane);      // wave-uniform j
        }
    }
    if (!diag) {
        if (live) t[r] = acc;
        return;
    }
    if (live) { t[r] = mine; y[r] = mine; }
}

// k_chol_bwd for a block of right-hand sides.  A lane carries the NB right-hand sides of group blockIdx.y (csrc/mik_dense_elem.h): every
// element of the turned chunk is read from LDS once for them.  t is the group's workspace, y column-major with the leading dimension ldy;
// only the live columns are stored there.
template <typename E, int NB>
__global__ void __launch_bounds__(MIK_DS_R) k_chol_bwd_nb(int n, int k0, int k1, const E *__restrict__ A, int64_t ld, E *t, E *y, int64_t ldy, int cols)
{
    using R = typename de_real<E>::type;
    constexpr int BC = MIK_CH_BC;
    static_assert(64 % BC == 0 && 64 / BC * BC == 64 && BC == 32, "a wave loads 64 / BC columns of BC elements per pass, BC passes per chunk");
    __shared__ E Ts[64 * (BC + 1)];
    const int lane = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * MIK_DS_R;
    const int r = r0 + lane;
    const bool live = r < k1;
    const bool diag = r0 == k0;                                // workgroup-uniform: this workgroup owns the diagonal block
    const int hi = min(k1 + MIK_CH_W, n);
    // the chunks of the columns [lo, hi) in descending order, lo = k0 for the workgroup of the diagonal block and k1 for the others;
    // k1 - k0 = W whenever there are columns above k1, so every chunk lies on one side of k1
    const int lo = diag ? k0 : k1;
    const int g0 = de_group_first<NB>();
    t += (int64_t)g0 * n;
    E acc[NB], mine[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) mine[b] = acc[b] = live ? t[(int64_t)r * NB + b] : de_zero<E>();
    const R d = (diag && live) ? de_re(A[(int64_t)r * ld + r]) : R(1);
    E reg[BC];
    int c_lo = lo + (hi - lo - 1) / BC * BC;
    if (hi > lo) ch_turn_load<E>(reg, A, ld, r0, k1, c_lo, hi, lane);
    for (; c_lo >= lo && hi > lo; c_lo -= BC) {                // uniform
        ch_turn_store<E>(Ts, reg, lane);
        if (c_lo - BC >= lo) ch_turn_load<E>(reg, A, ld, r0, k1, c_lo - BC, hi, lane);
        const int cnt = min(BC, hi - c_lo);
        if (c_lo >= k1) {                                      // the panel above: its solution is in t
            for (int c = cnt - 1; c >= 0; --c) {
                const E l = Ts[lane * (BC + 1) + c];
#pragma unroll
                for (int b = 0; b < NB; ++b) de_msub_lc(acc[b], l, t[(int64_t)(c_lo + c) * NB + b]);
            }
        } else {                                               // the diagonal block: steps j descending
            for (int c = cnt - 1; c >= 0; --c) de_step<false, false>(acc, mine, d, de_conj(Ts[lane * (BC + 1) + c]), c_lo + c - k0, lane);      // wave-uniform j
        }
    }
    if (!diag) {
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) t[(int64_t)r * NB + b] = acc[b];
        }
        return;
    }
    if (!live) return;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        t[(int64_t)r * NB + b] = mine[b];
        if (de_col_live<NB>(g0, b, cols)) y[(int64_t)(g0 + b) * ldy + r] = mine[b];
    }
}
