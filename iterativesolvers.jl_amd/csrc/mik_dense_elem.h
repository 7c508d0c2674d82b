// mik_dense_elem.h -- what the dense kernels on a column-major device matrix share: csrc/mik_dense_stationary.h (jacobi, gauss_seidel,
// sor, ssor), csrc/mik_dense_lu.h (lu!) and csrc/mik_dense_chol.h (cholesky!).  Each piece is written here once:
//   the element   a real, or an interleaved (re, im) pair (de_cx), and its operations de_*: every rounding sequence of the three bit
//                 contracts is one of these.  The complex products are cx_msub of csrc/mik_complex.h.
//   de_walk       a row's chain acc -= A[r,c] x[c] over a column range, the next batch's loads issued first; de_walk_nb: the chains of the
//                 NB right-hand sides a lane of a block solve carries, every A[r,c] loaded once for them
//   de_step       one serial step of a diagonal block in a wave: quotient, broadcast, the rows on one side subtract
//   k_dense_fwd   one panel of a forward substitution, unit diagonal (lu) or a division by the real diagonal (cholesky); k_dense_fwd_nb:
//                 the same panel for a block of right-hand sides
//   k_dense_trail one 64 x 64 tile of a trailing update, general (A22 -= L21 U12) or Hermitian (A22 -= L21 L21^H, lower tiles)
// No fma, no matrix cores, no reciprocal (the library is built -ffp-contract=off): a product and the difference that takes it are rounded
// on their own, and an element meets its k in one fixed order.
#pragma once
#include "mik_internal.h"
#include "mik_complex.h"

constexpr int MIK_DS_W = 64;            // columns per panel of a substitution and of a factorisation
constexpr int MIK_DS_R = 64;            // rows per workgroup of a substitution (one wave: a row sweep over n rows spreads over n / 64 compute units)
constexpr int MIK_DS_U = 16;            // column loads per batch; two batches in flight
constexpr int MIK_DS_T = 64;            // tile edge of a trailing update (rows and columns)
constexpr int MIK_DS_THREADS = 256;     // workgroup of a trailing update: 16 x 16 lanes, 4 x 4 elements each
constexpr int MIK_DS_G = 32;            // columns per pass of a block solve: the workspace of a handle is n x G
static_assert(MIK_DS_W == 64 && MIK_DS_R == MIK_DS_W && MIK_DS_T == 64 && MIK_DS_THREADS == 256, "the tile loaders and the one-wave panels are written for these sizes");

// ---- the element ---------------------------------------------------------------------------------------------------------------------
template <typename R> struct alignas(2 * sizeof(R)) de_cx { R re, im; };       // moved as one 8- or 16-byte access
template <typename E> struct de_real { using type = E; };
template <typename R> struct de_real<de_cx<R>> { using type = R; };

template <typename E> __device__ __forceinline__ E de_zero() { return E{}; }
__device__ __forceinline__ float de_re(float a) { return a; }
__device__ __forceinline__ double de_re(double a) { return a; }
template <typename R> __device__ __forceinline__ R de_re(de_cx<R> a) { return a.re; }
__device__ __forceinline__ void de_set_real(float &a, float d) { a = d; }
__device__ __forceinline__ void de_set_real(double &a, double d) { a = d; }
template <typename R> __device__ __forceinline__ void de_set_real(de_cx<R> &a, R d) { a.re = d; a.im = R(0); }
__device__ __forceinline__ float de_conj(float a) { return a; }
__device__ __forceinline__ double de_conj(double a) { return a; }
template <typename R> __device__ __forceinline__ de_cx<R> de_conj(de_cx<R> a) { return de_cx<R>{a.re, -a.im}; }
// a = a - l w: the rounded product, then the rounded difference (per component in the complex types)
__device__ __forceinline__ void de_msub(float &a, float l, float w) { const float p = l * w; a = a - p; }
__device__ __forceinline__ void de_msub(double &a, double l, double w) { const double p = l * w; a = a - p; }
template <typename R> __device__ __forceinline__ void de_msub(de_cx<R> &a, de_cx<R> l, de_cx<R> w) { cx_msub(l.re, l.im, w.re, w.im, a.re, a.im); }
// a = a - l conj(m) and a = a - conj(l) y
template <typename E> __device__ __forceinline__ void de_msub_cj(E &a, E l, E m) { de_msub(a, l, de_conj(m)); }
template <typename E> __device__ __forceinline__ void de_msub_lc(E &a, E l, E y) { de_msub(a, de_conj(l), y); }
// a / d for a real d: one division per component
__device__ __forceinline__ float de_div(float a, float d) { return a / d; }
__device__ __forceinline__ double de_div(double a, double d) { return a / d; }
template <typename R> __device__ __forceinline__ de_cx<R> de_div(de_cx<R> a, R d) { return de_cx<R>{a.re / d, a.im / d}; }

// right-hand sides a lane of a block solve carries: 2 of a real type, 1 of a complex one.  The groups of a pass run side by side on
// different compute units (a solve occupies n / 64 of them), while the NB chains of a lane share one wave's instruction issue in the serial
// steps of a diagonal block: measured with 8 / 4, 4 / 2 and 2 / 1, every width from 1 to 32 columns was fastest with
// the smallest, and a complex block gains nothing from a second column per lane.
template <typename E> struct de_block { static constexpr int NB = sizeof(E) == sizeof(typename de_real<E>::type) ? 2 : 1; };
static_assert(MIK_DS_G % de_block<double>::NB == 0 && MIK_DS_G % de_block<de_cx<double>>::NB == 0, "a pass is whole groups");

// c ? a : b per component: v_cndmask, where a guarded assignment of a pair becomes an exec-masked block and `?:` on a pair goes through memory
__device__ __forceinline__ float de_select(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ double de_select(bool c, double a, double b) { return c ? a : b; }
template <typename R> __device__ __forceinline__ de_cx<R> de_select(bool c, de_cx<R> a, de_cx<R> b) { return de_cx<R>{c ? a.re : b.re, c ? a.im : b.im}; }

// the value lane j holds, in every lane; j is wave-uniform, so this is a register read (v_readlane), not a trip through the LDS crossbar
__device__ __forceinline__ float ds_bcast(float v, int j)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}
__device__ __forceinline__ double ds_bcast(double v, int j)
{
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), j);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <typename R> __device__ __forceinline__ de_cx<R> ds_bcast(de_cx<R> v, int j) { return de_cx<R>{ds_bcast(v.re, j), ds_bcast(v.im, j)}; }

// ---- the row walk --------------------------------------------------------------------------------------------------------------------
enum { MIK_DS_ALL = 0, MIK_DS_BELOW = 1, MIK_DS_ABOVE = 2, MIK_DS_OFFDIAG = 3 };   // which columns c of [lo, hi) row r takes: all, c < r, c > r, c != r

template <int PRED> __device__ __forceinline__ bool ds_take(int c, int r)
{
    return PRED == MIK_DS_ALL || (PRED == MIK_DS_BELOW && c < r) || (PRED == MIK_DS_ABOVE && c > r) || (PRED == MIK_DS_OFFDIAG && c != r);
}

// acc = acc - (Ar[c * ld] * x[c]) over the columns c of [lo, hi) that PRED admits, ascending or descending.  Ar = A + r; lo and hi are
// wave-uniform.  The loads of the next batch are issued before the chain of the current one is evaluated.  A column PRED refuses is
// computed and dropped by a select (none with MIK_DS_ALL).
// The columns that remain are counted down for a real element and recomputed from c for a complex one.  It is one loop either way, but
// the compiler schedules the two forms differently, and each element kind needs its own: counted, a complex batch fetches its 16 x[c]
// four at a time (four scalar round trips per batch, 5 % of a Cholesky solve); recomputed, a real walk holds 8 more registers and
// k_ds_row, k_ds_panel and the LU's forward panel lose an occupancy step.
template <typename E, bool ASC, int PRED>
__device__ __forceinline__ E de_walk(E acc, const E *__restrict__ Ar, int64_t ld, const E *__restrict__ x, int lo, int hi, int r)
{
    constexpr int U = MIK_DS_U;
    constexpr bool COUNTED = sizeof(E) == sizeof(typename de_real<E>::type);
    int left = hi - lo;
    int c = ASC ? lo : hi - 1;                      // first column of the current batch, in walking order
    const auto rest = [&]() { return COUNTED ? left : ASC ? hi - c : c - lo + 1; };
    E cur[U], nxt[U];
    if (rest() >= U) {
#pragma unroll
        for (int q = 0; q < U; ++q) cur[q] = Ar[(int64_t)(ASC ? c + q : c - q) * ld];
    }
    while (rest() >= U) {
        const int cn = ASC ? c + U : c - U;
        const bool more = rest() >= 2 * U;
        if (more) {
#pragma unroll
            for (int q = 0; q < U; ++q) nxt[q] = Ar[(int64_t)(ASC ? cn + q : cn - q) * ld];
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int cc = ASC ? c + q : c - q;
            E s = acc;
            de_msub(s, cur[q], x[cc]);
            acc = de_select(ds_take<PRED>(cc, r), s, acc);
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < U; ++q) cur[q] = nxt[q];
        }
        c = cn;
        left -= U;
    }
    for (; rest() > 0; --left, c += ASC ? 1 : -1) {
        E s = acc;
        de_msub(s, Ar[(int64_t)c * ld], x[c]);
        acc = de_select(ds_take<PRED>(c, r), s, acc);
    }
    return acc;
}

// The walk for the NB right-hand sides b a lane of a block solve carries: acc[b] = acc[b] - (Ar[c * ld] * x[c * NB + b]) over all columns c
// of [lo, hi).  x holds the right-hand sides interleaved (the NB values of a column side by side): a column's values are one uniform
// load, and every Ar[c * ld] is loaded once and used NB times.  Per b it is de_walk's chain: the same operands in the same order.  The
// columns are counted down in every element type: recomputed from c, as de_walk does for a complex element, the compiler fetches the
// 16 NB x values of a batch at once and spills scalar registers (208 in ComplexF64 at NB = 4).
template <typename E, int NB, bool ASC>
__device__ __forceinline__ void de_walk_nb(E (&acc)[NB], const E *__restrict__ Ar, int64_t ld, const E *__restrict__ x, int lo, int hi)
{
    constexpr int U = MIK_DS_U;
    int left = hi - lo;
    int c = ASC ? lo : hi - 1;                      // first column of the current batch, in walking order
    const auto sub = [&](E a, int cc) {
#pragma unroll
        for (int b = 0; b < NB; ++b) de_msub(acc[b], a, x[(int64_t)cc * NB + b]);
    };
    E cur[U], nxt[U];
    if (left >= U) {
#pragma unroll
        for (int q = 0; q < U; ++q) cur[q] = Ar[(int64_t)(ASC ? c + q : c - q) * ld];
    }
    while (left >= U) {
        const int cn = ASC ? c + U : c - U;
        const bool more = left >= 2 * U;
        if (more) {
#pragma unroll
            for (int q = 0; q < U; ++q) nxt[q] = Ar[(int64_t)(ASC ? cn + q : cn - q) * ld];
        }
#pragma unroll
        for (int q = 0; q < U; ++q) sub(cur[q], ASC ? c + q : c - q);
        if (more) {
#pragma unroll
            for (int q = 0; q < U; ++q) cur[q] = nxt[q];
        }
        c = cn;
        left -= U;
    }
    for (; left > 0; --left, c += ASC ? 1 : -1) sub(Ar[(int64_t)c * ld], c);
}

// ---- one serial step of a diagonal block: lane = row of the block, j the wave-uniform step.  The quotient of lane j is the block's
// solution j: every lane receives it, lane j keeps its own in `mine`, and the rows on one side of j (BELOW: lane > j, a forward
// substitution; else lane < j, a backward one) subtract coeff times it.  UNIT: a unit diagonal, no division: the quotient is acc itself,
// which lane j keeps from step j on, so neither d nor `mine` is touched.  The step is a wave's serial chain -- every instruction in it is
// paid W times per launch.
template <bool UNIT, bool BELOW, typename E, typename R>
__device__ __forceinline__ void de_step(E &acc, E &mine, R d, E coeff, int j, int lane)
{
    const E quo = UNIT ? acc : de_div(acc, d);
    const E bj = ds_bcast(quo, j);
    if (!UNIT) mine = de_select(lane == j, quo, mine);
    E s = acc;
    de_msub(s, coeff, bj);
    acc = de_select(BELOW ? lane > j : lane < j, s, acc);
}

// The step for the NB right-hand sides a lane of a block solve carries.  Every instruction of the serial chain waits for the one before
// it; the NB quotient, broadcast and subtract sequences wait on nothing of each other's, so written stage by stage they fill those waits.
// Per right-hand side it is the sequence above: the same operations on the same operands.
template <bool UNIT, bool BELOW, int NB, typename E, typename R>
__device__ __forceinline__ void de_step(E (&acc)[NB], E (&mine)[NB], R d, E coeff, int j, int lane)
{
    E bj[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {                  // NB independent quotients and broadcasts, side by side in the step
        const E quo = UNIT ? acc[b] : de_div(acc[b], d);
        bj[b] = ds_bcast(quo, j);
        if (!UNIT) mine[b] = de_select(lane == j, quo, mine[b]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        E s = acc[b];
        de_msub(s, coeff, bj[b]);
        acc[b] = de_select(BELOW ? lane > j : lane < j, s, acc[b]);
    }
}

// ---- panel k0 / W of a forward substitution with a lower factor, launched over the rows [k0, n) in workgroups of W rows.  src is the
// right-hand side in the first launch (every row is touched there first) and t afterwards (lu: always t, which the gather has filled); t
// holds the solved entries below k0 and every other row's accumulator.
//   every workgroup:   its rows' chains -= L[r, c] t[c] over the previous panel's columns c in [k0 - W, k0), ascending
//   workgroup 0 only:  the diagonal block: W serial steps j, t[k0 + j] = acc (UNIT) or acc / re(L[k0 + j, k0 + j]), the rows below
//                      subtract L[r, k0 + j] t[k0 + j]
// A dead lane reads row k0 (in bounds) and stores nothing.  With a division only coefficients strictly below the diagonal are loaded (the
// strict upper triangle of a Cholesky factor is never read); UNIT loads the step's whole column of the block, whose upper part is U and
// is dropped by the step's select -- a lane-dependent mask costs an exec round per load, a third of a launch of the LU's solve.
template <typename E, bool UNIT>
__global__ void __launch_bounds__(MIK_DS_R) k_dense_fwd(int n, int k0, const E *__restrict__ A, int64_t ld, const E *src, E *t)
{
    using R = typename de_real<E>::type;
    const int lane = (int)threadIdx.x;
    const int r = k0 + (int)blockIdx.x * MIK_DS_R + lane;
    const bool live = r < n;
    const E *Ar = A + (live ? r : k0);
    E acc = live ? src[r] : de_zero<E>();
    if (k0 > 0) acc = de_walk<E, true, MIK_DS_ALL>(acc, Ar, ld, t, k0 - MIK_DS_W, k0, r);
    if (blockIdx.x == 0) {
        const int m = min(MIK_DS_W, n - k0);
        const R d = (!UNIT && live) ? de_re(Ar[(int64_t)r * ld]) : R(1);
        E mine = acc;
        for (int j0 = 0; j0 < m; j0 += MIK_DS_U) {
            E a[MIK_DS_U];
#pragma unroll
            for (int q = 0; q < MIK_DS_U; ++q) a[q] = (j0 + q < m && (UNIT || (lane > j0 + q && live))) ? Ar[(int64_t)(k0 + j0 + q) * ld] : de_zero<E>();
#pragma unroll
            for (int q = 0; q < MIK_DS_U; ++q)
                if (j0 + q < m) de_step<UNIT, true>(acc, mine, d, a[q], j0 + q, lane);      // wave-uniform
        }
        if (!UNIT) acc = mine;
    }
    if (live) t[r] = acc;
}

// ---- the NB right-hand sides a lane of a substitution carries.  A solve runs in passes of at most G columns; group blockIdx.y of a pass is
// its columns [c0, c0 + NB), c0 = blockIdx.y * NB, of which those below `cols` (the pass's column count) are live.  The group's workspace
// is n rows of NB values side by side, NB * n elements after the previous group's: with NB = 1 and one group, the plain work vector of a
// vector solve.  A dead column (only the last group has any, and none with NB = 1) carries a copy of the group's first column, which is
// always live, through the workspace, and nothing of it is stored into Y.
template <int NB> __device__ __forceinline__ int de_group_first() { return (int)blockIdx.y * NB; }
template <int NB> __device__ __forceinline__ bool de_col_live(int c0, int b, int cols) { return NB == 1 || c0 + b < cols; }

// ---- k_dense_fwd for a block of right-hand sides: the same panel, launched over the rows (grid x) and the column groups of the pass
// (grid y).  src, column-major with the leading dimension lds, is the right-hand side in the first launch; src = nullptr afterwards (lu:
// always, the gather has filled t): the accumulators are in t.
template <typename E, bool UNIT, int NB>
__global__ void __launch_bounds__(MIK_DS_R) k_dense_fwd_nb(int n, int k0, const E *__restrict__ A, int64_t ld, const E *src, int64_t lds, int cols, E *t)
{
    using R = typename de_real<E>::type;
    const int lane = (int)threadIdx.x;
    const int r = k0 + (int)blockIdx.x * MIK_DS_R + lane;
    const bool live = r < n;
    const E *Ar = A + (live ? r : k0);
    const int c0 = de_group_first<NB>();
    t += (int64_t)c0 * n;
    E acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int col = de_col_live<NB>(c0, b, cols) ? c0 + b : c0;
        const E *from = src ? src + (int64_t)col * lds + r : t + (int64_t)r * NB + b;      // `?:` on the addresses: on a pair it goes through memory
        acc[b] = live ? *from : de_zero<E>();
    }
    if (k0 > 0) de_walk_nb<E, NB, true>(acc, Ar, ld, t, k0 - MIK_DS_W, k0);
    if (blockIdx.x == 0) {
        const int m = min(MIK_DS_W, n - k0);
        const R d = (!UNIT && live) ? de_re(Ar[(int64_t)r * ld]) : R(1);
        E mine[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) mine[b] = acc[b];
        for (int j0 = 0; j0 < m; j0 += MIK_DS_U) {
            E a[MIK_DS_U];
#pragma unroll
            for (int q = 0; q < MIK_DS_U; ++q) a[q] = (j0 + q < m && (UNIT || (lane > j0 + q && live))) ? Ar[(int64_t)(k0 + j0 + q) * ld] : de_zero<E>();
#pragma unroll
            for (int q = 0; q < MIK_DS_U; ++q)
                if (j0 + q < m) de_step<UNIT, true>(acc, mine, d, a[q], j0 + q, lane);      // wave-uniform
        }
        if (!UNIT) {
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = mine[b];
        }
    }
    if (live) {
#pragma unroll
        for (int b = 0; b < NB; ++b) t[(int64_t)r * NB + b] = acc[b];
    }
}

// ---- one tile of a trailing update for the full panel [k0, k0 + W): tile (blockIdx.x, blockIdx.y) of T x T elements from
// (k0 + W, k0 + W), each element's k ascending, a 4 x 4 register block per lane.  Rs[k * T + i] = L21[r0 + i, k0 + k] in both forms.
//   general (lu)       A22[i,c] -= L21[i,k] U12[k,c]: Cs[k * CP + c] = U12[k0 + k, c0 + c], loaded along U12's columns; 16-byte rows on a
//                      pitch that spreads the banks; the whole panel in one pass
//   HERM (cholesky)    A22[i,c] -= L21[i,k] conj(L21[c,k]): Cs[k * T + c] = L21[c0 + c, k0 + k], a second tile of rows; the lower tiles
//                      only, the diagonal tiles masked to r >= c; KC columns k per pass, so that both tiles stay within 32 KB
template <typename E, bool HERM> struct de_trail {
    static constexpr int KC = !HERM ? MIK_DS_W : sizeof(E) <= 4 ? 64 : sizeof(E) <= 8 ? 32 : 16;
    static constexpr int CP = HERM ? MIK_DS_T : MIK_DS_T + 16 / (int)sizeof(E);
};

template <typename E, bool HERM>
__global__ void __launch_bounds__(MIK_DS_THREADS) k_dense_trail(int n, int k0, E *A, int64_t ld)
{
    constexpr int W = MIK_DS_W, T = MIK_DS_T, KC = de_trail<E, HERM>::KC, CP = de_trail<E, HERM>::CP;
    static_assert(HERM || KC == T, "the general form turns the whole U12 tile in one pass");
    if (HERM && blockIdx.x < blockIdx.y) return;               // workgroup-uniform
    __shared__ __attribute__((aligned(16))) E Rs[KC * T];
    __shared__ __attribute__((aligned(16))) E Cs[KC * CP];
    const int t = (int)threadIdx.x;
    const int k1 = k0 + W;
    const int r0 = k1 + (int)blockIdx.x * T, c0 = k1 + (int)blockIdx.y * T;
    const int i0 = 4 * (t & 15), j0 = 4 * (t >> 4);
    E acc[4][4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = r0 + i0 + a, c = c0 + j0 + b;
            acc[a][b] = (r < n && (HERM ? r >= c : c < n)) ? A[(int64_t)c * ld + r] : de_zero<E>();
        }
    const int q = t & 63, s = t >> 6;
    for (int kb = 0; kb < W; kb += KC) {
        if (kb) __syncthreads();                               // the previous pass has been read
#pragma unroll
        for (int it = 0; it < KC / 4; ++it) {
            const int k = s + 4 * it;
            const E *col = A + (int64_t)(k0 + kb + k) * ld;
            Rs[k * T + q] = r0 + q < n ? col[r0 + q] : de_zero<E>();
            if (HERM) Cs[k * T + q] = c0 + q < n ? col[c0 + q] : de_zero<E>();
        }
        if (!HERM) {
#pragma unroll
            for (int it = 0; it < T / 4; ++it) {
                const int c = s + 4 * it;
                Cs[q * CP + c] = c0 + c < n ? A[(int64_t)(c0 + c) * ld + k0 + q] : de_zero<E>();
            }
        }
        __syncthreads();
#pragma clang loop unroll_count(HERM ? 4 : 8)
        for (int k = 0; k < KC; ++k) {
            E l[4], u[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) l[a] = Rs[k * T + i0 + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) u[b] = Cs[k * CP + j0 + b];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    if (HERM) de_msub_cj(acc[a][b], l[a], u[b]);
                    else de_msub(acc[a][b], l[a], u[b]);
                }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = r0 + i0 + a, c = c0 + j0 + b;
            if (r < n && (HERM ? r >= c : c < n)) A[(int64_t)c * ld + r] = acc[a][b];
        }
}
