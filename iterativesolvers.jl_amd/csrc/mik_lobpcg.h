// mik_lobpcg.h -- kernels behind lobpcg (src/lobpcg.jl): every sweep works on a block of up to MIK_BLK_MAX columns.
//
//   k_spmm_rowgather   Y[:, j] = A * X[:, j] for a block of CB columns          -- mul!(AX, A, X), src/lobpcg.jl:124-139
//       k_spmv_rowgather with CB right-hand sides: the row-block's val[] / col[] tile is filled by LDS-DMA ONCE per column block, a lane
//       walks ITS row and, for every entry, gathers X[column, j0 .. j0 + CB) -- per column the same products in the same ascending
//       column order from +0 as k_spmv_rowgather, so the bits are mik_spmv's.  Operators without split-off long rows only.
//   k_block_gram       segment sums of X[:, i] .* Y[:, j] for a TP x TQ tile of pairs  -- mul!(G, adjoint(X), Y), :262-270, :217, :375
//       Written in the segment helpers of csrc/mik_kernels.h (seg_load, seg_dot, pair_put / pair_total) that k_multidot and k_gram use: the
//       thread / segment / wave-tree / 4-wave-sum shape of OpDot in k_map, so every pair has the bits of mik_dot after the finaliser.
//   k_block_rdiv       X <- X * inv(R), R upper triangular                       -- rdiv!, :345-355
//   k_block_update     Pout = R * Vr (+ P * Vp); Xout = X * Vx (+ Pout)           -- update_X_P!, :629-690
//       One lane per row: a row's values stay in registers, every product and every sum rounded on its own, columns ascending, the
//       first product opening a sum (the definition of k_basis_rotate).  The small matrices sit in LDS (every lane reads the same
//       address: a broadcast).
#pragma once
#include "mik_kernels.h"

#ifdef __HIPCC__

constexpr int MIK_BLK_MAX = 32;      // widest block of the four entries
constexpr int MIK_SPMM_E = 4;        // entries of a row in flight per lane (x MIK_SPMM_E * CB gathers)
constexpr int MIK_GRAM_TP = 4, MIK_GRAM_TQ = 4;   // pairs per workgroup: TP columns of X against TQ columns of Y

// ---------------------------------------------------------------------------------------------
// Y[:, j0 : j0 + CB) = A * X[:, j0 : j0 + CB), j0 = blockIdx.y * CB
// ---------------------------------------------------------------------------------------------
template <typename T, int CB>
__global__ __launch_bounds__(MIK_BLOCK) void k_spmm_rowgather(int n, int b, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                               const T *__restrict__ val, const T *__restrict__ X, int64_t ldx,
                                                               T *__restrict__ Y, int64_t ldy)
{
    constexpr int TILE = MIK_SPMV_TILE;                // entries per pass, as k_spmv_rowgather
    constexpr int VW = VT<T>::W;
    constexpr int VP = 1024 / (int)sizeof(T);          // entries per 1-KiB DMA piece of val
    constexpr int CP = 256;                            // entries per 1-KiB DMA piece of col
    constexpr int E = MIK_SPMM_E;
    __shared__ __attribute__((aligned(16))) T sval[TILE];
    __shared__ __attribute__((aligned(16))) int scol[TILE];

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int r0 = (int)blockIdx.x * MIK_BLOCK;
    const int r = r0 + t;
    const int j0 = (int)blockIdx.y * CB;
    const int bw = min(CB, b - j0);
    const T *__restrict__ Xb = X + (int64_t)j0 * ldx;
    int ks = 0, ke = 0;
    if (r < n) { ks = rowptr[r]; ke = rowptr[r + 1]; }
    const int kb = rowptr[r0] & ~3;                    // 16-byte aligned start of both streams
    const int kend = rowptr[min(r0 + MIK_BLOCK, n)];

    T acc[CB];
#pragma unroll
    for (int jj = 0; jj < CB; ++jj) acc[jj] = T(0);
    for (int kc = kb; kc < kend; kc += TILE) {
        const int cnt = min(TILE, kend - kc);
        // wave wv issues pieces wv, wv + 4, ...; reads past kend stay inside the padded allocation (2 * MIK_SPMV_TILE entries of slack)
#pragma unroll
        for (int p = 0; p < TILE / VP / 4; ++p) {
            const int piece = wv + 4 * p;
            if (piece * VP < cnt)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(val + kc + piece * VP + lane * VW),
                                                 (__attribute__((address_space(3))) void *)(sval + piece * VP), 16, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < TILE / CP / 4; ++p) {
            const int piece = wv + 4 * p;
            if (piece * CP < cnt)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(col + kc + piece * CP + lane * 4),
                                                 (__attribute__((address_space(3))) void *)(scol + piece * CP), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // ---- this lane's row, ascending column order, CB right-hand sides per entry ----
        int a = max(ks, kc) - kc;
        int len = min(ke, kc + cnt) - kc - a;
        while (len > 0) {
            T q[E];
            int cc[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const int s = min(a + i, TILE - 1);
                cc[i] = i < len ? scol[s] : 0;                       // slots past the row gather a valid address
                q[i] = sval[s];
            }
            T xv[E][CB];
#pragma unroll
            for (int i = 0; i < E; ++i)
#pragma unroll
                for (int jj = 0; jj < CB; ++jj) xv[i][jj] = Xb[(int64_t)(jj < bw ? jj : 0) * ldx + cc[i]];   // columns past the block: column j0 again
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i < len) {
#pragma unroll
                    for (int jj = 0; jj < CB; ++jj) { const T p = q[i] * xv[i][jj]; acc[jj] = acc[jj] + p; }
                }
            a += E;
            len -= E;
        }
        if (kc + TILE < kend) __syncthreads();         // workgroup-uniform: another pass will overwrite the tile
    }
    if (r < n) {
#pragma unroll
        for (int jj = 0; jj < CB; ++jj)
            if (jj < bw) Y[(int64_t)(j0 + jj) * ldy + r] = acc[jj];
    }
}

// ---------------------------------------------------------------------------------------------
// seg_out[(j * p + i) * nseg + s] = segment sum s of X[:, i] .* Y[:, j]; blockIdx.y = tile of TP x TQ pairs
// ---------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_block_gram(int64_t n, int64_t nseg, int p, int q, const T *__restrict__ X, int64_t ldx,
                                                           const T *__restrict__ Y, int64_t ldy, T *__restrict__ seg_out)
{
    constexpr int TP = MIK_GRAM_TP, TQ = MIK_GRAM_TQ;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<T>;
    __shared__ T lds[TP * TQ][4];
    const int tiles_p = (p + TP - 1) / TP;
    const int i0 = ((int)blockIdx.y % tiles_p) * TP, j0 = ((int)blockIdx.y / tiles_p) * TQ;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<T>::W * threadIdx.x;
        T xr[TP][SEG_REGS<T>], yr[TQ][SEG_REGS<T>];
#pragma unroll
        for (int a = 0; a < TP; ++a) seg_load<T, VEC>(X + (int64_t)min(i0 + a, p - 1) * ldx, base, n, 0, xr[a]);   // columns past the block: the last one again
#pragma unroll
        for (int c = 0; c < TQ; ++c) seg_load<T, VEC>(Y + (int64_t)min(j0 + c, q - 1) * ldy, base, n, 0, yr[c]);
#pragma unroll
        for (int c = 0; c < TQ; ++c)
#pragma unroll
            for (int a = 0; a < TP; ++a) pair_put(seg_dot<T, VEC>(xr[a], yr[c], base, n), lds[c * TP + a]);
        __syncthreads();
        if (threadIdx.x < TP * TQ) {
            const int a = (int)threadIdx.x % TP, c = (int)threadIdx.x / TP;
            if (i0 + a < p && j0 + c < q) seg_out[((int64_t)(j0 + c) * p + (i0 + a)) * nseg + s] = pair_total(lds[threadIdx.x]);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// X <- X * inv(R): for i ascending, X[:, i] -= X[:, j] * R[j, i] (j < i ascending), then X[:, i] /= R[i, i]
// ---------------------------------------------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(MIK_BLOCK) void k_block_rdiv(int64_t n, int s, const T *__restrict__ Rd /* device, s x s, leading dimension s */,
                                                           T *__restrict__ X, int64_t ldx)
{
    __shared__ T Rs[S * S];                                 // Rs[j * S + i] = R[j, i]
    for (int idx = (int)threadIdx.x; idx < S * S; idx += MIK_BLOCK) {
        const int j = idx / S, i = idx % S;
        Rs[idx] = (i < s && j <= i) ? Rd[(int64_t)i * s + j] : T(1);
    }
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; row < n; row += (int64_t)gridDim.x * MIK_BLOCK) {
        T x[S];
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] = i < s ? X[(int64_t)i * ldx + row] : T(0);
        // Column j is complete once the columns before it have been subtracted: divide it, then subtract it from every column behind it.
        // Each x[i] still sees its subtractions for j = 0 .. i-1 ascending and then its division -- the loop of the definition, reordered
        // so that one row R[j, j:] of the factor is live at a time (the fence keeps the compiler from hoisting all S * S / 2 of them).
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (j < s) {
                x[j] = x[j] / Rs[j * S + j];
#pragma unroll
                for (int i = j + 1; i < S; ++i) { const T pr = x[j] * Rs[j * S + i]; x[i] = x[i] - pr; }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < S; ++i)
            if (i < s) X[(int64_t)i * ldx + row] = x[i];
    }
}

// ---------------------------------------------------------------------------------------------
// Pout = rot(R, Vr) (+ rot(P, Vp)); Xout = rot(X, Vx) (+ Pout)
// ---------------------------------------------------------------------------------------------
// acc[jj] = (...(W[row, 0] * F[0, jj] + W[row, 1] * F[1, jj]) + ...) + W[row, k - 1] * F[k - 1, jj]; F in LDS, row c at F + c * LB
template <typename T, int LB>
__device__ __forceinline__ void blk_rot_row(const T *__restrict__ Wm, int64_t ld, int k, const T *F, int64_t row, T (&acc)[LB])
{
    constexpr int U = 4;                                    // columns of the block in flight per lane
    {
        const T v = Wm[row];
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) acc[jj] = v * F[jj];
    }
    int c = 1;
    for (; c + U <= k; c += U) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Wm[(int64_t)(c + u) * ld + row];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) { const T pr = v[u] * F[(c + u) * LB + jj]; acc[jj] = acc[jj] + pr; }
    }
    for (; c < k; ++c) {
        const T v = Wm[(int64_t)c * ld + row];
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) { const T pr = v * F[c * LB + jj]; acc[jj] = acc[jj] + pr; }
    }
}

template <typename T, int LB>
__global__ __launch_bounds__(MIK_BLOCK) void k_block_update(int64_t n, int sx, int b1, int b2, const T *__restrict__ X, int64_t ldx,
                                                             const T *__restrict__ R, int64_t ldr, const T *__restrict__ P, int64_t ldp,
                                                             const T *__restrict__ Vd /* device, (sx + b1 + b2) x sx, packed */,
                                                             T *__restrict__ Xout, int64_t ldxo, T *__restrict__ Pout, int64_t ldpo)
{
    __shared__ T Fs[3 * MIK_BLK_MAX * LB];                  // Fs[c * LB + jj] = V[c, jj]: rows [0, sx) Vx, then Vr, then Vp
    const int k = sx + b1 + b2;
    for (int idx = (int)threadIdx.x; idx < k * LB; idx += MIK_BLOCK) {
        const int c = idx / LB, jj = idx % LB;
        Fs[idx] = jj < sx ? Vd[(int64_t)jj * k + c] : T(0);
    }
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; row < n; row += (int64_t)gridDim.x * MIK_BLOCK) {
        T pout[LB], acc[LB];
        if (b1 > 0) {
            blk_rot_row<T, LB>(R, ldr, b1, Fs + sx * LB, row, pout);
            if (b2 > 0) {
                blk_rot_row<T, LB>(P, ldp, b2, Fs + (sx + b1) * LB, row, acc);
#pragma unroll
                for (int jj = 0; jj < LB; ++jj) pout[jj] = pout[jj] + acc[jj];
            }
#pragma unroll
            for (int jj = 0; jj < LB; ++jj)
                if (jj < sx) Pout[(int64_t)jj * ldpo + row] = pout[jj];
        }
        blk_rot_row<T, LB>(X, ldx, sx, Fs, row, acc);
        if (b1 > 0) {
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) acc[jj] = acc[jj] + pout[jj];
        }
#pragma unroll
        for (int jj = 0; jj < LB; ++jj)
            if (jj < sx) Xout[(int64_t)jj * ldxo + row] = acc[jj];
    }
}

#endif  // __HIPCC__
