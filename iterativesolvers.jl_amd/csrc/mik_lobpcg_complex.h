// mik_lobpcg_complex.h -- the four block kernels of lobpcg (csrc/mik_lobpcg.h) for ComplexF64 / ComplexF32 (MIK_C64 / MIK_C32, interleaved
// re, im): DESIGN.md section 20.  R is the component type; blocks are column-major with leading dimensions in ELEMENTS and need element
// alignment only (8 bytes).  Arithmetic: z * w = cx_mul (csrc/mik_complex.h: four rounded products, one rounded difference, one rounded
// sum), sums componentwise, re and im each their own chain, nothing contracted.
//
//   k_cspmm          Y[:, j] = A * X[:, j] for a block of CB columns: a lane owns a row and walks it in ascending entry order from (+0, +0),
//                    adding cx_mul(val, x[col]) per column -- the row sum of k_spmv_complex, so column j has the bits of mik_spmv.  The
//                    row block's val / col tile is staged in LDS once per column block by guarded loads (the complex upload pads val by two
//                    entries and col by none, so nothing past the block's last entry is touched).  Operators without long rows only.
//   k_cblock_gram    segment sums of conj(X[:, i]) .* Y[:, j] for a TP x TQ tile of pairs: cseg_dot's products and two accumulators, the
//                    segment shape of the complex mik_dot over the 2 n reals, pair_put / pair_total = block_tree_256.
//   k_cblock_rdiv    X <- X * inv(R): X[:, i] -= cx_mul(X[:, j], R[j, i]) for j < i ascending, then (re / d, im / d), d = real(R[i, i]).
//                    A lane owns a row and works through it in panels of PW columns: the finished columns before the panel are re-read from
//                    memory (this lane wrote them) and subtracted, j ascending, then the loop of k_block_rdiv runs on the panel in registers.
//   k_cblock_update  Pout = rot(R, Vr) (+ rot(P, Vp)); Xout = rot(X, Vx) (+ Pout): rot opens every sum with cx_mul(W[row, 0], F[0, jj]) and adds
//                    cx_mul(W[row, c], F[c, jj]), c ascending.  blockIdx.y owns a panel of LB output columns; only that panel's columns of V
//                    sit in LDS.
// The bits of rdiv and update do not depend on the panel width: a column's chain of operations is the same however the columns are grouped.
#pragma once
#include "mik_complex.h"
#include "mik_lobpcg.h"

#ifdef __HIPCC__

constexpr int MIK_CSPMM_TILE = 1024;     // entries of a row block staged in LDS per pass (16 KiB of values at ComplexF64 + 4 KiB of columns)
constexpr int MIK_CSPMM_CB = 4;          // widest column block (instances 1, 2, 4); measured: DESIGN.md section 20
constexpr int MIK_CSPMM_E = 2;           // entries of a row in flight per lane (x MIK_CSPMM_E * CB gathers)
constexpr int MIK_CSPMM_WG_PER_CU = 8;   // grid cap of k_cspmm: what is resident with 20 KiB of LDS a workgroup

// Columns of its row a lane keeps in registers.  k_cblock_rdiv: a panel of 8 columns for both types -- the
// compiler keeps a row of the factor and its products live next to the panel, and a 16-column panel costs 178 VGPRs at ComplexF64 and
// runs into the accumulation registers at ComplexF32.  k_cblock_update: 2 x 128 bytes of Pout / Xout.
template <typename R> struct CBlk;
template <> struct CBlk<double> { static constexpr int RDIV_PW = 8, UPD_LB = 8; };
template <> struct CBlk<float> { static constexpr int RDIV_PW = 8, UPD_LB = 16; };

// one element at p: an 8-byte access for ComplexF32, two for ComplexF64 (whose base may sit 8 bytes past a 16-byte boundary)
template <typename R> __device__ __forceinline__ CxVal<R> cx_ld(const R *p)
{
    if constexpr (sizeof(R) == 4) {
        const float2 v = *reinterpret_cast<const float2 *>(p);
        return CxVal<R>{v.x, v.y};
    } else {
        return CxVal<R>{p[0], p[1]};
    }
}
template <typename R> __device__ __forceinline__ void cx_st(R *p, R re, R im)
{
    if constexpr (sizeof(R) == 4) {
        *reinterpret_cast<float2 *>(p) = make_float2(re, im);
    } else {
        p[0] = re;
        p[1] = im;
    }
}

// ---------------------------------------------------------------------------------------------
// Y[:, j0 : j0 + CB) = A * X[:, j0 : j0 + CB), j0 = blockIdx.y * CB; blockIdx.x strides over the 256-row blocks
// ---------------------------------------------------------------------------------------------
template <typename R, int CB>
__global__ __launch_bounds__(MIK_BLOCK) void k_cspmm(int n_rows, int nb, int b, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      const R *__restrict__ val, const R *__restrict__ X, int64_t ldx, R *__restrict__ Y, int64_t ldy)
{
    constexpr int TILE = MIK_CSPMM_TILE, E = MIK_CSPMM_E;
    __shared__ R sval[2 * TILE];
    __shared__ int scol[TILE];
    const int tid = (int)threadIdx.x;
    const int j0 = (int)blockIdx.y * CB;
    const int bw = min(CB, b - j0);
    const R *__restrict__ Xb = X + 2 * (int64_t)j0 * ldx;
    for (int blk = (int)blockIdx.x; blk < nb; blk += (int)gridDim.x) {
        const int r0 = blk * MIK_BLOCK, r = r0 + tid;
        const int e0 = rowptr[r0], e1 = rowptr[min(r0 + MIK_BLOCK, n_rows)];
        int lo = 0, hi = 0;
        if (r < n_rows) { lo = rowptr[r]; hi = rowptr[r + 1]; }
        R ar[CB], ai[CB];
#pragma unroll
        for (int jj = 0; jj < CB; ++jj) { ar[jj] = R(0); ai[jj] = R(0); }
        for (int cb = e0; cb < e1; cb += TILE) {                         // workgroup-uniform bounds
            const int cnt = min(TILE, e1 - cb);
            for (int j = tid; j < cnt; j += MIK_BLOCK) {                 // nothing at or past e1 is read
                const CxVal<R> v = cx_ld<R>(val + 2 * (int64_t)(cb + j));
                sval[2 * j] = v.re;
                sval[2 * j + 1] = v.im;
                scol[j] = col[cb + j];
            }
            __syncthreads();
            // ---- this lane's row, ascending entry order, CB right-hand sides per entry ----
            int a = max(lo, cb) - cb;
            int len = min(hi, cb + cnt) - cb - a;
            while (len > 0) {
                R qr[E], qi[E];
                int cc[E];
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    const int s = min(a + i, TILE - 1);
                    cc[i] = i < len ? scol[s] : 0;                       // slots past the row gather a valid address
                    qr[i] = sval[2 * s];
                    qi[i] = sval[2 * s + 1];
                }
                CxVal<R> xv[E][CB];
#pragma unroll
                for (int i = 0; i < E; ++i)
#pragma unroll
                    for (int jj = 0; jj < CB; ++jj) xv[i][jj] = cx_ld<R>(Xb + 2 * ((int64_t)(jj < bw ? jj : 0) * ldx + cc[i]));   // columns past the block: column j0 again
#pragma unroll
                for (int i = 0; i < E; ++i)
                    if (i < len) {
#pragma unroll
                        for (int jj = 0; jj < CB; ++jj) {
                            const CxVal<R> p = cx_mul(qr[i], qi[i], xv[i][jj].re, xv[i][jj].im);
                            ar[jj] = ar[jj] + p.re;
                            ai[jj] = ai[jj] + p.im;
                        }
                    }
                a += E;
                len -= E;
            }
            __syncthreads();                                             // the next pass, or the next row block, overwrites the tile
        }
        if (r < n_rows) {
#pragma unroll
            for (int jj = 0; jj < CB; ++jj)
                if (jj < bw) cx_st<R>(Y + 2 * ((int64_t)(j0 + jj) * ldy + r), ar[jj], ai[jj]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// seg_out[(2 * (j * p + i) + c) * nseg + s] = segment sum s of the real (c = 0) / imaginary (c = 1) part of conj(X[:, i]) .* Y[:, j];
// n2 = 2 n reals, ldx2 / ldy2 in reals; blockIdx.y = tile of TP x TQ pairs
// ---------------------------------------------------------------------------------------------
template <typename R, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_cblock_gram(int64_t n2, int64_t nseg, int p, int q, const R *__restrict__ X, int64_t ldx2,
                                                            const R *__restrict__ Y, int64_t ldy2, R *__restrict__ seg_out)
{
    constexpr int TP = MIK_GRAM_TP, TQ = MIK_GRAM_TQ;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    __shared__ R lds[2 * TP * TQ][4];
    const int tiles_p = (p + TP - 1) / TP;
    const int i0 = ((int)blockIdx.y % tiles_p) * TP, j0 = ((int)blockIdx.y / tiles_p) * TQ;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        R xr[TP][SEG_REGS<R>], yr[TQ][SEG_REGS<R>];
#pragma unroll
        for (int a = 0; a < TP; ++a) seg_load<R, VEC>(X + (int64_t)min(i0 + a, p - 1) * ldx2, base, n2, 0, xr[a]);   // columns past the block: the last one again
#pragma unroll
        for (int c = 0; c < TQ; ++c) seg_load<R, VEC>(Y + (int64_t)min(j0 + c, q - 1) * ldy2, base, n2, 0, yr[c]);
#pragma unroll
        for (int c = 0; c < TQ; ++c)
#pragma unroll
            for (int a = 0; a < TP; ++a) {
                R re, im;
                cseg_dot<R>(xr[a], yr[c], base, n2, re, im);
                pair_put(re, lds[2 * (c * TP + a)]);
                pair_put(im, lds[2 * (c * TP + a) + 1]);
            }
        __syncthreads();
        if (threadIdx.x < 2 * TP * TQ) {
            const int pr = (int)threadIdx.x / 2, part = (int)threadIdx.x & 1;
            const int a = pr % TP, c = pr / TP;
            if (i0 + a < p && j0 + c < q) seg_out[(2 * ((int64_t)(j0 + c) * p + (i0 + a)) + part) * nseg + s] = pair_total(lds[threadIdx.x]);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// X <- X * inv(R); S: the widest block of the instance (the factor's tile in LDS), PW <= S: columns of a panel
// ---------------------------------------------------------------------------------------------
template <typename R, int S, int PW>
__global__ __launch_bounds__(MIK_BLOCK) void k_cblock_rdiv(int64_t n, int s, const R *__restrict__ Rd /* device, s x s, leading dimension s */,
                                                            R *X, int64_t ldx)
{
    __shared__ R Rs[2 * S * S];                             // Rs[2 * (j * S + i)] = R[j, i]
    for (int idx = (int)threadIdx.x; idx < S * S; idx += MIK_BLOCK) {
        const int j = idx / S, i = idx % S;
        const bool in = i < s && j <= i;
        Rs[2 * idx] = in ? Rd[2 * ((int64_t)i * s + j)] : R(1);
        Rs[2 * idx + 1] = in ? Rd[2 * ((int64_t)i * s + j) + 1] : R(0);
    }
    __syncthreads();
#pragma nounroll
    for (int64_t row = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; row < n; row += (int64_t)gridDim.x * MIK_BLOCK) {
#pragma unroll
        for (int c0 = 0; c0 < S; c0 += PW) {
            if (c0 < s) {
                R xr[PW], xi[PW];
#pragma unroll
                for (int i = 0; i < PW; ++i) {
                    xr[i] = R(0);
                    xi[i] = R(0);
                    if (c0 + i < s) {
                        const CxVal<R> v = cx_ld<R>(X + 2 * ((int64_t)(c0 + i) * ldx + row));
                        xr[i] = v.re;
                        xi[i] = v.im;
                    }
                }
                // the finished columns before the panel, as this lane stored them, j ascending
#pragma nounroll
                for (int j = 0; j < c0; ++j) {
                    asm volatile("" ::: "memory");          // the factor is re-read from LDS row by row, not hoisted out of the row loop
                    const CxVal<R> xj = cx_ld<R>(X + 2 * ((int64_t)j * ldx + row));
#pragma unroll
                    for (int i = 0; i < PW; ++i) {
                        const CxVal<R> pr = cx_mul(xj.re, xj.im, Rs[2 * (j * S + c0 + i)], Rs[2 * (j * S + c0 + i) + 1]);
                        xr[i] = xr[i] - pr.re;
                        xi[i] = xi[i] - pr.im;
                    }
                }
                // the panel: column j is complete once the columns before it have been subtracted -- divide it, then subtract it from every
                // column behind it (k_block_rdiv's order; the fence keeps one row of the factor live at a time)
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    if (c0 + j < s) {
                        const R d = Rs[2 * ((c0 + j) * S + c0 + j)];
                        xr[j] = xr[j] / d;
                        xi[j] = xi[j] / d;
#pragma unroll
                        for (int i = j + 1; i < PW; ++i) {
                            const CxVal<R> pr = cx_mul(xr[j], xi[j], Rs[2 * ((c0 + j) * S + c0 + i)], Rs[2 * ((c0 + j) * S + c0 + i) + 1]);
                            xr[i] = xr[i] - pr.re;
                            xi[i] = xi[i] - pr.im;
                        }
                    }
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int i = 0; i < PW; ++i)
                    if (c0 + i < s) cx_st<R>(X + 2 * ((int64_t)(c0 + i) * ldx + row), xr[i], xi[i]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Pout = rot(R, Vr) (+ rot(P, Vp)); Xout = rot(X, Vx) (+ Pout), output columns [blockIdx.y * LB, blockIdx.y * LB + LB)
// ---------------------------------------------------------------------------------------------
// acc[jj] = (...(W[row, 0] * F[0, jj] + W[row, 1] * F[1, jj]) + ...) + W[row, k - 1] * F[k - 1, jj]; F in LDS, F[c, jj] at F + 2 * (c * LB + jj)
template <typename R, int LB>
__device__ __forceinline__ void cblk_rot_row(const R *__restrict__ Wm, int64_t ld, int k, const R *F, int64_t row, R (&ar)[LB], R (&ai)[LB])
{
    constexpr int U = 2;                                    // columns of the block in flight per lane
    {
        const CxVal<R> v = cx_ld<R>(Wm + 2 * row);
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            const CxVal<R> pr = cx_mul(v.re, v.im, F[2 * jj], F[2 * jj + 1]);
            ar[jj] = pr.re;
            ai[jj] = pr.im;
        }
    }
    int c = 1;
    for (; c + U <= k; c += U) {
        CxVal<R> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = cx_ld<R>(Wm + 2 * ((int64_t)(c + u) * ld + row));
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) {
                const CxVal<R> pr = cx_mul(v[u].re, v[u].im, F[2 * ((c + u) * LB + jj)], F[2 * ((c + u) * LB + jj) + 1]);
                ar[jj] = ar[jj] + pr.re;
                ai[jj] = ai[jj] + pr.im;
            }
    }
    for (; c < k; ++c) {
        const CxVal<R> v = cx_ld<R>(Wm + 2 * ((int64_t)c * ld + row));
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            const CxVal<R> pr = cx_mul(v.re, v.im, F[2 * (c * LB + jj)], F[2 * (c * LB + jj) + 1]);
            ar[jj] = ar[jj] + pr.re;
            ai[jj] = ai[jj] + pr.im;
        }
    }
}

template <typename R, int LB>
__global__ __launch_bounds__(MIK_BLOCK) void k_cblock_update(int64_t n, int sx, int b1, int b2, const R *__restrict__ X, int64_t ldx,
                                                              const R *__restrict__ Rm, int64_t ldr, const R *__restrict__ P, int64_t ldp,
                                                              const R *__restrict__ Vd /* device, (sx + b1 + b2) x sx, packed */,
                                                              R *__restrict__ Xout, int64_t ldxo, R *__restrict__ Pout, int64_t ldpo)
{
    __shared__ R Fs[2 * 3 * MIK_BLK_MAX * LB];              // Fs[2 * (c * LB + jj)] = V[c, c0 + jj]: rows [0, sx) Vx, then Vr, then Vp
    const int k = sx + b1 + b2;
    const int c0 = (int)blockIdx.y * LB;                    // this workgroup's panel of output columns
    for (int idx = (int)threadIdx.x; idx < k * LB; idx += MIK_BLOCK) {
        const int c = idx / LB, jj = idx % LB;
        const bool in = c0 + jj < sx;
        Fs[2 * idx] = in ? Vd[2 * ((int64_t)(c0 + jj) * k + c)] : R(0);
        Fs[2 * idx + 1] = in ? Vd[2 * ((int64_t)(c0 + jj) * k + c) + 1] : R(0);
    }
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; row < n; row += (int64_t)gridDim.x * MIK_BLOCK) {
        R pr[LB], pi[LB], ar[LB], ai[LB];
        if (b1 > 0) {
            cblk_rot_row<R, LB>(Rm, ldr, b1, Fs + 2 * sx * LB, row, pr, pi);
            if (b2 > 0) {
                cblk_rot_row<R, LB>(P, ldp, b2, Fs + 2 * (sx + b1) * LB, row, ar, ai);
#pragma unroll
                for (int jj = 0; jj < LB; ++jj) { pr[jj] = pr[jj] + ar[jj]; pi[jj] = pi[jj] + ai[jj]; }
            }
#pragma unroll
            for (int jj = 0; jj < LB; ++jj)
                if (c0 + jj < sx) cx_st<R>(Pout + 2 * ((int64_t)(c0 + jj) * ldpo + row), pr[jj], pi[jj]);
        }
        cblk_rot_row<R, LB>(X, ldx, sx, Fs, row, ar, ai);
        if (b1 > 0) {
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) { ar[jj] = ar[jj] + pr[jj]; ai[jj] = ai[jj] + pi[jj]; }
        }
#pragma unroll
        for (int jj = 0; jj < LB; ++jj)
            if (c0 + jj < sx) cx_st<R>(Xout + 2 * ((int64_t)(c0 + jj) * ldxo + row), ar[jj], ai[jj]);
    }
}

#endif  // __HIPCC__
