// mik_dense_cmul.h -- kernels of the dense matrix-vector product on a COMPLEX column-major device matrix (MIK_C64 / MIK_C32, interleaved
// re, im): mul!(y, A, x) and mul!(y, adjoint(A), x) for A::Matrix{ComplexF64 / ComplexF32} (test/cg.jl:27, test/gmres.jl:16).
// DESIGN.md section 18; the contract is the one of include/mik.h ("dense operator").
//
// The kernels are templates on the component type R; a matrix of m x n complex elements is walked as 2 m x n reals (lda2 = 2 lda), so a
// 16-byte load is one ComplexF64 row or two ComplexF32 rows of a column.  Nothing is contracted: every product and every sum is rounded.
//   N form  y = A x:   chunks of MIK_DM_C columns; p_c[i] = serial sum from (+0, +0) over the chunk's columns ascending of
//                      cx_mul(A[i, j], x[j]), re and im each their own chain; y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ... componentwise -- the
//                      partials are [chunk][row] complex elements, which k_dense_n_combine<R> sums as 2 m reals.
//   T form  y = A' x:  y[j] = mik_dot(A[:, j], x) of the complex mik_dot (cx_dot_acc in csrc/mik_complex.h): per element
//                      re = ar xr + ai xi, im = ar xi - ai xr, one tree for re and one for im (pair_put / pair_total = block_tree_256,
//                      then k_finalize_store<R> over [column][re, im][segment]).
#pragma once
#include "mik_internal.h"
#include "mik_kernels.h"
#include "mik_complex.h"
#include "mik_dense_mul.h"

constexpr int MIK_CDM_R = 512;         // rows per workgroup of the complex N form: 256 lanes x 16 bytes x (ComplexF64: 2 passes, ComplexF32: 1 pass)
constexpr int MIK_CDM_U = 8;           // columns whose loads a lane issues before it consumes the first (as MIK_DM_U: the same 16-byte loads in flight
                                       // per lane as the real kernel of the same component type)
constexpr int MIK_CDM_TCOLS = 32;      // columns a workgroup of the T form sweeps per segment of x it holds in registers
constexpr int MIK_CDM_TQ = 4;          // ... of which 4 are in flight at a time

// ---- N form ---------------------------------------------------------------------------------------------------------------------
// CW complex rows of a column (col: its first real) starting at row r, as 2 CW reals.  FULL: one unconditional 16-byte load.  Otherwise
// scalar loads from rows clamped into [0, m): branch-free; what a clamped row computes is never stored.
template <typename R, bool FULL, bool NT>
__device__ __forceinline__ void cdm_load(const R *__restrict__ col, int64_t r, int64_t m, R (&v)[VT<R>::W])
{
    constexpr int W = VT<R>::W, CW = W / 2;
    if (FULL) {
        auto cv = NT ? vload_nt(col + 2 * r) : vload(col + 2 * r);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = el<R>(cv, e);
    } else {
#pragma unroll
        for (int e = 0; e < CW; ++e) {
            const int64_t i = (r + e < m) ? r + e : m - 1;
            v[2 * e] = col[2 * i];
            v[2 * e + 1] = col[2 * i + 1];
        }
    }
}

// acc += a * (xr + xi i) for the CW complex rows of one 16-byte group: the rounded product, then one rounded add per component
template <typename R>
__device__ __forceinline__ void cdm_madd(const R (&a)[VT<R>::W], R xr, R xi, R (&acc)[VT<R>::W])
{
#pragma unroll
    for (int e = 0; e < VT<R>::W; e += 2) cx_madd(a[e], a[e + 1], xr, xi, acc[e], acc[e + 1]);
}

// p_c of one chunk for the rows of one lane: U columns are requested before the first is consumed, the consumption order is the column
// order.  xq points at the first real of the chunk's first element of x; x is uniform over the workgroup: scalar loads of exactly the
// elements 0 .. jn - 1.
template <typename R, bool FULL, bool NT, int P, int U>
__device__ __forceinline__ void cdm_chunk(const R *__restrict__ Ac, int64_t lda2, const R *__restrict__ xq, int jn, int64_t r0, int64_t m,
                                          R (&acc)[P][VT<R>::W])
{
    constexpr int W = VT<R>::W, CW = W / 2;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int e = 0; e < W; ++e) acc[p][e] = R(0);
    int j = 0;
    for (; j + U <= jn; j += U) {
        R a[U][P][W];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int p = 0; p < P; ++p) cdm_load<R, FULL, NT>(Ac + (int64_t)(j + u) * lda2, r0 + (int64_t)p * MIK_BLOCK * CW, m, a[u][p]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const R xr = xq[2 * (j + u)], xi = xq[2 * (j + u) + 1];
#pragma unroll
            for (int p = 0; p < P; ++p) cdm_madd<R>(a[u][p], xr, xi, acc[p]);
        }
    }
    for (; j < jn; ++j) {
        R a[P][W];
#pragma unroll
        for (int p = 0; p < P; ++p) cdm_load<R, FULL, NT>(Ac + (int64_t)j * lda2, r0 + (int64_t)p * MIK_BLOCK * CW, m, a[p]);
        const R xr = xq[2 * j], xi = xq[2 * j + 1];
#pragma unroll
        for (int p = 0; p < P; ++p) cdm_madd<R>(a[p], xr, xi, acc[p]);
    }
}

// y = A x: out[2 * (c * out_stride + i)] = p_c[i] (re, im).  grid = (row blocks of RW rows, chunks [grid-stride]).  Rows across lanes:
// lane t owns, per pass p, the CW consecutive rows starting at blockIdx.x * RW + p * 256 * CW + CW * t -- one 16-byte load per column
// when VEC and the row block is whole; the scalar variant owns the same rows and gives the same bits.
template <typename R, int RW, bool VEC, bool NT, int C>
__global__ __launch_bounds__(MIK_BLOCK) void k_cdense_n(int64_t m, int64_t n, const R *__restrict__ A, int64_t lda, const R *__restrict__ x,
                                                         R *__restrict__ out, int64_t out_stride)
{
    constexpr int W = VT<R>::W, CW = W / 2, P = RW / (MIK_BLOCK * CW);
    static_assert(P >= 1 && P * MIK_BLOCK * CW == RW, "rows per workgroup: whole passes of 256 lanes x 16 bytes");
    const int64_t lda2 = 2 * lda;
    const int64_t r0 = (int64_t)blockIdx.x * RW + (int64_t)CW * threadIdx.x;
    const bool full = VEC && ((int64_t)blockIdx.x + 1) * RW <= m;
    for (int64_t c = blockIdx.y; c * C < n; c += gridDim.y) {
        const int64_t j0 = c * C;
        const int jn = (int)((n - j0 < C) ? n - j0 : C);
        R acc[P][W];
        R *__restrict__ o = out + 2 * c * out_stride;
        if (full) {
            cdm_chunk<R, true, NT, P, MIK_CDM_U>(A + j0 * lda2, lda2, x + 2 * j0, jn, r0, m, acc);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                typename VT<R>::vec ov;
#pragma unroll
                for (int e = 0; e < W; ++e) el<R>(ov, e) = acc[p][e];
                vstore(o + 2 * (r0 + (int64_t)p * MIK_BLOCK * CW), ov);
            }
        } else {
            cdm_chunk<R, false, false, P, MIK_CDM_U>(A + j0 * lda2, lda2, x + 2 * j0, jn, r0, m, acc);
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int e = 0; e < CW; ++e) {
                    const int64_t r = r0 + (int64_t)p * MIK_BLOCK * CW + e;
                    if (r < m) { o[2 * r] = acc[p][2 * e]; o[2 * r + 1] = acc[p][2 * e + 1]; }
                }
        }
    }
}

// ---- T form ---------------------------------------------------------------------------------------------------------------------
// The thread sums (re, im) of Q columns against a segment that lies wholly inside the 2 m reals, 16-byte aligned: l ascending, then the
// elements of a 16-byte group ascending, as k_cvec walks them, each element by cx_dot_acc; the Q x L loads are requested before the
// first is consumed.
template <typename R, bool NT, int Q>
__device__ __forceinline__ void cdm_dot_cols_full(const R *__restrict__ A0, int64_t lda2, int64_t base, const R (&w)[SEG_REGS<R>], R (&re)[Q], R (&im)[Q])
{
    constexpr int W = VT<R>::W;
    typename VT<R>::vec cv[Q][MIK_RED_L];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int l = 0; l < MIK_RED_L; ++l) {
            const R *p = A0 + (int64_t)q * lda2 + base + (int64_t)l * MIK_BLOCK * W;
            cv[q][l] = NT ? vload_nt(p) : vload(p);
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        R a0 = R(0), a1 = R(0);
#pragma unroll
        for (int l = 0; l < MIK_RED_L; ++l)
#pragma unroll
            for (int e = 0; e < W; e += 2) cx_dot_acc(el<R>(cv[q][l], e), el<R>(cv[q][l], e + 1), w[l * W + e], w[l * W + e + 1], a0, a1);
        re[q] = a0;
        im[q] = a1;
    }
}

// ... of one column of any segment: a 16-byte load when VEC and the group lies inside n2, else the elements inside n2 one by one
template <typename R, bool VEC>
__device__ __forceinline__ void cdm_dot_col(const R *__restrict__ col, int64_t base, int64_t n2, const R (&w)[SEG_REGS<R>], R &re, R &im)
{
    constexpr int W = VT<R>::W;
    R a0 = R(0), a1 = R(0);
#pragma unroll
    for (int l = 0; l < MIK_RED_L; ++l) {
        const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
        if (VEC && i + W <= n2) {
            auto cv = vload(col + i);
#pragma unroll
            for (int e = 0; e < W; e += 2) cx_dot_acc(el<R>(cv, e), el<R>(cv, e + 1), w[l * W + e], w[l * W + e + 1], a0, a1);
        } else {
#pragma unroll
            for (int e = 0; e < W; e += 2)
                if (i + e < n2) cx_dot_acc(col[i + e], col[i + e + 1], w[l * W + e], w[l * W + e + 1], a0, a1);
        }
    }
    re = a0;
    im = a1;
}

// Segment sums of conj(A[:, j]) .* x for every column j: seg_out[(2 j + c) * nseg + s], c = 0: re, 1: im.  m2 = 2 m reals; the segments are
// those of the real 2 m-vector (= the segments of the complex m-vector).  grid = (segments [grid-stride], column batches [grid-stride]).
// k_dense_t's scheme: a workgroup holds its segment of x in registers and sweeps MIK_CDM_TCOLS columns against it, MIK_CDM_TQ at a time.
template <typename R, bool VEC, bool NT>
__global__ __launch_bounds__(MIK_BLOCK) void k_cdense_t(int64_t m2, int64_t nseg, int64_t n, const R *__restrict__ A, int64_t lda,
                                                         const R *__restrict__ x, R *__restrict__ seg_out)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<R>;
    constexpr int Q = MIK_CDM_TQ;
    __shared__ R lds[2 * Q][4];
    const int64_t lda2 = 2 * lda;
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<R>::W * threadIdx.x;
        const bool full = VEC && (s + 1) * SEG <= m2;
        R xr[SEG_REGS<R>];
        seg_load<R, VEC>(x, base, m2, 0, xr);
        for (int64_t jb = (int64_t)blockIdx.y * MIK_CDM_TCOLS; jb < n; jb += (int64_t)gridDim.y * MIK_CDM_TCOLS) {
            const int64_t je = (jb + MIK_CDM_TCOLS < n) ? jb + MIK_CDM_TCOLS : n;
            for (int64_t j = jb; j < je; j += Q) {
                const int k = (int)((je - j < Q) ? je - j : Q);
                R re[Q], im[Q];
                if (full && k == Q) {
                    cdm_dot_cols_full<R, NT, Q>(A + j * lda2, lda2, base, xr, re, im);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        re[q] = R(0); im[q] = R(0);
                        if (q < k) cdm_dot_col<R, VEC>(A + (j + q) * lda2, base, m2, xr, re[q], im[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) { pair_put(re[q], lds[2 * q]); pair_put(im[q], lds[2 * q + 1]); }
                __syncthreads();
                if ((int)threadIdx.x < 2 * k) seg_out[(2 * j + threadIdx.x) * nseg + s] = pair_total(lds[threadIdx.x]);
                __syncthreads();
            }
        }
    }
}
