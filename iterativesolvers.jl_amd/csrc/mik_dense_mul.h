// mik_dense_mul.h -- kernels of the dense matrix-vector product on a column-major device matrix: mul!(y, A, x) and mul!(y, adjoint(A), x)
// for A::Matrix (src/cg.jl:54,137; src/gmres.jl:245,287; src/lsqr.jl, src/lsmr.jl, src/qmr.jl, src/svdl.jl for the adjoint).
//
// The arithmetic is the contract of include/mik.h ("dense operator"): no FMA, every product and every sum rounded on its own.
//   N form  y = A x:   the columns are cut into chunks of MIK_DM_C; p_c[i] = serial sum from +0 over the chunk's columns ascending of
//                      A[i, j] * x[j];  y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ...   A row's result depends on (n, C) only.
//   block   Y = A X:   the N form for up to MIK_DM_GW right-hand sides through one read of A (k_dense_nb); k_dense_n is the same body
//                      (dm_rows) with one right-hand side, so a column of Y has the bits of y = A x by construction.
//   T form  y = A' x:  y[j] = mik_dot(A[:, j], x): the segment toolkit (seg_load / seg_dot_col), the shape of block_tree_256 and
//                      k_finalize_store -- the bits of mik_dot by construction.
// The kernels are templates on the chunk so that scripts/micro/dense_chunk.hip can time other chunks than the library's one.
#pragma once
#include "mik_internal.h"
#include "mik_kernels.h"

constexpr int MIK_DM_C = 64;           // columns per chunk of the N form (one compile-time constant for both dtypes)
constexpr double MIK_DM_STREAM_BYTES = 192.0e6;   // a matrix of more bytes is read with non-temporal loads: the caches cannot keep it between products
constexpr int MIK_DM_R = 1024;         // rows per workgroup of the N form: 256 lanes x 16 bytes x (fp64: 2 passes, fp32: 1 pass)
constexpr int MIK_DM_U = 8;            // columns whose loads a lane issues before it consumes the first: 8 x 16 B x passes in flight per lane
constexpr int MIK_DM_GW = 8;           // right-hand sides a workgroup of the block form (Y = A X) carries through one read of A
constexpr int MIK_DM_BMAX = 32;        // widest block of mik_dense_mm (the width of mik_spmm and the other block entries)
constexpr int MIK_DM_UB = 4;           // ... with 4 columns in flight, so that the 4 rows x 8 accumulators of a Float64 lane fit next to the loads
constexpr int MIK_DM_UN = 1;           // ... and 1 in its scalar-load rows
constexpr int MIK_DM_TCOLS = 32;       // columns a workgroup of the T form sweeps per segment of x it holds in registers
constexpr int MIK_DM_TQ = 4;           // ... of which 4 are in flight at a time (4 x 2 x 16 B per lane = 32 KiB per workgroup)

// ---- N form ---------------------------------------------------------------------------------------------------------------------
// W elements of a column starting at row r.  FULL: the whole row block lies inside m and every column start is 16-byte aligned -- one
// unconditional 16-byte load.  Otherwise scalar loads from rows clamped into [0, m): branch-free, so that the loads of several columns
// stay in flight together; what a clamped row computes is never stored.
template <typename T, bool FULL, bool NT>
__device__ __forceinline__ void dm_load(const T *__restrict__ col, int64_t r, int64_t m, T (&v)[VT<T>::W])
{
    constexpr int W = VT<T>::W;
    if (FULL) {
        auto cv = NT ? vload_nt(col + r) : vload(col + r);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = el<T>(cv, e);
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = col[(r + e < m) ? r + e : m - 1];
    }
}

// p_c of one chunk for the rows of one lane, for G right-hand sides at once: the serial sums from +0 over the chunk's jn columns
// ascending.  U columns are requested before the first is consumed; the consumption order is the column order, and every element of A
// is multiplied into the G accumulators of its row -- each product and each sum rounded on its own, so a right-hand side gets the bits
// it gets alone (G = 1).  xq[g] points at the chunk's first element of right-hand side g; x is uniform over the workgroup: scalar loads
// of exactly the elements 0 .. jn - 1.
template <typename T, bool FULL, bool NT, int P, int G, int U>
__device__ __forceinline__ void dm_chunk(const T *__restrict__ Ac, int64_t lda, const T *const (&xq)[G], int jn, int64_t r0, int64_t m,
                                         T (&acc)[G][P][VT<T>::W])
{
    constexpr int W = VT<T>::W;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int e = 0; e < W; ++e) acc[g][p][e] = T(0);
    int j = 0;
    for (; j + U <= jn; j += U) {
        T a[U][P][W];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int p = 0; p < P; ++p) dm_load<T, FULL, NT>(Ac + (int64_t)(j + u) * lda, r0 + (int64_t)p * MIK_BLOCK * W, m, a[u][p]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const T xj = xq[g][j + u];
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int e = 0; e < W; ++e) { T pr = a[u][p][e] * xj; acc[g][p][e] = acc[g][p][e] + pr; }
            }
    }
    for (; j < jn; ++j) {
        T a[P][W];
#pragma unroll
        for (int p = 0; p < P; ++p) dm_load<T, FULL, NT>(Ac + (int64_t)j * lda, r0 + (int64_t)p * MIK_BLOCK * W, m, a[p]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const T xj = xq[g][j];
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int e = 0; e < W; ++e) { T pr = a[p][e] * xj; acc[g][p][e] = acc[g][p][e] + pr; }
        }
    }
}

// The chunks of one workgroup against its MIK_DM_R rows, for w <= G right-hand sides x[:, 0 .. w - 1] (leading dimension ldx):
// out[g * col_stride + c * chunk_stride + i] = p_c[i] of right-hand side g.  grid = (row blocks, chunks [grid-stride]).
// Rows across lanes: lane t owns, per pass p, the W consecutive rows starting at blockIdx.x * R + p * 256 * W + W * t (a 16-byte load
// per column when VEC and the row block is whole; the scalar variant owns the same rows).  A row's arithmetic does not depend on which
// variant or lane computes it, nor on G or w: the surplus accumulators g >= w read right-hand side w - 1 again (no address outside the
// block is formed) and are never stored.
template <typename T, bool VEC, bool NT, int C, int G, int U>
__device__ __forceinline__ void dm_rows(int64_t m, int64_t n, const T *__restrict__ A, int64_t lda, const T *__restrict__ x, int64_t ldx, int w,
                                        T *__restrict__ out, int64_t col_stride, int64_t chunk_stride)
{
    constexpr int W = VT<T>::W, P = MIK_DM_R / (MIK_BLOCK * W);
    // the clamped scalar loads carry a 64-bit address per element: next to G > 1 sets of accumulators they keep fewer columns in flight, so that
    // the ragged last row block does not set the register allocation of the whole kernel
    constexpr int UN = G > 1 ? MIK_DM_UN : U;
    const int64_t r0 = (int64_t)blockIdx.x * MIK_DM_R + (int64_t)W * threadIdx.x;
    const bool full = VEC && ((int64_t)blockIdx.x + 1) * MIK_DM_R <= m;
    for (int64_t c = blockIdx.y; c * C < n; c += gridDim.y) {
        const int64_t j0 = c * C;
        const int jn = (int)((n - j0 < C) ? n - j0 : C);
        const T *xq[G];
#pragma unroll
        for (int g = 0; g < G; ++g) xq[g] = x + (int64_t)(g < w ? g : w - 1) * ldx + j0;
        T acc[G][P][W];
        T *__restrict__ o = out + c * chunk_stride;
        if (full) {
            dm_chunk<T, true, NT, P, G, U>(A + j0 * lda, lda, xq, jn, r0, m, acc);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g >= w) break;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    typename VT<T>::vec ov;
#pragma unroll
                    for (int e = 0; e < W; ++e) el<T>(ov, e) = acc[g][p][e];
                    vstore(o + g * col_stride + r0 + (int64_t)p * MIK_BLOCK * W, ov);
                }
            }
        } else {
            dm_chunk<T, false, false, P, G, UN>(A + j0 * lda, lda, xq, jn, r0, m, acc);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g >= w) break;
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const int64_t r = r0 + (int64_t)p * MIK_BLOCK * W + e;
                        if (r < m) o[g * col_stride + r] = acc[g][p][e];
                    }
            }
        }
    }
}

// y = A x: one right-hand side, out[c * out_stride + i] = p_c[i].
template <typename T, bool VEC, bool NT, int C>
__global__ __launch_bounds__(MIK_BLOCK) void k_dense_n(int64_t m, int64_t n, const T *__restrict__ A, int64_t lda, const T *__restrict__ x,
                                                        T *__restrict__ out, int64_t out_stride)
{
    dm_rows<T, VEC, NT, C, 1, MIK_DM_U>(m, n, A, lda, x, 0, 1, out, 0, out_stride);
}

// Y[:, g] = A X[:, g] for the w <= G right-hand sides of one group: A is read once for all of them.
template <typename T, bool VEC, bool NT, int C, int G>
__global__ __launch_bounds__(MIK_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void k_dense_nb(int64_t m, int64_t n, const T *__restrict__ A, int64_t lda, const T *__restrict__ X,
                                                         int64_t ldx, int w, T *__restrict__ out, int64_t col_stride, int64_t chunk_stride)
{
    dm_rows<T, VEC, NT, C, G, MIK_DM_UB>(m, n, A, lda, X, ldx, w, out, col_stride, chunk_stride);
}

// y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ... over nc >= 2 chunk partials, one lane per row, one wave per workgroup (n = 16384: 256
// workgroups instead of 64).  The sum is one serial chain per row; PF independent loads are requested ahead of it, so a row costs
// nc / PF memory round trips.  PF never changes a bit.  grid.y = right-hand sides: column g reads its partials part_col elements
// after those of column g - 1 and writes ldy elements after it (one right-hand side: grid.y = 1).
constexpr int MIK_DM_CB = 64;          // threads per workgroup of the combine kernel
constexpr int MIK_DM_PF = 32;          // partials requested ahead of the chain
template <typename T, int PF>
__global__ __launch_bounds__(MIK_DM_CB) void k_dense_n_combine(int64_t m, int64_t nc, const T *__restrict__ part, int64_t stride, T *__restrict__ y,
                                                               int64_t part_col, int64_t ldy)
{
    const int64_t i = (int64_t)blockIdx.x * MIK_DM_CB + threadIdx.x;
    if (i >= m) return;
    part += (int64_t)blockIdx.y * part_col;
    y += (int64_t)blockIdx.y * ldy;
    T acc = part[i];
    int64_t c = 1;
    for (; c + PF <= nc; c += PF) {
        T v[PF];
#pragma unroll
        for (int q = 0; q < PF; ++q) v[q] = part[(c + q) * stride + i];
#pragma unroll
        for (int q = 0; q < PF; ++q) acc = acc + v[q];
    }
    for (; c + 8 <= nc; c += 8) {
        T v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = part[(c + q) * stride + i];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = acc + v[q];
    }
    for (; c < nc; ++c) acc = acc + part[c * stride + i];
    y[i] = acc;
}

// ---- T form ---------------------------------------------------------------------------------------------------------------------
// seg_dot_col for Q columns of a segment that lies wholly inside m, 16-byte aligned: the same per-thread order (l ascending, then e
// ascending, every product rounded before it is added), but the Q x L loads are requested before the first is consumed.
template <typename T, bool NT, int Q>
__device__ __forceinline__ void dm_dot_cols_full(const T *__restrict__ A0, int64_t lda, int64_t base, const T (&w)[SEG_REGS<T>], T (&acc)[Q])
{
    constexpr int W = VT<T>::W;
    typename VT<T>::vec cv[Q][MIK_RED_L];
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int l = 0; l < MIK_RED_L; ++l) {
            const T *p = A0 + (int64_t)q * lda + base + (int64_t)l * MIK_BLOCK * W;
            cv[q][l] = NT ? vload_nt(p) : vload(p);
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        T a = T(0);
#pragma unroll
        for (int l = 0; l < MIK_RED_L; ++l)
#pragma unroll
            for (int e = 0; e < W; ++e) { T p = el<T>(cv[q][l], e) * w[l * W + e]; a = a + p; }
        acc[q] = a;
    }
}

// Segment sums of A[:, j] .* x for every column j: seg_out[j * nseg + s].  grid = (segments [grid-stride], column batches [grid-stride]).
// A workgroup holds its segment of x in registers (read once per pass) and sweeps MIK_DM_TCOLS columns against it, MIK_DM_TQ at a
// time: every column is read once.  Per column: the thread sums of seg_dot_col, the wave tree, the 4 wave sums left to right
// (pair_put / pair_total = the shape of block_tree_256) -- what OpDot in k_map gives mik_dot.
template <typename T, bool VEC, bool NT>
__global__ __launch_bounds__(MIK_BLOCK) void k_dense_t(int64_t m, int64_t nseg, int64_t n, const T *__restrict__ A, int64_t lda,
                                                        const T *__restrict__ x, T *__restrict__ seg_out)
{
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * SEG_REGS<T>;
    constexpr int Q = MIK_DM_TQ;
    __shared__ T lds[Q][4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)VT<T>::W * threadIdx.x;
        const bool full = VEC && (s + 1) * SEG <= m;
        T xr[SEG_REGS<T>];
        seg_load<T, VEC>(x, base, m, 0, xr);
        for (int64_t jb = (int64_t)blockIdx.y * MIK_DM_TCOLS; jb < n; jb += (int64_t)gridDim.y * MIK_DM_TCOLS) {
            const int64_t je = (jb + MIK_DM_TCOLS < n) ? jb + MIK_DM_TCOLS : n;
            for (int64_t j = jb; j < je; j += Q) {
                const int k = (int)((je - j < Q) ? je - j : Q);
                T acc[Q];
                if (full && k == Q) {
                    dm_dot_cols_full<T, NT, Q>(A + j * lda, lda, base, xr, acc);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; ++q) acc[q] = (q < k) ? seg_dot_col<T, VEC>(A + (j + q) * lda, base, m, 0, xr) : T(0);
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) pair_put(acc[q], lds[q]);
                __syncthreads();
                if ((int)threadIdx.x < k) seg_out[(j + threadIdx.x) * nseg + s] = pair_total(lds[threadIdx.x]);
                __syncthreads();
            }
        }
    }
}
