// mik_svdl.h -- kernels behind svdl (src/svdl.jl): the basis rotation of the thick restart and the two sweeps of one classical
// Gram-Schmidt pass with the squared norm of the vector riding on each of them.
//
//   k_basis_rotate   Y[:, 0:l] = V[:, 0:k] * F[0:k, 0:l]            -- src/svdl.jl:384, :392, :470, :471, :231, :237
//       A lane owns W = 16 B / sizeof(T) consecutive rows and LB output columns: W * LB accumulators in registers.  It walks the k
//       columns of V once (coalesced 16-byte loads, four columns in flight) and multiplies by the row F[c, j0 .. j0 + LB) that the
//       workgroup staged in LDS (every lane reads the same address: a broadcast, no bank conflict).  Every product and every sum is
//       rounded on its own, columns ascending, the first product opening the sum -- an output element depends on its own row only, so
//       the bits do not depend on the launch shape.  blockIdx.y selects the block of LB output columns (l > 32 reads V twice).
//   k_multidot_sq    k_multidot (h = Q' q) + the segment sums of q .* q   -- src/svdl.jl:569-570 (oldqnorm and Q'q from one read of q)
//   k_gemv_n_sq      k_gemv_n (q += alpha * Q h) + the segment sums of the new q .* q   -- :570-571 (q -= Q h and norm(q) from one sweep)
//       Both keep the thread / segment / tree shape of OpDot in k_map, so each squared norm has the bits mik_nrm2 would give.
#pragma once
#include "mik_kernels.h"

#ifdef __HIPCC__

constexpr int MIK_ROT_MAX = 64;      // 1 <= l <= k <= MIK_ROT_MAX
constexpr int MIK_ROT_UNROLL = 4;    // columns of V in flight per lane

template <typename T, bool VEC>
__device__ __forceinline__ void rot_load(const T *__restrict__ col, int64_t i, int64_t n, bool full, T (&v)[VT<T>::W])
{
    constexpr int W = VT<T>::W;
    if (VEC && full) {
        auto cv = vload(col + i);
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = el<T>(cv, e);
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[e] = (i + e < n) ? col[i + e] : T(0);
    }
}

template <typename T, bool VEC, int LB>
__global__ __launch_bounds__(MIK_BLOCK) void k_basis_rotate(int64_t n, int k, int l, const T *__restrict__ V, int64_t ldv,
                                                             const T *__restrict__ F /* device, k x l, leading dimension k */,
                                                             T *__restrict__ Y, int64_t ldy)
{
    constexpr int W = VT<T>::W;
    constexpr int U = MIK_ROT_UNROLL;
    __shared__ T Fs[MIK_ROT_MAX * LB];                      // Fs[c * LB + jj] = F[c, j0 + jj]
    const int j0 = (int)blockIdx.y * LB;
    const int lb = min(LB, l - j0);
    for (int idx = (int)threadIdx.x; idx < k * LB; idx += MIK_BLOCK) {
        const int c = idx / LB, jj = idx % LB;
        Fs[idx] = jj < lb ? F[(int64_t)(j0 + jj) * k + c] : T(0);
    }
    __syncthreads();
    const int64_t groups = (n + W - 1) / W;
    for (int64_t g = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; g < groups; g += (int64_t)gridDim.x * MIK_BLOCK) {
        const int64_t i = g * W;
        const bool full = i + W <= n;
        T acc[LB][W];
        T v[U][W];
        rot_load<T, VEC>(V, i, n, full, v[0]);
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            const T f = Fs[jj];
#pragma unroll
            for (int e = 0; e < W; ++e) acc[jj][e] = v[0][e] * f;
        }
        int c = 1;
        for (; c + U <= k; c += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) rot_load<T, VEC>(V + (int64_t)(c + u) * ldv, i, n, full, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int jj = 0; jj < LB; ++jj) {
                    const T f = Fs[(c + u) * LB + jj];
#pragma unroll
                    for (int e = 0; e < W; ++e) { T p = v[u][e] * f; acc[jj][e] = acc[jj][e] + p; }
                }
            }
        }
        for (; c < k; ++c) {
            rot_load<T, VEC>(V + (int64_t)c * ldv, i, n, full, v[0]);
#pragma unroll
            for (int jj = 0; jj < LB; ++jj) {
                const T f = Fs[c * LB + jj];
#pragma unroll
                for (int e = 0; e < W; ++e) { T p = v[0][e] * f; acc[jj][e] = acc[jj][e] + p; }
            }
        }
#pragma unroll
        for (int jj = 0; jj < LB; ++jj) {
            if (jj < lb) {
                T *__restrict__ out = Y + (int64_t)(j0 + jj) * ldy + i;
                if (VEC && full) {
                    typename VT<T>::vec o;
#pragma unroll
                    for (int e = 0; e < W; ++e) el<T>(o, e) = acc[jj][e];
                    vstore(out, o);
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (i + e < n) out[e] = acc[jj][e];
                }
            }
        }
    }
}

// k_multidot with one more reduced column: seg_out[j][s] = segment sum of Q[:, j] .* q for j < k, seg_out[k][s] = that of q .* q.
template <typename T, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_multidot_sq(int64_t n, int64_t nseg, int k, const T *__restrict__ Q, int64_t ldq,
                                                            const T *__restrict__ q, T *__restrict__ seg_out /* [k + 1][nseg] */, int nt)
{
    constexpr int W = VT<T>::W;
    constexpr int L = MIK_RED_L;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * W * L;
    __shared__ T lds4[4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)W * threadIdx.x;
        T wr[L * W];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
            if (VEC && i + W <= n) {
                auto wv = vload(q + i);
#pragma unroll
                for (int e = 0; e < W; ++e) wr[l * W + e] = el<T>(wv, e);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) wr[l * W + e] = (i + e < n) ? q[i + e] : T(0);
            }
        }
        for (int j = 0; j < k; ++j) {
            const T *__restrict__ col = Q + (int64_t)j * ldq;
            T acc = T(0);
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
                if (VEC && i + W <= n) {
                    auto cv = nt ? vload_nt(col + i) : vload(col + i);
#pragma unroll
                    for (int e = 0; e < W; ++e) { T p = el<T>(cv, e) * wr[l * W + e]; acc = acc + p; }
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (i + e < n) { T p = col[i + e] * wr[l * W + e]; acc = acc + p; }
                }
            }
            T tot = block_tree_256(acc, lds4);
            if (threadIdx.x == 0) seg_out[(int64_t)j * nseg + s] = tot;
        }
        T acc = T(0);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
#pragma unroll
            for (int e = 0; e < W; ++e)
                if (i + e < n) { T p = wr[l * W + e] * wr[l * W + e]; acc = acc + p; }
        }
        T tot = block_tree_256(acc, lds4);
        if (threadIdx.x == 0) seg_out[(int64_t)k * nseg + s] = tot;
    }
}

// k_gemv_n with the segment sums of the updated y .* y: seg_out[s].
template <typename T, bool VEC>
__global__ __launch_bounds__(MIK_BLOCK) void k_gemv_n_sq(int64_t n, int64_t nseg, int k, const T *__restrict__ V, int64_t ldv,
                                                          const T *__restrict__ cf, T alpha, T *__restrict__ y, T *__restrict__ seg_out, int nt)
{
    constexpr int W = VT<T>::W;
    constexpr int L = MIK_RED_L;
    constexpr int64_t SEG = (int64_t)MIK_BLOCK * W * L;
    __shared__ T lds4[4];
    for (int64_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const int64_t base = s * SEG + (int64_t)W * threadIdx.x;
        T yr[L * W];
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
            if (VEC && i + W <= n) {
                auto yv = vload<T>(y + i);
#pragma unroll
                for (int e = 0; e < W; ++e) yr[l * W + e] = el<T>(yv, e);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e) yr[l * W + e] = (i + e < n) ? y[i + e] : T(0);
            }
        }
        for (int j = 0; j < k; ++j) {
            const T *__restrict__ col = V + (int64_t)j * ldv;
            const T temp = alpha * cf[j];
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
                if (VEC && i + W <= n) {
                    auto cv = nt ? vload_nt(col + i) : vload(col + i);
#pragma unroll
                    for (int e = 0; e < W; ++e) { T p = temp * el<T>(cv, e); yr[l * W + e] = yr[l * W + e] + p; }
                } else {
#pragma unroll
                    for (int e = 0; e < W; ++e)
                        if (i + e < n) { T p = temp * col[i + e]; yr[l * W + e] = yr[l * W + e] + p; }
                }
            }
        }
        T acc = T(0);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int64_t i = base + (int64_t)l * MIK_BLOCK * W;
            if (VEC && i + W <= n) {
                typename VT<T>::vec yv;
#pragma unroll
                for (int e = 0; e < W; ++e) { el<T>(yv, e) = yr[l * W + e]; T p = yr[l * W + e] * yr[l * W + e]; acc = acc + p; }
                vstore(y + i, yv);
            } else {
#pragma unroll
                for (int e = 0; e < W; ++e)
                    if (i + e < n) { y[i + e] = yr[l * W + e]; T p = yr[l * W + e] * yr[l * W + e]; acc = acc + p; }
            }
        }
        T tot = block_tree_256(acc, lds4);
        if (threadIdx.x == 0) seg_out[s] = tot;
    }
}

#endif  // __HIPCC__
