// mik_svdl.h -- the kernel of svdl (src/svdl.jl) that is its own: the basis rotation of the thick restart.  (The two sweeps of a classical
// Gram-Schmidt pass with the squared norm riding on them are the SQ instances of k_multidot / k_gemv_n, csrc/mik_kernels.h.)
//
//   k_basis_rotate   Y[:, 0:l] = V[:, 0:k] * F[0:k, 0:l]            -- src/svdl.jl:384, :392, :470, :471, :231, :237
//       A lane owns W = 16 B / sizeof(T) consecutive rows and LB output columns: W * LB accumulators in registers.  It walks the k
//       columns of V once (coalesced 16-byte loads, four columns in flight) and multiplies by the row F[c, j0 .. j0 + LB) that the
//       workgroup staged in LDS (every lane reads the same address: a broadcast, no bank conflict).  Every product and every sum is
//       rounded on its own, columns ascending, the first product opening the sum -- an output element depends on its own row only, so
//       the bits do not depend on the launch shape.  blockIdx.y selects the block of LB output columns (l > 32 reads V twice).
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

#endif  // __HIPCC__
