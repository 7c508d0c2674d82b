// Micro-benchmark (development): which chunk C should the N form of the dense operator (csrc/mik_dense_mul.h) cut the columns into, and
// where does its time go?  The library's own kernels, instantiated for C = 32 / 64 / 128 / 256, on an n x n matrix of non-zero values
// (Float64 and Float32; n = 1024, 4096, 16384).  Every timed window holds enough back-to-back launches to last about 40 ms (the length
// scripts/dense_operator_bench.py uses); the candidates alternate inside every repetition; median of 9 windows after 2 warm-up rounds.
// One JSON line per (dtype, n, C): microseconds of the whole product with the library's launch (at most 4 workgroups per compute unit,
// k_dense_n_combine with PF = 32 loads ahead), of k_dense_n alone, of the combine kernel alone with PF = 32 and with PF = 8, and of the
// whole product with one workgroup per (row block, chunk).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I iterativesolvers.jl_amd/csrc -o /tmp/dense_chunk scripts/micro/dense_chunk.hip && /tmp/dense_chunk
#include "mik_dense_mul.h"

#include <algorithm>
#include <cstdio>
#include <vector>

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

enum { WHOLE = 0, SWEEP = 1, COMBINE32 = 2, COMBINE8 = 3, UNCAPPED = 4, PARTS = 5 };

template <typename T, int C>
static void product(int part, int64_t n, const T *A, const T *x, T *work, T *y, int nt, int64_t cap, hipStream_t s)
{
    const int64_t nc = (n + C - 1) / C, m_pad = (n + MIK_DM_R - 1) / MIK_DM_R * MIK_DM_R;
    T *out = nc == 1 ? y : work;
    const int64_t gx = m_pad / MIK_DM_R;
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(nc, part == UNCAPPED ? nc : std::max<int64_t>(1, cap / gx)));
    if (part == WHOLE || part == SWEEP || part == UNCAPPED) {
        if (nt) hipLaunchKernelGGL((k_dense_n<T, true, true, C>), grid, dim3(MIK_BLOCK), 0, s, n, n, A, n, x, out, m_pad);
        else hipLaunchKernelGGL((k_dense_n<T, true, false, C>), grid, dim3(MIK_BLOCK), 0, s, n, n, A, n, x, out, m_pad);
    }
    if (nc == 1) return;
    const dim3 cg((unsigned)((n + MIK_DM_CB - 1) / MIK_DM_CB));
    if (part == WHOLE || part == COMBINE32 || part == UNCAPPED) hipLaunchKernelGGL((k_dense_n_combine<T, 32>), cg, dim3(MIK_DM_CB), 0, s, n, nc, (const T *)out, m_pad, y, (int64_t)0, (int64_t)0);
    if (part == COMBINE8) hipLaunchKernelGGL((k_dense_n_combine<T, 8>), cg, dim3(MIK_DM_CB), 0, s, n, nc, (const T *)out, m_pad, y, (int64_t)0, (int64_t)0);
}

template <typename T>
static int run(const char *name, int64_t n, int reps, int64_t cap)
{
    T *A, *x, *y, *work;
    const int64_t m_pad = (n + MIK_DM_R - 1) / MIK_DM_R * MIK_DM_R;
    CK(hipMalloc(&A, sizeof(T) * n * n)); CK(hipMalloc(&x, sizeof(T) * n)); CK(hipMalloc(&y, sizeof(T) * n));
    CK(hipMalloc(&work, sizeof(T) * ((n + 31) / 32) * m_pad));
    CK(hipMemset(A, 0x3f, sizeof(T) * n * n)); CK(hipMemset(x, 0x3f, sizeof(T) * n));      // 0x3f3f...: a small positive normal number of either type
    CK(hipMemset(work, 0x3f, sizeof(T) * ((n + 31) / 32) * m_pad));
    const int nt = (double)n * (double)n * sizeof(T) > 192.0e6 ? 1 : 0;
    const int inner = (int)std::max<double>(2.0, 40e-3 / ((double)n * n * sizeof(T) / 3.0e12 + 5e-6));      // ~40 ms per window of whole products
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> us[4][PARTS];
    for (int rep = -2; rep < reps; ++rep)                                // two warm-up rounds
        for (int part = 0; part < PARTS; ++part)
            for (int v = 0; v < 4; ++v) {
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < inner; ++i) {
                    if (v == 0) product<T, 32>(part, n, A, x, work, y, nt, cap, 0);
                    if (v == 1) product<T, 64>(part, n, A, x, work, y, nt, cap, 0);
                    if (v == 2) product<T, 128>(part, n, A, x, work, y, nt, cap, 0);
                    if (v == 3) product<T, 256>(part, n, A, x, work, y, nt, cap, 0);
                }
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
                float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
                if (rep >= 0) us[v][part].push_back(ms * 1e3f / inner);
            }
    CK(hipGetLastError());
    const int Cs[4] = {32, 64, 128, 256};
    for (int v = 0; v < 4; ++v) {
        double med[PARTS];
        for (int part = 0; part < PARTS; ++part) { std::sort(us[v][part].begin(), us[v][part].end()); med[part] = us[v][part][us[v][part].size() / 2]; }
        std::printf("{\"dtype\": \"%s\", \"n\": %lld, \"C\": %d, \"calls_per_window\": %d, \"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f, \"matrix_TBps\": %.3f, "
                    "\"k_dense_n_us\": %.1f, \"combine_pf32_us\": %.1f, \"combine_pf8_us\": %.1f, \"one_workgroup_per_chunk_us\": %.1f}\n", name, (long long)n, Cs[v], inner,
                    med[WHOLE], (double)us[v][WHOLE].front(), (double)us[v][WHOLE].back(), (double)n * n * sizeof(T) / (med[WHOLE] * 1e-6) / 1e12, med[SWEEP], med[COMBINE32],
                    med[COMBINE8], med[UNCAPPED]);
    }
    std::fflush(stdout);
    CK(hipFree(A)); CK(hipFree(x)); CK(hipFree(y)); CK(hipFree(work));
    return 0;
}

int main()
{
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int64_t cap = (int64_t)4 * prop.multiProcessorCount;           // the library's launch
    for (int64_t n : {1024, 4096, 16384}) {
        if (run<double>("float64", n, 9, cap)) return 1;
        if (run<float>("float32", n, 9, cap)) return 1;
    }
    return 0;
}
