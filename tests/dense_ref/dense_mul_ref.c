/* dense_mul_ref.c -- C99 restatement of the arithmetic contract of the dense operator (include/mik.h, "dense operator"), test
 * infrastructure only.  Built with -ffp-contract=off: every product and every sum is rounded on its own.
 *
 *   dmr_mul_chunked   y = A x in the chunked order: the columns are cut into chunks of C consecutive columns; p_c[i] is the serial sum
 *                     from +0, over the chunk's columns ascending, of A[i,j] * x[j]; y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ...;
 *                     n = 0 gives +0.
 *   dmr_mul_serial    y = A x in the order of Julia's generic column-oriented mul!: y = 0, then for every column j ascending
 *                     y[i] = y[i] + A[i,j] * x[j].
 * A is column-major m x n with leading dimension lda >= m; rows at or past m are never read. */
#include <stdint.h>

#define DMR_DEFINE(T, SFX)                                                                                                      \
    void dmr_mul_chunked_##SFX(int64_t m, int64_t n, const T *A, int64_t lda, const T *x, T *y, int64_t C)                       \
    {                                                                                                                            \
        for (int64_t i = 0; i < m; ++i) {                                                                                        \
            T tot = (T)0;                                                                                                        \
            for (int64_t j0 = 0; j0 < n; j0 += C) {                                                                              \
                const int64_t j1 = j0 + C < n ? j0 + C : n;                                                                      \
                T p = (T)0;                                                                                                      \
                for (int64_t j = j0; j < j1; ++j) {                                                                              \
                    const T pr = A[i + j * lda] * x[j];                                                                          \
                    p = p + pr;                                                                                                  \
                }                                                                                                                \
                tot = j0 == 0 ? p : tot + p;                                                                                     \
            }                                                                                                                    \
            y[i] = tot;                                                                                                          \
        }                                                                                                                        \
    }                                                                                                                            \
    void dmr_mul_serial_##SFX(int64_t m, int64_t n, const T *A, int64_t lda, const T *x, T *y)                                   \
    {                                                                                                                            \
        for (int64_t i = 0; i < m; ++i) y[i] = (T)0;                                                                             \
        for (int64_t j = 0; j < n; ++j) {                                                                                        \
            const T b = x[j];                                                                                                    \
            for (int64_t i = 0; i < m; ++i) {                                                                                    \
                const T pr = A[i + j * lda] * b;                                                                                 \
                y[i] = y[i] + pr;                                                                                                \
            }                                                                                                                    \
        }                                                                                                                        \
    }

DMR_DEFINE(double, f64)
DMR_DEFINE(float, f32)
