/* dense_lu_ref.c -- the bit contract of lu!(A) / ldiv!(y, F, x) on a dense matrix, restated as three unblocked functions with the loops in
 * the obvious order (C99, compiled by the tests with -ffp-contract=off).  Column-major, leading dimension ld, 0-based inside; ipiv is
 * returned 1-based like LAPACK's.
 *   dlr_factor   A <- L\U with partial pivoting: the pivot of column j is the FIRST row i >= j with the largest |A[i,j]| (strict >); the
 *                multiplier is A[i,j] / pivot; A[i,c] = A[i,c] - m * A[j,c].  Returns 0, or the 1-based index of the first column whose
 *                pivot is exactly zero (the factorisation stops there, as the SingularException does).
 *   dlr_pivots   the row interchanges on a vector, in order
 *   dlr_solve    the unit-lower chain of every row in ascending column order, then the upper chain of every row in descending column
 *                order with the division by U[i,i] last */
#include <math.h>
#include <stdint.h>

#define DEFINE(T, SFX, ABS)                                                                                  \
    int64_t dlr_factor_##SFX(int64_t n, T *A, int64_t ld, int64_t *ipiv)                                     \
    {                                                                                                        \
        for (int64_t j = 0; j < n; ++j) {                                                                    \
            int64_t p = j;                                                                                   \
            T best = ABS(A[j * ld + j]);                                                                     \
            for (int64_t i = j + 1; i < n; ++i) {                                                            \
                const T a = ABS(A[j * ld + i]);                                                              \
                if (a > best) { best = a; p = i; }                                                           \
            }                                                                                                \
            ipiv[j] = p + 1;                                                                                 \
            if (best == (T)0) return j + 1;                                                                  \
            if (p != j)                                                                                      \
                for (int64_t c = 0; c < n; ++c) {                                                            \
                    const T t = A[c * ld + j];                                                               \
                    A[c * ld + j] = A[c * ld + p];                                                           \
                    A[c * ld + p] = t;                                                                       \
                }                                                                                            \
            const T piv = A[j * ld + j];                                                                     \
            for (int64_t i = j + 1; i < n; ++i) {                                                            \
                const T m = A[j * ld + i] / piv;                                                             \
                A[j * ld + i] = m;                                                                           \
                for (int64_t c = j + 1; c < n; ++c) {                                                        \
                    const T prod = m * A[c * ld + j];                                                        \
                    A[c * ld + i] = A[c * ld + i] - prod;                                                    \
                }                                                                                            \
            }                                                                                                \
        }                                                                                                    \
        return 0;                                                                                            \
    }                                                                                                        \
    void dlr_pivots_##SFX(int64_t n, const int64_t *ipiv, T *x)                                              \
    {                                                                                                        \
        for (int64_t j = 0; j < n; ++j) {                                                                    \
            const int64_t p = ipiv[j] - 1;                                                                   \
            const T t = x[j];                                                                                \
            x[j] = x[p];                                                                                     \
            x[p] = t;                                                                                        \
        }                                                                                                    \
    }                                                                                                        \
    void dlr_solve_##SFX(int64_t n, const T *LU, int64_t ld, T *x)                                           \
    {                                                                                                        \
        for (int64_t i = 0; i < n; ++i) {                                                                    \
            T acc = x[i];                                                                                    \
            for (int64_t c = 0; c < i; ++c) {                                                                \
                const T prod = LU[c * ld + i] * x[c];                                                        \
                acc = acc - prod;                                                                            \
            }                                                                                                \
            x[i] = acc;                                                                                      \
        }                                                                                                    \
        for (int64_t i = n - 1; i >= 0; --i) {                                                               \
            T acc = x[i];                                                                                    \
            for (int64_t c = n - 1; c > i; --c) {                                                            \
                const T prod = LU[c * ld + i] * x[c];                                                        \
                acc = acc - prod;                                                                            \
            }                                                                                                \
            x[i] = acc / LU[i * ld + i];                                                                     \
        }                                                                                                    \
    }

DEFINE(double, f64, fabs)
DEFINE(float, f32, fabsf)
