/* dense_chol_ref.c -- the bit contract of cholesky!(Hermitian(A, :L)) / ldiv!(y, F, x) on a dense matrix, restated as unblocked functions
 * with the loops in the obvious order (C99, compiled by the tests with -ffp-contract=off).  Column-major, leading dimension ld, 0-based
 * inside.  Complex matrices are interleaved (re, im) pairs of the real type; a complex product is four rounded products, one rounded
 * difference and one rounded sum (cx_mul of csrc/mik_complex.h), every subtraction is componentwise.
 *   dcr_factor   the lower triangle of A <- L.  Column j: d = re(A[j,j]) - sum over k < j ascending of (lr lr + li li) of L[j,k]; !(d > 0)
 *                (a NaN too) returns j + 1 and leaves the columns >= j as they are at that moment; L[j,j] = sqrt(d) with imaginary part +0;
 *                for i > j, a = A[i,j] - sum over k < j ascending of L[i,k] conj(L[j,k]), L[i,j] = a / L[j,j] per component.  Returns 0 on
 *                success.  Only the lower triangle and the real parts of the diagonal are read; the strict upper triangle is not touched.
 *   dcr_solve    forward: acc = x[i], k < i ascending acc -= L[i,k] w[k], w[i] = acc / L[i,i]; backward: acc = w[i], k > i DESCENDING
 *                acc -= conj(L[k,i]) y[k], y[i] = acc / L[i,i] */
#include <math.h>
#include <stdint.h>

#define DEFINE_REAL(T, SFX, SQRT)                                                                            \
    int64_t dcr_factor_##SFX(int64_t n, T *A, int64_t ld)                                                    \
    {                                                                                                        \
        for (int64_t j = 0; j < n; ++j) {                                                                    \
            T d = A[j * ld + j];                                                                             \
            for (int64_t k = 0; k < j; ++k) {                                                                \
                const T s = A[k * ld + j] * A[k * ld + j];                                                   \
                d = d - s;                                                                                   \
            }                                                                                                \
            if (!(d > (T)0)) return j + 1;                                                                   \
            const T ljj = SQRT(d);                                                                           \
            A[j * ld + j] = ljj;                                                                             \
            for (int64_t i = j + 1; i < n; ++i) {                                                            \
                T a = A[j * ld + i];                                                                         \
                for (int64_t k = 0; k < j; ++k) {                                                            \
                    const T p = A[k * ld + i] * A[k * ld + j];                                               \
                    a = a - p;                                                                               \
                }                                                                                            \
                A[j * ld + i] = a / ljj;                                                                     \
            }                                                                                                \
        }                                                                                                    \
        return 0;                                                                                            \
    }                                                                                                        \
    void dcr_solve_##SFX(int64_t n, const T *L, int64_t ld, T *x)                                            \
    {                                                                                                        \
        for (int64_t i = 0; i < n; ++i) {                                                                    \
            T acc = x[i];                                                                                    \
            for (int64_t k = 0; k < i; ++k) {                                                                \
                const T p = L[k * ld + i] * x[k];                                                            \
                acc = acc - p;                                                                               \
            }                                                                                                \
            x[i] = acc / L[i * ld + i];                                                                      \
        }                                                                                                    \
        for (int64_t i = n - 1; i >= 0; --i) {                                                               \
            T acc = x[i];                                                                                    \
            for (int64_t k = n - 1; k > i; --k) {                                                            \
                const T p = L[i * ld + k] * x[k];                                                            \
                acc = acc - p;                                                                               \
            }                                                                                                \
            x[i] = acc / L[i * ld + i];                                                                      \
        }                                                                                                    \
    }

/* (ar + ai i) -= (zr + zi i) (wr + wi i) */
#define CX_MSUB(T, ar, ai, zr, zi, wr, wi)                                                                   \
    do {                                                                                                     \
        const T p0_ = (zr) * (wr), p1_ = (zi) * (wi), p2_ = (zr) * (wi), p3_ = (zi) * (wr);                  \
        const T re_ = p0_ - p1_, im_ = p2_ + p3_;                                                            \
        ar = ar - re_;                                                                                       \
        ai = ai - im_;                                                                                       \
    } while (0)

#define RE(M, i, c) M[2 * ((c) * ld + (i))]
#define IM(M, i, c) M[2 * ((c) * ld + (i)) + 1]

#define DEFINE_CX(T, SFX, SQRT)                                                                              \
    int64_t dcr_factor_##SFX(int64_t n, T *A, int64_t ld)                                                    \
    {                                                                                                        \
        for (int64_t j = 0; j < n; ++j) {                                                                    \
            T d = RE(A, j, j);                                                                               \
            for (int64_t k = 0; k < j; ++k) {                                                                \
                const T p = RE(A, j, k) * RE(A, j, k), q = IM(A, j, k) * IM(A, j, k);                        \
                const T s = p + q;                                                                           \
                d = d - s;                                                                                   \
            }                                                                                                \
            if (!(d > (T)0)) return j + 1;                                                                   \
            const T ljj = SQRT(d);                                                                           \
            RE(A, j, j) = ljj;                                                                               \
            IM(A, j, j) = (T)0;                                                                              \
            for (int64_t i = j + 1; i < n; ++i) {                                                            \
                T ar = RE(A, i, j), ai = IM(A, i, j);                                                        \
                for (int64_t k = 0; k < j; ++k) CX_MSUB(T, ar, ai, RE(A, i, k), IM(A, i, k), RE(A, j, k), -IM(A, j, k));   \
                RE(A, i, j) = ar / ljj;                                                                      \
                IM(A, i, j) = ai / ljj;                                                                      \
            }                                                                                                \
        }                                                                                                    \
        return 0;                                                                                            \
    }                                                                                                        \
    void dcr_solve_##SFX(int64_t n, const T *L, int64_t ld, T *x)                                            \
    {                                                                                                        \
        for (int64_t i = 0; i < n; ++i) {                                                                    \
            T ar = x[2 * i], ai = x[2 * i + 1];                                                              \
            for (int64_t k = 0; k < i; ++k) CX_MSUB(T, ar, ai, RE(L, i, k), IM(L, i, k), x[2 * k], x[2 * k + 1]);          \
            x[2 * i] = ar / RE(L, i, i);                                                                     \
            x[2 * i + 1] = ai / RE(L, i, i);                                                                 \
        }                                                                                                    \
        for (int64_t i = n - 1; i >= 0; --i) {                                                               \
            T ar = x[2 * i], ai = x[2 * i + 1];                                                              \
            for (int64_t k = n - 1; k > i; --k) CX_MSUB(T, ar, ai, RE(L, k, i), -IM(L, k, i), x[2 * k], x[2 * k + 1]);     \
            x[2 * i] = ar / RE(L, i, i);                                                                     \
            x[2 * i + 1] = ai / RE(L, i, i);                                                                 \
        }                                                                                                    \
    }

DEFINE_REAL(double, f64, sqrt)
DEFINE_REAL(float, f32, sqrtf)
DEFINE_CX(double, c64, sqrt)
DEFINE_CX(float, c32, sqrtf)
