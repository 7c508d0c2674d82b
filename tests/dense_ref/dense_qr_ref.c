/* dense_qr_ref.c -- the bit contract of qr!(A) (Householder, no pivoting), lmul!(Q, y), lmul!(Q', y), F \ b and Matrix(F.Q) on a dense
 * m x n matrix, m >= n, restated as unblocked functions with the loops in the obvious order (C99, compiled by the tests with
 * -ffp-contract=off).  Column-major, leading dimension ld, 0-based inside.
 *   the reduction T over the absolute rows i of a range: 256 accumulators starting at +0, accumulator i mod 256 takes acc = acc + p_i in
 *                ascending i; each group of 64 accumulators is folded by a[l] += a[l + s], s = 32, 16, 8, 4, 2, 1; the four sums are added
 *                left to right.
 *   dqr_factor   column j: alpha = A[j,j], s = T(A[i,j] A[i,j]; j < i < m).  s == 0: tau[j] = 0, nothing stored.  Otherwise
 *                nrm = sqrt(alpha alpha + s), beta = -copysign(nrm, alpha), tau[j] = (beta - alpha) / beta, A[i,j] /= alpha - beta for i > j,
 *                A[j,j] = beta; then reflector j on every column c > j.  Returns 0, or the 1-based index of the first R[k,k] == 0.
 *   reflector j on a column a: skipped if tau[j] == 0; w = T(v_i a_i; j <= i < m) with v_j = 1, v_i = A[i,j]; t = tau[j] w;
 *                a_i = a_i - v_i t for j <= i < m.
 *   dqr_lmul     adjoint: the reflectors 0 ... n - 1 in ascending order (Q' y); else n - 1 ... 0 (Q y)
 *   dqr_solve    b (m values) <- Q' b, then x (n values): the upper chain of every row of R in descending column order, the division by
 *                R[i,i] last (the upper half of dlr_solve in dense_lu_ref.c)
 *   dqr_thin_q   Q (m x n) = Q applied to the first n columns of the m x m identity */
#include <math.h>
#include <stdint.h>

#define DEFINE(T, SFX, SQRT, COPYSIGN)                                                                       \
    static T dqr_fold_##SFX(T *acc)                                                                          \
    {                                                                                                        \
        for (int g = 0; g < 4; ++g)                                                                          \
            for (int s = 32; s > 0; s >>= 1)                                                                 \
                for (int l = 0; l < s; ++l) acc[64 * g + l] = acc[64 * g + l] + acc[64 * g + l + s];         \
        return ((acc[0] + acc[64]) + acc[128]) + acc[192];                                                   \
    }                                                                                                        \
    static void dqr_reflect_##SFX(int64_t m, int64_t j, const T *v, T tau, T *a)                             \
    {                                                                                                        \
        T acc[256];                                                                                          \
        if (tau == (T)0) return;                                                                             \
        for (int q = 0; q < 256; ++q) acc[q] = (T)0;                                                         \
        for (int64_t i = j; i < m; ++i) {                                                                    \
            const T vi = i == j ? (T)1 : v[i];                                                               \
            const T p = vi * a[i];                                                                           \
            acc[i % 256] = acc[i % 256] + p;                                                                 \
        }                                                                                                    \
        const T w = dqr_fold_##SFX(acc);                                                                     \
        const T t = tau * w;                                                                                 \
        for (int64_t i = j; i < m; ++i) {                                                                    \
            const T vi = i == j ? (T)1 : v[i];                                                               \
            const T p = vi * t;                                                                              \
            a[i] = a[i] - p;                                                                                 \
        }                                                                                                    \
    }                                                                                                        \
    int64_t dqr_factor_##SFX(int64_t m, int64_t n, T *A, int64_t ld, T *tau)                                 \
    {                                                                                                        \
        int64_t zero = 0;                                                                                    \
        for (int64_t j = 0; j < n; ++j) {                                                                    \
            T *col = A + j * ld;                                                                             \
            T acc[256];                                                                                      \
            for (int q = 0; q < 256; ++q) acc[q] = (T)0;                                                     \
            for (int64_t i = j + 1; i < m; ++i) {                                                            \
                const T p = col[i] * col[i];                                                                 \
                acc[i % 256] = acc[i % 256] + p;                                                             \
            }                                                                                                \
            const T s = dqr_fold_##SFX(acc);                                                                 \
            const T alpha = col[j];                                                                          \
            if (s == (T)0) {                                                                                 \
                tau[j] = (T)0;                                                                               \
            } else {                                                                                         \
                const T pa = alpha * alpha;                                                                  \
                const T nrm = SQRT(pa + s);                                                                  \
                const T beta = -COPYSIGN(nrm, alpha);                                                        \
                const T d = alpha - beta;                                                                    \
                tau[j] = (beta - alpha) / beta;                                                              \
                for (int64_t i = j + 1; i < m; ++i) col[i] = col[i] / d;                                     \
                col[j] = beta;                                                                               \
            }                                                                                                \
            if (col[j] == (T)0 && !zero) zero = j + 1;                                                       \
            for (int64_t c = j + 1; c < n; ++c) dqr_reflect_##SFX(m, j, col, tau[j], A + c * ld);            \
        }                                                                                                    \
        return zero;                                                                                         \
    }                                                                                                        \
    void dqr_lmul_##SFX(int64_t m, int64_t n, const T *A, int64_t ld, const T *tau, int adjoint, T *y)       \
    {                                                                                                        \
        if (adjoint)                                                                                         \
            for (int64_t j = 0; j < n; ++j) dqr_reflect_##SFX(m, j, A + j * ld, tau[j], y);                  \
        else                                                                                                 \
            for (int64_t j = n - 1; j >= 0; --j) dqr_reflect_##SFX(m, j, A + j * ld, tau[j], y);             \
    }                                                                                                        \
    void dqr_solve_##SFX(int64_t m, int64_t n, const T *A, int64_t ld, const T *tau, T *b, T *x)             \
    {                                                                                                        \
        dqr_lmul_##SFX(m, n, A, ld, tau, 1, b);                                                              \
        for (int64_t i = 0; i < n; ++i) x[i] = b[i];                                                         \
        for (int64_t i = n - 1; i >= 0; --i) {                                                               \
            T acc = x[i];                                                                                    \
            for (int64_t c = n - 1; c > i; --c) {                                                            \
                const T prod = A[c * ld + i] * x[c];                                                         \
                acc = acc - prod;                                                                            \
            }                                                                                                \
            x[i] = acc / A[i * ld + i];                                                                      \
        }                                                                                                    \
    }                                                                                                        \
    void dqr_thin_q_##SFX(int64_t m, int64_t n, const T *A, int64_t ld, const T *tau, T *Q, int64_t ldq)     \
    {                                                                                                        \
        for (int64_t c = 0; c < n; ++c) {                                                                    \
            for (int64_t i = 0; i < m; ++i) Q[c * ldq + i] = i == c ? (T)1 : (T)0;                           \
            dqr_lmul_##SFX(m, n, A, ld, tau, 0, Q + c * ldq);                                                \
        }                                                                                                    \
    }

DEFINE(double, f64, sqrt, copysign)
DEFINE(float, f32, sqrtf, copysignf)
