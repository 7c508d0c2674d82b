/* stationary_dense_ref.c -- a plain C99 restatement of IterativeSolvers.jl's src/stationary.jl (the dense stationary methods), the
 * checker of the device's dense stationary methods.  It keeps the reference's COLUMN loops (not the device's row view), loop for loop,
 * so that the order in which each x[row] / tmp[row] receives its terms is the reference's by construction.  Build with -O2
 * -ffp-contract=off (Julia never fuses a multiply and an add here).
 *
 * A is column-major with leading dimension ld, 0-based here.  Every function exists for Float64 data (suffix _f64) and Float32 data
 * (_f32) and returns 0, or the 1-based index check_diag throws.  omega arrives as a double; wide != 0 on Float32 data is a Float64
 * omega (sor!(x::Vector{Float32}, A, b, 1.2): x + omega * (tmp / d - x) has its inner difference in Float32, the product and the sum in
 * Float64, and is rounded once at the store), wide == 0 a Float32 or an Int one, converted to the element type first. */
#include <stdint.h>

#define AT(row, col) A[(row) + (col) * ld]

/* check_diag (:6-12) */
#define DST_CHECK(SFX, T)                                                                                                       \
    int64_t dst_check_diag_##SFX(int64_t n, const T *A, int64_t ld)                                                         \
    {                                                                                                                       \
        for (int64_t i = 0; i < n; ++i)                                                                                     \
            if (AT(i, i) == (T)0) return i + 1;                                                                             \
        return 0;                                                                                                           \
    }

/* jacobi! (:31-36) over iterate(::DenseJacobiIterable) (:48-72) */
#define DST_JACOBI(SFX, T)                                                                                                      \
    int64_t dst_jacobi_##SFX(int64_t n, const T *A, int64_t ld, const T *b, T *x, T *next, int64_t maxiter)                 \
    {                                                                                                                       \
        int64_t s = dst_check_diag_##SFX(n, A, ld);                                                                         \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            for (int64_t i = 0; i < n; ++i) next[i] = b[i];                                                                 \
            for (int64_t col = 0; col < n; ++col) {                                                                         \
                for (int64_t row = 0; row < col; ++row) { T p = AT(row, col) * x[col]; next[row] = next[row] - p; }         \
                for (int64_t row = col + 1; row < n; ++row) { T p = AT(row, col) * x[col]; next[row] = next[row] - p; }     \
            }                                                                                                               \
            for (int64_t col = 0; col < n; ++col) x[col] = next[col] / AT(col, col);                                        \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

/* gauss_seidel! (:91-96) over iterate(::DenseGaussSeidelIterable) (:108-129) */
#define DST_GS(SFX, T)                                                                                                          \
    int64_t dst_gauss_seidel_##SFX(int64_t n, const T *A, int64_t ld, const T *b, T *x, int64_t maxiter)                    \
    {                                                                                                                       \
        int64_t s = dst_check_diag_##SFX(n, A, ld);                                                                         \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            for (int64_t col = 0; col < n; ++col) {                                                                         \
                for (int64_t row = 0; row < col; ++row) { T p = AT(row, col) * x[col]; x[row] = x[row] - p; }               \
                x[col] = b[col];                                                                                            \
            }                                                                                                               \
            for (int64_t col = 0; col < n; ++col) {                                                                         \
                x[col] = x[col] / AT(col, col);                                                                             \
                for (int64_t row = col + 1; row < n; ++row) { T p = AT(row, col) * x[col]; x[row] = x[row] - p; }           \
            }                                                                                                               \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

/* s.x[col] += s.omega * (s.tmp[col] / s.A[col, col] - s.x[col])  (:181, :241, :259) with omega of type S */
#define DST_RELAX(T, S, w)                                                                                                      \
    do {                                                                                                                    \
        T q = tmp[col] / AT(col, col);                                                                                      \
        T dq = q - x[col];                                                                                                  \
        S wd = (w) * (S)dq;                                                                                                 \
        x[col] = (T)((S)x[col] + wd);                                                                                       \
    } while (0)

/* the forward sweep shared by sor! and ssor! (:172-185 = :232-245) */
#define DST_FORWARD(T, S, w)                                                                                                    \
    do {                                                                                                                    \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            for (int64_t row = 0; row < col; ++row) { T p = AT(row, col) * x[col]; tmp[row] = tmp[row] - p; }               \
            tmp[col] = b[col];                                                                                              \
        }                                                                                                                   \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            DST_RELAX(T, S, w);                                                                                             \
            for (int64_t row = col + 1; row < n; ++row) { T p = AT(row, col) * x[col]; tmp[row] = tmp[row] - p; }           \
        }                                                                                                                   \
    } while (0)

/* the backward sweep of ssor! (:247-260) */
#define DST_BACKWARD(T, S, w)                                                                                                   \
    do {                                                                                                                    \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            tmp[col] = b[col];                                                                                              \
            for (int64_t row = col + 1; row < n; ++row) { T p = AT(row, col) * x[col]; tmp[row] = tmp[row] - p; }           \
        }                                                                                                                   \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            for (int64_t row = 0; row < col; ++row) { T p = AT(row, col) * x[col]; tmp[row] = tmp[row] - p; }               \
            DST_RELAX(T, S, w);                                                                                             \
        }                                                                                                                   \
    } while (0)

/* sor! (:149-154) / ssor! (:209-214): symmetric != 0 adds the backward sweep to every iteration */
#define DST_SOR(SFX, T)                                                                                                         \
    int64_t dst_sor_##SFX(int64_t n, const T *A, int64_t ld, const T *b, T *x, T *tmp, double omega, int wide, int symmetric, \
                          int64_t maxiter)                                                                                  \
    {                                                                                                                       \
        int64_t s = dst_check_diag_##SFX(n, A, ld);                                                                         \
        if (s) return s;                                                                                                    \
        const T wt = (T)omega;                                                                                              \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            if (wide) { DST_FORWARD(T, double, omega); if (symmetric) DST_BACKWARD(T, double, omega); }                     \
            else      { DST_FORWARD(T, T, wt);         if (symmetric) DST_BACKWARD(T, T, wt); }                             \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

#define DST_ALL(SFX, T) DST_CHECK(SFX, T) DST_JACOBI(SFX, T) DST_GS(SFX, T) DST_SOR(SFX, T)

DST_ALL(f64, double)
DST_ALL(f32, float)
