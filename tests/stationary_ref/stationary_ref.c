/* stationary_ref.c -- a plain C99 restatement of IterativeSolvers.jl's src/stationary_sparse.jl, the checker of the device's
 * stationary methods.  It keeps the reference's CSC COLUMN loops (not the device's row view), line for line, so that the order in
 * which each x[i] / y[i] receives its terms is the reference's by construction.  Build with -O2 -ffp-contract=off (Julia never fuses
 * a multiply and an add here).
 *
 * Arrays: SparseMatrixCSC fields with 0-based colptr / rowval (int64), nzval of the element type; diag[] holds 0-based positions.
 * Every function exists for Float64 data (suffix _f64) and Float32 data (_f32).  The relaxed substitutions of Float32 data take
 * Float64 alpha / beta when wide != 0 (sor!(x::Vector{Float32}, A, b, 1.2): alpha*x[col]/d + beta*y[col] is evaluated in Float64
 * and rounded once at the store), else Float32 ones. */
#include <stdint.h>
#include <string.h>

/* DiagonalIndices (:6-28): 0, or the 1-based first column whose diagonal is missing or zero (SingularException(col)). */
#define ST_DIAG(SFX, T)                                                                                                         \
    int64_t st_diag_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, int64_t *diag)           \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            int64_t r1 = colptr[col], r2 = colptr[col + 1] - 1;                                                             \
            int64_t lo = r1, hi = r2 + 1;                      /* searchsortedfirst(rowval, col, r1, r2) */                  \
            while (lo < hi) { int64_t mid = lo + (hi - lo) / 2; if (rowval[mid] < col) lo = mid + 1; else hi = mid; }       \
            r1 = lo;                                                                                                        \
            if (r1 > r2 || rowval[r1] != col || nzval[r1] == (T)0) return col + 1;                                          \
            diag[col] = r1;                                                                                                 \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

/* ldiv!(y, D, x) (:30-35) */
#define ST_LDIV(SFX, T)                                                                                                         \
    void st_ldiv_##SFX(int64_t n, const T *nzval, const int64_t *diag, T *y, const T *x)                                    \
    {                                                                                                                       \
        for (int64_t row = 0; row < n; ++row) y[row] = x[row] / nzval[diag[row]];                                           \
    }

/* forward_sub!(F, x) (:67-82) and forward_sub!(alpha, F, x, beta, y) (:88-103) */
#define ST_FWD(SFX, T, S, NAME)                                                                                                 \
    void NAME(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, const int64_t *diag, int relax,       \
              S alpha, T *x, S beta, const T *y)                                                                            \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            int64_t idx = diag[col];                                                                                        \
            if (relax) { S t = alpha * (S)x[col]; t = t / (S)nzval[idx]; S u = beta * (S)y[col]; x[col] = (T)(t + u); }     \
            else x[col] = x[col] / nzval[idx];                                                                              \
            for (int64_t i = idx + 1; i < colptr[col + 1]; ++i) { T p = nzval[i] * x[col]; x[rowval[i]] = x[rowval[i]] - p; } \
        }                                                                                                                   \
    }

/* backward_sub!(F, x) (:109-124) and backward_sub!(alpha, F, x, beta, y) (:127-142) */
#define ST_BWD(SFX, T, S, NAME)                                                                                                 \
    void NAME(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, const int64_t *diag, int relax,       \
              S alpha, T *x, S beta, const T *y)                                                                            \
    {                                                                                                                       \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            int64_t idx = diag[col];                                                                                        \
            if (relax) { S t = alpha * (S)x[col]; t = t / (S)nzval[idx]; S u = beta * (S)y[col]; x[col] = (T)(t + u); }     \
            else x[col] = x[col] / nzval[idx];                                                                              \
            for (int64_t i = colptr[col]; i < idx; ++i) { T p = nzval[i] * x[col]; x[rowval[i]] = x[rowval[i]] - p; }       \
        }                                                                                                                   \
    }

/* mul!(alpha, O::OffDiagonal, x, beta, y) (:148-171) */
#define ST_OFFDIAG(SFX, T)                                                                                                      \
    void st_offdiag_mul_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, const int64_t *diag, \
                              T alpha, const T *x, T beta, T *y)                                                            \
    {                                                                                                                       \
        if (beta != (T)1) {                                                                                                 \
            if (beta == (T)0) { for (int64_t i = 0; i < n; ++i) y[i] = (T)0; }                                              \
            else { for (int64_t i = 0; i < n; ++i) y[i] = beta * y[i]; }                                                    \
        }                                                                                                                   \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            T ax = alpha * x[col];                                                                                          \
            int64_t d = diag[col];                                                                                          \
            for (int64_t j = colptr[col]; j < d; ++j) { T p = nzval[j] * ax; y[rowval[j]] = y[rowval[j]] + p; }             \
            for (int64_t j = d + 1; j < colptr[col + 1]; ++j) { T p = nzval[j] * ax; y[rowval[j]] = y[rowval[j]] + p; }     \
        }                                                                                                                   \
    }

/* gauss_seidel_multiply!(alpha, U, x, beta, y, z) (:178-191) and (alpha, L, ...) (:196-208); z may be x */
#define ST_GSMUL(SFX, T)                                                                                                        \
    void st_gs_mul_upper_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, const int64_t *diag,\
                               T alpha, const T *x, T beta, const T *y, T *z)                                               \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            T ax = alpha * x[col];                                                                                          \
            for (int64_t j = colptr[col]; j < diag[col]; ++j) { T p = nzval[j] * ax; z[rowval[j]] = z[rowval[j]] + p; }     \
            z[col] = beta * y[col];                                                                                         \
        }                                                                                                                   \
    }                                                                                                                       \
    void st_gs_mul_lower_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const T *nzval, const int64_t *diag,\
                               T alpha, const T *x, T beta, const T *y, T *z)                                               \
    {                                                                                                                       \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            T ax = alpha * x[col];                                                                                          \
            z[col] = beta * y[col];                                                                                         \
            for (int64_t j = diag[col] + 1; j < colptr[col + 1]; ++j) { T p = nzval[j] * ax; z[rowval[j]] = z[rowval[j]] + p; } \
        }                                                                                                                   \
    }

ST_DIAG(f64, double)
ST_DIAG(f32, float)
ST_LDIV(f64, double)
ST_LDIV(f32, float)
ST_FWD(f64, double, double, st_forward_sub_f64)
ST_FWD(f32, float, float, st_forward_sub_f32)
ST_FWD(f32w, float, double, st_forward_sub_f32w)
ST_BWD(f64, double, double, st_backward_sub_f64)
ST_BWD(f32, float, float, st_backward_sub_f32)
ST_BWD(f32w, float, double, st_backward_sub_f32w)
ST_OFFDIAG(f64, double)
ST_OFFDIAG(f32, float)
ST_GSMUL(f64, double)
ST_GSMUL(f32, float)

/* The four iterables, `maxiter` iterations each (:225-234, :278-288, :322-336, :392-418).  Return 0, or the singular column.
 * x: the caller's vector; work: the iterable's temporary (next / tmp; unused by Gauss-Seidel).  SOR swaps x and next every
 * iteration: *which receives 0 if iterable.x is the caller's x at the end, 1 if it is `work`.  omega32 != 0 selects a Float32
 * omega for Float32 data (alpha, beta of the relaxed substitutions in Float32), else a Float64 one. */
#define ST_METHODS(SFX, T)                                                                                                      \
    int64_t st_jacobi_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const T *nz, const T *b, T *x, T *work, int64_t maxiter, int64_t *diag) \
    {                                                                                                                       \
        int64_t s = st_diag_##SFX(n, cp, rv, nz, diag);                                                                     \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            memcpy(work, b, sizeof(T) * (size_t)n);                                                                         \
            st_offdiag_mul_##SFX(n, cp, rv, nz, diag, (T)-1, x, (T)1, work);                                                \
            st_ldiv_##SFX(n, nz, diag, x, work);                                                                            \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }                                                                                                                       \
    int64_t st_gauss_seidel_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const T *nz, const T *b, T *x, int64_t maxiter, int64_t *diag)   \
    {                                                                                                                       \
        int64_t s = st_diag_##SFX(n, cp, rv, nz, diag);                                                                     \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            st_gs_mul_upper_##SFX(n, cp, rv, nz, diag, (T)-1, x, (T)1, b, x);                                               \
            st_forward_sub_##SFX(n, cp, rv, nz, diag, 0, (T)0, x, (T)0, 0);                                                 \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

ST_METHODS(f64, double)
ST_METHODS(f32, float)

/* forward / backward relaxed substitutions with omega's type: Float64 data always in Float64 (a Float32 omega is promoted) */
static void st_fwd_relax_f64(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const int64_t *dg, double omega, double *x, const double *y, int upper)
{
    double a = omega, b = 1.0 - omega;
    if (upper) st_backward_sub_f64(n, cp, rv, nz, dg, 1, a, x, b, y);
    else st_forward_sub_f64(n, cp, rv, nz, dg, 1, a, x, b, y);
}
static void st_fwd_relax_f32(int64_t n, const int64_t *cp, const int64_t *rv, const float *nz, const int64_t *dg, double omega, int omega32, float *x,
                             const float *y, int upper)
{
    if (omega32) {
        float a = (float)omega, b = 1.0f - a;
        if (upper) st_backward_sub_f32(n, cp, rv, nz, dg, 1, a, x, b, y);
        else st_forward_sub_f32(n, cp, rv, nz, dg, 1, a, x, b, y);
    } else {
        double a = omega, b = 1.0 - omega;
        if (upper) st_backward_sub_f32w(n, cp, rv, nz, dg, 1, a, x, b, y);
        else st_forward_sub_f32w(n, cp, rv, nz, dg, 1, a, x, b, y);
    }
}

#define ST_SOR(SFX, T, RELAX, ...)                                                                                              \
    int64_t st_sor_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const T *nz, const T *b, T *x, T *work, double omega, int omega32, \
                         int64_t maxiter, int64_t *diag, int *which)                                                        \
    {                                                                                                                       \
        int64_t s = st_diag_##SFX(n, cp, rv, nz, diag);                                                                     \
        if (s) return s;                                                                                                    \
        (void)omega32;                                                                                                      \
        T *cur = x, *nxt = work;                                                                                            \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            st_gs_mul_upper_##SFX(n, cp, rv, nz, diag, (T)-1, cur, (T)1, b, nxt);                                           \
            RELAX(n, cp, rv, nz, diag, omega, __VA_ARGS__ nxt, cur, 0);                                                     \
            T *t = cur; cur = nxt; nxt = t;                                                                                 \
        }                                                                                                                   \
        *which = cur == x ? 0 : 1;                                                                                          \
        return 0;                                                                                                           \
    }                                                                                                                       \
    int64_t st_ssor_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const T *nz, const T *b, T *x, T *tmp, double omega, int omega32, \
                          int64_t maxiter, int64_t *diag)                                                                   \
    {                                                                                                                       \
        int64_t s = st_diag_##SFX(n, cp, rv, nz, diag);                                                                     \
        if (s) return s;                                                                                                    \
        (void)omega32;                                                                                                      \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            st_gs_mul_upper_##SFX(n, cp, rv, nz, diag, (T)-1, x, (T)1, b, tmp);                                             \
            RELAX(n, cp, rv, nz, diag, omega, __VA_ARGS__ tmp, x, 0);                                                       \
            st_gs_mul_lower_##SFX(n, cp, rv, nz, diag, (T)-1, tmp, (T)1, b, x);                                             \
            RELAX(n, cp, rv, nz, diag, omega, __VA_ARGS__ x, tmp, 1);                                                       \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

ST_SOR(f64, double, st_fwd_relax_f64, )
ST_SOR(f32, float, st_fwd_relax_f32, omega32, )
