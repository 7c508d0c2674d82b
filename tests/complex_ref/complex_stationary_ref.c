/* complex_stationary_ref.c -- a plain C99 restatement of IterativeSolvers.jl's src/stationary_sparse.jl for ComplexF64 / ComplexF32
 * operators, the checker of the device's complex stationary methods.  As tests/stationary_ref/stationary_ref.c it keeps the reference's
 * CSC COLUMN loops (not the device's row view), so the order in which each x[i] / y[i] receives its terms is the reference's by
 * construction.  Build with gcc -std=c99 -O2 -ffp-contract=off -lm: nothing contracts except the two fma() calls of the widened division.
 *
 * Arrays: SparseMatrixCSC fields with 0-based colptr / rowval (int64); nzval and the vectors are interleaved (re, im) pairs of the
 * component type R; diag[] holds 0-based positions.  Suffix _f64: ComplexF64, _f32: ComplexF32.
 *
 * Element operations, in Julia's promotion order:
 *   z * w      (zr wr - zi wi, zr wi + zi wr): four rounded products, one rounded difference, one rounded sum
 *   z + w      componentwise
 *   z / w      64-bit components: the robust division of Baudin and Smith (Base's method for ComplexF64); 32-bit components: Base's
 *              widened method -- the four components converted to double, mag = 1 / fma(c, c, d d), re = fma(a, c, b d) mag,
 *              im = fma(b, c, -(a d)) mag, each rounded to float once.  Base's branches for infinite divisors are not restated.
 *   relaxed substitution  x = alpha * x / d + beta * y with a REAL alpha (omega) and beta = one(T) - omega COMPLEX (imaginary part +0.0),
 *              evaluated in the real type E of promote(real(T), typeof(omega)): (alpha xr, alpha xi) / E(d) + beta * E(y), rounded to T
 *              once per component.  _f32w: ComplexF32 data with a Float64 omega (E = double: the 64-bit division). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

/* ---- z / w ---------------------------------------------------------------------------------------------------------------------- */
static double cs_div2(double a, double b, double c, double d, double r, double t)
{
    if (r != 0.0) {
        double br = b * r;
        if (br != 0.0) return (a + br) * t;
        double at = a * t, bt = b * t;
        return at + bt * r;
    }
    double bc = b / c;
    return (a + d * bc) * t;
}
static void cs_div1(double a, double b, double c, double d, double *p, double *q)
{
    double r = d / c;
    double t = 1.0 / (c + d * r);
    *p = cs_div2(a, b, c, d, r, t);
    *q = cs_div2(b, -a, c, d, r, t);
}
static void cs_div_d(double a, double b, double c, double d, double *re, double *im)
{
    const double half_ov = DBL_MAX / 2.0;                           /* floatmax / 2 */
    const double two_un_eps = DBL_MIN * 2.0 / DBL_EPSILON;          /* floatmin * 2 / eps */
    const double bs = 2.0 / (DBL_EPSILON * DBL_EPSILON);            /* 2 / eps^2 */
    double ab = fabs(a) >= fabs(b) ? fabs(a) : fabs(b), cd = fabs(c) >= fabs(d) ? fabs(c) : fabs(d);
    double s = 1.0, p, q;
    if (ab >= half_ov) { a = a * 0.5; b = b * 0.5; s = s * 2.0; }
    if (cd >= half_ov) { c = c * 0.5; d = d * 0.5; s = s * 0.5; }
    if (ab <= two_un_eps) { a = a * bs; b = b * bs; s = s / bs; }
    if (cd <= two_un_eps) { c = c * bs; d = d * bs; s = s * bs; }
    if (fabs(d) <= fabs(c)) cs_div1(a, b, c, d, &p, &q);
    else { cs_div1(b, a, d, c, &p, &q); q = -q; }
    *re = p * s;
    *im = q * s;
}
static void cs_div_f(float af, float bf, float cf, float df, float *re, float *im)
{
    double a = (double)af, b = (double)bf, c = (double)cf, d = (double)df;
    double dd = d * d, bd = b * d, ad = a * d;
    double mag = 1.0 / fma(c, c, dd);
    double r = fma(a, c, bd) * mag, i = fma(b, c, -ad) * mag;
    *re = (float)r;
    *im = (float)i;
}
/* for the tests of the division itself: out = (a + b i) / (c + d i) */
void cst_div_f64(double a, double b, double c, double d, double *out) { cs_div_d(a, b, c, d, &out[0], &out[1]); }
void cst_div_f32(float a, float b, float c, float d, float *out) { cs_div_f(a, b, c, d, &out[0], &out[1]); }

/* ---- z * w ---------------------------------------------------------------------------------------------------------------------- */
static void cs_mul_d(double zr, double zi, double wr, double wi, double *re, double *im)
{
    double a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
    *re = a - b;
    *im = c + d;
}
static void cs_mul_f(float zr, float zi, float wr, float wi, float *re, float *im)
{
    float a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
    *re = a - b;
    *im = c + d;
}

/* DiagonalIndices (:6-28): 0, or the 1-based first column whose diagonal is missing or zero (iszero: both parts, either sign) */
#define CST_DIAG(SFX, R)                                                                                                        \
    int64_t cst_diag_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, int64_t *diag)          \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            int64_t r1 = colptr[col], r2 = colptr[col + 1] - 1;                                                             \
            int64_t lo = r1, hi = r2 + 1;                                                                                   \
            while (lo < hi) { int64_t mid = lo + (hi - lo) / 2; if (rowval[mid] < col) lo = mid + 1; else hi = mid; }       \
            r1 = lo;                                                                                                        \
            if (r1 > r2 || rowval[r1] != col || (nzval[2 * r1] == (R)0 && nzval[2 * r1 + 1] == (R)0)) return col + 1;       \
            diag[col] = r1;                                                                                                 \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

/* ldiv!(y, D, x) (:30-35) */
#define CST_LDIV(SFX, R, DIV)                                                                                                   \
    void cst_ldiv_##SFX(int64_t n, const R *nzval, const int64_t *diag, R *y, const R *x)                                   \
    {                                                                                                                       \
        for (int64_t row = 0; row < n; ++row)                                                                               \
            DIV(x[2 * row], x[2 * row + 1], nzval[2 * diag[row]], nzval[2 * diag[row] + 1], &y[2 * row], &y[2 * row + 1]);  \
    }

/* the diagonal step of a substitution: x[col] = x[col] / d, or alpha * x[col] / d + beta * y[col] in E */
#define CST_SOLVE(R, E, DIV, EDIV, EMUL)                                                                                        \
    if (relax) {                                                                                                            \
        E ar = alpha * (E)x[2 * col], ai = alpha * (E)x[2 * col + 1], qr, qi, ur, ui;                                       \
        EDIV(ar, ai, (E)nzval[2 * idx], (E)nzval[2 * idx + 1], &qr, &qi);                                                   \
        EMUL(ber, bei, (E)y[2 * col], (E)y[2 * col + 1], &ur, &ui);                                                         \
        x[2 * col] = (R)(qr + ur);                                                                                          \
        x[2 * col + 1] = (R)(qi + ui);                                                                                      \
    } else DIV(x[2 * col], x[2 * col + 1], nzval[2 * idx], nzval[2 * idx + 1], &x[2 * col], &x[2 * col + 1]);
/* x[row] -= A[row, col] * x[col], in R */
#define CST_ELIM(R, MUL)                                                                                                        \
    { R pr, pi; MUL(nzval[2 * i], nzval[2 * i + 1], x[2 * col], x[2 * col + 1], &pr, &pi);                                  \
      x[2 * rowval[i]] = x[2 * rowval[i]] - pr; x[2 * rowval[i] + 1] = x[2 * rowval[i] + 1] - pi; }

/* forward_sub!(F, x) (:67-82) and forward_sub!(alpha, F, x, beta, y) (:88-103) */
#define CST_FWD(NAME, R, E, DIV, MUL, EDIV, EMUL)                                                                               \
    void NAME(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, const int64_t *diag, int relax,       \
              E alpha, R *x, E ber, E bei, const R *y)                                                                      \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            int64_t idx = diag[col];                                                                                        \
            CST_SOLVE(R, E, DIV, EDIV, EMUL)                                                                                \
            for (int64_t i = idx + 1; i < colptr[col + 1]; ++i) CST_ELIM(R, MUL)                                            \
        }                                                                                                                   \
    }
/* backward_sub!(F, x) (:109-124) and backward_sub!(alpha, F, x, beta, y) (:127-142) */
#define CST_BWD(NAME, R, E, DIV, MUL, EDIV, EMUL)                                                                               \
    void NAME(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, const int64_t *diag, int relax,       \
              E alpha, R *x, E ber, E bei, const R *y)                                                                      \
    {                                                                                                                       \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            int64_t idx = diag[col];                                                                                        \
            CST_SOLVE(R, E, DIV, EDIV, EMUL)                                                                                \
            for (int64_t i = colptr[col]; i < idx; ++i) CST_ELIM(R, MUL)                                                    \
        }                                                                                                                   \
    }

/* y[row] += A[row, col] * ax */
#define CST_SCATTER(R, MUL, V)                                                                                                  \
    { R pr, pi; MUL(nzval[2 * j], nzval[2 * j + 1], axr, axi, &pr, &pi);                                                    \
      V[2 * rowval[j]] = V[2 * rowval[j]] + pr; V[2 * rowval[j] + 1] = V[2 * rowval[j] + 1] + pi; }

/* mul!(alpha, O::OffDiagonal, x, beta, y) (:148-171); alpha, beta: (re, im) */
#define CST_OFFDIAG(SFX, R, MUL)                                                                                                \
    void cst_offdiag_mul_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, const int64_t *diag,\
                               const R *alpha, const R *x, const R *beta, R *y)                                             \
    {                                                                                                                       \
        if (!(beta[0] == (R)1 && beta[1] == (R)0)) {                                                                        \
            if (beta[0] == (R)0 && beta[1] == (R)0) { for (int64_t i = 0; i < 2 * n; ++i) y[i] = (R)0; }                    \
            else { for (int64_t i = 0; i < n; ++i) MUL(beta[0], beta[1], y[2 * i], y[2 * i + 1], &y[2 * i], &y[2 * i + 1]); } \
        }                                                                                                                   \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            R axr, axi;                                                                                                     \
            MUL(alpha[0], alpha[1], x[2 * col], x[2 * col + 1], &axr, &axi);                                                \
            int64_t d = diag[col];                                                                                          \
            for (int64_t j = colptr[col]; j < d; ++j) CST_SCATTER(R, MUL, y)                                                \
            for (int64_t j = d + 1; j < colptr[col + 1]; ++j) CST_SCATTER(R, MUL, y)                                        \
        }                                                                                                                   \
    }

/* gauss_seidel_multiply!(alpha, U, x, beta, y, z) (:178-191) and (alpha, L, ...) (:196-208); z may be x */
#define CST_GSMUL(SFX, R, MUL)                                                                                                  \
    void cst_gs_mul_upper_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, const int64_t *diag,\
                                const R *alpha, const R *x, const R *beta, const R *y, R *z)                                \
    {                                                                                                                       \
        for (int64_t col = 0; col < n; ++col) {                                                                             \
            R axr, axi;                                                                                                     \
            MUL(alpha[0], alpha[1], x[2 * col], x[2 * col + 1], &axr, &axi);                                                \
            for (int64_t j = colptr[col]; j < diag[col]; ++j) CST_SCATTER(R, MUL, z)                                        \
            MUL(beta[0], beta[1], y[2 * col], y[2 * col + 1], &z[2 * col], &z[2 * col + 1]);                                \
        }                                                                                                                   \
    }                                                                                                                       \
    void cst_gs_mul_lower_##SFX(int64_t n, const int64_t *colptr, const int64_t *rowval, const R *nzval, const int64_t *diag,\
                                const R *alpha, const R *x, const R *beta, const R *y, R *z)                                \
    {                                                                                                                       \
        for (int64_t col = n - 1; col >= 0; --col) {                                                                        \
            R axr, axi;                                                                                                     \
            MUL(alpha[0], alpha[1], x[2 * col], x[2 * col + 1], &axr, &axi);                                                \
            MUL(beta[0], beta[1], y[2 * col], y[2 * col + 1], &z[2 * col], &z[2 * col + 1]);                                \
            for (int64_t j = diag[col] + 1; j < colptr[col + 1]; ++j) CST_SCATTER(R, MUL, z)                                \
        }                                                                                                                   \
    }

CST_DIAG(f64, double)
CST_DIAG(f32, float)
CST_LDIV(f64, double, cs_div_d)
CST_LDIV(f32, float, cs_div_f)
CST_FWD(cst_forward_sub_f64, double, double, cs_div_d, cs_mul_d, cs_div_d, cs_mul_d)
CST_FWD(cst_forward_sub_f32, float, float, cs_div_f, cs_mul_f, cs_div_f, cs_mul_f)
CST_FWD(cst_forward_sub_f32w, float, double, cs_div_f, cs_mul_f, cs_div_d, cs_mul_d)
CST_BWD(cst_backward_sub_f64, double, double, cs_div_d, cs_mul_d, cs_div_d, cs_mul_d)
CST_BWD(cst_backward_sub_f32, float, float, cs_div_f, cs_mul_f, cs_div_f, cs_mul_f)
CST_BWD(cst_backward_sub_f32w, float, double, cs_div_f, cs_mul_f, cs_div_d, cs_mul_d)
CST_OFFDIAG(f64, double, cs_mul_d)
CST_OFFDIAG(f32, float, cs_mul_f)
CST_GSMUL(f64, double, cs_mul_d)
CST_GSMUL(f32, float, cs_mul_f)

/* the relaxed substitutions with omega's type: alpha = omega (real), beta = one(T) - omega = (1 - omega, +0.0) */
static void cst_relax_f64(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const int64_t *dg, double omega, int omega32, double *x,
                          const double *y, int upper)
{
    double a = omega, b = 1.0 - omega;
    (void)omega32;                                          /* ComplexF64 data: a Float32 or an Int omega is promoted to Float64 */
    if (upper) cst_backward_sub_f64(n, cp, rv, nz, dg, 1, a, x, b, 0.0, y);
    else cst_forward_sub_f64(n, cp, rv, nz, dg, 1, a, x, b, 0.0, y);
}
static void cst_relax_f32(int64_t n, const int64_t *cp, const int64_t *rv, const float *nz, const int64_t *dg, double omega, int omega32, float *x,
                          const float *y, int upper)
{
    if (omega32) {
        float a = (float)omega, b = 1.0f - a;
        if (upper) cst_backward_sub_f32(n, cp, rv, nz, dg, 1, a, x, b, 0.0f, y);
        else cst_forward_sub_f32(n, cp, rv, nz, dg, 1, a, x, b, 0.0f, y);
    } else {
        double a = omega, b = 1.0 - omega;
        if (upper) cst_backward_sub_f32w(n, cp, rv, nz, dg, 1, a, x, b, 0.0, y);
        else cst_forward_sub_f32w(n, cp, rv, nz, dg, 1, a, x, b, 0.0, y);
    }
}

/* The four iterables, `maxiter` iterations each (:225-234, :278-288, :322-336, :392-418), as in stationary_ref.c: return 0 or the singular
 * column; SOR swaps x and work every iteration (*which = 1: iterable.x is `work`).  -one(T) = (-1.0, -0.0), one(T) = (1.0, +0.0).
 * omega32 != 0: a Float32 or an Int omega (ComplexF32 data then evaluates the relaxed substitutions in Float32). */
#define CST_METHODS(SFX, R)                                                                                                     \
    int64_t cst_jacobi_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const R *nz, const R *b, R *x, R *work, int64_t maxiter, int64_t *diag) \
    {                                                                                                                       \
        const R m1[2] = {(R)-1, -(R)0}, p1[2] = {(R)1, (R)0};                                                               \
        int64_t s = cst_diag_##SFX(n, cp, rv, nz, diag);                                                                    \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            memcpy(work, b, 2 * sizeof(R) * (size_t)n);                                                                     \
            cst_offdiag_mul_##SFX(n, cp, rv, nz, diag, m1, x, p1, work);                                                    \
            cst_ldiv_##SFX(n, nz, diag, x, work);                                                                           \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }                                                                                                                       \
    int64_t cst_gauss_seidel_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const R *nz, const R *b, R *x, int64_t maxiter, int64_t *diag)  \
    {                                                                                                                       \
        const R m1[2] = {(R)-1, -(R)0}, p1[2] = {(R)1, (R)0};                                                               \
        int64_t s = cst_diag_##SFX(n, cp, rv, nz, diag);                                                                    \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            cst_gs_mul_upper_##SFX(n, cp, rv, nz, diag, m1, x, p1, b, x);                                                   \
            cst_forward_sub_##SFX(n, cp, rv, nz, diag, 0, (R)0, x, (R)0, (R)0, 0);                                          \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }                                                                                                                       \
    int64_t cst_sor_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const R *nz, const R *b, R *x, R *work, double omega, int omega32, \
                          int64_t maxiter, int64_t *diag, int *which)                                                       \
    {                                                                                                                       \
        const R m1[2] = {(R)-1, -(R)0}, p1[2] = {(R)1, (R)0};                                                               \
        int64_t s = cst_diag_##SFX(n, cp, rv, nz, diag);                                                                    \
        if (s) return s;                                                                                                    \
        R *cur = x, *nxt = work;                                                                                            \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            cst_gs_mul_upper_##SFX(n, cp, rv, nz, diag, m1, cur, p1, b, nxt);                                               \
            cst_relax_##SFX(n, cp, rv, nz, diag, omega, omega32, nxt, cur, 0);                                              \
            R *t = cur; cur = nxt; nxt = t;                                                                                 \
        }                                                                                                                   \
        *which = cur == x ? 0 : 1;                                                                                          \
        return 0;                                                                                                           \
    }                                                                                                                       \
    int64_t cst_ssor_##SFX(int64_t n, const int64_t *cp, const int64_t *rv, const R *nz, const R *b, R *x, R *tmp, double omega, int omega32, \
                           int64_t maxiter, int64_t *diag)                                                                  \
    {                                                                                                                       \
        const R m1[2] = {(R)-1, -(R)0}, p1[2] = {(R)1, (R)0};                                                               \
        int64_t s = cst_diag_##SFX(n, cp, rv, nz, diag);                                                                    \
        if (s) return s;                                                                                                    \
        for (int64_t it = 0; it < maxiter; ++it) {                                                                          \
            cst_gs_mul_upper_##SFX(n, cp, rv, nz, diag, m1, x, p1, b, tmp);                                                 \
            cst_relax_##SFX(n, cp, rv, nz, diag, omega, omega32, tmp, x, 0);                                                \
            cst_gs_mul_lower_##SFX(n, cp, rv, nz, diag, m1, tmp, p1, b, x);                                                 \
            cst_relax_##SFX(n, cp, rv, nz, diag, omega, omega32, x, tmp, 1);                                                \
        }                                                                                                                   \
        return 0;                                                                                                           \
    }

CST_METHODS(f64, double)
CST_METHODS(f32, float)
