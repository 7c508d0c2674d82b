/* complex_solvers_ref.c -- C99 restatement of what DESIGN.md section 19 fixes for the layer bicgstabl, minres and chebyshev stand on, on
 * the complex element types (interleaved re, im): gemv_t and the Gram matrix (every entry a dot with the (W, L) tree), the four axpy_dot
 * forms, both minres_update forms, the BiCGStab minimal-residual update, the two Chebyshev sweeps, and the small LU solve with LAPACK's
 * pivot rule.  Test infrastructure: it shares no code with the library (nor with complex_ref.c) and is built by the tests
 * (gcc -std=c99 -O2 -ffp-contract=off), once per component type through the self-include below.
 *
 *   z * w     = (zr wr - zi wi) + (zr wi + zi wr) i          every product rounded, nothing fused
 *   a * z     = (a zr) + (a zi) i                            a real
 *   dot(x, y) = sum conj(x_i) y_i; per element re = xr yr + xi yi, im = xr yi - xi yr, then one tree for re and one for im
 *   norm(x)   = sqrt of the tree sum over the 2 n reals of x_i^2 inside the safe range, else the scaled second pass
 */
#ifndef CS_BODY
#define CS_BODY
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define CS_THREADS 256
#define CS_FIN 1024

#define R double
#define SFX(name) name##_f64
#define CS_SQRT sqrt
#define CS_FABS fabs
#define CS_LO 0x1p-900
#define CS_HI 0x1p+900
#define CS_EC 1022
#include "complex_solvers_ref.c"
#undef R
#undef SFX
#undef CS_SQRT
#undef CS_FABS
#undef CS_LO
#undef CS_HI
#undef CS_EC

#define R float
#define SFX(name) name##_f32
#define CS_SQRT sqrtf
#define CS_FABS fabsf
#define CS_LO 0x1p-70f
#define CS_HI 0x1p+100f
#define CS_EC 126
#include "complex_solvers_ref.c"

#else /* ---- the body, once per R ---- */

/* ---- the two-level tree ---- */
static R SFX(wave64)(R *v)                                  /* shuffle-down tree, offsets 32 .. 1 */
{
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

static R SFX(block)(R *t)                                   /* 256 thread sums: 4 wave trees, the wave sums left to right */
{
    R tot = SFX(wave64)(t);
    for (int w = 1; w < 4; ++w) tot = tot + SFX(wave64)(t + 64 * w);
    return tot;
}

static R SFX(level2)(const R *S, int64_t m)                 /* 1024 threads stride over the segment sums; 16 wave sums left to right */
{
    R t[CS_FIN];
    for (int i = 0; i < CS_FIN; ++i) {
        R a = 0;
        for (int64_t j = i; j < m; j += CS_FIN) a = a + S[j];
        t[i] = a;
    }
    R tot = SFX(wave64)(t);
    for (int w = 1; w < 16; ++w) tot = tot + SFX(wave64)(t + 64 * w);
    return tot;
}

/* element i of thread t, slot (l, e), segment s of the shape (W, L) over items of any kind */
static int64_t SFX(item)(int64_t s, int t, int l, int e, int W, int L)
{
    return s * (int64_t)CS_THREADS * W * L + (int64_t)l * CS_THREADS * W + (int64_t)W * t + e;
}

static void SFX(dot)(int64_t n, const R *x, const R *y, int W, int L, R *out)
{
    const int64_t seg = (int64_t)CS_THREADS * W * L, nseg = (n + seg - 1) / seg;
    R *sr = (R *)malloc(sizeof(R) * (size_t)(nseg + 1)), *si = (R *)malloc(sizeof(R) * (size_t)(nseg + 1));
    for (int64_t s = 0; s < nseg; ++s) {
        R tr[CS_THREADS], ti[CS_THREADS];
        for (int t = 0; t < CS_THREADS; ++t) {
            R ar = 0, ai = 0;
            for (int l = 0; l < L; ++l)
                for (int e = 0; e < W; ++e) {
                    const int64_t i = SFX(item)(s, t, l, e, W, L);
                    if (i >= n) continue;
                    const R p = x[2 * i] * y[2 * i], q = x[2 * i + 1] * y[2 * i + 1], u = x[2 * i] * y[2 * i + 1], v = x[2 * i + 1] * y[2 * i];
                    const R re = p + q, im = u - v;
                    ar = ar + re;
                    ai = ai + im;
                }
            tr[t] = ar;
            ti[t] = ai;
        }
        sr[s] = SFX(block)(tr);
        si[s] = SFX(block)(ti);
    }
    out[0] = SFX(level2)(sr, nseg);
    out[1] = SFX(level2)(si, nseg);
    free(sr);
    free(si);
}

/* tree sum of (x_i scale)^2 over the 2 n reals of a complex n-vector: the real shape is (2 W, L) */
static R SFX(sumsq)(int64_t n, const R *x, int W, int L, R scale)
{
    const int64_t m = 2 * n, Wr = 2 * W, seg = (int64_t)CS_THREADS * Wr * L, nseg = (m + seg - 1) / seg;
    R *ss = (R *)malloc(sizeof(R) * (size_t)(nseg + 1));
    for (int64_t s = 0; s < nseg; ++s) {
        R tt[CS_THREADS];
        for (int t = 0; t < CS_THREADS; ++t) {
            R a = 0;
            for (int l = 0; l < L; ++l)
                for (int e = 0; e < Wr; ++e) {
                    const int64_t i = SFX(item)(s, t, l, e, (int)Wr, L);
                    if (i >= m) continue;
                    const R v = scale == (R)1 ? x[i] : x[i] * scale;
                    const R p = v * v;
                    a = a + p;
                }
            tt[t] = a;
        }
        ss[s] = SFX(block)(tt);
    }
    const R tot = SFX(level2)(ss, nseg);
    free(ss);
    return tot;
}

static R SFX(norm)(int64_t n, const R *x, int W, int L)
{
    const R t = SFX(sumsq)(n, x, W, L, (R)1);
    if (t >= CS_LO && t <= CS_HI) return CS_SQRT(t);
    if (n <= 0) return 0;
    R amax = 0;
    for (int64_t i = 0; i < 2 * n; ++i) {
        const R a = CS_FABS(x[i]);
        if (a != a) return a;
        if (a > amax) amax = a;
    }
    if (amax == 0 || isinf(amax)) return amax;
    int e;
    (void)frexp((double)amax, &e);
    if (e > CS_EC) e = CS_EC;
    if (e < -CS_EC) e = -CS_EC;
    const R sc = (R)ldexp(1.0, -e), sinv = (R)ldexp(1.0, e);
    return CS_SQRT(SFX(sumsq)(n, x, W, L, sc)) * sinv;
}

static void SFX(mul)(R zr, R zi, R wr, R wi, R *pr, R *pi)
{
    const R a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
    *pr = a - b;
    *pi = c + d;
}

/* y += t x over n complex elements, t complex */
static void SFX(caxpy)(int64_t n, R tr, R ti, const R *x, R *y)
{
    for (int64_t i = 0; i < n; ++i) {
        R pr, pi;
        SFX(mul)(tr, ti, x[2 * i], x[2 * i + 1], &pr, &pi);
        y[2 * i] = y[2 * i] + pr;
        y[2 * i + 1] = y[2 * i + 1] + pi;
    }
}

/* ---- h[j] = dot(V[:, j], w), j < k ---- */
void SFX(cs_gemv_t)(int64_t n, int k, const R *V, int64_t ldv, const R *w, int W, int L, R *h)
{
    for (int j = 0; j < k; ++j) SFX(dot)(n, V + 2 * (int64_t)j * ldv, w, W, L, h + 2 * j);
}

/* ---- M = V' V, k x k column-major: the upper triangle from the dots, the lower its conjugate, the diagonal's imaginary part +0 ---- */
void SFX(cs_gram)(int64_t n, int k, const R *V, int64_t ldv, int W, int L, R *M)
{
    for (int r = 0; r < k; ++r)
        for (int c = r; c < k; ++c) {
            R d[2];
            SFX(dot)(n, V + 2 * (int64_t)r * ldv, V + 2 * (int64_t)c * ldv, W, L, d);
            R *up = M + 2 * ((int64_t)c * k + r), *lo = M + 2 * ((int64_t)r * k + c);
            if (r == c) { up[0] = d[0]; up[1] = 0; continue; }
            up[0] = d[0]; up[1] = d[1];
            lo[0] = d[0]; lo[1] = -d[1];
        }
}

/* ---- y += alpha x (x NULL: no update; real_alpha: alpha[0] times each component); then out = dot(z, y) (2 reals), or, z NULL,
 *      out[0] = norm(y) ---- */
void SFX(cs_axpy_dot)(int64_t n, int real_alpha, const R *alpha, const R *x, R *y, const R *z, int W, int L, R *out)
{
    if (x) {
        if (real_alpha)
            for (int64_t i = 0; i < 2 * n; ++i) { const R p = alpha[0] * x[i]; y[i] = y[i] + p; }
        else SFX(caxpy)(n, alpha[0], alpha[1], x, y);
    }
    if (z) SFX(dot)(n, z, y, W, L, out);
    else out[0] = SFX(norm)(n, y, W, L);
}

/* ---- src/minres.jl:115, :138-144; sc = {inv_h3, neg_h1, neg_h0, inv_h2, rhs0}, each (re, im); real_sc: only the re parts count and
 *      multiply as real x complex ---- */
void SFX(cs_minres_update)(int64_t n, int real_sc, const R *sc, R *v_next, const R *v_curr, const R *w_curr, const R *w_prev, R *w_next, R *x)
{
    for (int64_t i = 0; i < n; ++i) {
        R wr, wi, pr, pi;
        if (real_sc) {
            v_next[2 * i] = v_next[2 * i] * sc[0];
            v_next[2 * i + 1] = v_next[2 * i + 1] * sc[0];
            wr = v_curr[2 * i]; wi = v_curr[2 * i + 1];
            if (w_curr) { pr = sc[2] * w_curr[2 * i]; pi = sc[2] * w_curr[2 * i + 1]; wr = wr + pr; wi = wi + pi; }
            if (w_prev) { pr = sc[4] * w_prev[2 * i]; pi = sc[4] * w_prev[2 * i + 1]; wr = wr + pr; wi = wi + pi; }
            wr = wr * sc[6]; wi = wi * sc[6];
            pr = sc[8] * wr; pi = sc[8] * wi;
        } else {
            SFX(mul)(v_next[2 * i], v_next[2 * i + 1], sc[0], sc[1], &pr, &pi);
            v_next[2 * i] = pr; v_next[2 * i + 1] = pi;
            wr = v_curr[2 * i]; wi = v_curr[2 * i + 1];
            if (w_curr) { SFX(mul)(sc[2], sc[3], w_curr[2 * i], w_curr[2 * i + 1], &pr, &pi); wr = wr + pr; wi = wi + pi; }
            if (w_prev) { SFX(mul)(sc[4], sc[5], w_prev[2 * i], w_prev[2 * i + 1], &pr, &pi); wr = wr + pr; wi = wi + pi; }
            SFX(mul)(wr, wi, sc[6], sc[7], &pr, &pi);
            wr = pr; wi = pi;
            SFX(mul)(sc[8], sc[9], wr, wi, &pr, &pi);
        }
        w_next[2 * i] = wr; w_next[2 * i + 1] = wi;
        x[2 * i] = x[2 * i] + pr; x[2 * i + 1] = x[2 * i + 1] + pi;
    }
}

/* ---- src/bicgstabl.jl:126-132 as the three mul!(y, V, c, alpha, 1) of the reference, alpha = -/+(1 + 0 i): t_j = alpha gamma_j, columns
 *      ascending; x is updated from rs[:, 1] BEFORE that column changes; returns norm(rs[:, 1]) ---- */
R SFX(cs_mr_update)(int64_t n, int l, R *us, int64_t ldu, R *rs, int64_t ldr, R *x, const R *gamma, int W, int L)
{
    R tn[16], tp[16];
    for (int j = 0; j < l; ++j) {
        SFX(mul)((R)-1, (R)0, gamma[2 * j], gamma[2 * j + 1], &tn[2 * j], &tn[2 * j + 1]);
        SFX(mul)((R)1, (R)0, gamma[2 * j], gamma[2 * j + 1], &tp[2 * j], &tp[2 * j + 1]);
    }
    for (int j = 0; j < l; ++j) SFX(caxpy)(n, tn[2 * j], tn[2 * j + 1], us + 2 * (int64_t)(j + 1) * ldu, us);       /* :127 */
    for (int j = 0; j < l; ++j) SFX(caxpy)(n, tp[2 * j], tp[2 * j + 1], rs + 2 * (int64_t)j * ldr, x);              /* :128 */
    for (int j = 0; j < l; ++j) SFX(caxpy)(n, tn[2 * j], tn[2 * j + 1], rs + 2 * (int64_t)(j + 1) * ldr, rs);       /* :129 */
    return SFX(norm)(n, rs, W, L);                                                                                   /* :132 */
}

/* ---- src/chebyshev.jl:51-54 and :35-45 with their real scalars ---- */
R SFX(cs_axpy2_nrm2)(int64_t n, R alpha, const R *u, R *x, const R *c, R *r, int W, int L)
{
    for (int64_t i = 0; i < 2 * n; ++i) {
        const R t = alpha * u[i];
        x[i] = x[i] + t;
        const R s = alpha * c[i];
        r[i] = r[i] - s;
    }
    return SFX(norm)(n, r, W, L);
}

void SFX(cs_cheb_direction)(int64_t n, const R *r, R beta, int first, R *u)
{
    for (int64_t i = 0; i < 2 * n; ++i) {
        R c = r[i];
        if (!first) { const R t = beta * c; c = c + t; }
        u[i] = c;
    }
}

/* ---- LU with partial pivoting on a small column-major complex matrix, then the two triangular solves, in place.  The pivot of column j
 *      is the FIRST row i >= j with the largest |re| + |im| (LAPACK's izamax); quotients by Smith's scaling.  Returns 8 on a zero column. */
static void SFX(div)(R zr, R zi, R wr, R wi, R *qr, R *qi)
{
    if (CS_FABS(wr) >= CS_FABS(wi)) {
        const R t = wi / wr, d = wr + wi * t;
        *qr = (zr + zi * t) / d;
        *qi = (zi - zr * t) / d;
    } else {
        const R t = wr / wi, d = wr * t + wi;
        *qr = (zr * t + zi) / d;
        *qi = (zi * t - zr) / d;
    }
}

int SFX(cs_lu_solve)(R *A, int64_t lda, int n, R *b)
{
#define AT(i, j) (A + 2 * ((int64_t)(j) * lda + (i)))
    for (int j = 0; j < n; ++j) {
        int p = j;
        R best = CS_FABS(AT(j, j)[0]) + CS_FABS(AT(j, j)[1]);
        for (int i = j + 1; i < n; ++i) {
            const R a = CS_FABS(AT(i, j)[0]) + CS_FABS(AT(i, j)[1]);
            if (a > best) { best = a; p = i; }
        }
        if (best == 0) return 8;
        if (p != j) {
            for (int c = 0; c < n; ++c)
                for (int q = 0; q < 2; ++q) { const R t = AT(j, c)[q]; AT(j, c)[q] = AT(p, c)[q]; AT(p, c)[q] = t; }
            for (int q = 0; q < 2; ++q) { const R t = b[2 * j + q]; b[2 * j + q] = b[2 * p + q]; b[2 * p + q] = t; }
        }
        for (int i = j + 1; i < n; ++i) {
            R mr, mi, pr, pi;
            SFX(div)(AT(i, j)[0], AT(i, j)[1], AT(j, j)[0], AT(j, j)[1], &mr, &mi);
            AT(i, j)[0] = mr; AT(i, j)[1] = mi;
            for (int c = j + 1; c < n; ++c) {
                SFX(mul)(mr, mi, AT(j, c)[0], AT(j, c)[1], &pr, &pi);
                AT(i, c)[0] = AT(i, c)[0] - pr;
                AT(i, c)[1] = AT(i, c)[1] - pi;
            }
            SFX(mul)(mr, mi, b[2 * j], b[2 * j + 1], &pr, &pi);
            b[2 * i] = b[2 * i] - pr;
            b[2 * i + 1] = b[2 * i + 1] - pi;
        }
    }
    for (int j = n - 1; j >= 0; --j) {
        R qr, qi, pr, pi;
        SFX(div)(b[2 * j], b[2 * j + 1], AT(j, j)[0], AT(j, j)[1], &qr, &qi);
        b[2 * j] = qr; b[2 * j + 1] = qi;
        for (int i = 0; i < j; ++i) {
            SFX(mul)(qr, qi, AT(i, j)[0], AT(i, j)[1], &pr, &pi);
            b[2 * i] = b[2 * i] - pr;
            b[2 * i + 1] = b[2 * i + 1] - pi;
        }
    }
#undef AT
    return 0;
}

#endif
