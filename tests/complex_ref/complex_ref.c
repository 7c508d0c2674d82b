/* complex_ref.c -- C99 restatement of the orders DESIGN.md section 17 fixes for the complex element types (interleaved re, im):
 * the dot tree with a (W, L) argument, the norm over the 2 n reals, the SpMV row orders (serial, wave shape, left-to-right segments),
 * the Modified Gram-Schmidt pass, gemv_n and the axpy family.  Test infrastructure: it shares no code with the library and is built
 * by the tests (gcc -std=c99 -O2 -ffp-contract=off), once per component type through the self-include below.
 *
 *   z * w     = (zr wr - zi wi) + (zr wi + zi wr) i          every product rounded, nothing fused
 *   dot(x, y) = sum conj(x_i) y_i; per element re = xr yr + xi yi, im = xr yi - xi yr, then one tree for re and one for im
 */
#ifndef CR_BODY
#define CR_BODY
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define CR_THREADS 256
#define CR_FIN 1024

#define R double
#define SFX(name) name##_f64
#define CR_SQRT sqrt
#define CR_FABS fabs
#define CR_LO 0x1p-900
#define CR_HI 0x1p+900
#define CR_EC 1022
#include "complex_ref.c"
#undef R
#undef SFX
#undef CR_SQRT
#undef CR_FABS
#undef CR_LO
#undef CR_HI
#undef CR_EC

#define R float
#define SFX(name) name##_f32
#define CR_SQRT sqrtf
#define CR_FABS fabsf
#define CR_LO 0x1p-70f
#define CR_HI 0x1p+100f
#define CR_EC 126
#include "complex_ref.c"

#else /* ---- the body, once per R ---- */

/* wave-64 shuffle-down tree (offsets 32 .. 1); v is destroyed, the sum is returned */
static R SFX(wave)(R *v)
{
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

/* 256 per-thread sums -> wave trees, then the 4 wave sums left to right */
static R SFX(block256)(R *t)
{
    R w0 = SFX(wave)(t), w1 = SFX(wave)(t + 64), w2 = SFX(wave)(t + 128), w3 = SFX(wave)(t + 192);
    R tot = w0;
    tot = tot + w1;
    tot = tot + w2;
    tot = tot + w3;
    return tot;
}

/* level 2: 1024 virtual threads, thread t adds S[t], S[t + 1024], ... from +0; wave trees; the 16 wave sums left to right */
static R SFX(level2)(const R *S, int64_t m)
{
    R t[CR_FIN];
    for (int i = 0; i < CR_FIN; ++i) {
        R a = 0;
        for (int64_t j = i; j < m; j += CR_FIN) a = a + S[j];
        t[i] = a;
    }
    R tot = SFX(wave)(t);
    for (int w = 1; w < 16; ++w) tot = tot + SFX(wave)(t + 64 * w);
    return tot;
}

/* out[0] + out[1] i = dot(x, y) over n complex elements with the level-1 shape (W, L): segments of 256 W L elements, thread t owns,
 * for l < L, the W elements from l * 256 W + W t */
void SFX(cr_dot)(int64_t n, const R *x, const R *y, int W, int L, R *out)
{
    const int64_t seg = (int64_t)CR_THREADS * W * L, nseg = (n + seg - 1) / seg;
    R *sr = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1)), *si = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1));
    for (int64_t s = 0; s < nseg; ++s) {
        R tr[CR_THREADS], ti[CR_THREADS];
        for (int t = 0; t < CR_THREADS; ++t) {
            R ar = 0, ai = 0;
            for (int l = 0; l < L; ++l)
                for (int e = 0; e < W; ++e) {
                    const int64_t i = s * seg + (int64_t)l * CR_THREADS * W + (int64_t)W * t + e;
                    if (i >= n) continue;
                    const R xr = x[2 * i], xi = x[2 * i + 1], yr = y[2 * i], yi = y[2 * i + 1];
                    const R p = xr * yr, q = xi * yi, u = xr * yi, v = xi * yr;
                    const R re = p + q, im = u - v;
                    ar = ar + re;
                    ai = ai + im;
                }
            tr[t] = ar;
            ti[t] = ai;
        }
        sr[s] = SFX(block256)(tr);
        si[s] = SFX(block256)(ti);
    }
    out[0] = SFX(level2)(sr, nseg);
    out[1] = SFX(level2)(si, nseg);
    free(sr);
    free(si);
}

/* tree sum of (x_i * scale)^2 over m REALS with the real shape (Wr, L) -- the sum of squares behind norm(x) */
static R SFX(sumsq)(int64_t m, const R *x, int Wr, int L, R scale)
{
    const int64_t seg = (int64_t)CR_THREADS * Wr * L, nseg = (m + seg - 1) / seg;
    R *ss = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1));
    for (int64_t s = 0; s < nseg; ++s) {
        R tt[CR_THREADS];
        for (int t = 0; t < CR_THREADS; ++t) {
            R a = 0;
            for (int l = 0; l < L; ++l)
                for (int e = 0; e < Wr; ++e) {
                    const int64_t i = s * seg + (int64_t)l * CR_THREADS * Wr + (int64_t)Wr * t + e;
                    if (i >= m) continue;
                    const R v = scale == (R)1 ? x[i] : x[i] * scale;
                    const R p = v * v;
                    a = a + p;
                }
            tt[t] = a;
        }
        ss[s] = SFX(block256)(tt);
    }
    const R tot = SFX(level2)(ss, nseg);
    free(ss);
    return tot;
}

/* norm of a complex n-vector = the real norm over its 2 n interleaved reals: sqrt of the tree sum of squares inside the safe range, else
 * the scaled second pass (amax, exact power-of-two scale, the same tree).  W: complex elements per 16 bytes. */
R SFX(cr_nrm2)(int64_t n, const R *x, int W, int L)
{
    const int64_t m = 2 * n;
    const R t = SFX(sumsq)(m, x, 2 * W, L, (R)1);
    if (t >= CR_LO && t <= CR_HI) return CR_SQRT(t);
    if (m <= 0) return 0;
    R amax = 0;
    for (int64_t i = 0; i < m; ++i) {
        const R a = CR_FABS(x[i]);
        if (a != a) return a;
        if (a > amax) amax = a;
    }
    if (amax == 0 || isinf(amax)) return amax;
    int e;
    (void)frexp((double)amax, &e);
    if (e > CR_EC) e = CR_EC;
    if (e < -CR_EC) e = -CR_EC;
    const R s = (R)ldexp(1.0, -e), sinv = (R)ldexp(1.0, e);
    const R t2 = SFX(sumsq)(m, x, 2 * W, L, s);
    return CR_SQRT(t2) * sinv;
}

/* ---- the axpy family ---- */
void SFX(cr_axpy)(int64_t n, const R *alpha, const R *x, R *y)          /* y += alpha x, alpha complex */
{
    const R ar = alpha[0], ai = alpha[1];
    for (int64_t i = 0; i < n; ++i) {
        const R xr = x[2 * i], xi = x[2 * i + 1];
        const R a = ar * xr, b = ai * xi, c = ar * xi, d = ai * xr;
        const R pr = a - b, pi = c + d;
        y[2 * i] = y[2 * i] + pr;
        y[2 * i + 1] = y[2 * i + 1] + pi;
    }
}
void SFX(cr_xpby)(int64_t n, const R *x, const R *beta, R *y)           /* y = x + beta y, beta complex */
{
    const R br = beta[0], bi = beta[1];
    for (int64_t i = 0; i < n; ++i) {
        const R yr = y[2 * i], yi = y[2 * i + 1];
        const R a = br * yr, b = bi * yi, c = br * yi, d = bi * yr;
        const R pr = a - b, pi = c + d;
        y[2 * i] = x[2 * i] + pr;
        y[2 * i + 1] = x[2 * i + 1] + pi;
    }
}
void SFX(cr_scal)(int64_t n, const R *alpha, R *x)                      /* x *= alpha, alpha complex */
{
    const R ar = alpha[0], ai = alpha[1];
    for (int64_t i = 0; i < n; ++i) {
        const R xr = x[2 * i], xi = x[2 * i + 1];
        const R a = xr * ar, b = xi * ai, c = xr * ai, d = xi * ar;
        x[2 * i] = a - b;
        x[2 * i + 1] = c + d;
    }
}
/* a real scalar: real * complex = (a zr) + (a zi) i, i.e. the real operation over the 2 n reals */
void SFX(cr_raxpy)(int64_t n, R a, const R *x, R *y) { for (int64_t i = 0; i < 2 * n; ++i) { const R p = a * x[i]; y[i] = y[i] + p; } }
void SFX(cr_rxpby)(int64_t n, const R *x, R b, R *y) { for (int64_t i = 0; i < 2 * n; ++i) { const R p = b * y[i]; y[i] = x[i] + p; } }
void SFX(cr_rscal)(int64_t n, R a, R *x) { for (int64_t i = 0; i < 2 * n; ++i) x[i] = x[i] * a; }
void SFX(cr_sub)(int64_t n, const R *x, R *y) { for (int64_t i = 0; i < 2 * n; ++i) y[i] = y[i] - x[i]; }

/* ---- SpMV on CSR (0-based), columns ascending within a row ---- */
static void SFX(prod)(const R *val, const R *x, int64_t k, int64_t c, R *pr, R *pi)
{
    const R ar = val[2 * k], ai = val[2 * k + 1], xr = x[2 * c], xi = x[2 * c + 1];
    const R a = ar * xr, b = ai * xi, cc = ar * xi, d = ai * xr;
    *pr = a - b;
    *pi = cc + d;
}

/* one segment of a long row with the wave shape: lane l adds, from +0 and ascending, the products of the groups l, l + 64, ... of `group`
 * consecutive entries; then the wave tree */
static void SFX(wave_row)(const int *col, const R *val, const R *x, int64_t k0, int len, int group, R *sr, R *si)
{
    R lr[64], li[64];
    for (int l = 0; l < 64; ++l) {
        R ar = 0, ai = 0;
        for (int g = l; g * group < len; g += 64)
            for (int q = 0; q < group; ++q) {
                const int e = g * group + q;
                if (e >= len) break;
                R pr, pi;
                SFX(prod)(val, x, k0 + e, col[k0 + e], &pr, &pi);
                ar = ar + pr;
                ai = ai + pi;
            }
        lr[l] = ar;
        li[l] = ai;
    }
    *sr = SFX(wave)(lr);
    *si = SFX(wave)(li);
}

/* rows of at most long_row entries: serial from +0 in ascending column order; longer rows: segments of `segment` entries, each with the wave
 * shape, the segment sums added left to right */
void SFX(cr_spmv)(int64_t n_rows, const int *rowptr, const int *col, const R *val, const R *x, R *y, int long_row, int segment, int group)
{
    for (int64_t r = 0; r < n_rows; ++r) {
        const int lo = rowptr[r], len = rowptr[r + 1] - lo;
        R sr = 0, si = 0;
        if (len <= long_row) {
            for (int e = 0; e < len; ++e) {
                R pr, pi;
                SFX(prod)(val, x, (int64_t)lo + e, col[lo + e], &pr, &pi);
                sr = sr + pr;
                si = si + pi;
            }
        } else {
            for (int o = 0; o < len; o += segment) {
                R tr, ti;
                SFX(wave_row)(col, val, x, (int64_t)lo + o, len - o < segment ? len - o : segment, group, &tr, &ti);
                if (o == 0) { sr = tr; si = ti; }
                else { sr = sr + tr; si = si + ti; }
            }
        }
        y[2 * r] = sr;
        y[2 * r + 1] = si;
    }
}

/* ---- Modified Gram-Schmidt, src/orthogonalize.jl:67-79: h[i] = dot(V[:, i], w); w -= h[i] V[:, i]; nrm = norm(w); w *= inv(nrm) ---- */
R SFX(cr_mgs)(int64_t n, int k, const R *V, int64_t ldv, R *w, R *h, int W, int L)
{
    for (int i = 0; i < k; ++i) {
        const R *v = V + 2 * (int64_t)i * ldv;
        SFX(cr_dot)(n, v, w, W, L, h + 2 * i);
        const R hr = h[2 * i], hi = h[2 * i + 1];
        for (int64_t j = 0; j < n; ++j) {
            const R vr = v[2 * j], vi = v[2 * j + 1];
            const R a = hr * vr, b = hi * vi, c = hr * vi, d = hi * vr;
            const R pr = a - b, pi = c + d;
            w[2 * j] = w[2 * j] - pr;
            w[2 * j + 1] = w[2 * j + 1] - pi;
        }
    }
    const R nrm = SFX(cr_nrm2)(n, w, W, L);
    const R inv = (R)1 / nrm;
    for (int64_t j = 0; j < 2 * n; ++j) w[j] = w[j] * inv;
    return nrm;
}

/* ---- y += alpha V[:, 1:k] c: t_j = alpha c_j; y = y + t_j V[:, j], columns ascending ---- */
void SFX(cr_gemv_n)(int64_t n, int k, const R *V, int64_t ldv, const R *c, const R *alpha, R *y)
{
    for (int j = 0; j < k; ++j) {
        const R a = alpha[0] * c[2 * j], b = alpha[1] * c[2 * j + 1], cc = alpha[0] * c[2 * j + 1], d = alpha[1] * c[2 * j];
        const R tr = a - b, ti = cc + d;
        SFX(cr_axpy)(n, (const R[2]){tr, ti}, V + 2 * (int64_t)j * ldv, y);
    }
}

#endif
