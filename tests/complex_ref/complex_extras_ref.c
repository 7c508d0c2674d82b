/* complex_extras_ref.c -- C99 restatement of what DESIGN.md section 22 fixes for qmr on the complex element types (interleaved re, im):
 * the three fused sweeps mik_axpy2_dot, mik_scal2 and mik_qmr_update in the statement order of src/qmr.jl, and the product with
 * adjoint(A) as SparseArrays runs it on a SparseMatrixCSC (a loop over the columns of A).  Test infrastructure: written from src/qmr.jl
 * and the contract in include/mik.h, it shares no code with the library and is built by the tests
 * (gcc -std=c99 -O2 -ffp-contract=off), once per component type through the self-include below.
 *
 *   z * w     = (zr wr - zi wi) + (zr wi + zi wr) i          every product rounded, nothing fused
 *   y += a x  : the product z * w with z = a, w = x, then one rounded add per component
 *   x *= a    : the product z * w with z = x, w = a
 *   dot(z, y) = sum conj(z_i) y_i; per element re = zr yr + zi yi, im = zr yi - zi yr, then one tree for re and one for im:
 *               level 1 over segments of 256 W L elements (thread t owns, for l < L, the W elements from l 256 W + W t and adds them
 *               in that order from +0; wave-64 shuffle-down trees; the 4 wave sums left to right), level 2 over the segment sums
 *               (1024 threads, thread t adds S[t], S[t + 1024], ... from +0; wave trees; the 16 wave sums left to right)
 */
#ifndef CE_BODY
#define CE_BODY
#include <stdint.h>
#include <stdlib.h>

#define CE_THREADS 256
#define CE_FIN 1024

#define R double
#define SFX(name) name##_f64
#include "complex_extras_ref.c"
#undef R
#undef SFX

#define R float
#define SFX(name) name##_f32
#include "complex_extras_ref.c"

#else /* ---- the body, once per R ---- */

/* (pr, pi) = (zr + zi i) (wr + wi i) */
static void SFX(mul)(R zr, R zi, R wr, R wi, R *pr, R *pi)
{
    const R a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
    *pr = a - b;
    *pi = c + d;
}

/* y_i += s x_i */
static void SFX(madd)(const R *s, const R *x, R *y, int64_t i)
{
    R pr, pi;
    SFX(mul)(s[0], s[1], x[2 * i], x[2 * i + 1], &pr, &pi);
    y[2 * i] = y[2 * i] + pr;
    y[2 * i + 1] = y[2 * i + 1] + pi;
}

/* y_i += s x_i with a real s: real x complex */
static void SFX(rmadd)(R s, const R *x, R *y, int64_t i)
{
    const R p = s * x[2 * i], q = s * x[2 * i + 1];
    y[2 * i] = y[2 * i] + p;
    y[2 * i + 1] = y[2 * i + 1] + q;
}

static R SFX(wave)(R *v)
{
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

static R SFX(block)(R *t)
{
    R tot = SFX(wave)(t);
    for (int w = 1; w < CE_THREADS / 64; ++w) tot = tot + SFX(wave)(t + 64 * w);
    return tot;
}

static R SFX(final)(const R *S, int64_t m)
{
    R t[CE_FIN];
    for (int i = 0; i < CE_FIN; ++i) {
        R a = 0;
        for (int64_t j = i; j < m; j += CE_FIN) a = a + S[j];
        t[i] = a;
    }
    R tot = SFX(wave)(t);
    for (int w = 1; w < CE_FIN / 64; ++w) tot = tot + SFX(wave)(t + 64 * w);
    return tot;
}

/* out = dot(z, y) = sum conj(z_i) y_i on the tree described above */
static void SFX(dot_zy)(int64_t n, const R *z, const R *y, int W, int L, R *out)
{
    const int64_t seg = (int64_t)CE_THREADS * W * L, nseg = (n + seg - 1) / seg;
    R *sr = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1)), *si = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1));
    for (int64_t s = 0; s < nseg; ++s) {
        R tr[CE_THREADS], ti[CE_THREADS];
        for (int t = 0; t < CE_THREADS; ++t) {
            R ar = 0, ai = 0;
            for (int l = 0; l < L; ++l)
                for (int e = 0; e < W; ++e) {
                    const int64_t i = s * seg + (int64_t)l * CE_THREADS * W + (int64_t)W * t + e;
                    if (i >= n) continue;
                    const R zr = z[2 * i], zi = z[2 * i + 1], yr = y[2 * i], yi = y[2 * i + 1];
                    const R p = zr * yr, q = zi * yi, u = zr * yi, v = zi * yr;
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
    out[0] = SFX(final)(sr, nseg);
    out[1] = SFX(final)(si, nseg);
    free(sr);
    free(si);
}

/* mik_axpy2_dot: y += a x1; y += b x2 (x2 may be NULL); z != NULL: out = dot(z, y).  real_scalars: a[0] and b[0] are reals that multiply
 * as real x complex.  -- src/qmr.jl: the two axpy! of a Lanczos vector and vw = dot(v_next, w_next) */
void SFX(ce_axpy2_dot)(int64_t n, int real_scalars, const R *a, const R *x1, const R *b, const R *x2, R *y, const R *z, int W, int L, R *out)
{
    for (int64_t i = 0; i < n; ++i) {
        if (real_scalars) SFX(rmadd)(a[0], x1, y, i); else SFX(madd)(a, x1, y, i);
        if (x2) { if (real_scalars) SFX(rmadd)(b[0], x2, y, i); else SFX(madd)(b, x2, y, i); }
    }
    if (z) SFX(dot_zy)(n, z, y, W, L, out);
}

/* mik_scal2: x *= a; y *= b  -- rmul!(v_next, inv(delta)); rmul!(w_next, inv(beta)) */
void SFX(ce_scal2)(int64_t n, const R *a, R *x, const R *b, R *y)
{
    for (int64_t i = 0; i < n; ++i) {
        R pr, pi;
        SFX(mul)(x[2 * i], x[2 * i + 1], a[0], a[1], &pr, &pi);
        x[2 * i] = pr; x[2 * i + 1] = pi;
        SFX(mul)(y[2 * i], y[2 * i + 1], b[0], b[1], &pr, &pi);
        y[2 * i] = pr; y[2 * i + 1] = pi;
    }
}

/* mik_qmr_update: p = v; p += neg_h1 p_curr (if p_curr); p += neg_h0 p_prev (if p_prev); p *= inv; x += g p; p_out = p.
 * Element i of p_prev is read before element i of p_out is written, so p_out may be p_prev. */
void SFX(ce_qmr_update)(int64_t n, const R *v, const R *neg_h1, const R *p_curr, const R *neg_h0, const R *p_prev, const R *inv, const R *g, R *x,
                        R *p_out)
{
    for (int64_t i = 0; i < n; ++i) {
        R p[2] = {v[2 * i], v[2 * i + 1]};
        if (p_curr) SFX(madd)(neg_h1, p_curr + 2 * i, p, 0);
        if (p_prev) SFX(madd)(neg_h0, p_prev + 2 * i, p, 0);
        R sr, si;
        SFX(mul)(p[0], p[1], inv[0], inv[1], &sr, &si);
        p[0] = sr; p[1] = si;
        SFX(madd)(g, p, x + 2 * i, 0);
        p_out[2 * i] = p[0];
        p_out[2 * i + 1] = p[1];
    }
}

/* y = adjoint(A) x for A (m x n) in CSC with 0-based colptr / rowval: y[j] = sum over the stored entries of column j, in storage order,
 * of conj(a) x[row] -- mul!(y, adjoint(A), x) of SparseArrays */
void SFX(ce_adj_mul)(int64_t n_cols, const int64_t *colptr, const int64_t *rowval, const R *nzval, const R *x, R *y)
{
    for (int64_t j = 0; j < n_cols; ++j) {
        R sr = 0, si = 0;
        for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k) {
            R pr, pi;
            SFX(mul)(nzval[2 * k], -nzval[2 * k + 1], x[2 * rowval[k]], x[2 * rowval[k] + 1], &pr, &pi);
            sr = sr + pr;
            si = si + pi;
        }
        y[2 * j] = sr;
        y[2 * j + 1] = si;
    }
}

#endif
