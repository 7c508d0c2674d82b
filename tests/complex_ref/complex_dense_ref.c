/* complex_dense_ref.c -- C99 restatement of the orders DESIGN.md section 18 fixes for the dense operator on a complex column-major
 * matrix (interleaved re, im; lda in elements).  Test infrastructure: it shares no code with the library and is built by the tests
 * (gcc -std=c99 -O2 -ffp-contract=off), once per component type through the self-include below.
 *
 *   y = A x    chunks of C columns; p_c[i] = serial sum from (+0, +0) over the chunk's columns ascending of the rounded product
 *              A[i,j] x[j] = (ar xr - ai xi) + (ar xi + ai xr) i; y[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ... componentwise
 *   y = A' x   y[j] = sum_i conj(A[i,j]) x[i]: per element re = ar xr + ai xi, im = ar xi - ai xr, then the two-level tree of shape
 *              (W, L) for re and for im: segments of 256 W L elements, thread t owns, for l < L, the W elements from l 256 W + W t;
 *              wave-64 shuffle-down trees, the 4 wave sums left to right; level 2: 1024 threads, thread t adds the segment sums
 *              t, t + 1024, ... from +0, wave trees, the 16 wave sums left to right
 */
#ifndef CD_BODY
#define CD_BODY
#include <stdint.h>
#include <stdlib.h>

#define CD_THREADS 256
#define CD_FIN 1024

#define R double
#define SFX(name) name##_f64
#include "complex_dense_ref.c"
#undef R
#undef SFX

#define R float
#define SFX(name) name##_f32
#include "complex_dense_ref.c"

#else /* ---- the body, once per R ---- */

void SFX(cd_mul_n)(int64_t m, int64_t n, const R *A, int64_t lda, const R *x, R *y, int C)
{
    for (int64_t i = 0; i < m; ++i) {
        R yr = 0, yi = 0;
        for (int64_t j0 = 0; j0 < n; j0 += C) {
            R pr = 0, pi = 0;
            for (int64_t j = j0; j < n && j < j0 + C; ++j) {
                const R ar = A[2 * (j * lda + i)], ai = A[2 * (j * lda + i) + 1], xr = x[2 * j], xi = x[2 * j + 1];
                const R a = ar * xr, b = ai * xi, c = ar * xi, d = ai * xr;
                const R re = a - b, im = c + d;
                pr = pr + re;
                pi = pi + im;
            }
            if (j0 == 0) { yr = pr; yi = pi; }
            else { yr = yr + pr; yi = yi + pi; }
        }
        y[2 * i] = yr;
        y[2 * i + 1] = yi;
    }
}

static R SFX(cd_wave)(R *v)
{
    for (int off = 32; off >= 1; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0];
}

static R SFX(cd_level2)(const R *S, int64_t m)
{
    R t[CD_FIN];
    for (int i = 0; i < CD_FIN; ++i) {
        R a = 0;
        for (int64_t j = i; j < m; j += CD_FIN) a = a + S[j];
        t[i] = a;
    }
    R tot = SFX(cd_wave)(t);
    for (int w = 1; w < 16; ++w) tot = tot + SFX(cd_wave)(t + 64 * w);
    return tot;
}

void SFX(cd_mul_t)(int64_t m, int64_t n, const R *A, int64_t lda, const R *x, R *y, int W, int L)
{
    const int64_t seg = (int64_t)CD_THREADS * W * L, nseg = (m + seg - 1) / seg;
    R *sr = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1)), *si = (R *)malloc(sizeof(R) * (size_t)(nseg > 0 ? nseg : 1));
    for (int64_t j = 0; j < n; ++j) {
        const R *col = A + 2 * j * lda;
        for (int64_t s = 0; s < nseg; ++s) {
            R tr[CD_THREADS], ti[CD_THREADS];
            for (int t = 0; t < CD_THREADS; ++t) {
                R accr = 0, acci = 0;
                for (int l = 0; l < L; ++l)
                    for (int e = 0; e < W; ++e) {
                        const int64_t i = s * seg + (int64_t)l * CD_THREADS * W + (int64_t)W * t + e;
                        if (i >= m) continue;
                        const R ar = col[2 * i], ai = col[2 * i + 1], xr = x[2 * i], xi = x[2 * i + 1];
                        const R p = ar * xr, q = ai * xi, u = ar * xi, v = ai * xr;
                        const R re = p + q, im = u - v;
                        accr = accr + re;
                        acci = acci + im;
                    }
                tr[t] = accr;
                ti[t] = acci;
            }
            for (int c = 0; c < 2; ++c) {
                R *t4 = c ? ti : tr;
                R tot = SFX(cd_wave)(t4);
                tot = tot + SFX(cd_wave)(t4 + 64);
                tot = tot + SFX(cd_wave)(t4 + 128);
                tot = tot + SFX(cd_wave)(t4 + 192);
                (c ? si : sr)[s] = tot;
            }
        }
        y[2 * j] = SFX(cd_level2)(sr, nseg);
        y[2 * j + 1] = SFX(cd_level2)(si, nseg);
    }
    free(sr);
    free(si);
}

#endif
