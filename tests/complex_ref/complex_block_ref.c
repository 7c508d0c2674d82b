/* complex_block_ref.c -- C99 restatement of the four block entries of lobpcg for the complex element types (DESIGN.md section 20;
 * interleaved re, im; blocks column-major, leading dimensions in elements).  Test infrastructure: it shares no code with the library and
 * is built by the tests (gcc -std=c99 -O2 -ffp-contract=off), once per component type through the self-include below.
 *
 *   spmm     column j of Y = cr_spmv(A, column j of X): the row orders of complex_ref.c
 *   gram     G[i, j] = cr_dot(X[:, i], Y[:, j]): the dot tree of complex_ref.c with its (W, L) argument
 *   rdiv     for i ascending: X[:, i] = X[:, i] - X[:, j] * R[j, i] for j < i ascending, then X[:, i] = (re / d, im / d), d = real(R[i, i])
 *   update   Pout = rot(R, Vr) (+ rot(P, Vp)); Xout = rot(X, Vx) (+ Pout); rot opens a sum with its first product, columns ascending
 *   z * w  = (zr wr - zi wi) + (zr wi + zi wr) i          every product rounded, nothing fused; sums componentwise
 */
#ifndef CB_BODY
#define CB_BODY
#include "complex_ref.c"        /* cr_dot_*, cr_spmv_* */
#undef R
#undef SFX
#undef CR_SQRT
#undef CR_FABS
#undef CR_LO
#undef CR_HI
#undef CR_EC

#define R double
#define SFX(name) name##_f64
#include "complex_block_ref.c"
#undef R
#undef SFX

#define R float
#define SFX(name) name##_f32
#include "complex_block_ref.c"

#else /* ---- the body, once per R ---- */

void SFX(cb_spmm)(int64_t n_rows, const int *rowptr, const int *col, const R *val, int b, const R *X, int64_t ldx, R *Y, int64_t ldy,
                  int long_row, int segment, int group)
{
    for (int j = 0; j < b; ++j) SFX(cr_spmv)(n_rows, rowptr, col, val, X + 2 * (int64_t)j * ldx, Y + 2 * (int64_t)j * ldy, long_row, segment, group);
}

void SFX(cb_gram)(int64_t n, int p, int q, const R *X, int64_t ldx, const R *Y, int64_t ldy, int W, int L, R *G, int64_t ldg)
{
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < p; ++i) SFX(cr_dot)(n, X + 2 * (int64_t)i * ldx, Y + 2 * (int64_t)j * ldy, W, L, G + 2 * ((int64_t)j * ldg + i));
}

/* 0, or 1 + the first column whose diagonal entry has a non-zero imaginary part (nothing is changed then) */
int SFX(cb_rdiv)(int64_t n, int s, const R *Rm, int64_t ldr, R *X, int64_t ldx)
{
    for (int i = 0; i < s; ++i)
        if (!(Rm[2 * ((int64_t)i * ldr + i) + 1] == 0)) return 1 + i;
    for (int64_t r = 0; r < n; ++r)
        for (int i = 0; i < s; ++i) {
            R xr = X[2 * ((int64_t)i * ldx + r)], xi = X[2 * ((int64_t)i * ldx + r) + 1];
            for (int j = 0; j < i; ++j) {
                const R zr = X[2 * ((int64_t)j * ldx + r)], zi = X[2 * ((int64_t)j * ldx + r) + 1];
                const R wr = Rm[2 * ((int64_t)i * ldr + j)], wi = Rm[2 * ((int64_t)i * ldr + j) + 1];
                const R a = zr * wr, b = zi * wi, c = zr * wi, d = zi * wr;
                const R pr = a - b, pi = c + d;
                xr = xr - pr;
                xi = xi - pi;
            }
            const R d = Rm[2 * ((int64_t)i * ldr + i)];
            X[2 * ((int64_t)i * ldx + r)] = xr / d;
            X[2 * ((int64_t)i * ldx + r) + 1] = xi / d;
        }
    return 0;
}

/* out[jj] = (...(W[r, 0] F[0, jj] + W[r, 1] F[1, jj]) + ...) + W[r, k-1] F[k-1, jj] for jj < cols; F: rows of V from row f0, leading dimension ldv */
static void SFX(cb_rot_row)(const R *Wm, int64_t ld, int k, const R *V, int64_t ldv, int f0, int cols, int64_t r, R *out)
{
    for (int jj = 0; jj < cols; ++jj) {
        R sr = 0, si = 0;
        for (int c = 0; c < k; ++c) {
            const R zr = Wm[2 * ((int64_t)c * ld + r)], zi = Wm[2 * ((int64_t)c * ld + r) + 1];
            const R wr = V[2 * ((int64_t)jj * ldv + f0 + c)], wi = V[2 * ((int64_t)jj * ldv + f0 + c) + 1];
            const R a = zr * wr, b = zi * wi, cc = zr * wi, d = zi * wr;
            const R pr = a - b, pi = cc + d;
            if (c == 0) { sr = pr; si = pi; }
            else { sr = sr + pr; si = si + pi; }
        }
        out[2 * jj] = sr;
        out[2 * jj + 1] = si;
    }
}

void SFX(cb_update)(int64_t n, int sx, int b1, int b2, const R *X, int64_t ldx, const R *Rm, int64_t ldr, const R *P, int64_t ldp, const R *V,
                    int64_t ldv, R *Xout, int64_t ldxo, R *Pout, int64_t ldpo)
{
    R pout[64], acc[64];                                 /* sx <= 32 */
    for (int64_t r = 0; r < n; ++r) {
        if (b1 > 0) {
            SFX(cb_rot_row)(Rm, ldr, b1, V, ldv, sx, sx, r, pout);
            if (b2 > 0) {
                SFX(cb_rot_row)(P, ldp, b2, V, ldv, sx + b1, sx, r, acc);
                for (int q = 0; q < 2 * sx; ++q) pout[q] = pout[q] + acc[q];
            }
            for (int jj = 0; jj < sx; ++jj) {
                Pout[2 * ((int64_t)jj * ldpo + r)] = pout[2 * jj];
                Pout[2 * ((int64_t)jj * ldpo + r) + 1] = pout[2 * jj + 1];
            }
        }
        SFX(cb_rot_row)(X, ldx, sx, V, ldv, 0, sx, r, acc);
        if (b1 > 0)
            for (int q = 0; q < 2 * sx; ++q) acc[q] = acc[q] + pout[q];
        for (int jj = 0; jj < sx; ++jj) {
            Xout[2 * ((int64_t)jj * ldxo + r)] = acc[2 * jj];
            Xout[2 * ((int64_t)jj * ldxo + r) + 1] = acc[2 * jj + 1];
        }
    }
}

#endif
