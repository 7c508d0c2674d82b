// mik_krylov.hip -- L2 Krylov helpers (orthogonalize_and_normalize!, gemv) and the L3 iterables
// (CGIterable / PCGIterable, GMRESIterable) of include/mik.h.
//
// Host-side control flow restates the reference's iterate() methods (src/cg.jl:43-100,
// src/gmres.jl:57-106); all vector arithmetic runs in the kernels of mik_kernels.h.
#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cmath>
#include <map>
#include <new>
#include <tuple>

#include "mik_kernels.h"
#include "mik_mgs_res.h"
#include "mik_complex.h"
#include "mik_iter.h"
#include "mik_mail.h"

// =============================================================================================
// Hessenberg least squares (host) -- src/hessenberg.jl:15-46
// =============================================================================================

// LinearAlgebra.givensAlgorithm(f, g): LAPACK xLARTG-style plane rotation with power-of-two
// rescaling; [c s; -s c] * [f; g] = [r; 0].
template <typename T> static void givens_algorithm(T f, T g, T &cs, T &sn, T &r)
{
    // safmn2 = LinearAlgebra.floatmin2(T) = 2^trunc(log2(floatmin(T) / eps(T)) / 2) with eps(T) = the spacing at 1
    // (2^-52 / 2^-23, NOT LAPACK's unit roundoff): 2^-485 for Float64 (0x21a0000000000000), 2^-51 for Float32.
    const T eps = std::numeric_limits<T>::epsilon();
    const T safmin = std::numeric_limits<T>::min();
    const T safmn2 = std::pow(T(2), T((int)(std::log(safmin / eps) / std::log(T(2)) / T(2))));
    const T safmx2 = T(1) / safmn2;
    if (g == T(0)) { cs = T(1); sn = T(0); r = f; return; }
    if (f == T(0)) { cs = T(0); sn = T(1); r = g; return; }
    T f1 = f, g1 = g;
    T scale = std::max(std::fabs(f1), std::fabs(g1));
    int count = 0;
    if (scale >= safmx2) {
        do { ++count; f1 *= safmn2; g1 *= safmn2; scale = std::max(std::fabs(f1), std::fabs(g1)); } while (scale >= safmx2);
        r = std::sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
        for (int i = 0; i < count; ++i) r *= safmx2;
    } else if (scale <= safmn2) {
        do { ++count; f1 *= safmx2; g1 *= safmx2; scale = std::max(std::fabs(f1), std::fabs(g1)); } while (scale <= safmn2);
        r = std::sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
        for (int i = 0; i < count; ++i) r *= safmn2;
    } else {
        r = std::sqrt(f1 * f1 + g1 * g1); cs = f1 / r; sn = g1 / r;
    }
    if (std::fabs(f) > std::fabs(g) && cs < T(0)) { cs = -cs; sn = -sn; r = -r; }
}

template <typename T> static void hessenberg_ldiv(T *H, int64_t ldh, int width, T *rhs)
{
    auto at = [&](int i, int j) -> T & { return H[(size_t)j * ldh + i]; };
    for (int i = 0; i < width; ++i) {
        T c, s, rr;
        givens_algorithm(at(i, i), at(i + 1, i), c, s, rr);
        at(i, i) = c * at(i, i) + s * at(i + 1, i);
        for (int j = i + 1; j < width; ++j) {
            const T tmp = -s * at(i, j) + c * at(i + 1, j);
            at(i, j) = c * at(i, j) + s * at(i + 1, j);
            at(i + 1, j) = tmp;
        }
        const T tmp = -s * rhs[i] + c * rhs[i + 1];
        rhs[i] = c * rhs[i] + s * rhs[i + 1];
        rhs[i + 1] = tmp;
    }
    // UpperTriangular back substitution, column sweep from the last column
    for (int j = width - 1; j >= 0; --j) {
        rhs[j] = rhs[j] / at(j, j);
        const T t = rhs[j];
        for (int i = 0; i < j; ++i) rhs[i] = rhs[i] - t * at(i, j);
    }
}

extern "C" int mik_hessenberg_ldiv(int dtype, void *H, int64_t ldh, int width, void *rhs)
{
    if (!H || !rhs || width < 0 || ldh < width + 1) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_hessenberg_ldiv(dtype, H, ldh, width, rhs);
    if (dtype == MIK_F64) hessenberg_ldiv<double>((double *)H, ldh, width, (double *)rhs);
    else if (dtype == MIK_F32) hessenberg_ldiv<float>((float *)H, ldh, width, (float *)rhs);
    else return MIK_ERR_INVALID;
    return MIK_OK;
}

// =============================================================================================
// gemv-N and orthogonalisation
// =============================================================================================
// Cache hints of a pass of the multi-launch Modified Gram-Schmidt chain (OpMgsPass::nt: 1 = v, 2 = z, 4 = w load, 8 = w store non-temporal).
// The column that is subtracted in this pass and not needed again is streamed; when three vectors cannot share the 256 MB Infinity Cache
// anyway, w is streamed too (load and store), so that the column projected on in this pass -- the one the NEXT pass subtracts -- is what
// the cache keeps.  Measured at 256^3 fp64 (gmres!(30), 60 inner iterations, one box, round 5): mask 0: 1,879 us per inner iteration,
// 1 (v): 1,651, 3 (v, z): 1,684, 9: 1,648, 5: 1,660, 11: 1,686, 15 (all): 1,835, 13 (v, w): 1,622.
static inline int mik_mgs_pass_hints(const mik_ctx *ctx, int64_t n, size_t es)
{
    (void)ctx;
    return (double)n * (double)es > 96.0e6 ? 13 : 1;
}

template <typename T>
static int gemv_n_dev(mik_ctx *ctx, int64_t n, int k, const T *V, int64_t ldv, const T *cf_dev, T alpha, T *y)
{
    return launch_gemv_n<T>(ctx, n, k, V, ldv, cf_dev, alpha, y, mik_basis_nt<T>(n, k));
}

// Copy k host scalars into the coefficient area of the context (device), at element `slot`.
template <typename T> static int coef_upload(mik_ctx *ctx, int slot, const T *host, int k)
{
    if ((size_t)(slot + k) * sizeof(T) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "coefficient block too large (k = %d)", k);
    MIK_HIP(ctx, mik_wait(ctx));                        // staging buffer must be idle
    memcpy((T *)ctx->coef_host + slot, host, sizeof(T) * k);
    MIK_HIP(ctx, hipMemcpyAsync((T *)ctx->coef + slot, (T *)ctx->coef_host + slot, sizeof(T) * k, hipMemcpyHostToDevice, ctx->stream));
    return MIK_OK;
}

template <typename T> static int coef_download(mik_ctx *ctx, int slot, T *host, int k)
{
    return mik_read_scalars<T>(ctx, (const T *)ctx->coef + slot, k, host);
}

template <typename T>
static int gemv_n_impl(mik_ctx *ctx, int64_t n, int k, const void *V, int64_t ldv, const void *c, const void *alpha, void *y)
{
    if (k == 0 || n == 0) return MIK_OK;
    MIK_TRY(coef_upload<T>(ctx, 0, (const T *)c, k));
    return gemv_n_dev<T>(ctx, n, k, (const T *)V, ldv, (const T *)ctx->coef, *(const T *)alpha, (T *)y);
}

extern "C" int mik_gemv_n(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *c,
                          const void *alpha, void *y)
{
    if (!ctx || n < 0 || k < 0 || !alpha || (k && !c) || (n && k && (!V || !y)) || ldv < n) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_gemv_n(ctx, dtype, n, k, V, ldv, c, alpha, y);
    if (dtype == MIK_F64) return gemv_n_impl<double>(ctx, n, k, V, ldv, c, alpha, y);
    if (dtype == MIK_F32) return gemv_n_impl<float>(ctx, n, k, V, ldv, c, alpha, y);
    return MIK_ERR_INVALID;
}

template <typename T> static int finalize_store(mik_ctx *ctx, int64_t nseg, int cols, T *out_dev)
{
    hipLaunchKernelGGL((k_finalize_store<T>), dim3(cols), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)ctx->partials, nseg,
                       nseg, out_dev, (const int *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T> static int finalize_nrm_inv(mik_ctx *ctx, int64_t nseg, T *out_dev)
{
    hipLaunchKernelGGL((k_finalize_nrm_inv<T>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)ctx->partials, nseg, out_dev);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T>
static int multidot(mik_ctx *ctx, int64_t n, int k, const T *V, int64_t ldv, const T *w, T *out_dev)
{
    return launch_multidot<T>(ctx, n, k, V, ldv, w, out_dev, mik_basis_nt<T>(n, k));
}

// orthogonalize_and_normalize!(V[:, 1:k], w, h, method) -> nrm   -- src/orthogonalize.jl:13-79
// Coefficient area layout (elements of T): [0, k) = h, [k] = nrm, [k+1] = 1/nrm, [k+2, 2k+2) = DGKS correction.

// Workspace the chains below need in ctx->partials.
template <typename T> static size_t orthogonalize_workspace(int64_t n, int k)
{
    const int64_t nseg = mik_nseg<T>(n);
    return sizeof(T) * std::max<size_t>((size_t)std::max<int64_t>(nseg, 1) * (size_t)std::max(k, 1), 2 * 1024);
}

template <typename T> static T dgks_small_norm(const T *v, int len)
{
    T s = T(0);
    for (int j = 0; j < len; ++j) { T p = v[j] * v[j]; s = s + p; }
    return (T)std::sqrt(s);
}

// Where the sums of the Gram-Schmidt reductions live: the one thing the three transports do differently.
//   LOCAL     one GPU: the finalisers leave the totals in ctx->coef.
//   CALLBACK  a row partition coupled by the host's reduce(): every total goes to the host, is summed over the ranks there in rank order and
//             comes back as a kernel argument; a norm is sqrt of that sum, taken on the host.
//   LINK      a row partition with a device-driven link (csrc/mik_comm.hip "mik_plink"): the finaliser adds the rank totals itself (plink_fin_sum: the
//             additions of reduce(), the same bits), so the dependent reductions of an Arnoldi column run back to back on the stream and the host
//             waits once per column (once per DGKS round).
// A rank with no local rows takes part in every exchange like the others.
template <typename T> struct GsSums {
    enum Mode { LOCAL, CALLBACK, LINK };
    mik_ctx *ctx;
    const mik_partition *part;      // NULL: LOCAL
    Mode mode;
    int64_t n, nseg;
    int k;
    T *h;                           // host, k coefficients (CALLBACK: written as the reductions finish)
    T *hd, *partials;
    T nrm_cb = T(0);                // CALLBACK: the last norm (NaN: its sum of squares was outside the safe range)

    GsSums(mik_ctx *c, const mik_partition *p, int64_t n_, int k_, T *h_)
        : ctx(c), part(p), mode(!p ? LOCAL : p->link ? LINK : CALLBACK), n(n_), nseg(mik_nseg<T>(n_)), k(k_), h(h_), hd((T *)c->coef),
          partials((T *)c->partials) {}

    int ready()
    {
        if ((size_t)(2 * k + 4) * sizeof(T) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "orthogonalize: k = %d too large", k);
        MIK_TRY(mik_ensure_partials(ctx, orthogonalize_workspace<T>(n, k)));
        partials = (T *)ctx->partials;
        return MIK_OK;
    }
    // values[0, count): this rank's partial sums -> the sums over the ranks in rank order (CALLBACK)
    int reduce(T *values, int count) const
    {
        if (!part->reduce || count <= 0) return MIK_OK;
        if (part->reduce(part->user, sizeof(T) == 8 ? MIK_F64 : MIK_F32, count, values) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "gmres: reduce callback failed");
        return MIK_OK;
    }
    // The segment sums in ctx->partials -> their total into coefficient slot `slot`.  norm: nrm into `slot` and 1 / nrm into slot + 1 (NaN and 1
    // outside the safe range: w is then left unscaled).  CALLBACK: the total goes to the host, into h[slot] or, for a norm, into nrm_cb.
    int finish(int slot, bool norm)
    {
        if (mode == LINK) return plink_fin_sum(part->link, partials, nseg, hd + slot, norm ? 1 : 0);
        if (mode == LOCAL) return norm ? finalize_nrm_inv<T>(ctx, nseg, hd + slot) : finalize_store<T>(ctx, nseg, 1, hd + slot);
        T v;
        MIK_TRY(finalize_store<T>(ctx, nseg, 1, hd + slot));
        MIK_TRY(coef_download<T>(ctx, slot, &v, 1));
        MIK_TRY(reduce(&v, 1));
        if (norm) nrm_cb = mik_nrm_in_range(v) ? (T)std::sqrt(v) : std::numeric_limits<T>::quiet_NaN();
        else h[slot] = v;
        return MIK_OK;
    }
    // coef[slot, slot + k): this rank's k projections -> their sums over the ranks (CALLBACK: through the host, also left in `host`)
    int sum_vec(int slot, T *host)
    {
        if (mode == LINK) return plink_sum_vec(part->link, hd + slot, k);
        if (mode == LOCAL) return MIK_OK;
        MIK_TRY(coef_download<T>(ctx, slot, host, k));
        MIK_TRY(reduce(host, k));
        return coef_upload<T>(ctx, slot, host, k);
    }
    // the coefficient h[i] as a sweep reads it: from the device, or (CALLBACK) the host value it already has -- no upload per pass
    Coef<T> coef(int i) const { return mode == CALLBACK ? coef_val<T>(h[i]) : coef_ptr<T>(hd + i); }
    // The host wait: vec[0, k) from coefficient slot `slot`, and the norm (CALLBACK: both are on the host already).  LINK: every wait checks the mailbox.
    int wait(int slot, T *vec, T *nrm)
    {
        if (mode == CALLBACK) { *nrm = nrm_cb; return MIK_OK; }
        if (slot == 0) {                                                 // h and nrm are adjacent: one read
            std::vector<T> out((size_t)k + 1);
            MIK_TRY(coef_download<T>(ctx, 0, out.data(), k + 1));
            for (int j = 0; j < k; ++j) vec[j] = out[(size_t)j];
            *nrm = out[(size_t)k];
        } else {
            MIK_TRY(coef_download<T>(ctx, slot, vec, k));
            MIK_TRY(coef_download<T>(ctx, k, nrm, 1));
        }
        return mode == LINK ? plink_check(part->link, "gmres (row-partitioned)") : MIK_OK;
    }
    // norm(x) when its plain sum of squares left the safe range: the recomputation of include/mik.h "Norms".  Over a partition: amax = the maximum
    // over the ranks of the local max |x_i| (CALLBACK: through the sum callback, every rank contributing its value in its own slot of a P-vector of
    // zeros, 0 + ... + a_q + 0 being exact; LINK: gathered through the mailboxes), the same power of two on every rank, then the sum over the ranks
    // of the local tree sums of the scaled squares.  oracle/orc_impl.inc safe_nrm_ with a partition is this arithmetic.
    int scaled_norm(const T *x, T *out)
    {
        if (mode == LOCAL) return mik_safe_norm_slow<T>(ctx, n, x, out);
        const bool link = mode == LINK;
        const int P = link ? plink_nranks(part->link) : part->nranks, rank = link ? plink_rank(part->link) : part->rank;
        if (!link && (P < 1 || P > 256 || rank < 0 || rank >= P)) return mik_fail(ctx, MIK_ERR_RANGE, "gmres (row-partitioned): scaled norm needs 1 <= nranks <= 256");
        if (link && (size_t)(P + 2) * sizeof(T) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "gmres (row-partitioned): scaled norm with %d ranks", P);
        T *scr = (T *)((unsigned char *)ctx->coef + mik_ctx::COEF_SAFE_SLOT);   // LINK: P scalars (P <= 64: the mailbox's limit)
        const int grid = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + MIK_BLOCK - 1) / MIK_BLOCK, 1024);
        MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)std::max<int64_t>(std::max<int64_t>(nseg, grid), 1)));
        partials = (T *)ctx->partials;
        hipLaunchKernelGGL((k_amax<T>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, n, x, partials);
        MIK_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL((k_amax<T>), dim3(1), dim3(MIK_BLOCK), 0, ctx->stream, (int64_t)grid, (const T *)partials, scr + (link ? rank : 0));
        MIK_LAUNCH_CHECK(ctx);
        std::vector<T> v((size_t)P, T(0));
        if (link) MIK_TRY(plink_gather(part->link, scr));
        MIK_HIP(ctx, hipMemcpyAsync(link ? v.data() : &v[(size_t)rank], scr, sizeof(T) * (link ? (size_t)P : 1), hipMemcpyDeviceToHost, ctx->stream));
        MIK_HIP(ctx, mik_wait(ctx));
        MIK_TRY(link ? plink_check(part->link, "gmres (row-partitioned)") : reduce(v.data(), P));
        T amax = T(0), sc, sinv;
        for (T a : v) amax = (a > amax || a != a) ? a : amax;
        if (!mik_nrm_scale(amax, sc, sinv)) { *out = amax; return MIK_OK; }
        OpScaledSq<T> op{x, sc};
        MIK_TRY((launch_map<T>(ctx, n, op, mik_aligned16(x), partials, nullptr)));
        MIK_TRY(link ? plink_fin_sum(part->link, partials, nseg, scr, 0) : finalize_store<T>(ctx, nseg, 1, scr));
        T t2;
        MIK_HIP(ctx, hipMemcpyAsync(&t2, scr, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        MIK_HIP(ctx, mik_wait(ctx));
        MIK_TRY(link ? plink_check(part->link, "gmres (row-partitioned)") : reduce(&t2, 1));
        *out = (T)std::sqrt(t2) * sinv;
        return MIK_OK;
    }
    // w .*= inv(nrm) once the host has the closing norm.  `scaled`: the kernels have done it already -- unless the norm came back NaN (its sum of
    // squares was outside the safe range and they multiplied by 1): then the scaled norm first.
    int rescale(T *w, T *nrm, bool scaled)
    {
        if (*nrm != *nrm) { MIK_TRY(scaled_norm(w, nrm)); scaled = false; }
        if (scaled) return MIK_OK;
        OpScal<T> sc{w, coef_val<T>(T(1) / *nrm)};                           // (the same IEEE quotient the device forms)
        return launch_map<T>(ctx, n, sc, mik_aligned16(w), (T *)nullptr, nullptr);
    }
    // after finish(k, true): w .*= inv(nrm) on the device (CALLBACK: on the host's norm), the host wait for h and nrm
    int close(T *w, T *nrm)
    {
        if (mode != CALLBACK) {
            OpScal<T> sc{w, coef_ptr<T>(hd + k + 1)};
            MIK_TRY((launch_map<T>(ctx, n, sc, mik_aligned16(w), (T *)nullptr, nullptr)));
        }
        MIK_TRY(wait(0, h, nrm));
        return rescale(w, nrm, mode != CALLBACK);
    }
};

// h = V' w summed over the ranks into coefficient slot `slot` (CALLBACK: also into `host`), then w -= V h   -- src/orthogonalize.jl:15-17, :27, :30
template <typename T> static int gs_project(GsSums<T> &S, const T *V, int64_t ldv, T *w, int slot, T *host)
{
    if (S.k == 0) return MIK_OK;
    MIK_TRY(multidot<T>(S.ctx, S.n, S.k, V, ldv, w, S.hd + slot));
    MIK_TRY(S.sum_vec(slot, host));
    return gemv_n_dev<T>(S.ctx, S.n, S.k, V, ldv, S.hd + slot, T(-1), w);
}

// The DGKS loop of src/orthogonalize.jl:26-36 from a given state {w unscaled, h in S.h, nrm, projection size}, then the normalisation: every round
// is a batched dot summed over the ranks, the update, the norm and one host wait.  Entered by the chain below and by the single launch's hand-back.
template <typename T> static int gs_dgks(GsSums<T> &S, const T *V, int64_t ldv, T *w, T *nrm, T projection_size)
{
    MIK_TRY(S.ready());
    const int k = S.k;
    OpDot<T> dn{w, w};
    std::vector<T> corr((size_t)std::max(k, 1));
    const T eta = T(1) / std::sqrt(T(2));                                // :20
    while (*nrm < eta * projection_size) {                               // :26
        MIK_TRY(gs_project<T>(S, V, ldv, w, k + 2, corr.data()));        // :27, :30
        MIK_TRY((launch_map<T>(S.ctx, S.n, dn, mik_aligned16(w), S.partials, nullptr)));
        MIK_TRY(S.finish(k, true));                                      // :32
        MIK_TRY(S.wait(k + 2, corr.data(), nrm));
        if (*nrm != *nrm) MIK_TRY(S.scaled_norm(w, nrm));
        projection_size = dgks_small_norm<T>(corr.data(), k);            // :28
        for (int j = 0; j < k; ++j) S.h[j] = S.h[j] + corr[(size_t)j];   // :31
    }
    return S.rescale(w, nrm, false);                                     // :36
}

// orthogonalize_and_normalize! as a chain of launches: h into S.h (host), nrm, w normalised.  `cols` (ModifiedGramSchmidt on one GPU only): V is
// a vector of k separate device vectors -- the method of src/orthogonalize.jl:53-65.
template <typename T>
static int gs_orthogonalize(GsSums<T> S, const T *V, int64_t ldv, T *w, T *nrm, int method, const T *const *cols = nullptr)
{
    MIK_TRY(S.ready());
    mik_ctx *ctx = S.ctx;
    const int64_t n = S.n, nseg = S.nseg;
    const int k = S.k;
    T *hd = S.hd, *part = S.partials;
    const bool vecw = mik_aligned16(w);
    bool vec = vecw && (cols || (mik_aligned16(V) && (ldv % VT<T>::W == 0)));
    auto col = [&](int i) -> const T * { return cols ? cols[i] : V + (int64_t)i * ldv; };
    if (cols) for (int i = 0; i < k; ++i) vec = vec && mik_aligned16(cols[i]);
    const int hints = mik_mgs_pass_hints(ctx, n, sizeof(T));
    OpDot<T> dn{w, w};

    const bool lean = method == MIK_MGS && ctx->tuning[MIK_KNOB_GS] != 1;
    if (lean && S.mode == S.LOCAL && nseg <= 1024) {
        // src/orthogonalize.jl:69-76, launch-lean form for n up to ~1M: every pass finalises the
        // previous pass's reduction itself (k_map_pro), so the chain is k + 2 launches instead of
        // 2k + 3.  Segment sums ping-pong between two buffers (a pass reads one while writing the other).
        T *P[2] = {part, part + 1024};
        const int m = (int)nseg;
        if (k > 0) {
            OpDot<T> d0{col(0), w};
            MIK_TRY((launch_map<T>(ctx, n, d0, vec, P[0], nullptr)));
            for (int i = 0; i + 1 < k; ++i) {
                OpMgsPass<T, false> op{w, col(i), col(i + 1), coef_val<T>(T(0))};
                MIK_TRY((launch_map_pro<T, 1>(ctx, n, op, vec, P[(i + 1) & 1], P[i & 1], m, hd + i)));
            }
            OpMgsPass<T, true> last{w, col(k - 1), nullptr, coef_val<T>(T(0))};
            MIK_TRY((launch_map_pro<T, 1>(ctx, n, last, vec, P[k & 1], P[(k - 1) & 1], m, hd + k - 1)));
        } else {
            MIK_TRY((launch_map<T>(ctx, n, dn, vecw, P[0], nullptr)));
        }
        OpScal<T> sc{w, coef_val<T>(T(0))};                                // w .*= inv(norm(w))  :75-76
        MIK_TRY((launch_map_pro<T, 2>(ctx, n, sc, vecw, (T *)nullptr, P[k & 1], m, hd + k)));
        MIK_TRY(S.wait(0, S.h, nrm));
        return S.rescale(w, nrm, true);
    }
    if (lean && S.mode == S.LINK && nseg <= mik_resident_cap(ctx)) {
        // the same over the link: every pass finalises AND exchanges the previous reduction itself (csrc/mik_comm.hip plink_mgs_lean).
        // At most one segment per compute unit (256 on an unpartitioned MI355X): every workgroup of a pass spins on the mailbox, and ranks that share a GPU must all be resident on it.
        MIK_TRY(plink_mgs_lean(S.part->link, n, k, V, ldv, w, hd, part, vec, vecw, hints));
        MIK_TRY(S.wait(0, S.h, nrm));
        return S.rescale(w, nrm, true);
    }
    if (method == MIK_MGS) {
        // src/orthogonalize.jl:69-76.  Pass i subtracts h[i] * V[:, i] from w and, in the same sweep,
        // accumulates the next projection dot(V[:, i+1], w) -- or norm(w)^2 on the last pass.
        if (k > 0) {
            OpDot<T> d0{col(0), w};
            MIK_TRY((launch_map<T>(ctx, n, d0, vec, part, nullptr)));
            MIK_TRY(S.finish(0, false));
            for (int i = 0; i + 1 < k; ++i) {
                OpMgsPass<T, false> op{w, col(i), col(i + 1), S.coef(i), hints};
                MIK_TRY((launch_map<T>(ctx, n, op, vec, part, nullptr)));
                MIK_TRY(S.finish(i + 1, false));
            }
            OpMgsPass<T, true> last{w, col(k - 1), nullptr, S.coef(k - 1), hints};
            MIK_TRY((launch_map<T>(ctx, n, last, vec, part, nullptr)));
        } else {
            MIK_TRY((launch_map<T>(ctx, n, dn, vecw, part, nullptr)));
        }
    } else {
        // src/orthogonalize.jl:15-17 / :43-45: h = V' w (batched dot), w -= V h (axpy sweep), norm
        MIK_TRY(gs_project<T>(S, V, ldv, w, 0, S.h));
        MIK_TRY((launch_map<T>(ctx, n, dn, vecw, part, nullptr)));
    }
    MIK_TRY(S.finish(k, true));
    if (method != MIK_DGKS) return S.close(w, nrm);                     // w .*= inv(nrm)  :76 / :48
    MIK_TRY(S.wait(0, S.h, nrm));                                        // DGKS, src/orthogonalize.jl:19-36: the loop condition lives on the host
    if (*nrm != *nrm) MIK_TRY(S.scaled_norm(w, nrm));
    return gs_dgks<T>(S, V, ldv, w, nrm, dgks_small_norm<T>(S.h, k));   // :22
}

extern "C" int mik_orthogonalize(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *w, void *h,
                                 void *nrm, int method)
{
    if (!ctx || n < 0 || k < 0 || !nrm || (k && (!h || !V)) || (n && !w) || (k && ldv < n)) return MIK_ERR_INVALID;
    if (method != MIK_MGS && method != MIK_CGS && method != MIK_DGKS) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_orthogonalize(ctx, dtype, n, k, V, ldv, w, h, nrm, method);
    if (dtype == MIK_F64) return gs_orthogonalize<double>(GsSums<double>(ctx, nullptr, n, k, (double *)h), (const double *)V, ldv, (double *)w, (double *)nrm, method);
    if (dtype == MIK_F32) return gs_orthogonalize<float>(GsSums<float>(ctx, nullptr, n, k, (float *)h), (const float *)V, ldv, (float *)w, (float *)nrm, method);
    return MIK_ERR_INVALID;
}

extern "C" int mik_orthogonalize_vectors(mik_ctx *ctx, int dtype, int64_t n, int k, const void *const *V, void *w, void *h, void *nrm)
{
    if (!ctx || n < 0 || k < 0 || !nrm || (k && (!h || !V)) || (n && !w)) return MIK_ERR_INVALID;
    for (int i = 0; i < k; ++i) if (!V[i] && n) return MIK_ERR_INVALID;
    if (dtype == MIK_F64) return gs_orthogonalize<double>(GsSums<double>(ctx, nullptr, n, k, (double *)h), nullptr, 0, (double *)w, (double *)nrm, MIK_MGS, (const double *const *)V);
    if (dtype == MIK_F32) return gs_orthogonalize<float>(GsSums<float>(ctx, nullptr, n, k, (float *)h), nullptr, 0, (float *)w, (float *)nrm, MIK_MGS, (const float *const *)V);
    return MIK_ERR_INVALID;
}

// =============================================================================================
// CGIterable / PCGIterable
// =============================================================================================
// (level2_sum_spread / FinScratch: csrc/mik_iter.h -- shared with the mailbox finalisers of csrc/mik_comm.hip)

// the same for TWO reductions finalised by one launch (the fused PCG tail): one ticket, the last arrival adds both sets
template <typename T> struct FinScratch2 { T ws[MIK_FIN_WGS]; T ws2[MIK_FIN_WGS]; unsigned ticket; };

template <typename T>
__device__ __forceinline__ bool level2_sum_spread2(const T *__restrict__ S1, const T *__restrict__ S2, int64_t m, FinScratch2<T> *fs, T &tot1, T &tot2)
{
    const int w = blockIdx.x, lane = threadIdx.x;              // blockDim.x == 64, gridDim.x == MIK_FIN_WGS
    T a1 = T(0), a2 = T(0);
    int64_t j = 64 * (int64_t)w + lane;
    for (; j + 15 * (int64_t)MIK_FIN_THREADS < m; j += 16 * (int64_t)MIK_FIN_THREADS) {
        T v[16], z[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) { v[q] = S1[j + q * (int64_t)MIK_FIN_THREADS]; z[q] = S2[j + q * (int64_t)MIK_FIN_THREADS]; }
#pragma unroll
        for (int q = 0; q < 16; ++q) { a1 = a1 + v[q]; a2 = a2 + z[q]; }
    }
    for (; j < m; j += MIK_FIN_THREADS) { a1 = a1 + S1[j]; a2 = a2 + S2[j]; }
    a1 = wave_tree(a1);
    a2 = wave_tree(a2);
    bool last = false;
    if (lane == 0) {
        __hip_atomic_store(&fs->ws[w], a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&fs->ws2[w], a2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned tk = __hip_atomic_fetch_add(&fs->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tk == (unsigned)gridDim.x - 1u) {
            T t = __hip_atomic_load(&fs->ws[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            T z = __hip_atomic_load(&fs->ws2[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int q = 1; q < MIK_FIN_WGS; ++q) {
                t = t + __hip_atomic_load(&fs->ws[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                z = z + __hip_atomic_load(&fs->ws2[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(&fs->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tot1 = t; tot2 = z;
            last = true;
        }
    }
    return last;
}

// after norm(r) of cg_iterator! (src/cg.jl:140-152), for all four initialising kernels.  x_pending is NOT touched: the device struct
// of a single-GPU iterable comes straight from hipMalloc, so k_cg_fin_init / k_cg_set_init clear the flag themselves; a
// row-partitioned one is zeroed at creation and may be initialised again after a batch whose head ran ahead over RCCL, where
// only a tail clears the flag -- k_cgd_fin_init / k_cgd_fix_init have always left it as it is, and still do.
template <typename T> __device__ __forceinline__ void cg_init_scalars(CgDev<T> *d, T tot, T res, T reltol, T abstol, long long maxiter)
{
    const T a = reltol * res;
    d->rr = tot;
    d->res = res;
    d->prev_res = T(1);                       // one(residual)      :146
    d->rho = T(1);                            // one(eltype(x))     :151
    d->tol = a > abstol ? a : abstol;         // :141
    d->beta = (res * res) / (T(1) * T(1));    // what the first iterate() will use (:50)
    d->alpha = T(0);
    d->dot_uc = T(0);
    d->done = (0 >= maxiter || res <= d->tol) ? 1 : 0;
    d->nhist = 0;
}

template <typename T>
__global__ __launch_bounds__(MIK_FIN_THREADS) void k_cg_fin_init(const T *__restrict__ S, int64_t m, CgDev<T> *d, T reltol, T abstol,
                                                                 long long maxiter)
{
    __shared__ T lds16[16];
    T tot = level2_sum(S, m, lds16);
    if (threadIdx.x == 0) { cg_init_scalars(d, tot, mik_sqrt(tot), reltol, abstol, maxiter); d->x_pending = 0; }   // the host re-does this if tot is out of range
}

// the same with a residual norm the host obtained through the scaled pass (mik_safe_norm_slow)
template <typename T> __global__ void k_cg_set_init(CgDev<T> *d, T res, T reltol, T abstol, long long maxiter)
{
    cg_init_scalars(d, res * res, res, reltol, abstol, maxiter);
    d->x_pending = 0;
}

// alpha = residual^2 / dot(u, c) (src/cg.jl:55) or rho / dot(u, c) (:90)
template <typename T>
__global__ __launch_bounds__(64) void k_cg_fin_alpha(const T *__restrict__ S, int64_t m, CgDev<T> *d, int pcg, FinScratch<T> *fs)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) d->x_pending = 0;      // the sweep over u before this launch applied it (OpXpbyX)
    if (d->done) return;
    T tot;
    if (level2_sum_spread(S, m, fs, tot)) {
        d->dot_uc = tot;
        const T num = pcg ? d->rho : d->res * d->res;
        d->alpha = num / tot;
    }
}

// rho = dot(c, r); beta = rho / rho_prev (src/cg.jl:81-85)
template <typename T>
__global__ __launch_bounds__(64) void k_cg_fin_rho(const T *__restrict__ S, int64_t m, CgDev<T> *d, FinScratch<T> *fs)
{
    if (d->done) return;
    T tot;
    if (level2_sum_spread(S, m, fs, tot)) {
        const T rho_prev = d->rho;
        d->rho = tot;
        d->beta = tot / rho_prev;
    }
}

// residual = norm(r) (src/cg.jl:61-62 / :96), history, and the stopping test of :36 for the NEXT
// iterate() call (iteration index `it_next`)
template <typename T>
__device__ __forceinline__ void cg_res_scalars(CgDev<T> *d, T tot, T res, T *__restrict__ hist, long long it_next, long long maxiter,
                                               CgMirror *mirror, unsigned long long seq, int hist_index, int pcg_fused = 0)
{
    const T prev = d->res;
    d->rr = tot;
    d->prev_res = prev;
    d->res = res;
    d->beta = pcg_fused ? d->beta_rho : (res * res) / (prev * prev);    // :50 of the next step (PCG: rho / rho_prev, :85)
    hist[hist_index] = res;                   // step `hist_index` of this host call (the host zeroes mirror->nhist)
    const int dn = (it_next >= maxiter || res <= d->tol) ? 1 : 0;
    if (dn) d->done = 1;
    mirror->res = (double)res;
    mirror->prev_res = (double)prev;
    mirror->done = dn;
    mirror->nhist = hist_index + 1;
    __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename T>
__global__ __launch_bounds__(64) void k_cg_fin_res(const T *__restrict__ S, int64_t m, CgDev<T> *d, T *__restrict__ hist,
                                                    long long it_next, long long maxiter, CgMirror *mirror,
                                                    unsigned long long seq, int hist_index, FinScratch<T> *fs, int fuse_x)
{
    if (d->done) {
        // a no-op step (the stopping test fired earlier in this batch): still publish, state unchanged
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    T tot;
    if (level2_sum_spread(S, m, fs, tot)) {
        if (fuse_x) d->x_pending = 1;          // r of this step is final; its x .+= alpha .* u rides on the next sweep over u
        if (!mik_nrm_in_range(tot)) {
            // |r|^2 underflowed / overflowed (or r is exactly zero): x and r of this step are final, its norm is not.
            // Freeze the batch (later steps become no-ops) and let the host finish the step with the scaled norm.
            d->done = 1;
            mirror->done = 0;
            mirror->nhist = hist_index;
            mirror->range = 1;
            __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        cg_res_scalars(d, tot, mik_sqrt(tot), hist, it_next, maxiter, mirror, seq, hist_index);
    }
}

// closes a step whose residual norm the host computed through the scaled pass
template <typename T>
__global__ void k_cg_fix_res(CgDev<T> *d, T res, T *__restrict__ hist, long long it_next, long long maxiter, CgMirror *mirror,
                             unsigned long long seq, int hist_index, int pcg_fused = 0)
{
    d->done = 0;
    mirror->range = 0;
    cg_res_scalars(d, res * res, res, hist, it_next, maxiter, mirror, seq, hist_index, pcg_fused);
}

// the tail finaliser of the fused PCG step: residual = norm(r) as k_cg_fin_res, and rho = dot(Pl \\ r, r), beta = rho / rho_prev of
// the NEXT step (src/cg.jl:81-85) from the second reduction of the same sweep
template <typename T>
__global__ __launch_bounds__(64) void k_cg_fin_res2(const T *__restrict__ S1, const T *__restrict__ S2, int64_t m, CgDev<T> *d, T *__restrict__ hist,
                                                     long long it_next, long long maxiter, CgMirror *mirror, unsigned long long seq, int hist_index,
                                                     FinScratch2<T> *fs)
{
    if (d->done) {
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    T tot, tot2;
    if (level2_sum_spread2(S1, S2, m, fs, tot, tot2)) {
        d->x_pending = 1;                      // r of this step is final; its x .+= alpha .* u rides on the next sweep over u
        const T rho_prev = d->rho;
        d->rho = tot2;
        d->beta_rho = tot2 / rho_prev;
        if (!mik_nrm_in_range(tot)) {          // as k_cg_fin_res: freeze the batch, the host finishes the step with the scaled norm
            d->done = 1;
            mirror->done = 0;
            mirror->nhist = hist_index;
            mirror->range = 1;
            __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
        cg_res_scalars(d, tot, mik_sqrt(tot), hist, it_next, maxiter, mirror, seq, hist_index, 1);
    }
}

static int cg_profile_collect(mik_cg *it)
{
    // called after the host has seen the last tail of a call: every bracketed launch has finished except those of a head
    // enqueued ahead, whose events stay in the list until the next call (or a flush) finds them complete
    size_t i = 0;
    for (; i + 1 < it->ev_used; i += 2) {
        if (hipEventQuery(it->ev[i + 1]) != hipSuccess) { (void)hipGetLastError(); break; }
        float ms = 0.f;
        const int kind = it->ev_kind[i / 2];
        if (hipEventElapsedTime(&ms, it->ev[i], it->ev[i + 1]) == hipSuccess) { it->kern_ms[kind] += ms; it->kern_launches[kind] += 1; }
    }
    size_t keep = 0;
    for (size_t j = i; j + 1 < it->ev_used; j += 2, keep += 2) {
        std::swap(it->ev[keep], it->ev[j]);
        std::swap(it->ev[keep + 1], it->ev[j + 1]);
        it->ev_kind[keep / 2] = it->ev_kind[j / 2];
    }
    it->ev_used = keep;
    return MIK_OK;
}

static void cg_profile_flush(mik_cg *it)
{
    if (!it->ev_used) return;
    (void)hipStreamSynchronize(it->ctx->stream);
    (void)cg_profile_collect(it);
}

// HIP events on the ctx stream around one launch of the step (kind: 0 = SpMV, 1 = xpby, 2 = update)
struct CgProfileScope {
    mik_cg *it; bool on;
    CgProfileScope(mik_cg *it_, int kind) : it(it_), on(it_->profile == 2 || (it_->profile == 1 && kind == 0))
    {
        if (!on) return;
        if (it->ev_used + 2 > it->ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            it->ev.push_back(a); it->ev.push_back(b);
            it->ev_kind.push_back(0);
        }
        it->ev_kind[it->ev_used / 2] = kind;
        (void)hipEventRecord(it->ev[it->ev_used], it->ctx->stream);
    }
    ~CgProfileScope()
    {
        if (!on) return;
        (void)hipEventRecord(it->ev[it->ev_used + 1], it->ctx->stream);
        it->ev_used += 2;
    }
};

// Cache hints of the two vector kernels of a CG step (results unchanged).  x is touched once per iteration, c
// and u are dead / about to be overwritten after the update, and r has just been read for the last time in
// u .= r .+ beta .* u: streaming them past L2 (non-temporal) leaves the cache to the operator's gather and
// took the in-loop SpMV from 322 to 307 us and the step from 546 to 507 us at 256^3.
// bits 0-2: xpby {r load, u load, u store}; bits 3-7: update {x, c load, u load, r load, r store}.
// Masks (found by sweeps of single-bit flips inside the CG loop at 256^3 in round 2): 57 for the classic step; 248 when x .+= alpha .* u rides on the next sweep over u (OpXpbyX /
// OpCgUpdateR: bit 3 = x of that sweep): x, c and both directions of r in the update streamed, r read with the default policy by
// the sweep that follows.  With k_spmv_sdiab2 the r STORE is the bit that matters: streamed, it leaves the Infinity Cache to
// what the SpMV reads (in-loop SpMV 62 -> 48 us = its back-to-back time; 121 -> 249: 4,330 -> 4,520 it/s), and r then read
// cached rather than streamed takes 8 us off the update that wrote it (249 -> 248: 4,720 it/s).
// (With an operator whose SpMV itself streams gigabytes -- CSR, per-row values -- the earlier mask 121 stays: 248 cost the CSR
// loop 10 us per step.)
static inline int cg_stream_hints(const mik_ctx *ctx, bool fused_x = false, const mik_csr *A = nullptr)
{
    (void)ctx;
    return fused_x ? (mik_spmv_is_light(A) ? 248 : 121) : 57;
}

// ---- the vector sweeps of a step, each written once: the single-GPU head / tail below and the phases of the row-partitioned
// iterable (cgd_phase_impl) call them.  `vec`: every vector the sweep touches is 16-byte aligned at its first row.

// hints of the sweep over u when it reads r (cg_stream_hints: bit 3 = the x that rides on it)
static inline int cg_sweep_u_hints(const mik_cg *it) { return it->fuse_x ? cg_stream_hints(it->ctx, true, it->A) & 15 : cg_stream_hints(it->ctx) & 7; }

// u .= src .+ beta .* u on rows [lo, lo + len) (src/cg.jl:50-51; :86 with src = c = Pl \ r), and with fuse_x the pending
// x .+= alpha .* u of the previous step on the u this sweep reads anyway (OpXpbyX)
template <typename T> static int cg_sweep_u(mik_cg *it, const T *src, int64_t lo, int64_t len, bool vec, int hints)
{
    CgDev<T> *d = (CgDev<T> *)it->dev;
    T *x = (T *)it->x, *u = (T *)it->u;
    if (it->fuse_x) {
        OpXpbyX<T> op{src + lo, u + lo, x + lo, coef_ptr<T>(&d->beta), coef_ptr<T>(&d->alpha), &d->done, &d->x_pending, hints};
        return launch_map<T>(it->ctx, len, op, vec, (T *)nullptr, (const int *)nullptr);
    }
    OpXpby<T> op{src + lo, u + lo, coef_ptr<T>(&d->beta), hints};
    return launch_map<T>(it->ctx, len, op, vec, (T *)nullptr, &d->done);
}

// x .+= alpha .* u (left to the next sweep over u with fuse_x); r .-= alpha .* c; local |r|^2 -> seg_vec      src/cg.jl:58-62
// alpha: the stored scalar (coef_ptr) or, with fuse_x only, formed by the sweep from the ranks' dot(u, c) (CoefAlphaRanks)
template <typename T, typename C> static int cg_update_xr(mik_cg *it, C alpha, bool vec)
{
    CgDev<T> *d = (CgDev<T> *)it->dev;
    T *x = (T *)it->x, *u = (T *)it->u, *r = (T *)it->r, *c = (T *)it->c;
    if (it->fuse_x) {
        OpCgUpdateR<T, C> up{r, c, alpha, cg_stream_hints(it->ctx, true, it->A) >> 3};
        return launch_map<T>(it->ctx, it->n, up, vec, (T *)it->seg_vec, &d->done);
    }
    if constexpr (std::is_same<C, Coef<T>>::value) {
        OpCgUpdate<T> up{x, r, u, c, alpha, cg_stream_hints(it->ctx) >> 3};
        return launch_map<T>(it->ctx, it->n, up, vec, (T *)it->seg_vec, &d->done);
    }
    return mik_fail(it->ctx, MIK_ERR_INVALID, "cg: alpha formed inside the sweep needs the x update on the next sweep over u");
}

template <typename T> __global__ void k_cg_clear_pending(CgDev<T> *d) { d->x_pending = 0; }

// the x .+= alpha .* u that is still due when no sweep over u follows
template <typename T> static int cg_flush_x(mik_cg *it)
{
    mik_ctx *ctx = it->ctx;
    CgDev<T> *d = (CgDev<T> *)it->dev;
    T *x = (T *)it->x, *u = (T *)it->u;
    OpXFlush<T> op{u, x, coef_ptr<T>(&d->alpha), &d->x_pending};
    MIK_TRY((launch_map<T>(ctx, it->n, op, mik_aligned16(x) && mik_aligned16(u), (T *)nullptr, (const int *)nullptr)));
    hipLaunchKernelGGL((k_cg_clear_pending<T>), dim3(1), dim3(1), 0, ctx->stream, d);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// r = b - A x0 with the local |r|^2 -> seg_vec (src/cg.jl:130-138); x0 = the vector the operator is applied to, NULL: x is zero, r = b
template <typename T> static int cg_init_residual(mik_cg *it, const T *x0, bool vec)
{
    mik_ctx *ctx = it->ctx;
    T *c = (T *)it->c;
    it->mv_products = x0 ? 1 : 0;                                         // :134 / :136
    if (x0) {
        if (it->A) MIK_TRY(mik_spmv_launch<T>(ctx, it->A, x0, c, false, nullptr, nullptr));   // :137
        else if (it->op_mul(it->op_user, x0, c) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "cg: the operator callback failed");
    }
    OpSubNrm<T> op{(const T *)it->b, x0 ? c : nullptr, (T *)it->r};       // copyto!(r, b) :130, r = b - c :138
    return launch_map<T>(ctx, it->n, op, vec, (T *)it->seg_vec, nullptr);
}

// The HEAD of one iterate() (u = r + beta u [after c = Pl \ r, rho]; c = A u; alpha); cg_enqueue_tail is the other half
// (cg_run_batch, csrc/mik_iter.h).  Behind a stop its kernels early-exit on the device's `done` flag.
template <typename T> static int cg_enqueue_head(mik_cg *it)
{
    mik_ctx *ctx = it->ctx;
    CgDev<T> *d = (CgDev<T> *)it->dev;
    const int *done = &d->done;
    const int64_t n = it->n, nseg = mik_nseg<T>(n);
    T *x = (T *)it->x, *u = (T *)it->u, *r = (T *)it->r, *c = (T *)it->c;
    const bool vec = mik_aligned16(x) && mik_aligned16(u) && mik_aligned16(r) && mik_aligned16(c) && (!it->diag || mik_aligned16(it->diag));
    const int pcg = (it->diag || it->pl_fn) ? 1 : 0;
    if (it->pcg_fused) {
        // c = Pl \ r and rho = dot(c, r) (src/cg.jl:79-85) came with the previous tail (cg init for the first step): nothing to do here
    } else if (it->diag) {
        // c = Pl \ r; rho = dot(c, r)                                   src/cg.jl:79-82
        OpJacobiDot<T> pj{r, (const T *)it->diag, c, cg_stream_hints(ctx) != 0};
        MIK_TRY((launch_map<T>(ctx, n, pj, vec, (T *)it->seg_vec, done)));
    } else if (it->pl_fn) {
        // any Pl: ldiv!(c, Pl, r) through the callback, then the dot as its own sweep
        if (it->pl_fn(it->pl_user, c, r) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "cg: the preconditioner callback failed");
        OpDot<T> dcr{c, r};
        MIK_TRY((launch_map<T>(ctx, n, dcr, vec, (T *)it->seg_vec, done)));
    }
    if (pcg && !it->pcg_fused) {
        hipLaunchKernelGGL((k_cg_fin_rho<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)it->seg_vec, nseg, d, (FinScratch<T> *)it->fin);
        MIK_LAUNCH_CHECK(ctx);
    }
    {   // u .= r .+ beta .* u (src/cg.jl:50-51); PCG: u .= c .+ beta .* u (:86), and c = Pl \\ r is dead after this sweep: streamed
        CgProfileScope ps(it, 1);
        const int pcg_hints = it->fuse_x ? (cg_stream_hints(ctx, true, it->A) & 8) | 1 : cg_stream_hints(ctx) & 1;
        MIK_TRY(cg_sweep_u<T>(it, pcg ? c : r, 0, n, vec, pcg ? pcg_hints : cg_sweep_u_hints(it)));
    }
    // c = A * u with the dot(u, c) epilogue                             src/cg.jl:54-55
    if (it->A) {
        CgProfileScope ps(it, 0);
        MIK_TRY(mik_spmv_launch<T>(ctx, it->A, u, c, true, (T *)it->seg_spmv, done));
    } else {
        // any operator: mul!(c, A, u) through the callback; dot(u, c) as its own sweep with the vector tree shape
        if (it->op_mul(it->op_user, u, c) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "cg: the operator callback failed");
        OpDot<T> duc{u, c};
        MIK_TRY((launch_map<T>(ctx, n, duc, vec, (T *)it->seg_vec, done)));
    }
    hipLaunchKernelGGL((k_cg_fin_alpha<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)(it->A ? it->seg_spmv : it->seg_vec), it->A ? mik_spmv_nwg(n) : nseg,
                       d, pcg, (FinScratch<T> *)it->fin);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

template <typename T> static int cg_enqueue_tail(mik_cg *it, long long it_next, int hist_index)
{
    mik_ctx *ctx = it->ctx;
    CgDev<T> *d = (CgDev<T> *)it->dev;
    const int *done = &d->done;
    const int64_t n = it->n, nseg = mik_nseg<T>(n);
    T *x = (T *)it->x, *u = (T *)it->u, *r = (T *)it->r, *c = (T *)it->c;
    const bool vec = mik_aligned16(x) && mik_aligned16(u) && mik_aligned16(r) && mik_aligned16(c) && (!it->diag || mik_aligned16(it->diag));
    // x .+= alpha .* u; r .-= alpha .* c; norm(r)                       src/cg.jl:58-62
    if (it->pcg_fused) {
        {
            CgProfileScope ps(it, 2);
            // r is not read again before the next tail (the head reads c = Pl \\ r, u, x): both directions streamedherwise.
            // c too (bits 5, 6; round 4): c = Pl \\ r stored with the default policy shares the 256 MB Infinity Cache with the u the head writes for the SpMV --
            // streamed, the in-loop SpMV runs at its back-to-back time (73 -> 52 us) and this sweep pays most of it back (99 -> 116 us): 280.7 -> 275.6 us
            // per step, ten words per row + the operator at the copy ceiling (profiles/r04_pcg_kernel_stats.txt).
            OpPcgUpdateR<T> up{r, c, (const T *)it->diag, coef_ptr<T>(&d->alpha), 120};
            MIK_TRY((launch_map2<T>(ctx, n, up, vec, (T *)it->seg_vec, (T *)it->seg_vec2, done)));
        }
        it->seq += 1;
        hipLaunchKernelGGL((k_cg_fin_res2<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)it->seg_vec, (const T *)it->seg_vec2, nseg, d, (T *)it->hist,
                           it_next, (long long)it->maxiter, it->mirror, it->seq, hist_index, (FinScratch2<T> *)((unsigned char *)it->fin + 512));
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    {
        CgProfileScope ps(it, 2);
        MIK_TRY(cg_update_xr<T>(it, coef_ptr<T>(&d->alpha), vec));
    }
    it->seq += 1;
    hipLaunchKernelGGL((k_cg_fin_res<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)it->seg_vec, nseg, d, (T *)it->hist,
                       it_next, (long long)it->maxiter, it->mirror, it->seq, hist_index, (FinScratch<T> *)it->fin, it->fuse_x ? 1 : 0);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

// Wait until the device has published step `seq` in the host-mapped mirror (bounded spin).
int cg_wait_mirror(mik_cg *it)
{
    return mik_wait_seq(it->ctx, &it->mirror->seq, it->seq, "cg", "step", "a step");
}

template <typename T> static int cg_fetch_state(mik_cg *it, CgDev<T> *host)
{
    mik_ctx *ctx = it->ctx;
    MIK_HIP(ctx, hipMemcpyAsync(ctx->coef_host, it->dev, sizeof(CgDev<T>), hipMemcpyDeviceToHost, ctx->stream));
    MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(host, ctx->coef_host, sizeof(CgDev<T>));
    return MIK_OK;
}

template <typename T>
static int cg_init_impl(mik_cg *it, double abstol, double reltol, int initially_zero)
{
    mik_ctx *ctx = it->ctx;
    const int64_t n = it->n, nseg = mik_nseg<T>(n);
    T *u = (T *)it->u, *r = (T *)it->r, *c = (T *)it->c;
    OpFill<T> z{u, T(0)};                                                 // u .= 0          :129
    MIK_TRY((launch_map<T>(ctx, n, z, mik_aligned16(u), (T *)nullptr, nullptr)));
    const bool vec = mik_aligned16(r) && mik_aligned16(it->b) && mik_aligned16(c);
    MIK_TRY(cg_init_residual<T>(it, initially_zero ? nullptr : (const T *)it->x, vec));
    hipLaunchKernelGGL((k_cg_fin_init<T>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)it->seg_vec, nseg,
                       (CgDev<T> *)it->dev, (T)reltol, (T)abstol, (long long)it->maxiter);
    MIK_LAUNCH_CHECK(ctx);
    CgDev<T> h;
    MIK_TRY(cg_fetch_state<T>(it, &h));
    if (!mik_nrm_in_range(h.rr)) {
        // badly scaled system (or r = 0): the over-/underflow-safe norm, then the same scalar set-up
        T res;
        MIK_TRY(mik_safe_norm_slow<T>(ctx, n, r, &res));
        hipLaunchKernelGGL((k_cg_set_init<T>), dim3(1), dim3(1), 0, ctx->stream, (CgDev<T> *)it->dev, res, (T)reltol, (T)abstol, (long long)it->maxiter);
        MIK_LAUNCH_CHECK(ctx);
        MIK_TRY(cg_fetch_state<T>(it, &h));
    }
    it->residual = (double)h.res;
    it->prev_residual = (double)h.prev_res;
    it->tol = (double)h.tol;
    it->dev_done = h.done != 0;
    if (it->pcg_fused) {
        // rho of the FIRST step (src/cg.jl:79-85 with rho_prev = one): later steps get theirs from the tail of the step before
        OpJacobiDot<T> pj{r, (const T *)it->diag, c, 0};
        MIK_TRY((launch_map<T>(ctx, n, pj, vec && mik_aligned16(it->diag), (T *)it->seg_vec, (const int *)nullptr)));
        hipLaunchKernelGGL((k_cg_fin_rho<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)it->seg_vec, nseg, (CgDev<T> *)it->dev, (FinScratch<T> *)it->fin);
        MIK_LAUNCH_CHECK(ctx);
    }
    return MIK_OK;
}

static int cg_create_common(mik_ctx *ctx, const mik_csr *A, int dtype, int64_t n, mik_mul_fn op_mul, void *op_user, const void *jacobi_diag,
                            mik_ldiv_fn pl_fn, void *pl_user, void *x, const void *b, void *u, void *r, void *c, double abstol, double reltol,
                            int64_t maxiter, int initially_zero, mik_cg **out)
{
    MIK_REFUSE_COMPLEX(ctx, A, "mik_cg_create");
    if (n && (!x || !b || !u || !r || !c)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cg_create: NULL vector");
    mik_cg *it = new (std::nothrow) mik_cg();
    if (!it) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_cg_create: host allocation failed");
    it->ctx = ctx; it->A = A; it->dtype = dtype; it->n = n;
    it->op_mul = op_mul; it->op_user = op_user; it->pl_fn = pl_fn; it->pl_user = pl_user;
    it->x = x; it->b = b; it->u = u; it->r = r; it->c = c; it->diag = jacobi_diag;
    it->maxiter = maxiter;
    it->fuse_x = A != nullptr && !pl_fn && (ctx->tuning[MIK_KNOB_CG_STEP] & 1) == 0;       // development knob MIK_KNOB_CG_STEP bit 0: x updated by the step's own sweep
    it->pcg_fused = it->fuse_x && jacobi_diag != nullptr && (ctx->tuning[MIK_KNOB_CG_STEP] & 2) == 0;   // bit 1: the three-sweep PCG step
    const size_t es = mik_dtype_size(dtype);
    const int64_t nseg = dtype == MIK_F64 ? mik_nseg<double>(n) : mik_nseg<float>(n);
    const int64_t nb = mik_spmv_nwg(n);
    hipError_t e;
    (void)hipSetDevice(ctx->device);
    if ((e = hipMalloc(&it->dev, 256)) != hipSuccess || (e = hipMalloc(&it->fin, 1024)) != hipSuccess ||       // [0, 512): FinScratch; [512, 1024): FinScratch2
        (e = hipMemsetAsync(it->fin, 0, 1024, ctx->stream)) != hipSuccess ||
        (it->pcg_fused && (e = hipMalloc(&it->seg_vec2, es * (size_t)std::max<int64_t>(nseg, 1))) != hipSuccess) || (e = hipMalloc(&it->seg_spmv, es * (size_t)std::max<int64_t>(nb, 1))) != hipSuccess ||
        (e = hipMalloc(&it->seg_vec, es * (size_t)std::max<int64_t>(nseg, 1))) != hipSuccess ||
        (e = hipMalloc(&it->hist, es * 64)) != hipSuccess) {
        mik_cg_destroy(it);
        return mik_fail(ctx, MIK_ERR_NOMEM, "mik_cg_create: hipMalloc: %s", hipGetErrorString(e));
    }
    it->hist_cap = 64;
    if ((e = hipHostMalloc((void **)&it->mirror, sizeof(CgMirror), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) {
        mik_cg_destroy(it);
        return mik_fail(ctx, MIK_ERR_NOMEM, "mik_cg_create: hipHostMalloc: %s", hipGetErrorString(e));
    }
    memset(it->mirror, 0, sizeof(CgMirror));
    int rc = dtype == MIK_F64 ? cg_init_impl<double>(it, abstol, reltol, initially_zero)
                              : cg_init_impl<float>(it, abstol, reltol, initially_zero);
    if (rc) { mik_cg_destroy(it); return rc; }
    *out = it;
    return MIK_OK;
}

extern "C" int mik_cg_create(mik_ctx *ctx, const mik_csr *A, void *x, const void *b, void *u, void *r, void *c,
                             const void *jacobi_diag, double abstol, double reltol, int64_t maxiter, int initially_zero,
                             mik_cg **out)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (!A || A->n_rows != A->n_cols) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_cg_create: A must be square");
    return cg_create_common(ctx, A, A->dtype, A->n_rows, nullptr, nullptr, jacobi_diag, nullptr, nullptr, x, b, u, r, c, abstol, reltol, maxiter,
                            initially_zero, out);
}

// the operator of a *_create_op call: a CSR handle or a callback
static int resolve_operator(mik_ctx *ctx, const mik_operator *A, const char *who, const mik_csr **csr, int *dtype, int64_t *n)
{
    if (!A || (!A->csr && !A->mul)) return mik_fail(ctx, MIK_ERR_INVALID, "%s: the operator needs a csr handle or a mul callback", who);
    if (A->csr) {
        if (A->csr->n_rows != A->csr->n_cols) return mik_fail(ctx, MIK_ERR_MISMATCH, "%s: A must be square", who);
        *csr = A->csr; *dtype = A->csr->dtype; *n = A->csr->n_rows;
        return MIK_OK;
    }
    if ((A->dtype != MIK_F64 && A->dtype != MIK_F32) || A->n < 0) return mik_fail(ctx, MIK_ERR_INVALID, "%s: bad dtype / size of the callback operator", who);
    *csr = nullptr; *dtype = A->dtype; *n = A->n;
    return MIK_OK;
}

extern "C" int mik_cg_create_op(mik_ctx *ctx, const mik_operator *A, const mik_precond *Pl, void *x, const void *b, void *u, void *r, void *c,
                                double abstol, double reltol, int64_t maxiter, int initially_zero, mik_cg **out)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    const mik_csr *csr = nullptr;
    int dtype = MIK_F64;
    int64_t n = 0;
    MIK_TRY(resolve_operator(ctx, A, "mik_cg_create_op", &csr, &dtype, &n));
    if (Pl && Pl->diag && Pl->ldiv) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cg_create_op: Pl has both a diagonal and a callback");
    return cg_create_common(ctx, csr, dtype, n, csr ? nullptr : A->mul, A->user, Pl ? Pl->diag : nullptr, Pl ? Pl->ldiv : nullptr,
                            Pl ? Pl->user : nullptr, x, b, u, r, c, abstol, reltol, maxiter, initially_zero, out);
}

extern "C" int mik_cg_destroy(mik_cg *it)
{
    if (!it) return MIK_OK;
    if (it->ctx) (void)hipStreamSynchronize(it->ctx->stream);
    if (it->dev) (void)hipFree(it->dev);
    if (it->fin) (void)hipFree(it->fin);
    if (it->hist) (void)hipFree(it->hist);
    if (it->seg_spmv) (void)hipFree(it->seg_spmv);
    if (it->seg_vec) (void)hipFree(it->seg_vec);
    if (it->seg_vec2) (void)hipFree(it->seg_vec2);
    for (hipEvent_t e : it->ev) (void)hipEventDestroy(e);
    if (it->mirror) (void)hipHostFree(it->mirror);
    delete it;
    return MIK_OK;
}

// The ranks of cg_run_batch (csrc/mik_iter.h) for one single-GPU iterable.
template <typename T> struct CgLocal {
    mik_cg *it;
    T res = T(0);                  // scaled_norm -> close_frozen
    mik_cg &base() { return *it; }
    int head(int64_t) { return cg_enqueue_head<T>(it); }
    int tail(int64_t iteration, int64_t j) { return cg_enqueue_tail<T>(it, (long long)(iteration + 1), (int)j); }
    int flush_x() { return cg_flush_x<T>(it); }
    int wait(CgMirror *m) { MIK_TRY(cg_wait_mirror(it)); *m = *it->mirror; return MIK_OK; }
    // nothing to do: every head clears the flag (k_cg_fin_alpha, before it looks at `done`), the one enqueued ahead included
    int clear_pending() { return MIK_OK; }
    int scaled_norm() { return mik_safe_norm_slow<T>(it->ctx, it->n, (const T *)it->r, &res); }
    int close_frozen(int64_t it_next, int hist_index)
    {
        it->seq += 1;
        hipLaunchKernelGGL((k_cg_fix_res<T>), dim3(1), dim3(1), 0, it->ctx->stream, (CgDev<T> *)it->dev, res, (T *)it->hist, (long long)it_next,
                           (long long)it->maxiter, it->mirror, it->seq, hist_index, it->pcg_fused ? 1 : 0);
        MIK_LAUNCH_CHECK(it->ctx);
        return MIK_OK;
    }
    int collect(const CgMirror &m, double *, double *, double *residuals, int64_t, int64_t *steps_done)
    {
        mik_ctx *ctx = it->ctx;
        const int64_t nd = m.nhist;
        if (nd == 1) {
            if (residuals) residuals[0] = m.res;
        } else if (nd > 1) {
            std::vector<T> tmp((size_t)nd);
            MIK_HIP(ctx, hipMemcpyAsync(tmp.data(), it->hist, sizeof(T) * (size_t)nd, hipMemcpyDeviceToHost, ctx->stream));
            MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (residuals) for (int64_t j = 0; j < nd; ++j) residuals[j] = (double)tmp[j];
        }
        if (nd > 0) {
            it->residual = m.res;
            it->prev_residual = m.prev_res;
        }
        it->dev_done = m.done != 0;
        it->mv_products += nd;
        *steps_done = nd;
        if (it->profile) cg_profile_collect(it);
        return MIK_OK;
    }
};

template <typename T>
static int cg_iterate_many_impl(mik_cg *it, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done)
{
    mik_ctx *ctx = it->ctx;
    *steps_done = 0;
    // done(it, iteration)                                               src/cg.jl:36
    if (max_steps <= 0 || iteration >= it->maxiter || it->residual <= it->tol) return MIK_OK;
    max_steps = std::min(max_steps, it->maxiter - iteration);
    if ((it->op_mul || it->pl_fn) && max_steps > 1) {
        // Host callbacks run when a step is ENQUEUED: a batch would call mul! / ldiv! for steps that the device-side stopping
        // test later turns into no-ops, and the caller may count those calls.  One host wait per step, like the reference's loop.
        int64_t total = 0;
        for (int64_t j = 0; j < max_steps; ++j) {
            int64_t nd1 = 0;
            double res1 = 0;
            MIK_TRY(cg_iterate_many_impl<T>(it, iteration + j, 1, &res1, &nd1));
            if (nd1 == 0) break;
            if (residuals) residuals[total] = res1;
            total += 1;
        }
        *steps_done = total;
        return MIK_OK;
    }
    if (max_steps > it->hist_cap) {
        MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MIK_HIP(ctx, hipFree(it->hist));
        it->hist = nullptr;
        MIK_HIP(ctx, hipMalloc(&it->hist, sizeof(T) * (size_t)max_steps));
        it->hist_cap = max_steps;
    }
    // The device is idle here (the previous call waited for its last step), so the host may reset the
    // step counter in the host-mapped mirror directly.  The stopping flag only needs clearing if a previous
    // call left it set while the host test above said "not done" (e.g. the caller restarted the count).
    it->mirror->nhist = 0;
    it->mirror->range = 0;
    if (it->dev_done) MIK_HIP(ctx, hipMemsetAsync(&((CgDev<T> *)it->dev)->done, 0, sizeof(int), ctx->stream));
    // the head of the step AFTER this call goes on the stream before the host waits (never with host callbacks, whose call
    // count the caller may observe; MIK_KNOB_NO_LOOKAHEAD: off)
    const bool ahead_ok = ctx->tuning[MIK_KNOB_NO_LOOKAHEAD] == 0 && !it->op_mul && !it->pl_fn && iteration + max_steps < it->maxiter;
    CgLocal<T> rk{it};
    return cg_run_batch(rk, iteration, max_steps, ahead_ok, residuals, steps_done);
}

extern "C" int mik_cg_iterate_many(mik_cg *it, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done)
{
    if (!it || !steps_done || iteration < 0) return MIK_ERR_INVALID;
    return it->dtype == MIK_F64 ? cg_iterate_many_impl<double>(it, iteration, max_steps, residuals, steps_done)
                                : cg_iterate_many_impl<float>(it, iteration, max_steps, residuals, steps_done);
}

extern "C" int mik_cg_iterate(mik_cg *it, int64_t iteration, double *residual, int *done)
{
    if (!it || !done) return MIK_ERR_INVALID;
    int64_t nd = 0;
    double res = 0;
    int rc = mik_cg_iterate_many(it, iteration, 1, &res, &nd);
    if (rc) return rc;
    *done = nd == 0 ? 1 : 0;
    if (residual) *residual = it->residual;
    return MIK_OK;
}

extern "C" int mik_cg_fused_x(const mik_cg *it, int *fused)
{
    if (!it || !fused) return MIK_ERR_INVALID;
    *fused = it->fuse_x ? 1 : 0;
    return MIK_OK;
}

extern "C" int mik_cg_profile(mik_cg *it, int enable, double *spmv_ms_total, int64_t *spmv_launches)
{
    if (!it) return MIK_ERR_INVALID;
    cg_profile_flush(it);
    if (spmv_ms_total) *spmv_ms_total = it->kern_ms[0];
    if (spmv_launches) *spmv_launches = it->kern_launches[0];
    if (enable >= 0) {
        it->profile = enable;
        if (enable) { for (int q = 0; q < 3; ++q) { it->kern_ms[q] = 0; it->kern_launches[q] = 0; } it->ev_used = 0; }
    }
    return MIK_OK;
}

// The same for the row-partitioned iterable: HIP events on the compute stream around every SpMV launch of its steps (one per step with
// flag-ordered halos; the interior and the boundary launch when the halo is ordered by events and an interior range is set).
extern "C" int mik_cgd_profile(mik_cgd *it, int enable, double *spmv_ms_total, int64_t *spmv_launches)
{
    if (!it) return MIK_ERR_INVALID;
    return mik_cg_profile(&it->base, enable > 1 ? 1 : enable, spmv_ms_total, spmv_launches);
}

extern "C" int mik_cg_profile_kernels(const mik_cg *it, double *ms_total, int64_t *launches)
{
    if (!it) return MIK_ERR_INVALID;
    cg_profile_flush(const_cast<mik_cg *>(it));
    for (int q = 0; q < 3; ++q) {
        if (ms_total) ms_total[q] = it->kern_ms[q];
        if (launches) launches[q] = it->kern_launches[q];
    }
    return MIK_OK;
}

extern "C" int mik_cg_state(const mik_cg *it, double *residual, double *prev_residual, double *tol, int64_t *maxiter,
                            int64_t *mv_products, int *converged)
{
    if (!it) return MIK_ERR_INVALID;
    if (residual) *residual = it->residual;
    if (prev_residual) *prev_residual = it->prev_residual;
    if (tol) *tol = it->tol;
    if (maxiter) *maxiter = it->maxiter;
    if (mv_products) *mv_products = it->mv_products;
    if (converged) *converged = it->residual <= it->tol ? 1 : 0;   // src/cg.jl:32
    return MIK_OK;
}

// =============================================================================================
// GMRESIterable
// =============================================================================================
struct mik_gmres {
    mik_ctx *ctx = nullptr;
    const mik_csr *A = nullptr;
    int dtype = MIK_F64;
    int64_t n = 0, ldv = 0;
    void *x = nullptr;
    const void *b = nullptr;
    const void *pl = nullptr, *pr = nullptr;   // diagonal left / right preconditioners (device n-vectors) or NULL = Identity()
    mik_mul_fn op_mul = nullptr;                // A as a callback (A == nullptr): mik_gmres_create_op
    void *op_user = nullptr;
    mik_ldiv_fn pl_fn = nullptr, pr_fn = nullptr;   // Pl / Pr as callbacks
    void *pl_user = nullptr, *pr_user = nullptr;
    void *V = nullptr;        // device n x (restart + 1), column-major   src/gmres.jl:13
    void *Ax = nullptr;       // device work vector                        src/gmres.jl:125
    std::vector<double> H64; std::vector<float> H32;             // (restart+1) x restart   :14
    std::vector<double> nv64; std::vector<float> nv32;           // Residual.nullvec        :27
    double current = 1, accumulator = 1, res_beta = 1;           // Residual                :24-29
    double g_beta = 1, tol = 0;
    int k = 1, restart = 0, method = MIK_MGS;
    int64_t maxiter = 0, mv_products = 0;
    bool dist = false;        // row-partitioned: SpMV input goes through part.x_ext + halo(), sums through reduce()
    mik_partition part{};
    // single-launch Modified Gram-Schmidt (k_mgs_fused): slot buffers [2][restart + 1][256] and the host-mapped mirror of (h, nrm)
    void *mgs_P = nullptr;
    int mgs_G = 1, mgs_stride = 256;  // segments per workgroup of the single-launch kernels; slots per row of mgs_P
    int mgs_res_S = 0;               // > 0: Modified Gram-Schmidt runs in the resident-w form (k_mgs_resident) with this many segments per workgroup
    int gs_timeouts = 0;             // how often a single-launch column came back timed out (mik_dev_gmres_form)
    bool fused_off = false;          // latched when the single-launch kernel's bounded spin expired once: multi-launch chains from then on
    unsigned *xl_chk = nullptr;      // device, 2 words: XCC id + 1 of the participants of the XCD-local form (k_mgs_fused XL), per parity
    bool xl_off = false;             // the XCD-local form failed once (its workgroups were not on one XCD, or a wait expired): all-XCD form from then on
    bool xl_last = false;            // the column last enqueued used the XCD-local form
    int mgs_rounds = 1;              // DGKS rounds the single-launch kernel runs before it hands back to the host loop
    MgsMirror *mgs_mirror = nullptr;          // two mirrors (bytes apart: mgs_mirror_stride), used alternately
    size_t mgs_mirror_stride = 0;
    unsigned long long mgs_seq = 0, mgs_slot_seq[2] = {0, 0};
    int mgs_parity = 0;
    int pre_k = 0, pre_slot = 0;              // Arnoldi column already enqueued ahead of the host (0 = none) and its mirror
};

template <typename T> static int gather_launch(mik_ctx *ctx, int64_t m, const int *idx, const T *x, T *out, const int *done);

// mul!(dst, A, src) on this rank's rows; with a partition, src is staged in x_ext and the halo callback
// fills its ghost tail before the local block is applied.                src/gmres.jl:245,287,293,301
template <typename T> static int gm_spmv(mik_gmres *g, const T *src, T *dst)
{
    mik_ctx *ctx = g->ctx;
    if (g->op_mul) {                                    // any operator: mul!(dst, A, src) through the callback
        if (g->op_mul(g->op_user, src, dst) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "gmres: the operator callback failed");
        return MIK_OK;
    }
    if (!g->dist) return mik_spmv_launch<T>(ctx, g->A, src, dst, false, nullptr, nullptr);
    T *ext = (T *)g->part.x_ext;
    if (src != ext && g->n > 0) MIK_HIP(ctx, hipMemcpyAsync(ext, src, sizeof(T) * (size_t)g->n, hipMemcpyDeviceToDevice, ctx->stream));
    if (g->part.n_send > 0) MIK_TRY(gather_launch<T>(ctx, g->part.n_send, g->part.send_idx, ext, (T *)g->part.send_buf, nullptr));
    if (g->part.link) MIK_TRY(plink_halo(g->part.link, g->part.send_buf, ext + g->n));     // device-driven: push, land -- no host in between
    else if (g->part.halo && g->part.halo(g->part.user) != 0) return mik_fail(ctx, MIK_ERR_CALLBACK, "gmres: halo callback failed");
    return mik_spmv_launch<T>(ctx, g->A, ext, dst, false, nullptr, nullptr);
}

// the Gram-Schmidt sums of this iterable: one GPU, or its row partition (through the callbacks or the link)
template <typename T> static GsSums<T> gm_sums(mik_gmres *g, int k, T *h) { return GsSums<T>(g->ctx, g->dist ? &g->part : nullptr, g->n, k, h); }

template <typename T> static std::vector<T> &gm_H(mik_gmres *g);
template <> std::vector<double> &gm_H<double>(mik_gmres *g) { return g->H64; }
template <> std::vector<float> &gm_H<float>(mik_gmres *g) { return g->H32; }
template <typename T> static std::vector<T> &gm_nv(mik_gmres *g);
template <> std::vector<double> &gm_nv<double>(mik_gmres *g) { return g->nv64; }
template <> std::vector<float> &gm_nv<float>(mik_gmres *g) { return g->nv32; }

// ldiv!(y, P, x) for the left (side 0) or right (side 1) preconditioner: fused diagonal sweep or the callback
template <typename T> static int gm_ldiv(mik_gmres *g, int side, T *y, const T *x)
{
    const void *diag = side ? g->pr : g->pl;
    mik_ldiv_fn fn = side ? g->pr_fn : g->pl_fn;
    if (diag) {
        OpDivide<T> dv{x, (const T *)diag, y};
        return launch_map<T>(g->ctx, g->n, dv, mik_aligned16(x) && mik_aligned16(y) && mik_aligned16(diag), (T *)nullptr, nullptr);
    }
    if (fn && fn(side ? g->pr_user : g->pl_user, y, x) != 0) return mik_fail(g->ctx, MIK_ERR_CALLBACK, "gmres: the %s preconditioner callback failed", side ? "right" : "left");
    return MIK_OK;
}
static inline bool gm_has_pl(const mik_gmres *g) { return g->pl || g->pl_fn; }
static inline bool gm_has_pr(const mik_gmres *g) { return g->pr || g->pr_fn; }

// init!(arnoldi, x, b, Pl = Identity, Ax; initially_zero) -> beta      src/gmres.jl:235-255
template <typename T> static int gmres_init_residual(mik_gmres *g, int initially_zero, T *beta_out)
{
    mik_ctx *ctx = g->ctx;
    const int64_t n = g->n;
    const int64_t nseg = mik_nseg<T>(n);
    T *V0 = (T *)g->V;
    const T *b = (const T *)g->b;
    MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)std::max<int64_t>(nseg, 1) * (size_t)(g->restart + 1)));
    const bool vec = mik_aligned16(b) && mik_aligned16(V0) && mik_aligned16(g->Ax);
    if (initially_zero) {
        OpSubNrm<T> op{b, nullptr, V0};                                   // :241
        MIK_TRY((launch_map<T>(ctx, n, op, vec, (T *)ctx->partials, nullptr)));
    } else {
        MIK_TRY(gm_spmv<T>(g, (const T *)g->x, (T *)g->Ax));              // :245
        OpSubNrm<T> op{b, (const T *)g->Ax, V0};                          // :241,246
        MIK_TRY((launch_map<T>(ctx, n, op, vec, (T *)ctx->partials, nullptr)));
    }
    if (gm_has_pl(g)) {                                                   // ldiv!(Pl, first_col)  :249
        MIK_TRY(gm_ldiv<T>(g, 0, V0, V0));
        OpDot<T> dn{V0, V0};
        MIK_TRY((launch_map<T>(ctx, n, dn, mik_aligned16(V0), (T *)ctx->partials, nullptr)));
    }
    GsSums<T> S = gm_sums<T>(g, 0, nullptr);
    MIK_TRY(S.finish(0, true));                                           // :252
    return S.close(V0, beta_out);                                         // :253 (a badly scaled residual: the scaled norm first)
}

template <typename T> static int gmres_create_impl(mik_gmres *g, double abstol, double reltol, int initially_zero)
{
    const int m = g->restart;
    gm_H<T>(g).assign((size_t)(m + 1) * (size_t)std::max(m, 1), T(0));   // :14
    gm_nv<T>(g).assign((size_t)m + 1, T(1));                             // :27
    g->mv_products = initially_zero ? 1 : 0;                             // :122 (sic)
    T beta;
    MIK_TRY(gmres_init_residual<T>(g, initially_zero, &beta));           // :126
    g->current = (double)beta;
    g->accumulator = 1.0;                                                // :258
    g->res_beta = (double)beta;                                          // :259
    const T a = (T)reltol * beta;
    const T tol = a > (T)abstol ? a : (T)abstol;                         // :129
    g->tol = (double)tol;
    g->g_beta = (double)beta;                                            // :133
    g->k = 1;
    return MIK_OK;
}

struct GmresOpArgs {          // the callback forms of A / Pl / Pr (mik_gmres_create_op); all NULL for the CSR / diagonal entry points
    int dtype = MIK_F64;
    int64_t n = 0;
    mik_mul_fn mul = nullptr; void *mul_user = nullptr;
    mik_ldiv_fn pl = nullptr; void *pl_user = nullptr;
    mik_ldiv_fn pr = nullptr; void *pr_user = nullptr;
};

static int gmres_create_common(mik_ctx *ctx, const mik_csr *A, void *x, const void *b, const void *pl_diag, const void *pr_diag,
                               double abstol, double reltol, int restart, int64_t maxiter, int initially_zero, int orth_method,
                               const mik_partition *part, mik_gmres **out, const GmresOpArgs *op = nullptr)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (!A && !(op && op->mul)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create: NULL operator");
    MIK_REFUSE_COMPLEX(ctx, A, "mik_gmres_create");
    if (A && !part && A->n_rows != A->n_cols) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_gmres_create: A must be square");
    if (part) {
        if (part->nranks < 1 || part->rank < 0 || part->rank >= part->nranks) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: bad rank %d of %d", part->rank, part->nranks);
        if (part->n_ext != A->n_cols || part->n_ext < A->n_rows) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_gmres_create_partitioned: A_loc must be n_loc x n_ext");
        if ((part->n_ext && !part->x_ext) || part->n_send < 0 || (part->n_send && (!part->send_idx || !part->send_buf)))
            return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: NULL halo buffers");
        if (part->link) {
            if (!plink_ready(part->link)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: the link is not connected (mik_plink_connect, mik_comm_mailbox_connect)");
            if (plink_ctx(part->link) != ctx) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: the link's communicator lives on another context (stream)");
            if (plink_rank(part->link) != part->rank || plink_nranks(part->link) != part->nranks)
                return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_gmres_create_partitioned: the link belongs to rank %d of %d", plink_rank(part->link), plink_nranks(part->link));
        } else if (part->nranks > 1 && (!part->reduce || !part->halo))
            return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: nranks > 1 needs the callbacks or a connected link");
    }
    if (restart < 1) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create: restart must be >= 1");
    if (orth_method != MIK_MGS && orth_method != MIK_CGS && orth_method != MIK_DGKS) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create: bad orth_method");
    const int64_t n = A ? A->n_rows : op->n;
    const int dtype = A ? A->dtype : op->dtype;
    if (n && (!x || !b)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create: NULL vector");
    if ((size_t)(2 * restart + 6) * 8 > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_gmres_create: restart %d too large", restart);
    mik_gmres *g = new (std::nothrow) mik_gmres();
    if (!g) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_gmres_create: host allocation failed");
    g->ctx = ctx; g->A = A; g->dtype = dtype; g->n = n; g->x = x; g->b = b; g->pl = pl_diag; g->pr = pr_diag;
    if (op) { g->op_mul = A ? nullptr : op->mul; g->op_user = op->mul_user; g->pl_fn = op->pl; g->pl_user = op->pl_user; g->pr_fn = op->pr; g->pr_user = op->pr_user; }
    g->restart = restart; g->maxiter = maxiter; g->method = orth_method;
    if (part) { g->dist = true; g->part = *part; }
    g->ldv = (n + 63) / 64 * 64;
    if (g->ldv == 0) g->ldv = 64;
    const size_t es = mik_dtype_size(dtype);
    hipError_t e;
    (void)hipSetDevice(ctx->device);
    if ((e = hipMalloc(&g->V, es * (size_t)g->ldv * (size_t)(restart + 1))) != hipSuccess ||
        (e = hipMalloc(&g->Ax, es * (size_t)g->ldv)) != hipSuccess) {
        mik_gmres_destroy(g);
        return mik_fail(ctx, MIK_ERR_NOMEM, "mik_gmres_create: hipMalloc of the Krylov basis (%lld x %d): %s", (long long)n, restart + 1, hipGetErrorString(e));
    }
    {
        const int64_t nseg = dtype == MIK_F64 ? mik_nseg<double>(n) : mik_nseg<float>(n);
        // single-launch Gram-Schmidt: G = 1 / 2 / 4 / 8 reduction segments per workgroup, one workgroup per compute unit at most;
        // G > 1 needs the library's own 16-byte aligned V (always the case here)
        // (a row partition: only with a device-driven link, Modified Gram-Schmidt and restart <= 62 -- the totals of a launch's passes travel
        // between the ranks through one vector slot per pass, csrc/mik_mail.h MailSumPass)
        const bool part_ok = !part || (part->link && restart <= MIK_MAIL_VEC - 2);   // (one vector mail slot per column total and the norm; DGKS: per round)
        // every workgroup of the launch waits for all the others: at most one per compute unit of THIS device (mik_resident_cap: 256 on an
        // unpartitioned MI355X, so up to 2048 segments; a 32-CU partition: up to 256), G = the smallest of 1 / 2 / 4 / 8 segments per workgroup that fits
        const int64_t cap = std::min(mik_resident_cap(ctx), 256);        // (the slot layout of k_mgs_fused / k_cgs_fused holds 256 workgroups)
        const int G = nseg <= cap ? 1 : nseg <= 2 * cap ? 2 : nseg <= 4 * cap ? 4 : 8;
        // Beyond that: Modified Gram-Schmidt in its "resident w" form (csrc/mik_mgs_res.h) -- one workgroup per compute unit keeps its part of w in
        // registers and LDS between the passes; S consecutive segments per workgroup, as long as at least 0.6 of w fits (86 segments per workgroup:
        // 22.5 M fp64 / 45 M fp32 elements on 256 CUs).  Single GPU only; MIK_KNOB_GS = 6 keeps the chains.
        const int64_t res_S = (nseg + mik_resident_cap(ctx) - 1) / mik_resident_cap(ctx);
        const bool resident = !part && orth_method == MIK_MGS && nseg > 8 * cap && res_S <= MIK_MGS_RES_MAX_S(MIK_MGS_RES_RR, MIK_MGS_RES_RL) && restart <= 254 && g->ldv % 4 == 0 && A != nullptr &&
                              ctx->tuning[MIK_KNOB_GS] != 6 && ctx->lds_per_cu >= 160 * 1024;
        if (resident) g->mgs_res_S = (int)res_S;
        if (resident || (part_ok && nseg >= 1 && nseg <= 8 * cap && restart <= 254 && (G == 1 || g->ldv % 4 == 0))) {
            g->mgs_G = resident ? 1 : G;
            g->mgs_stride = resident ? (int)((nseg + 63) / 64 * 64) : std::max<int>(256, (int)((nseg + g->mgs_G - 1) / g->mgs_G) * g->mgs_G);
            // k_cgs_fused: one more row per round (the final h values); DGKS: up to 3 rounds in the kernel
            g->mgs_rounds = orth_method == MIK_DGKS ? (ctx->tuning[MIK_KNOB_GS] == 3 ? 1 : 3) : 1;   // DGKS rounds the kernel runs before it hands back to the host loop (MIK_KNOB_GS = 3: one)
            if (part && orth_method == MIK_DGKS) g->mgs_rounds = std::max(1, std::min(g->mgs_rounds, MIK_MAIL_VEC / (restart + 1)));     // (the rounds of a launch share the 64 vector slots)
            const size_t pbytes = es * 2 * (size_t)g->mgs_rounds * (size_t)(restart + 2) * (size_t)g->mgs_stride;
            if ((e = hipMalloc(&g->mgs_P, pbytes)) != hipSuccess || (e = hipMemsetAsync(g->mgs_P, 0xFF, pbytes, ctx->stream)) != hipSuccess ||
                (e = hipMalloc((void **)&g->xl_chk, 2 * sizeof(unsigned))) != hipSuccess || (e = hipMemsetAsync(g->xl_chk, 0, 2 * sizeof(unsigned), ctx->stream)) != hipSuccess ||
                (g->mgs_mirror_stride = (sizeof(MgsMirror) + es * (size_t)(restart + 2) + 255) / 256 * 256, false) ||
                (e = hipHostMalloc((void **)&g->mgs_mirror, 2 * g->mgs_mirror_stride, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) {
                mik_gmres_destroy(g);
                return mik_fail(ctx, MIK_ERR_NOMEM, "mik_gmres_create: single-launch Gram-Schmidt buffers: %s", hipGetErrorString(e));
            }
            memset(g->mgs_mirror, 0, 2 * g->mgs_mirror_stride);
        }
    }
    if ((e = hipMemsetAsync(g->V, 0, es * (size_t)g->ldv * (size_t)(restart + 1), ctx->stream)) != hipSuccess) {   // zeros(T, n, m+1) :13
        mik_gmres_destroy(g);
        return mik_fail(ctx, MIK_ERR_HIP, "mik_gmres_create: memset: %s", hipGetErrorString(e));
    }
    int rc = dtype == MIK_F64 ? gmres_create_impl<double>(g, abstol, reltol, initially_zero)
                              : gmres_create_impl<float>(g, abstol, reltol, initially_zero);
    if (rc) { mik_gmres_destroy(g); return rc; }
    *out = g;
    return MIK_OK;
}

extern "C" int mik_gmres_create(mik_ctx *ctx, const mik_csr *A, void *x, const void *b, const void *pl_diag, const void *pr_diag,
                                double abstol, double reltol, int restart, int64_t maxiter, int initially_zero, int orth_method,
                                mik_gmres **out)
{
    return gmres_create_common(ctx, A, x, b, pl_diag, pr_diag, abstol, reltol, restart, maxiter, initially_zero, orth_method, nullptr, out);
}

extern "C" int mik_gmres_create_op(mik_ctx *ctx, const mik_operator *A, const mik_precond *Pl, const mik_precond *Pr, void *x, const void *b,
                                   double abstol, double reltol, int restart, int64_t maxiter, int initially_zero, int orth_method,
                                   mik_gmres **out)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    const mik_csr *csr = nullptr;
    GmresOpArgs op;
    MIK_TRY(resolve_operator(ctx, A, "mik_gmres_create_op", &csr, &op.dtype, &op.n));
    if ((Pl && Pl->diag && Pl->ldiv) || (Pr && Pr->diag && Pr->ldiv)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_op: a preconditioner has both a diagonal and a callback");
    if (!csr) { op.mul = A->mul; op.mul_user = A->user; }
    if (Pl) { op.pl = Pl->ldiv; op.pl_user = Pl->user; }
    if (Pr) { op.pr = Pr->ldiv; op.pr_user = Pr->user; }
    return gmres_create_common(ctx, csr, x, b, Pl ? Pl->diag : nullptr, Pr ? Pr->diag : nullptr, abstol, reltol, restart, maxiter, initially_zero,
                               orth_method, nullptr, out, &op);
}

extern "C" int mik_gmres_create_partitioned(mik_ctx *ctx, const mik_csr *A_loc, void *x, const void *b, const void *pl_diag,
                                            const void *pr_diag, double abstol, double reltol, int restart, int64_t maxiter,
                                            int initially_zero, int orth_method, const mik_partition *part, mik_gmres **out)
{
    if (!part) return mik_fail(ctx, MIK_ERR_INVALID, "mik_gmres_create_partitioned: NULL partition");
    return gmres_create_common(ctx, A_loc, x, b, pl_diag, pr_diag, abstol, reltol, restart, maxiter, initially_zero, orth_method, part, out);
}

extern "C" int mik_gmres_destroy(mik_gmres *g)
{
    if (!g) return MIK_OK;
    if (g->ctx) (void)hipStreamSynchronize(g->ctx->stream);
    if (g->mgs_P) (void)hipFree(g->mgs_P);
    if (g->xl_chk) (void)hipFree(g->xl_chk);
    if (g->mgs_mirror) (void)hipHostFree(g->mgs_mirror);
    if (g->V) (void)hipFree(g->V);
    if (g->Ax) (void)hipFree(g->Ax);
    delete g;
    return MIK_OK;
}

// expand!(arnoldi, Pl, Pr, k, Ax): V[:, k+1] = Pl \ (A * (Pr \ V[:, k]))   src/gmres.jl:285-304 (kernels only)
template <typename T> static int gm_expand(mik_gmres *g, T *vk, T *vk1)
{
    mik_ctx *ctx = g->ctx;
    if (gm_has_pr(g)) {
        // Pl \ (A * (Pr \ v)) through the work vector Ax                  :297-304
        MIK_TRY(gm_ldiv<T>(g, 1, vk1, vk));                                // ldiv!(nextV, Pr, V[:, k])  :300
        MIK_TRY(gm_spmv<T>(g, vk1, (T *)g->Ax));
        MIK_HIP(ctx, hipMemcpyAsync(vk1, g->Ax, sizeof(T) * (size_t)g->n, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        MIK_TRY(gm_spmv<T>(g, vk, vk1));                                  // V[:, k+1] = A * V[:, k]   :287
    }
    if (gm_has_pl(g)) MIK_TRY(gm_ldiv<T>(g, 0, vk1, vk1));              // ldiv!(Pl, nextV)  :294 / :303
    return MIK_OK;
}

// orthogonalize_and_normalize! as ONE launch (k_mgs_fused / k_cgs_fused: up to 8 reduction segments per workgroup, one workgroup per compute unit;
// k_mgs_resident beyond) + one poll of a host-mapped mirror, where the k + 2 launches of the chain are pure dependent-launch latency.
// Split into "enqueue" (expand! + the kernel for Arnoldi column k) and "wait" (poll + read h, nrm), so that the column
// AFTER the current one can be put on the stream before the host has seen the current result: its inputs are all on the
// device, only "did the solve just converge?" is not known yet -- then the extra column is simply never read.
static inline MgsMirror *gm_mirror(mik_gmres *g, int slot) { return (MgsMirror *)((unsigned char *)g->mgs_mirror + (size_t)slot * g->mgs_mirror_stride); }

template <typename T> static int gm_expand(mik_gmres *g, T *vk, T *vk1);

template <typename T> static int gm_fused_enqueue(mik_gmres *g, int k, int slot)
{
    mik_ctx *ctx = g->ctx;
    const int64_t n = g->n;
    const int nseg = (int)mik_nseg<T>(n), G = g->mgs_G, m = (nseg + G - 1) / G, stride = g->mgs_stride;
    T *V = (T *)g->V;
    T *vk = V + (int64_t)(k - 1) * g->ldv, *w = V + (int64_t)k * g->ldv;
    MIK_TRY(gm_expand<T>(g, vk, w));
    const bool vec = mik_aligned16(V) && mik_aligned16(w) && (g->ldv % VT<T>::W == 0);
    g->mgs_seq += 1;
    g->mgs_slot_seq[slot] = g->mgs_seq;
#define MIK_CGS_GO(VECV, DG, GG)                                                                                                               \
    do {                                                                                                                                        \
        if (g->dist) {        /* a row partition with a link: column totals and the norm are summed over the ranks inside the launch */        \
            const PlinkMail pm = plink_mail(g->part.link);                                                                                      \
            const MailSumPass xch{pm.peers, pm.P, pm.rank, plink_next_vec_tag(g->part.link), pm.ticks, pm.err};                                 \
            hipLaunchKernelGGL((k_cgs_fused<T, VECV, DG, GG, MailSumPass>), dim3(m), dim3(MIK_BLOCK), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, \
                               g->restart, stride, nseg, g->mgs_rounds, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq, xch);                    \
        } else                                                                                                                                  \
            hipLaunchKernelGGL((k_cgs_fused<T, VECV, DG, GG>), dim3(m), dim3(MIK_BLOCK), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, g->restart, \
                               stride, nseg, g->mgs_rounds, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq, NoExchange{});                       \
    } while (0)
#define MIK_MGS_GO(VECV, GG)                                                                                                                   \
    do {                                                                                                                                        \
        if (g->dist) {        /* a row partition with a link: the totals of every pass are summed over the ranks inside the launch */          \
            const PlinkMail pm = plink_mail(g->part.link);                                                                                      \
            const MailSumPass xch{pm.peers, pm.P, pm.rank, plink_next_vec_tag(g->part.link), pm.ticks, pm.err};                                 \
            hipLaunchKernelGGL((k_mgs_fused<T, VECV, GG, false, MailSumPass>), dim3(m), dim3(MIK_BLOCK), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, \
                               g->restart, stride, nseg, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq, (unsigned *)nullptr, xch);              \
        } else                                                                                                                                  \
            hipLaunchKernelGGL((k_mgs_fused<T, VECV, GG>), dim3(m), dim3(MIK_BLOCK), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, g->restart, \
                               stride, nseg, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq, (unsigned *)nullptr, NoExchange{});                 \
    } while (0)
#define MIK_GS_GO(VECV, GG)                                                                          \
    do {                                                                                             \
        if (g->method == MIK_DGKS) MIK_CGS_GO(VECV, true, GG);                                       \
        else if (g->method == MIK_CGS) MIK_CGS_GO(VECV, false, GG);                                  \
        else MIK_MGS_GO(VECV, GG);                                                                   \
    } while (0)
    if (g->mgs_res_S > 0) {
        // the resident-w form: ceil(nseg / S) workgroups of 512 threads, one per compute unit (144 KB of static LDS each)
        const int S = g->mgs_res_S, wgs = (nseg + S - 1) / S;
        hipLaunchKernelGGL((k_mgs_resident<T, 512, MIK_MGS_RES_RR, MIK_MGS_RES_RL>), dim3(wgs), dim3(512), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, g->restart,
                           stride, nseg, S, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq);
        g->xl_last = false;
        MIK_LAUNCH_CHECK(ctx);
        g->mgs_parity ^= 1;
        return MIK_OK;
    }
    // Modified Gram-Schmidt on small systems: the XCD-local form (k_mgs_fused XL) -- at most 128 workgroups, all on the first XCD, a column
    // of at most 512 KB per pass: every column then comes through ONE XCD's share of the fabric (~1 MB per us).  fe_shell (363 KB columns):
    // GMRES(50) 64.2 -> 50.9 us per inner iteration; configs[2] (1 MB columns) would lose (36.5 -> 47.8 us) and keeps the device-wide
    // form.  MIK_KNOB_GS = 4: the device-wide form at every size.
    // (the form is compiled for the 8-XCD dispatch: blockIdx % 8 == 0 -> first XCD; up to 4 workgroups on each of that XCD's compute units)
    const bool xl = g->method == MIK_MGS && G == 1 && vec && mik_xcd_maps(ctx) && m <= 4 * (mik_cus(ctx) / mik_xcds(ctx)) && ((size_t)n * sizeof(T) <= (1u << 19) || ctx->tuning[MIK_KNOB_GS] == 5) && !g->xl_off && ctx->tuning[MIK_KNOB_GS] != 4 && g->xl_chk && !g->dist;   // (MIK_KNOB_GS = 5: whatever the column size)
    g->xl_last = xl;
    if (xl) {
        hipLaunchKernelGGL((k_mgs_fused<T, true, 1, true>), dim3(8 * m), dim3(MIK_BLOCK), 0, ctx->stream, n, k, (const T *)V, g->ldv, w, (T *)g->mgs_P, g->restart,
                           stride, nseg, g->mgs_parity, gm_mirror(g, slot), g->mgs_seq, g->xl_chk, NoExchange{});
    } else
    // G > 1 (more than 256 segments) is instantiated for 16-byte aligned bases only: gmres_create allocates V that way
    if (G == 1) { if (vec) MIK_GS_GO(true, 1); else MIK_GS_GO(false, 1); }
    else if (G == 2) MIK_GS_GO(true, 2);
    else if (G == 4) MIK_GS_GO(true, 4);
    else MIK_GS_GO(true, 8);
#undef MIK_GS_GO
#undef MIK_MGS_GO
#undef MIK_CGS_GO
    MIK_LAUNCH_CHECK(ctx);
    g->mgs_parity ^= 1;
    return MIK_OK;
}

constexpr int MIK_GS_TIMEOUT = -100;      // internal: the bounded spin of the single-launch Gram-Schmidt expired

template <typename T> static int gm_fused_wait(mik_gmres *g, int k, int slot, T *h_out, T *nrm_out, bool *rescaled)
{
    mik_ctx *ctx = g->ctx;
    MgsMirror *mir = gm_mirror(g, slot);
    MIK_TRY(mik_wait_seq(ctx, &mir->seq, g->mgs_slot_seq[slot], "gmres", "the Gram-Schmidt step", "the Gram-Schmidt step"));
    if (mir->err || ctx->tuning[MIK_KNOB_GS_TIMEOUT] == 1) return MIK_GS_TIMEOUT;        // (development knob MIK_KNOB_GS_TIMEOUT: pretend it happened)
    // a workgroup gave up waiting for a slot (GPU shared with other work?): the caller redoes the column
    const T *out = reinterpret_cast<const T *>(mir + 1);
    for (int j = 0; j < k; ++j) h_out[j] = out[j];
    *nrm_out = out[k];
    *rescaled = false;
    T *w = (T *)g->V + (int64_t)k * g->ldv;
    GsSums<T> S = gm_sums<T>(g, k, h_out);      // (over a partition every rank sees the same totals: all of them take the same branch together)
    if (g->method == MIK_DGKS && mir->pad) {    // the kernel stopped before the DGKS loop ended (round limit / unsafe norm): w is unscaled
        if (*nrm_out != *nrm_out) MIK_TRY(S.scaled_norm(w, nrm_out));
        MIK_TRY(gs_dgks<T>(S, (const T *)g->V, g->ldv, w, nrm_out, out[k + 1]));
        *rescaled = true;
        return MIK_OK;
    }
    if (out[k] != out[k]) {                     // sum of squares outside the safe range: the kernel left w unscaled
        MIK_TRY(S.rescale(w, nrm_out, true));
        *rescaled = true;
    }
    return MIK_OK;
}

// iterate(g::GMRESIterable, iteration)                                   src/gmres.jl:57-106
template <typename T> static int gmres_iterate_impl(mik_gmres *g, int64_t iteration, double *residual, int *done)
{
    mik_ctx *ctx = g->ctx;
    const int m = g->restart;
    const int64_t ldh = m + 1;
    std::vector<T> &H = gm_H<T>(g);
    std::vector<T> &nullvec = gm_nv<T>(g);
    auto Hat = [&](int i, int j) -> T & { return H[(size_t)j * ldh + i]; };
    auto is_done = [&](int64_t it) { return it >= g->maxiter || (T)g->current <= (T)g->tol; };   // :55, :51

    if (is_done(iteration)) { *done = 1; if (residual) *residual = g->current; return MIK_OK; }   // :59
    *done = 0;
    int k = g->k;                                                         // 1-based, as in the reference
    T *V = (T *)g->V;
    T *vk = V + (int64_t)(k - 1) * g->ldv, *vk1 = V + (int64_t)k * g->ldv;

    // expand! (:64, :285-304), then H[k+1, k] = orthogonalize_and_normalize!(V[:, 1:k], V[:, k+1], H[1:k, k], orth_meth)  :68-73
    T nrm;
    {
        if (g->mgs_P && (!g->dist || g->part.link) && !g->fused_off && ctx->tuning[MIK_KNOB_GS] != 1 && ctx->tuning[MIK_KNOB_GS] != 2) {    // MIK_KNOB_GS: 1 / 2 = the multi-launch chains, 4 = single launch on all XCDs
            // single-launch Gram-Schmidt, one column ahead of the host: column k is on the stream already if the previous
            // call put it there; column k + 1 goes on the stream BEFORE this call waits for column k (never across a restart,
            // never with host callbacks in expand!, whose call count the caller may observe)
            const int slot = g->pre_k == k ? g->pre_slot : 0;
            if (g->pre_k != k) MIK_TRY(gm_fused_enqueue<T>(g, k, slot));
            g->pre_k = 0;
            const bool ahead = k < m && iteration + 1 < g->maxiter && !g->op_mul && !g->pl_fn && !g->pr_fn && ctx->tuning[MIK_KNOB_NO_LOOKAHEAD] == 0;
            if (ahead) MIK_TRY(gm_fused_enqueue<T>(g, k + 1, slot ^ 1));
            bool rescaled = false;
            const int rcw = gm_fused_wait<T>(g, k, slot, &Hat(0, k - 1), &nrm, &rescaled);
            if (rcw == MIK_GS_TIMEOUT && g->dist)      // (no local fall-back over a partition: the ranks' exchange sequences would part ways)
                return mik_fail(ctx, MIK_ERR_HIP, "gmres (row-partitioned): a hand-off of the single-launch Gram-Schmidt timed out (a peer rank stopped, or the GPU is shared with other work)");
            if (rcw == MIK_GS_TIMEOUT) {
                g->gs_timeouts += 1;
                // The hand-off needs every workgroup resident; a GPU shared with other streams or processes can break that.
                // Not an error of the solve: drain the stream (a column enqueued ahead drains with it), switch this handle to the
                // multi-launch chains for good, and redo column k from V[:, k - 1], which the kernel never writes.
                MIK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                gm_mirror(g, 0)->err = 0;
                gm_mirror(g, 1)->err = 0;
                if (g->xl_last && !g->xl_off) g->xl_off = true;       // the XCD-local form: back to the all-XCD single launch, not to the chains
                else g->fused_off = true;
                g->pre_k = 0;
                MIK_TRY(gm_expand<T>(g, vk, vk1));
                MIK_TRY(gs_orthogonalize<T>(gm_sums<T>(g, k, &Hat(0, k - 1)), V, g->ldv, vk1, &nrm, g->method));
            } else {
                MIK_TRY(rcw);
                if (ahead && !rescaled) { g->pre_k = k + 1; g->pre_slot = slot ^ 1; }    // rescaled: column k + 1 was built on an unscaled w
            }
        } else {
            MIK_TRY(gm_expand<T>(g, vk, vk1));
            MIK_TRY(gs_orthogonalize<T>(gm_sums<T>(g, k, &Hat(0, k - 1)), V, g->ldv, vk1, &nrm, g->method));
        }
    }
    g->mv_products += 1;                                                  // :65
    Hat(k, k - 1) = nrm;

    // update_residual!                                                   :76, :224-233
    T current = (T)g->current, accumulator = (T)g->accumulator;
    if (Hat(k, k - 1) == T(0)) {
        current = T(0);
    } else {
        T dsum = T(0);
        for (int i = 0; i < k; ++i) { T p = nullvec[i] * Hat(i, k - 1); dsum = dsum + p; }
        nullvec[k] = -(dsum / Hat(k, k - 1));
        T sq = nullvec[k] * nullvec[k];
        accumulator = accumulator + sq;
        current = (T)g->res_beta / std::sqrt(accumulator);
    }
    g->current = (double)current;
    g->accumulator = (double)accumulator;

    k += 1;                                                               // :78

    if (k == m + 1 || is_done(iteration + 1)) {                           // :82
        // solve_least_squares!: rhs = [beta, 0, ...] of length k; H view = H[1:k, 1:k-1]   :85, :262-271
        std::vector<T> rhs((size_t)k, T(0));
        rhs[0] = (T)g->g_beta;
        hessenberg_ldiv<T>(H.data(), ldh, k - 1, rhs.data());
        // update_solution!: x += V[:, 1:k-1] * y                         :88, :273-276
        MIK_TRY(coef_upload<T>(ctx, 0, rhs.data(), k - 1));
        if (gm_has_pr(g)) {
            // x += Pr \ (V * y) with Ax as work space                     :278-283
            T *Ax = (T *)g->Ax;
            OpFill<T> z{Ax, T(0)};
            MIK_TRY((launch_map<T>(ctx, g->n, z, mik_aligned16(Ax), (T *)nullptr, nullptr)));
            MIK_TRY(gemv_n_dev<T>(ctx, g->n, k - 1, V, g->ldv, (const T *)ctx->coef, T(1), Ax));
            MIK_TRY(gm_ldiv<T>(g, 1, Ax, Ax));                               // ldiv!(Pr, Ax)  :281
            OpAxpy<T> ax{Ax, (T *)g->x, coef_val<T>(T(1))};
            MIK_TRY((launch_map<T>(ctx, g->n, ax, mik_aligned16(Ax) && mik_aligned16(g->x), (T *)nullptr, nullptr)));
        } else {
            MIK_TRY(gemv_n_dev<T>(ctx, g->n, k - 1, V, g->ldv, (const T *)ctx->coef, T(1), (T *)g->x));
        }
        k = 1;                                                            // :90
        g->pre_k = 0;                                                     // a column enqueued ahead belongs to the cycle that just ended
        if (!is_done(iteration)) {                                        // :93
            T beta;
            MIK_TRY(gmres_init_residual<T>(g, 0, &beta));                 // :96
            g->g_beta = (double)beta;
            g->accumulator = 1.0;                                         // :99, :258
            g->res_beta = (double)beta;                                   // :259
            g->mv_products += 1;                                          // :101
        }
    }
    g->k = k;
    if (residual) *residual = g->current;                                 // :105
    return MIK_OK;
}

extern "C" int mik_gmres_iterate(mik_gmres *g, int64_t iteration, double *residual, int *done)
{
    if (!g || !done || iteration < 0) return MIK_ERR_INVALID;
    return g->dtype == MIK_F64 ? gmres_iterate_impl<double>(g, iteration, residual, done)
                               : gmres_iterate_impl<float>(g, iteration, residual, done);
}

// Up to max_steps consecutive iterate() calls inside the library: the loop of gmres! (src/gmres.jl:207-214) without a
// trip through the host language per inner iteration (each step still waits once for its Hessenberg column).
extern "C" int mik_gmres_iterate_many(mik_gmres *g, int64_t iteration, int64_t max_steps, double *residuals, int64_t *steps_done)
{
    if (!g || !steps_done || iteration < 0) return MIK_ERR_INVALID;
    *steps_done = 0;
    for (int64_t j = 0; j < max_steps; ++j) {
        double res = 0;
        int done = 0;
        int rc = g->dtype == MIK_F64 ? gmres_iterate_impl<double>(g, iteration + j, &res, &done)
                                     : gmres_iterate_impl<float>(g, iteration + j, &res, &done);
        if (rc) return rc;
        if (done) break;
        if (residuals) residuals[j] = res;
        *steps_done = j + 1;
    }
    return MIK_OK;
}

// development introspection (include/mik_dev.h): which form the next Arnoldi column's orthogonalize_and_normalize! runs in
extern "C" int mik_dev_gmres_form(const mik_gmres *g, int *single_launch, int *segments_per_workgroup, int *xcd_local_last, int *timeouts)
{
    if (!g) return MIK_ERR_INVALID;
    const mik_ctx *ctx = g->ctx;
    const bool single = g->mgs_P && (!g->dist || g->part.link) && !g->fused_off && ctx->tuning[MIK_KNOB_GS] != 1 && ctx->tuning[MIK_KNOB_GS] != 2;
    if (single_launch) *single_launch = single ? 1 : 0;
    if (segments_per_workgroup) *segments_per_workgroup = g->mgs_P ? (g->mgs_res_S > 0 ? g->mgs_res_S : g->mgs_G) : 0;
    if (xcd_local_last) *xcd_local_last = g->xl_last ? 1 : 0;
    if (timeouts) *timeouts = g->gs_timeouts;
    return MIK_OK;
}

int mik_mgs_resident_max_s() { return MIK_MGS_RES_MAX_S(MIK_MGS_RES_RR, MIK_MGS_RES_RL); }

extern "C" int mik_dev_mgs_resident_shape(int *threads, int *register_rounds, int *lds_rounds)
{
    if (threads) *threads = 512;
    if (register_rounds) *register_rounds = MIK_MGS_RES_RR;
    if (lds_rounds) *lds_rounds = MIK_MGS_RES_RL;
    return MIK_OK;
}

extern "C" int mik_gmres_state(const mik_gmres *g, double *residual, double *tol, double *beta, int *k, int64_t *mv_products,
                               int *converged)
{
    if (!g) return MIK_ERR_INVALID;
    if (residual) *residual = g->current;
    if (tol) *tol = g->tol;
    if (beta) *beta = g->g_beta;
    if (k) *k = g->k;
    if (mv_products) *mv_products = g->mv_products;
    if (converged) *converged = g->current <= g->tol ? 1 : 0;            // src/gmres.jl:51
    return MIK_OK;
}

// =============================================================================================
// Row-partitioned CGIterable (one process per GPU)
// =============================================================================================
//
// New design (the reference is single-process): rank p owns a contiguous block of rows; the
// operator's local block is a CSR matrix whose columns are renumbered to [0, n_loc) for owned
// entries of x and [n_loc, n_loc + n_ghost) for halo entries received from the neighbours.  The
// host side (dist.py) runs the exchanges with torch.distributed (RCCL over xGMI on the GPU box,
// gloo in the CPU tests) between the phases below; every phase only enqueues kernels.
//
// The phases: mik_cgd_phase_id (include/mik.h) and, for the library's own loops only, cgd_phase_internal (csrc/mik_iter.h).
//
// Cross-rank sums run in rank order 0..P-1 on every rank, so all ranks hold bit-identical
// scalars and the history is reproducible (and equals the single-GPU path for P = 1).

template <typename T>
__global__ void k_gather(int64_t m, const int *__restrict__ idx, const T *__restrict__ x, T *__restrict__ out, const int *__restrict__ done)
{
    if (done && *done) return;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) out[i] = x[idx[i]];
}

// The rows the neighbours need, updated and packed in ONE launch (every send index occurs once): u = r + beta u (and the
// pending x update) exactly as OpXpbyX::apply does it, then the new u straight into the send buffer.
template <typename T>
__global__ __launch_bounds__(MIK_BLOCK) void k_cgd_early(int64_t m, const int *__restrict__ idx, const T *__restrict__ r, T *__restrict__ u, T *__restrict__ x,
                                                         const T *__restrict__ beta, const T *__restrict__ alpha, const int *__restrict__ done,
                                                         const int *__restrict__ pending, int fuse_x, T *__restrict__ out)
{
    const int dn = *done, pd = fuse_x ? *pending : 0;
    for (int64_t j = (int64_t)blockIdx.x * MIK_BLOCK + threadIdx.x; j < m; j += (int64_t)gridDim.x * MIK_BLOCK) {
        const int i = idx[j];
        T uo = u[i];
        if (pd) { T t = *alpha * uo; x[i] = x[i] + t; }
        if (!dn) { T t = *beta * uo; uo = r[i] + t; u[i] = uo; }
        out[j] = uo;
    }
}

template <typename T> static int gather_launch(mik_ctx *ctx, int64_t m, const int *idx, const T *x, T *out, const int *done)
{
    if (m <= 0) return MIK_OK;
    const int grid = (int)std::min<int64_t>((m + MIK_BLOCK - 1) / MIK_BLOCK, mik_max_grid(ctx));
    hipLaunchKernelGGL((k_gather<T>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, m, idx, x, out, done);
    MIK_LAUNCH_CHECK(ctx);
    return MIK_OK;
}

extern "C" int mik_gather(mik_ctx *ctx, int dtype, int64_t m, const int32_t *idx, const void *x, void *out)
{
    if (!ctx || m < 0 || (m && (!idx || !x || !out))) return MIK_ERR_INVALID;
    if (dtype == MIK_F64) return gather_launch<double>(ctx, m, idx, (const double *)x, (double *)out, nullptr);
    if (dtype == MIK_F32) return gather_launch<float>(ctx, m, idx, (const float *)x, (float *)out, nullptr);
    return MIK_ERR_INVALID;
}

// sum of the P per-rank partial sums, rank order
template <typename T> __device__ __forceinline__ T rank_sum(const T *__restrict__ all, int nranks)
{
    T s = all[0];
    for (int p = 1; p < nranks; ++p) s = s + all[p];
    return s;
}

// this rank's partial (level-2 sum of its segment sums, spread over MIK_FIN_WGS single-wave workgroups like k_cg_fin_*) into its slot
template <typename T>
__global__ __launch_bounds__(64) void k_cgd_fin_slot(const T *__restrict__ S, int64_t m, T *__restrict__ slot, const int *__restrict__ done, FinScratch<T> *fs)
{
    if (done && *done) return;
    T tot;
    if (level2_sum_spread(S, m, fs, tot)) *slot = tot;
}

// k_cgd_fin_slot for |r|^2 that also does what k_cgd_alpha did for this step (whose sweep formed alpha by itself: CoefAlphaRanks):
// the pending-x flag cleared, dot(u, c) and alpha stored for the head of the next step -- one launch less per step
template <typename T>
__global__ __launch_bounds__(64) void k_cgd_fin_slot_alpha(const T *__restrict__ S, int64_t m, T *__restrict__ slot, const int *__restrict__ done,
                                                           FinScratch<T> *fs, const T *__restrict__ dot_all, int nranks, CgDev<T> *d)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) d->x_pending = 0;     // the sweep over u of this step's head applied it (OpXpbyX)
    if (done && *done) return;
    T tot;
    if (level2_sum_spread(S, m, fs, tot)) {
        *slot = tot;
        const T dt = rank_sum(dot_all, nranks);
        d->dot_uc = dt;
        d->alpha = (d->res * d->res) / dt;
    }
}

template <typename T> __global__ void k_cgd_alpha(const T *__restrict__ dot_all, int nranks, CgDev<T> *d)
{
    d->x_pending = 0;                          // the sweep over u of this step's head applied it (OpXpbyX)
    if (d->done) return;
    const T tot = rank_sum(dot_all, nranks);
    d->dot_uc = tot;
    d->alpha = (d->res * d->res) / tot;
}

// the scalars of cg_init_scalars the host needs, into the mirror; one thread
template <typename T> __device__ __forceinline__ void cgd_publish_init(const CgDev<T> *d, CgMirror *mirror, unsigned long long seq)
{
    mirror->res = (double)d->res; mirror->prev_res = 1.0; mirror->done = d->done; mirror->nhist = 0;
    mirror->tol = (double)d->tol; mirror->tol_valid = 1;
    __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <typename T>
__global__ void k_cgd_fin_init(const T *__restrict__ rr_all, int nranks, CgDev<T> *d, T reltol, T abstol, long long maxiter, CgMirror *mirror,
                               unsigned long long seq)
{
    const T tot = rank_sum(rr_all, nranks);
    if (!mik_nrm_in_range(tot)) {
        // |r|^2 left the range of a safe sqrt(sum of squares) -- every rank sees the same total and takes this branch: the hosts
        // recompute the norm with a common scale (CGD_NORM_*) and finish the initialisation with k_cgd_fix_init
        d->done = 1; mirror->done = 0; mirror->range = 1;
        __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    cg_init_scalars(d, tot, mik_sqrt(tot), reltol, abstol, maxiter);
    cgd_publish_init(d, mirror, seq);
}

template <typename T>
__global__ void k_cgd_fin_res(const T *__restrict__ rr_all, int nranks, CgDev<T> *d, T *__restrict__ hist, long long it_next, long long maxiter,
                              CgMirror *mirror, unsigned long long seq, int hist_index, int fuse_x)
{
    if (d->done) { __hip_atomic_store(&mirror->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); return; }
    cgd_close_step<T>(d, rank_sum(rr_all, nranks), hist, it_next, maxiter, mirror, seq, hist_index, fuse_x);
}

// finishes cg_iterator! with a residual norm obtained through the scaled pass over the partition
template <typename T>
__global__ void k_cgd_fix_init(CgDev<T> *d, T res, T reltol, T abstol, long long maxiter, CgMirror *mirror, unsigned long long seq)
{
    cg_init_scalars(d, res * res, res, reltol, abstol, maxiter);
    mirror->range = 0;
    cgd_publish_init(d, mirror, seq);
}

extern "C" int mik_cgd_create(mik_ctx *ctx, const mik_csr *A_loc, void *x, const void *b, void *u_ext, void *r, void *c,
                              const int32_t *send_idx, int64_t n_send, void *send_buf, void *dot_all, void *rr_all, int rank,
                              int nranks, double abstol, double reltol, int64_t maxiter, int initially_zero, mik_cgd **out)
{
    if (!ctx || !out) return MIK_ERR_INVALID;
    *out = nullptr;
    if (!A_loc || A_loc->n_cols < A_loc->n_rows) return mik_fail(ctx, MIK_ERR_MISMATCH, "mik_cgd_create: local block must be n_loc x (n_loc + n_ghost)");
    MIK_REFUSE_COMPLEX(ctx, A_loc, "mik_cgd_create");
    if (nranks < 1 || rank < 0 || rank >= nranks || !dot_all || !rr_all || (n_send && (!send_idx || !send_buf)))
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_create: bad rank / comm buffers");
    const int64_t n = A_loc->n_rows;
    if (n && (!x || !b || !u_ext || !r || !c)) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_create: NULL vector");
    mik_cgd *it = new (std::nothrow) mik_cgd();
    if (!it) return mik_fail(ctx, MIK_ERR_NOMEM, "mik_cgd_create: host allocation failed");
    mik_cg &bs = it->base;
    bs.ctx = ctx; bs.A = A_loc; bs.dtype = A_loc->dtype; bs.n = n;
    bs.x = x; bs.b = b; bs.u = u_ext; bs.r = r; bs.c = c; bs.maxiter = maxiter;
    it->rank = rank; it->nranks = nranks; it->n_send = n_send; it->send_idx = send_idx; it->send_buf = send_buf;
    it->u_ext = u_ext; it->n_ext = A_loc->n_cols; it->dot_all = dot_all; it->rr_all = rr_all;
    it->abstol = abstol; it->reltol = reltol; it->initially_zero = initially_zero;
    const size_t es = mik_dtype_size(A_loc->dtype);
    const int64_t nseg = A_loc->dtype == MIK_F64 ? mik_nseg<double>(n) : mik_nseg<float>(n);
    const int64_t nb = mik_spmv_nwg(n);
    hipError_t e;
    (void)hipSetDevice(ctx->device);
    auto fail = [&](const char *what, hipError_t err) {
        int rc = mik_fail(ctx, MIK_ERR_NOMEM, "mik_cgd_create: %s: %s", what, hipGetErrorString(err));
        mik_cgd_destroy(it);
        return rc;
    };
    if ((e = hipMalloc(&bs.dev, 256)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&bs.seg_spmv, es * (size_t)std::max<int64_t>(nb, 1))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&bs.seg_vec, es * (size_t)std::max<int64_t>(nseg, 1))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&bs.hist, es * 1024)) != hipSuccess) return fail("hipMalloc", e);
    bs.hist_cap = 1024;
    if ((e = hipMalloc(&bs.fin, 256)) != hipSuccess || (e = hipMemsetAsync(bs.fin, 0, 256, ctx->stream)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipHostMalloc((void **)&bs.mirror, sizeof(CgMirror), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return fail("hipHostMalloc", e);
    memset(bs.mirror, 0, sizeof(CgMirror));
    if ((e = hipMemsetAsync(bs.dev, 0, 256, ctx->stream)) != hipSuccess) return fail("hipMemsetAsync", e);
    *out = it;
    return MIK_OK;
}

extern "C" int mik_cgd_set_interior(mik_cgd *it, int64_t rb_begin, int64_t rb_end)
{
    if (!it) return MIK_ERR_INVALID;
    const int64_t nb = mik_spmv_nwg(it->base.n);
    if (rb_begin < 0 || rb_end < rb_begin || rb_end > nb) return mik_fail(it->base.ctx, MIK_ERR_INVALID, "mik_cgd_set_interior: bad range");
    if (!mik_spmv_can_split(it->base.A)) return mik_fail(it->base.ctx, MIK_ERR_NOTIMPL, "mik_cgd_set_interior: the operator's layout cannot be launched over a row-block range");
    it->int_begin = rb_begin;
    it->int_end = rb_end;
    return MIK_OK;
}

void mik_cgd_group_forget(mik_cgd *it);   // mik_comm.hip

extern "C" int mik_cgd_destroy(mik_cgd *it)
{
    if (!it) return MIK_OK;
    mik_cgd_group_forget(it);
    mik_cg &bs = it->base;
    if (bs.ctx) (void)hipStreamSynchronize(bs.ctx->stream);
    if (it->link) { (void)mik_plink_destroy(it->link); it->link = nullptr; }
    if (bs.dev) (void)hipFree(bs.dev);
    if (bs.hist) (void)hipFree(bs.hist);
    if (bs.fin) (void)hipFree(bs.fin);
    if (bs.seg_spmv) (void)hipFree(bs.seg_spmv);
    if (bs.seg_vec) (void)hipFree(bs.seg_vec);
    if (bs.mirror) (void)hipHostFree(bs.mirror);
    delete it;
    return MIK_OK;
}

template <typename T> static int cgd_phase_impl(mik_cgd *it, int phase, int64_t iteration)
{
    mik_cg &bs = it->base;
    mik_ctx *ctx = bs.ctx;
    CgDev<T> *d = (CgDev<T> *)bs.dev;
    const int *done = &d->done;
    const int64_t n = bs.n, nseg = mik_nseg<T>(n), nb = mik_spmv_nwg(n);
    T *x = (T *)bs.x, *u = (T *)it->u_ext, *r = (T *)bs.r, *c = (T *)bs.c;
    T *dot_slot = (T *)it->dot_all + it->rank, *rr_slot = (T *)it->rr_all + it->rank;
    const bool vec = mik_aligned16(x) && mik_aligned16(u) && mik_aligned16(r) && mik_aligned16(c) && mik_aligned16(bs.b);
    switch (phase) {
    case MIK_CGD_INIT_A:
        if (!it->initially_zero) {
            MIK_HIP(ctx, hipMemcpyAsync(u, x, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
            MIK_TRY(gather_launch<T>(ctx, it->n_send, it->send_idx, u, (T *)it->send_buf, nullptr));
        }
        return MIK_OK;
    case MIK_CGD_INIT_B: {
        MIK_TRY(cg_init_residual<T>(&bs, it->initially_zero ? nullptr : u, vec));       // x (with its halo) is in u_ext
        hipLaunchKernelGGL((k_finalize_store<T>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)bs.seg_vec, nseg, (int64_t)0, rr_slot,
                           (const int *)nullptr);
        MIK_LAUNCH_CHECK(ctx);
        OpFill<T> z{u, T(0)};   // u .= 0 (src/cg.jl:129), halo included
        return launch_map<T>(ctx, it->n_ext, z, mik_aligned16(u), (T *)nullptr, nullptr);
    }
    case MIK_CGD_INIT_C:
        bs.seq += 1;
        hipLaunchKernelGGL((k_cgd_fin_init<T>), dim3(1), dim3(1), 0, ctx->stream, (const T *)it->rr_all, it->nranks, d, (T)it->reltol, (T)it->abstol,
                           (long long)bs.maxiter, bs.mirror, bs.seq);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    case MIK_CGD_STEP_A:
        MIK_TRY(cg_sweep_u<T>(&bs, r, 0, n, vec, cg_sweep_u_hints(&bs)));
        return gather_launch<T>(ctx, it->n_send, it->send_idx, u, (T *)it->send_buf, done);
    case CGD_STEP_A_EARLY:
    case CGD_STEP_A_BULK: {
        if (it->n_early <= 0) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_phase: no early rows (mik_cgd_set_halo_plan)");
        int64_t lo[3], hi[3];
        int nr = 0;
        if (phase == CGD_STEP_A_EARLY) {
            for (int q = 0; q < it->n_early; ++q) { lo[nr] = it->early_a[q]; hi[nr] = it->early_b[q]; ++nr; }
        } else {
            int64_t at = 0;
            for (int q = 0; q < it->n_early; ++q) {
                if (it->early_a[q] > at) { lo[nr] = at; hi[nr] = it->early_a[q]; ++nr; }
                at = it->early_b[q];
            }
            if (at < n) { lo[nr] = at; hi[nr] = n; ++nr; }
        }
        for (int q = 0; q < nr; ++q)
            MIK_TRY(cg_sweep_u<T>(&bs, r, lo[q], hi[q] - lo[q], vec && (lo[q] % VT<T>::W == 0), cg_sweep_u_hints(&bs)));
        if (phase == CGD_STEP_A_EARLY) return gather_launch<T>(ctx, it->n_send, it->send_idx, u, (T *)it->send_buf, done);
        return MIK_OK;
    }
    case CGD_STEP_A_EARLY_MERGED: {
        if (it->n_early <= 0 || !it->early_merged) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_phase: no merged early part");
        const int grid = (int)std::min<int64_t>((it->n_send + MIK_BLOCK - 1) / MIK_BLOCK, mik_max_grid(ctx));
        hipLaunchKernelGGL((k_cgd_early<T>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, it->n_send, it->send_idx, (const T *)r, u, x, (const T *)&d->beta,
                           (const T *)&d->alpha, done, (const int *)&d->x_pending, bs.fuse_x ? 1 : 0, (T *)it->send_buf);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    case CGD_X_FLUSH: return cg_flush_x<T>(&bs);
    case MIK_CGD_STEP_B:
    case CGD_STEP_B_NOFIN:
    case MIK_CGD_STEP_B_REST:        // the row-blocks before and after the interior range (all of them: STEP_B), then the local dot(u, c)
    case CGD_STEP_B_REST_NOFIN: {
        const bool rest = phase == MIK_CGD_STEP_B_REST || phase == CGD_STEP_B_REST_NOFIN;
        {
            CgProfileScope ps(&bs, 0);
            if (rest) MIK_TRY(mik_spmv_launch_outside<T>(ctx, bs.A, u, c, true, (T *)bs.seg_spmv, done, (int)it->int_begin, (int)it->int_end));
            else MIK_TRY(mik_spmv_launch<T>(ctx, bs.A, u, c, true, (T *)bs.seg_spmv, done));
        }
        if (phase == CGD_STEP_B_NOFIN || phase == CGD_STEP_B_REST_NOFIN) return MIK_OK;
        hipLaunchKernelGGL((k_cgd_fin_slot<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)bs.seg_spmv, nb, dot_slot, done, (FinScratch<T> *)bs.fin);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    case MIK_CGD_STEP_B_INTERIOR:    // the row-blocks that reference no halo column -- runs while the halo is in flight
        if (it->int_end <= it->int_begin) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_phase: no interior range set (mik_cgd_set_interior)");
        { CgProfileScope ps(&bs, 0); return mik_spmv_launch_range<T>(ctx, bs.A, u, c, true, (T *)bs.seg_spmv, done, (int)it->int_begin, (int)(it->int_end - it->int_begin)); }
    case MIK_CGD_STEP_C: {
        if (bs.fuse_x && (ctx->tuning[MIK_KNOB_CG_STEP] & 8) == 0) {   // alpha inside the sweep, its bookkeeping inside the finaliser (MIK_KNOB_CG_STEP bit 3: the separate k_cgd_alpha)
            MIK_TRY(cg_update_xr<T>(&bs, CoefAlphaRanks<T>{(const T *)it->dot_all, it->nranks, &d->res}, vec));
            hipLaunchKernelGGL((k_cgd_fin_slot_alpha<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)bs.seg_vec, nseg, rr_slot, done,
                               (FinScratch<T> *)bs.fin, (const T *)it->dot_all, it->nranks, d);
            MIK_LAUNCH_CHECK(ctx);
            return MIK_OK;
        }
        hipLaunchKernelGGL((k_cgd_alpha<T>), dim3(1), dim3(1), 0, ctx->stream, (const T *)it->dot_all, it->nranks, d);
        MIK_LAUNCH_CHECK(ctx);
        MIK_TRY(cg_update_xr<T>(&bs, coef_ptr<T>(&d->alpha), vec));
        hipLaunchKernelGGL((k_cgd_fin_slot<T>), dim3(MIK_FIN_WGS), dim3(64), 0, ctx->stream, (const T *)bs.seg_vec, nseg, rr_slot, done, (FinScratch<T> *)bs.fin);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    case MIK_CGD_STEP_D:
        if (it->hist_total >= bs.hist_cap) return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_phase: more than %lld steps enqueued without mik_cgd_wait", (long long)bs.hist_cap);
        it->hist_total += 1;
        bs.seq += 1;
        hipLaunchKernelGGL((k_cgd_fin_res<T>), dim3(1), dim3(1), 0, ctx->stream, (const T *)it->rr_all, it->nranks, d, (T *)bs.hist,
                           (long long)(iteration + 1), (long long)bs.maxiter, bs.mirror, bs.seq, (int)(it->hist_total - 1), bs.fuse_x ? 1 : 0);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    case CGD_NORM_AMAX: {          // (mik_safe_norm_slow, per rank)
        const int grid = (int)std::min<int64_t>((std::max<int64_t>(n, 1) + MIK_BLOCK - 1) / MIK_BLOCK, 1024);
        MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)std::max<int64_t>(std::max<int64_t>(nseg, grid), 1)));
        hipLaunchKernelGGL((k_amax<T>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, n, (const T *)r, (T *)ctx->partials);
        MIK_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL((k_amax<T>), dim3(1), dim3(MIK_BLOCK), 0, ctx->stream, (int64_t)grid, (const T *)ctx->partials, rr_slot);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    case CGD_NORM_SCALED_SQ: {
        MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)std::max<int64_t>(nseg, 1)));
        OpScaledSq<T> op{(const T *)r, (T)it->norm_scale};
        MIK_TRY((launch_map<T>(ctx, n, op, mik_aligned16(r), (T *)ctx->partials, nullptr)));
        hipLaunchKernelGGL((k_finalize_store<T>), dim3(1), dim3(MIK_FIN_THREADS), 0, ctx->stream, (const T *)ctx->partials, nseg, (int64_t)0, rr_slot,
                           (const int *)nullptr);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    }
    case CGD_FIX_STEP:
        bs.seq += 1;
        it->hist_total = it->norm_fix_index + 1;
        hipLaunchKernelGGL((k_cg_fix_res<T>), dim3(1), dim3(1), 0, ctx->stream, d, (T)it->norm_res, (T *)bs.hist, (long long)it->norm_it_next,
                           (long long)bs.maxiter, bs.mirror, bs.seq, it->norm_fix_index);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    case CGD_STEP_C_NOFIN: return cg_update_xr<T>(&bs, coef_ptr<T>(&d->alpha), vec);
    case CGD_CLEAR_PENDING:      // (applied by a no-op head, the head ahead or CGD_X_FLUSH)
        hipLaunchKernelGGL((k_cg_clear_pending<T>), dim3(1), dim3(1), 0, ctx->stream, d);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    case CGD_FIX_INIT:
        bs.seq += 1;
        hipLaunchKernelGGL((k_cgd_fix_init<T>), dim3(1), dim3(1), 0, ctx->stream, d, (T)it->norm_res, (T)it->reltol, (T)it->abstol, (long long)bs.maxiter,
                           bs.mirror, bs.seq);
        MIK_LAUNCH_CHECK(ctx);
        return MIK_OK;
    default:
        return mik_fail(ctx, MIK_ERR_INVALID, "mik_cgd_phase: unknown phase %d", phase);
    }
}

extern "C" int mik_cgd_phase(mik_cgd *it, int phase, int64_t iteration)
{
    if (!it || iteration < 0) return MIK_ERR_INVALID;
    return it->base.dtype == MIK_F64 ? cgd_phase_impl<double>(it, phase, iteration) : cgd_phase_impl<float>(it, phase, iteration);
}

int cgd_wait_raw(mik_cgd *it, CgMirror *m)
{
    MIK_TRY(cg_wait_mirror(&it->base));
    *m = *it->base.mirror;
    return MIK_OK;
}

int cgd_collect(mik_cgd *it, const CgMirror &m, double *residual, double *tol, int *done, double *history, int64_t cap, int64_t *steps)
{
    mik_cg &bs = it->base;
    mik_ctx *ctx = bs.ctx;
    const int64_t nd = m.nhist;
    if (history && nd == 1 && cap >= 1) {
        history[0] = m.res;                                   // the mirror carries the only residual: no copy
    } else if (history && nd > 0) {
        const int64_t take = std::min<int64_t>(nd, cap);
        const size_t es = mik_dtype_size(bs.dtype);
        std::vector<unsigned char> tmp((size_t)take * es);
        MIK_HIP(ctx, hipMemcpyAsync(tmp.data(), bs.hist, es * (size_t)take, hipMemcpyDeviceToHost, ctx->stream));
        MIK_HIP(ctx, mik_wait(ctx));
        for (int64_t j = 0; j < take; ++j)
            history[j] = bs.dtype == MIK_F64 ? ((const double *)tmp.data())[j] : (double)((const float *)tmp.data())[j];
    }
    if (bs.profile) (void)cg_profile_collect(&bs);           // the bracketed SpMV launches of the steps the host has now seen (mik_cgd_profile)
    // start a fresh history window for the next batch of steps (the device is idle: the host owns the mirror)
    bs.mirror->nhist = 0;
    it->hist_total = 0;
    bs.residual = m.res;
    bs.prev_residual = m.prev_res;
    if (m.tol_valid) bs.tol = m.tol;
    bs.mv_products += nd;
    if (residual) *residual = m.res;
    if (tol) *tol = bs.tol;
    if (done) *done = m.done;
    if (steps) *steps = nd;
    return MIK_OK;
}

// Block until every phase enqueued so far has run; returns the scalars of the last step and the
// residuals recorded since the previous wait (history[0..*steps-1], at most `cap`).  For hosts that drive the phases and the
// exchanges themselves: a norm outside the safe range is reported as MIK_ERR_RANGE (the step's x and r are final and x is
// flushed); mik_cgd_init / mik_cgd_iterate_many and the group calls recompute it with a common scale instead.
extern "C" int mik_cgd_wait(mik_cgd *it, double *residual, double *tol, int *done, double *history, int64_t cap, int64_t *steps)
{
    if (!it) return MIK_ERR_INVALID;
    CgMirror m;
    MIK_TRY(cgd_wait_raw(it, &m));
    if (m.range) {
        mik_ctx *ctx = it->base.ctx;
        if (it->base.fuse_x && it->initialised) {              // the frozen step's x .+= alpha .* u must not stay pending
            (void)mik_cgd_phase(it, CGD_X_FLUSH, 0);
            (void)mik_wait(ctx);
        }
        return mik_fail(ctx, MIK_ERR_RANGE, "cg (row-partitioned, host-driven phases): |r|^2 left the range of a safe norm; use mik_cgd_init / "
                                            "mik_cgd_iterate_many (or the group calls), which rescale across the ranks");
    }
    return cgd_collect(it, m, residual, tol, done, history, cap, steps);
}

// =============================================================================================
// helpers for BiCGStab(l) (src/bicgstabl.jl): batched dot to the host, small dense LU solve
// =============================================================================================

// h = V[:, 1:k]' * w -- mul!(h, adjoint(V), w) (src/orthogonalize.jl:15) and, column by column, the
// Gram matrix mul!(M, adjoint(rs), rs) of src/bicgstabl.jl:121.  h: HOST array of k scalars.
template <typename T> static int gemv_t_impl(mik_ctx *ctx, int64_t n, int k, const T *V, int64_t ldv, const T *w, T *h_host)
{
    if (k == 0) return MIK_OK;
    if ((size_t)k * sizeof(T) > mik_ctx::COEF_SAFE_SLOT) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_gemv_t: k = %d too large", k);
    const int64_t nseg = mik_nseg<T>(n);
    MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)std::max<int64_t>(nseg, 1) * (size_t)k));
    MIK_TRY(multidot<T>(ctx, n, k, V, ldv, w, (T *)ctx->coef));
    return coef_download<T>(ctx, 0, h_host, k);
}

extern "C" int mik_gemv_t(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, const void *w, void *h)
{
    if (!ctx || n < 0 || k < 0 || (k && (!h || !V || ldv < n)) || (n && k && !w)) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_gemv_t(ctx, dtype, n, k, V, ldv, w, h);
    if (dtype == MIK_F64) return gemv_t_impl<double>(ctx, n, k, (const double *)V, ldv, (const double *)w, (double *)h);
    if (dtype == MIK_F32) return gemv_t_impl<float>(ctx, n, k, (const float *)V, ldv, (const float *)w, (float *)h);
    return MIK_ERR_INVALID;
}

// M = V' * V for k <= 5 columns in one pass over V -- src/bicgstabl.jl:120 (M = rs' * rs)
template <typename T> static int gram_impl(mik_ctx *ctx, int64_t n, int k, const T *V, int64_t ldv, T *M)
{
    const int np = k * (k + 1) / 2;
    const int64_t nseg = mik_nseg<T>(n);
    T *hd = (T *)ctx->coef;
    if (nseg == 0) {
        for (int i = 0; i < k * k; ++i) M[i] = T(0);
        return MIK_OK;
    }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)nseg * (size_t)np));
    MIK_TRY(launch_gram<T>(ctx, n, k, V, ldv));
    MIK_TRY(finalize_store<T>(ctx, nseg, np, hd));
    std::vector<T> out((size_t)np);
    MIK_TRY(coef_download<T>(ctx, 0, out.data(), np));
    int p = 0;
    for (int r = 0; r < k; ++r)
        for (int c = r; c < k; ++c) { M[(size_t)c * k + r] = out[p]; M[(size_t)r * k + c] = out[p]; ++p; }
    return MIK_OK;
}

extern "C" int mik_gram(mik_ctx *ctx, int dtype, int64_t n, int k, const void *V, int64_t ldv, void *M)
{
    if (!ctx || n < 0 || k < 1 || !M || (n && (!V || ldv < n))) return MIK_ERR_INVALID;
    if (k > 5) return mik_fail(ctx, MIK_ERR_NOTIMPL, "mik_gram: k = %d (at most 5 columns; use mik_gemv_t per column)", k);
    if (mik_is_complex(dtype)) return mik_c_gram(ctx, dtype, n, k, V, ldv, M);
    if (dtype == MIK_F64) return gram_impl<double>(ctx, n, k, (const double *)V, ldv, (double *)M);
    if (dtype == MIK_F32) return gram_impl<float>(ctx, n, k, (const float *)V, ldv, (float *)M);
    return MIK_ERR_INVALID;
}

// src/bicgstabl.jl:127-132 in one sweep (k_bicg_mr); *out = norm(rs[:, 1])
template <typename T>
static int bicg_mr_impl(mik_ctx *ctx, int64_t n, int l, T *us, int64_t ldu, T *rs, int64_t ldr, T *x, const T *gamma, T *out)
{
    const int64_t nseg = mik_nseg<T>(n);
    if (nseg == 0) { *out = T(0); return MIK_OK; }
    MIK_TRY(mik_ensure_partials(ctx, sizeof(T) * (size_t)nseg));
    BicgGamma<T> gm{};
    for (int j = 0; j < l; ++j) gm.g[j] = gamma[j];
    const int grid = (int)std::min<int64_t>(nseg, mik_max_grid(ctx));
    const bool vec = mik_aligned16(us) && mik_aligned16(rs) && mik_aligned16(x) && (ldu % VT<T>::W == 0) && (ldr % VT<T>::W == 0);
    if (vec) hipLaunchKernelGGL((k_bicg_mr<T, true>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, n, nseg, l, us, ldu, rs, ldr, x, gm, (T *)ctx->partials, (const T *)nullptr);
    else hipLaunchKernelGGL((k_bicg_mr<T, false>), dim3(grid), dim3(MIK_BLOCK), 0, ctx->stream, n, nseg, l, us, ldu, rs, ldr, x, gm, (T *)ctx->partials, (const T *)nullptr);
    MIK_LAUNCH_CHECK(ctx);
    MIK_TRY(finalize_store<T>(ctx, nseg, 1, (T *)ctx->coef));
    T ss;
    MIK_TRY(coef_download<T>(ctx, 0, &ss, 1));
    if (mik_nrm_in_range(ss)) { *out = (T)std::sqrt(ss); return MIK_OK; }
    return mik_safe_norm_slow<T>(ctx, n, rs, out);                       // norm(rs[:, 1]) of a badly scaled residual
}

extern "C" int mik_bicgstab_mr_update(mik_ctx *ctx, int dtype, int64_t n, int l, void *us, int64_t ldu, void *rs, int64_t ldr, void *x,
                                      const void *gamma, void *out)
{
    if (!ctx || n < 0 || l < 1 || l > 8 || !gamma || !out || (n && (!us || !rs || !x || ldu < n || ldr < n))) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_bicgstab_mr_update(ctx, dtype, n, l, us, ldu, rs, ldr, x, gamma, out);
    if (dtype == MIK_F64) return bicg_mr_impl<double>(ctx, n, l, (double *)us, ldu, (double *)rs, ldr, (double *)x, (const double *)gamma, (double *)out);
    if (dtype == MIK_F32) return bicg_mr_impl<float>(ctx, n, l, (float *)us, ldu, (float *)rs, ldr, (float *)x, (const float *)gamma, (float *)out);
    return MIK_ERR_INVALID;
}

// Solve A x = b for a small dense column-major A (n x n, leading dimension lda) by LU with partial
// pivoting -- F = lu!(view(M, L, L)); ldiv!(gamma, F, view(M, L, 1)) at src/bicgstabl.jl:124-125.
// A is overwritten by its factors, b by the solution.  Returns MIK_ERR_SINGULAR on an exactly
// singular pivot (the reference throws SingularException).
template <typename T> static int lu_solve(T *A, int64_t lda, int n, T *b)
{
    auto at = [&](int i, int j) -> T & { return A[(size_t)j * lda + i]; };
    for (int j = 0; j < n; ++j) {
        int p = j;
        T best = std::fabs(at(j, j));
        for (int i = j + 1; i < n; ++i) { const T a = std::fabs(at(i, j)); if (a > best) { best = a; p = i; } }
        if (best == T(0)) return MIK_ERR_SINGULAR;
        if (p != j) {
            for (int c = 0; c < n; ++c) std::swap(at(j, c), at(p, c));
            std::swap(b[j], b[p]);
        }
        const T piv = at(j, j);
        for (int i = j + 1; i < n; ++i) {
            const T m = at(i, j) / piv;
            at(i, j) = m;
            for (int c = j + 1; c < n; ++c) at(i, c) = at(i, c) - m * at(j, c);
            b[i] = b[i] - m * b[j];
        }
    }
    for (int j = n - 1; j >= 0; --j) {
        b[j] = b[j] / at(j, j);
        const T t = b[j];
        for (int i = 0; i < j; ++i) b[i] = b[i] - t * at(i, j);
    }
    return MIK_OK;
}

extern "C" int mik_lu_solve(int dtype, void *A, int64_t lda, int n, void *b)
{
    if (!A || !b || n < 0 || lda < n) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_lu_solve(dtype, A, lda, n, b);
    if (dtype == MIK_F64) return lu_solve<double>((double *)A, lda, n, (double *)b);
    if (dtype == MIK_F32) return lu_solve<float>((float *)A, lda, n, (float *)b);
    return MIK_ERR_INVALID;
}

// LinearAlgebra.givensAlgorithm(f, g) -> (c, s, r) on the host -- used at src/hessenberg.jl:24 and
// src/minres.jl:129.  out = {c, s, r} of dtype.
extern "C" int mik_givens(int dtype, const void *f, const void *g, void *out)
{
    if (!f || !g || !out) return MIK_ERR_INVALID;
    if (mik_is_complex(dtype)) return mik_c_givens(dtype, f, g, out);
    if (dtype == MIK_F64) { double *o = (double *)out; givens_algorithm<double>(*(const double *)f, *(const double *)g, o[0], o[1], o[2]); return MIK_OK; }
    if (dtype == MIK_F32) { float *o = (float *)out; givens_algorithm<float>(*(const float *)f, *(const float *)g, o[0], o[1], o[2]); return MIK_OK; }
    return MIK_ERR_INVALID;
}
