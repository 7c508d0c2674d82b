"""The sweeps over a basis -- mik_gemv_t, mik_gemv_n, mik_svdl_reorth, mik_gram -- bit for bit against the CPU oracle, at the sizes where
the segment scaffold they share (csrc/mik_kernels.h: seg_load / seg_store / seg_dot / seg_axpy, pair_put / pair_total) changes path.

mik_svdl_reorth runs the very kernels of mik_gemv_t / mik_gemv_n (k_multidot / k_gemv_n with SQ = true), so the comparisons of
tests/test_gpu_svdl.py and tests/test_gpu_large_reductions.py against the composed calls have the same template on both sides: a slip in the
shared code would cancel there.  Here every expected value comes from the oracle (orc.dot in tree mode, orc.gemv_n, orc.nrm2), never from
another device entry.

With SEG = 256 * W * L (W, L from mik_reduce_shape): n = 1 (one thread, one element), SEG / 2 + 3 (one partial segment whose tail is no
multiple of W) and SEG + W + 1 (two segments, the second ragged); k = 1 and 5; both placements of lobpcg_gpu_util.Blk -- aligned (the
16-byte accesses) and one element off (the scalar ones) -- with a sentinel in everything of the buffers that belongs to no column, which
must survive the entries that write.  Data from lobpcg_gpu_util.wide: another association or a fused multiply-add moves bits.  No tolerance
anywhere.  The several-grid-pass and beyond-1024-segment shapes of these kernels are in tests/test_gpu_large_reductions.py and
tests/test_gpu_lobpcg_paths.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from lobpcg_gpu_util import DTYPES, Blk, code, wide

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
SENTINEL = 7.0
SIZES = ["one", "half_plus_3", "seg_plus_w_plus_1"]
PLACEMENTS = [False, True]                       # Blk(offset=...)


def size(name, W, L):
    SEG = 256 * W * L
    return {"one": 1, "half_plus_3": SEG // 2 + 3, "seg_plus_w_plus_1": SEG + W + 1}[name]


def shape(ctx, dt, name):
    W, L = ctx.reduce_shape(dt)
    n = size(name, W, L)
    assert n == 1 or (n % W != 0 and (n > 256 * W * L) == (name == "seg_plus_w_plus_1"))
    return W, L, n


def seed(dt, n, k, salt):
    return [np.dtype(dt).itemsize, n, k, salt]


def cols_of(V):
    return [np.ascontiguousarray(V[:, j]) for j in range(V.shape[1])]


def tree_dots(orc, V, w, W, L):
    return np.array([orc.dot(c, w, "tree", W, L) for c in cols_of(V)], V.dtype)


def vec(pkg, ctx, host, offset):
    """an n-vector as a one-column block: the same two placements, the same sentinel around it"""
    return Blk(pkg, ctx, np.asfortranarray(host.reshape(-1, 1)), offset, fill=SENTINEL)


def untouched(*blks):
    return all(np.all(b.padding() == b.dt.type(SENTINEL)) for b in blks)


# ---- the inputs and what the oracle makes of them: once per (dtype, n, k), shared by both placements, never written to --------------
@functools.lru_cache(maxsize=None)
def gemv_case(orc, dtn, n, k, W, L):
    dt = np.dtype(dtn).type
    rng = np.random.default_rng(seed(dt, n, k, 1))
    V, w, c = np.asfortranarray(wide(rng, (n, k), dt)), wide(rng, n, dt), wide(rng, k, dt)
    alphas = [dt(-1), dt(0.37)]
    out = dict(V=V, w=w, c=c, alphas=alphas, h=tree_dots(orc, V, w, W, L), y=[orc.gemv_n(V, c, w, float(a)) for a in alphas])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def orthonormal(rng, n, k, dt):
    """k orthonormal columns in float64, rounded to dt; n < k: a row of unit norm per row instead (every vector then lies in the span)"""
    G = wide(rng, (n, k), np.float64, span=8)
    U = np.linalg.qr(G)[0] if n >= k else np.linalg.qr(G.T)[0].T
    return np.asfortranarray(U.astype(dt))


def reorth_by_the_oracle(orc, Q, q, alpha, W, L):
    """include/mik.h: old = norm(q); q -= Q * (Q' q); if norm(q) <= alpha * old: once more; beta = norm(q); q .*= inv(beta) (not for beta = 0)"""
    dt = q.dtype.type
    old = dt(orc.nrm2(q, "tree", W, L))
    passes = 0
    while True:
        passes += 1
        q = orc.gemv_n(Q, tree_dots(orc, Q, q, W, L), q, -1.0)
        nw = dt(orc.nrm2(q, "tree", W, L))
        if passes == 2 or not (nw <= alpha * old):
            break
    if nw != 0:
        q = q * (dt(1) / nw)
    return q, nw, passes


@functools.lru_cache(maxsize=None)
def reorth_case(orc, dtn, n, k, W, L, kind):
    """generic: Q = U / 2 with U orthonormal, so that a pass leaves at least 3/4 of any q -- above alpha = 1 / sqrt(2): one pass.
    dependent: Q = U and q = U c + a small generic part (the construction of the rung test in tests/test_gpu_large_reductions.py): the
    first pass takes nearly all of q away, so a second one runs."""
    dt = np.dtype(dtn).type
    rng = np.random.default_rng(seed(dt, n, k, 2))
    U = orthonormal(rng, n, k, dt)
    g = wide(rng, n, dt, span=8)
    if kind == "generic":
        Q, q, want = np.asfortranarray(U * dt(0.5)), g, 1
    else:
        Q, want = U, 2
        q = (U.astype(np.float64) @ rng.standard_normal(k) * float(np.linalg.norm(g)) + 1e-4 * g).astype(dt)
    alpha = dt(1 / np.sqrt(2))
    qo, beta, passes = reorth_by_the_oracle(orc, Q, q, alpha, W, L)
    for a in (Q, q, qo):
        a.setflags(write=False)
    return dict(Q=Q, q=q, alpha=alpha, q_out=qo, beta=beta, passes=passes, want=want)


@functools.lru_cache(maxsize=None)
def gram_case(orc, dtn, n, W, L):
    dt = np.dtype(dtn).type
    V = np.asfortranarray(wide(np.random.default_rng(seed(dt, n, 3, 3)), (n, 3), dt))
    cs = cols_of(V)
    M = np.array([[orc.dot(cs[r], cs[c], "tree", W, L) for c in range(3)] for r in range(3)], dt)
    return V, M


# ---- the tests -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", PLACEMENTS)
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", SIZES)
@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_t_against_the_oracle(pkg, orc, ctx, dt, name, k, offset):
    W, L, n = shape(ctx, dt, name)
    case = gemv_case(orc, np.dtype(dt).name, n, k, W, L)
    V, w = Blk(pkg, ctx, case["V"], offset, fill=SENTINEL), vec(pkg, ctx, case["w"], offset)
    h = np.full(k, SENTINEL, dt)
    assert pkg.lib().mik_gemv_t(ctx.handle, code(pkg, dt), n, k, _vp(V.ptr), V.ld, _vp(w.ptr), h.ctypes.data_as(_vp)) == 0
    assert np.array_equal(h, case["h"]), (h, case["h"])


@pytest.mark.parametrize("offset", PLACEMENTS)
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", SIZES)
@pytest.mark.parametrize("dt", DTYPES)
def test_gemv_n_against_the_oracle(pkg, orc, ctx, dt, name, k, offset):
    W, L, n = shape(ctx, dt, name)
    case = gemv_case(orc, np.dtype(dt).name, n, k, W, L)
    V = Blk(pkg, ctx, case["V"], offset, fill=SENTINEL)
    for alpha, want in zip(case["alphas"], case["y"]):
        y = vec(pkg, ctx, case["w"], offset)
        a = np.array([alpha], dt)
        assert pkg.lib().mik_gemv_n(ctx.handle, code(pkg, dt), n, k, _vp(V.ptr), V.ld, case["c"].ctypes.data_as(_vp), a.ctypes.data_as(_vp), _vp(y.ptr)) == 0
        assert np.array_equal(y.get()[:, 0], want), alpha
        assert untouched(y, V), alpha
    assert np.array_equal(V.get(), case["V"])


@pytest.mark.parametrize("kind", ["generic", "dependent"])
@pytest.mark.parametrize("offset", PLACEMENTS)
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", SIZES)
@pytest.mark.parametrize("dt", DTYPES)
def test_svdl_reorth_against_the_oracle(pkg, orc, ctx, dt, name, k, offset, kind):
    W, L, n = shape(ctx, dt, name)
    case = reorth_case(orc, np.dtype(dt).name, n, k, W, L, kind)
    assert case["passes"] == case["want"]                                           # the inputs are what they are meant to be
    Q, q = Blk(pkg, ctx, case["Q"], offset, fill=SENTINEL), vec(pkg, ctx, case["q"], offset)
    a, beta, passes = np.array([case["alpha"]], dt), np.full(1, SENTINEL, dt), C.c_int(0)
    rc = pkg.lib().mik_svdl_reorth(ctx.handle, code(pkg, dt), n, k, _vp(Q.ptr), Q.ld, _vp(q.ptr), a.ctypes.data_as(_vp), beta.ctypes.data_as(_vp),
                                   C.byref(passes))
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)
    assert passes.value == case["passes"]
    assert beta[0] == case["beta"], (beta[0], case["beta"])
    assert np.array_equal(q.get()[:, 0], case["q_out"])
    assert untouched(q, Q) and np.array_equal(Q.get(), case["Q"])


@pytest.mark.parametrize("offset", PLACEMENTS)
@pytest.mark.parametrize("name", SIZES)
@pytest.mark.parametrize("dt", DTYPES)
def test_gram_of_three_columns_against_the_oracle(pkg, orc, ctx, dt, name, offset):
    W, L, n = shape(ctx, dt, name)
    Vh, want = gram_case(orc, np.dtype(dt).name, n, W, L)
    V = Blk(pkg, ctx, Vh, offset, fill=SENTINEL)
    M = np.full((3, 3), SENTINEL, dt, order="F")
    assert pkg.lib().mik_gram(ctx.handle, code(pkg, dt), n, 3, _vp(V.ptr), V.ld, M.ctypes.data_as(_vp)) == 0
    assert np.array_equal(M, want), (M, want)
