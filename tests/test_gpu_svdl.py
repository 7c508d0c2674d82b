"""svdl on the device: the two new entries of include/mik.h against their definitions bit for bit, and the driver against the reference's
own bounds and against the numpy double (tests/svdl_double.py)."""
import ctypes as C

import numpy as np
import pytest

from svdl_double import NumpyOps, basis_rotate
from test_svdl_host import big_case, diag_case, issue55_v0, rect_case

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
DTYPES = [np.float64, np.float32]
METHODS = ["ritz", "harmonic"]
KL = [(1, 1), (2, 1), (10, 5), (12, 6), (12, 12), (40, 20), (64, 64)]


def wide(rng, shape, dt):
    """mixed signs, magnitudes spanning 2^-30 .. 2^30: a fused multiply-add or another association changes bits"""
    a = rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-30, 30, size=shape)) * (1 + rng.random(shape))
    return a.astype(dt)


def rotate_raw(pkg, ctx, dt, n, k, l, Vptr, ldv, F, Yptr, ldy):
    F = np.asfortranarray(F, dt)
    return pkg.lib().mik_basis_rotate(ctx.handle, pkg._lib.dtype_code(dt), n, k, l, _vp(Vptr), ldv, F.ctypes.data_as(_vp), max(F.shape[0], 1), _vp(Yptr), ldy)


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 4097, 1_000_003])
def test_basis_rotate_equals_the_numpy_loop(pkg, ctx, dt, n):
    rng = np.random.default_rng(n)
    es = np.dtype(dt).itemsize
    for (k, l) in KL:
        V, F = wide(rng, (n, k), dt), wide(rng, (k, l), dt)
        want = basis_rotate(V, F)
        Vd = pkg.HipMatrix.from_numpy(V, ctx)                      # ld = n rounded up to 64: ldv > n unless n = 256
        Yd = pkg.HipMatrix(n, l, dt, ctx)
        assert rotate_raw(pkg, ctx, dt, n, k, l, Vd.buf.ptr, Vd.ld, F, Yd.buf.ptr, Yd.ld) == 0
        assert np.array_equal(Yd.to_numpy(), want), (n, k, l, "aligned")
        if n == 1_000_003 and (k, l) != (12, 6):
            continue
        # V and Y offset by one element, odd leading dimensions > n: the scalar-load variant
        ldv, ldy = n + 3 + (n % 2 == 0), n + 5 + (n % 2 == 0)
        vb, yb = pkg.HipVector(ldv * k + 1, dt, ctx), pkg.HipVector(ldy * l + 1, dt, ctx)
        host = np.zeros(ldv * k + 1, dt)
        for j in range(k):
            host[1 + j * ldv: 1 + j * ldv + n] = V[:, j]
        vb.copy_from_host(host)
        yb.fill_(0)
        assert rotate_raw(pkg, ctx, dt, n, k, l, vb.ptr + es, ldv, F, yb.ptr + es, ldy) == 0
        got = yb.to_numpy()
        got = np.stack([got[1 + j * ldy: 1 + j * ldy + n] for j in range(l)], axis=1)
        assert np.array_equal(got, want), (n, k, l, "offset")


def test_basis_rotate_refusals(pkg, ctx):
    V = pkg.HipMatrix(100, 70, np.float64, ctx)
    Y = pkg.HipMatrix(100, 70, np.float64, ctx)
    F = np.zeros((70, 70))
    assert rotate_raw(pkg, ctx, np.float64, 100, 4, 5, V.buf.ptr, V.ld, F[:4, :5], Y.buf.ptr, Y.ld) == 5        # l > k
    assert rotate_raw(pkg, ctx, np.float64, 100, 65, 3, V.buf.ptr, V.ld, F[:65, :3], Y.buf.ptr, Y.ld) == 5      # k > 64
    assert rotate_raw(pkg, ctx, np.float64, 100, 4, 0, V.buf.ptr, V.ld, F[:4, :1], Y.buf.ptr, Y.ld) == 5        # l < 1
    assert rotate_raw(pkg, ctx, np.float64, 100, 4, 2, V.buf.ptr, V.ld, F[:4, :2], V.col(3).ptr, V.ld) == 1     # Y overlaps V
    assert rotate_raw(pkg, ctx, np.float64, 100, 4, 2, V.buf.ptr, V.ld, F[:4, :2], V.col(4).ptr, V.ld) == 0     # the columns behind V: fine


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def chain(pkg, Q, k, q, alpha):
    """the composed existing calls that define mik_svdl_reorth"""
    T = q.dtype.type
    old = pkg.norm(q)
    pkg.gemv_n_(q, Q, k, pkg.gemv_t_(Q, k, q), -1)
    nw = pkg.norm(q)
    passes = 1
    if nw <= T(alpha) * old:
        pkg.gemv_n_(q, Q, k, pkg.gemv_t_(Q, k, q), -1)
        nw = pkg.norm(q)
        passes = 2
    q.scal_(T(1) / nw)
    return nw, passes


def reorth(pkg, ctx, Q, k, q, alpha):
    dt = q.dtype
    a, beta, passes = np.asarray([alpha], dt), np.zeros(1, dt), C.c_int(0)
    rc = pkg.lib().mik_svdl_reorth(ctx.handle, pkg._lib.dtype_code(dt), q.n, k, _vp(Q.buf.ptr), Q.ld, _vp(q.ptr), a.ctypes.data_as(_vp),
                                   beta.ctypes.data_as(_vp), C.byref(passes))
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)
    return beta[0], passes.value


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [255, 4097, 1_000_003])
def test_reorth_equals_the_composed_calls(pkg, ctx, dt, n):
    """q, beta and passes equal the chain bit for bit; afterwards max |Q'q| (float64, host) stays below sqrt(2) * n * eps(T)."""
    rng = np.random.default_rng(n + 1)
    T = np.dtype(dt).type
    alpha = T(1 / np.sqrt(2))
    Qh = np.linalg.qr(rng.standard_normal((n, 40)))[0].astype(dt)
    Q = pkg.HipMatrix.from_numpy(Qh, ctx)
    for k in (0, 1, 5, 12, 40):
        generic = rng.standard_normal(n).astype(dt)
        dependent = (Qh[:, :k].astype(np.float64) @ rng.standard_normal(k) + 1e-9 * rng.standard_normal(n)).astype(dt)
        cases = [("generic", generic, 1), ("dependent", dependent, 2 if k else 1)]
        if dt == np.float64:
            cases.append(("scaled 1e-200", generic * 1e-200, 1))          # the sum of squares underflows: the scaled recomputation of "Norms"
        for name, qh, want_passes in cases:
            q1, q2 = pkg.HipVector.from_numpy(qh, ctx), pkg.HipVector.from_numpy(qh, ctx)
            b1, p1 = chain(pkg, Q, k, q1, alpha)
            b2, p2 = reorth(pkg, ctx, Q, k, q2, alpha)
            assert p1 == p2 == want_passes, (name, k, p1, p2)
            assert b1 == b2, (name, k, b1, b2)
            got = q2.to_numpy()
            assert np.array_equal(q1.to_numpy(), got), (name, k)
            if k:
                defect = np.max(np.abs(Qh[:, :k].astype(np.float64).T @ got.astype(np.float64)))
                print(f"reorth {np.dtype(dt).name} n={n} k={k} {name}: passes {p2}, max|Q'q| = {defect:.3e}, bound {np.sqrt(2) * n * np.finfo(dt).eps:.3e}")
                assert defect < np.sqrt(2) * n * np.finfo(dt).eps
    # an unaligned q and an odd leading dimension: the scalar-load variant, same bits
    k = 5
    qh = rng.standard_normal(n).astype(dt)
    buf = pkg.HipVector(n + 1, dt, ctx)
    buf.copy_from_host(np.concatenate([[0], qh]).astype(dt))
    q2, q1 = buf.view(1, n), pkg.HipVector.from_numpy(qh, ctx)
    b1, p1 = chain(pkg, Q, k, q1, alpha)
    b2, p2 = reorth(pkg, ctx, Q, k, q2, alpha)
    assert (b1, p1) == (b2, p2) and np.array_equal(q1.to_numpy(), q2.to_numpy())


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------
def history_distance(a, b):
    """largest relative difference of :betas and of :ritz over the restarts both runs made"""
    nit = min(a.iters, b.iters)
    rb = max(abs(float(x) - float(y)) / abs(float(y)) for x, y in zip(a["betas"][:nit], b["betas"][:nit]))
    rr = max(float(np.max(np.abs(x.astype(float) - y.astype(float)) / np.abs(y.astype(float)))) for x, y in zip(a["ritz"][:nit], b["ritz"][:nit]))
    return max(rb, rr)


def device_vs_double(pkg, orc, A, kw, method):
    """The device and the double differ only in the reduction order inside norms and dots.  Yardstick: what a change of reduction order alone
    does to the double -- the double with the device tree against the double with sequential sums -- as the floor, 4 x the floor as the
    allowance (two orders can differ from a third by up to twice their own distance, times two for restarts the floor run did not see).
    Floors measured on the CPU (largest relative difference of :betas / :ritz): diagonal fp64 2.0e-15 (ritz) / 7.0e-15 (harmonic), fp32
    2.8e-7 / 5.7e-7; rectangular fp64 6.8e-15 / 9.9e-15, fp32 1.1e-6 / 1.2e-6 -- allowances 4 x those; the device measured 0 on the diagonal case and 5.4e-15 / 5.7e-15, 3.1e-6 / 1.9e-6 on the
    rectangular one.  The floor is recomputed here so
    that the comparison always uses the figure of the inputs at hand."""
    Ad = pkg.extras.with_adjoint_from_scipy(A.tocsc())
    s, L, h = pkg.svdl(Ad, method=method, log=True, **kw)
    _, _, ht = pkg.svdl(A, method=method, log=True, ops=NumpyOps(orc, A, "tree"), **kw)
    _, _, hs = pkg.svdl(A, method=method, log=True, ops=NumpyOps(orc, A, "seq"), **kw)
    floor = history_distance(ht, hs)
    dist = history_distance(h, ht)
    print(f"   device vs double: {dist:.3e}, floor {floor:.3e}, allowance {4 * floor:.3e}; restarts {h.iters} / {ht.iters}")
    assert h.iters == ht.iters
    assert dist <= 4 * floor
    return s, L, h, Ad


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_diagonal_matrix_on_the_device(pkg, orc, ctx, dt, method):
    """test/svdl.jl:15-53 through the device, the reference's bounds (see tests/test_svdl_host.py for what :38-46 assert)."""
    A, kw = diag_case(dt)
    n, ns, tol = 30, 5, 1e-5
    sigma, L, history, Ad = device_vs_double(pkg, orc, A, kw, method)
    assert isinstance(history, pkg.ConvergenceHistory)
    for key in ("conv", "ritz", "resnorm", "Bs", "betas"):
        assert key in history.data and len(history[key]) == history.iters
    assert np.linalg.norm(sigma - np.arange(n, n - 5, -1.0)) < 5 ** 2 * 1e-5
    with pytest.raises(pkg.ArgumentError):
        pkg.svdl(Ad, method="fakemethod", vecs="none", **kw)
    S, L = pkg.svdl(Ad, method=method, vecs="both", **kw)
    assert isinstance(S.U, pkg.HipMatrix)
    U, Vt = S.U.to_numpy(), S.Vt.copy()
    assert U.shape == (n, ns) and Vt.shape == (ns, n)
    su = np.array([np.sign(U[n - 1 - i, i]) for i in range(5)])
    sv = np.array([np.sign(Vt[i, n - 1 - i]) for i in range(5)])
    for i in range(5):
        U[n - 1 - i, i] -= su[i]
        Vt[i, n - 1 - i] -= sv[i]
    assert np.linalg.norm(U) < sigma[0] * np.sqrt(tol)
    assert np.linalg.norm(Vt) < sigma[0] * np.sqrt(tol)
    assert np.array_equal(su, sv)
    assert np.linalg.norm(sigma - S.S) < 2 * max(tol * ns * sigma[0], tol)
    sigma1, _ = pkg.svdl(Ad, nsv=1, tol=tol, reltol=tol, v0=issue55_v0(dt), method=method)
    assert abs(sigma[0] - sigma1[0]) < 10 * max(tol * sigma[0], tol)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_rectangular_matrix_on_the_device(pkg, orc, ctx, dt, method):
    """test/svdl.jl:55-66 through the device: 25e-5 against numpy.linalg.svd, convergence before maxiter."""
    Ad, A, kw = rect_case(dt)
    sigma, L, history, _ = device_vs_double(pkg, orc, A, kw, method)
    assert history.isconverged and np.all(history["conv"][-1]) and history.iters < kw["maxiter"]
    assert np.linalg.norm(sigma - np.linalg.svd(Ad, compute_uv=False)[:5]) < 5 ** 2 * 1e-5


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------
def test_a_size_where_the_kernels_matter(pkg, ctx):
    """m = 2^20 + 17, n = 2^20 (tests/test_svdl_host.py big_case; verified on the double at n = 2^14), fp64, defaults: converges within 60
    restarts, |sigma - d[:6]| < 36 * sqrt(eps), and with vecs = both the residuals |A v_i - sigma_i u_i| and the orthonormality defects
    |U'U - I|, |V'V - I| stay below sigma_1 * sqrt(tol)."""
    n = 2 ** 20
    A, d, kw = big_case(n)
    Ad = pkg.extras.with_adjoint_from_scipy(A)
    tol = np.sqrt(np.finfo(np.float64).eps)
    S, L, h = pkg.svdl(Ad, vecs="both", log=True, **kw)
    assert h.isconverged and np.all(h["conv"][-1]) and h.iters <= 60
    err = np.linalg.norm(S.S - d[:6])
    U, V = S.U.to_numpy(), S.V.to_numpy()
    res = max(np.linalg.norm(A @ V[:, i] - S.S[i] * U[:, i]) for i in range(6))
    du, dv = np.linalg.norm(U.T @ U - np.eye(6)), np.linalg.norm(V.T @ V - np.eye(6))
    print(f"large case: {h.iters} restarts, |sigma - exact| = {err:.3e} (bound {36 * tol:.3e}); max residual {res:.3e}, |U'U - I| = {du:.3e}, "
          f"|V'V - I| = {dv:.3e} (bound {S.S[0] * np.sqrt(tol):.3e})")
    assert err < 36 * tol
    assert res < S.S[0] * np.sqrt(tol) and du < S.S[0] * np.sqrt(tol) and dv < S.S[0] * np.sqrt(tol)


# ---- 11 ---------------------------------------------------------------------------------------------------------------------------
def test_no_device_allocation_inside_the_restart_loop(pkg, ctx, monkeypatch):
    Ad, A, kw = rect_case(np.float64)
    Adev = pkg.extras.with_adjoint_from_scipy(A)
    L = pkg.lib()
    real = L.mik_malloc
    count = [0]

    def counting(*args):
        count[0] += 1
        return real(*args)

    monkeypatch.setattr(L, "mik_malloc", counting)
    seen = []

    class History(pkg.ConvergenceHistory):
        def nextiter_(self, *a, **k):
            seen.append(count[0])
            return super().nextiter_(*a, **k)

    log = History(partial=True)
    pkg.svdl_method_(log, Adev, kw["nsv"], k=kw["k"], v0=kw["v0"], tol=kw["tol"], maxiter=kw["maxiter"])
    monkeypatch.undo()
    assert count[0] > 0 and len(seen) > 3
    assert len(set(seen[1:])) == 1, seen
