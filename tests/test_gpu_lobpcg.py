"""lobpcg on the device: the four block entries of include/mik.h against their definitions bit for bit, the driver against the numpy double
(tests/lobpcg_double.py) bit for bit, and against the reference's own bound."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as sp

from ladder import ladder
from lobpcg_double import block_rdiv, block_update
from lobpcg_gpu_util import DTYPES, Blk, both, code, dots, gram_raw, same_trace, spd_b, update_raw, wide
from stationary_host import arrow

pytestmark = pytest.mark.gpu
_vp = C.c_void_p


# ---- mik_spmm -----------------------------------------------------------------------------------------------------------------------
def spmm_operators(pkg, ctx, dt):
    out = []
    for N in (5, 12):
        n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, 3, dtype=dt)
        out.append((f"laplace {N}^3", pkg.HipCSR(n, n, cp, rv, nz, index_base=1, ctx=ctx)))
    out.append(("two long rows", pkg.HipCSR.from_scipy(arrow(900, ctx.spmv_long_row() + 44, dt), ctx)))
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(12, 3, dtype=dt)
    Ac = pkg.HipCSR(n, n, cp, rv, nz, index_base=1, ctx=ctx)
    assert Ac.compact(), "the 12^3 Laplacian runs on a sliced layout: its CSR arrays can be released"
    out.append(("compacted", Ac))
    return out


@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_equals_spmv_column_by_column(pkg, ctx, dt):
    rng = np.random.default_rng(1)
    L = pkg.lib()
    for name, A in spmm_operators(pkg, ctx, dt):
        n = A.n_rows
        for b in (1, 2, 3, 8, 9, 32):
            Xh = wide(rng, (n, b), dt)
            for offset in (False, True):
                X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, np.zeros((n, b), dt), offset)
                assert L.mik_spmm(ctx.handle, A.handle, b, _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld) == 0, L.mik_last_error(ctx.handle)
                want = np.stack([pkg.mul_(pkg.HipVector(n, dt, ctx), A, X.col(j)).to_numpy() for j in range(b)], axis=1)
                assert np.array_equal(Y.get(), want), (name, b, offset)


def test_spmm_refusals(pkg, ctx):
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(5, 3)
    A = pkg.HipCSR(n, n, cp, rv, nz, index_base=1, ctx=ctx)
    X, Y = pkg.HipMatrix(n, 40, np.float64, ctx), pkg.HipMatrix(n, 40, np.float64, ctx)
    L = pkg.lib()
    assert L.mik_spmm(ctx.handle, A.handle, 33, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld) == 5
    assert L.mik_spmm(ctx.handle, A.handle, 4, _vp(X.buf.ptr), X.ld, _vp(X.col(3).ptr), X.ld) == 1           # Y overlaps X
    assert L.mik_spmm(ctx.handle, A.handle, 4, _vp(X.buf.ptr), X.ld, _vp(X.col(4).ptr), X.ld) == 0           # the columns behind X: fine
    assert L.mik_spmm(ctx.handle, A.handle, 4, _vp(X.buf.ptr), n - 1, _vp(Y.buf.ptr), Y.ld) == 1             # leading dimension too small


# ---- mik_block_gram -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_block_gram_equals_dot_entry_by_entry(pkg, ctx, dt, n):
    rng = np.random.default_rng(n)
    for (p, q) in [(1, 1), (2, 3), (8, 8), (5, 32), (32, 32)]:
        Xh, Yh = wide(rng, (n, p), dt), wide(rng, (n, q), dt)
        for offset in (False, True):
            X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Yh, offset)
            assert np.array_equal(gram_raw(pkg, ctx, X, p, Y, q), dots(pkg, X, p, Y, q)), (n, p, q, offset)
            if p == q:
                assert np.array_equal(gram_raw(pkg, ctx, X, p, X, p), dots(pkg, X, p, X, p)), (n, p, "X == Y", offset)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rung", ["m1024", "m1025"])
def test_block_gram_on_each_side_of_the_level2_switch(pkg, ctx, dt, rung):
    W, Lr = ctx.reduce_shape(dt)
    m, n, _ = ladder(W, Lr, ctx.info()["sweep_grid_cap"])[rung]
    rng = np.random.default_rng(m)
    X, Y = Blk(pkg, ctx, wide(rng, (n, 8), dt), False), Blk(pkg, ctx, wide(rng, (n, 8), dt), False)
    assert np.array_equal(gram_raw(pkg, ctx, X, 8, Y, 8), dots(pkg, X, 8, Y, 8)), (rung, m, n)


def test_block_gram_refusals(pkg, ctx):
    X = pkg.HipMatrix(100, 40, np.float64, ctx)
    G = np.zeros((40, 40), order="F")
    L = pkg.lib()
    assert L.mik_block_gram(ctx.handle, 0, 100, 33, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 40) == 5
    assert L.mik_block_gram(ctx.handle, 0, 100, 2, 33, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 40) == 5
    assert L.mik_block_gram(ctx.handle, 0, 100, 4, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 3) == 1


# ---- mik_block_rdiv -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 4097])
def test_block_rdiv_equals_the_numpy_loop(pkg, ctx, dt, n):
    """off-diagonal magnitudes in 2^-3 .. 2, diagonal in 1 .. 8: a column grows by at most a factor 2^2 per earlier column, so 32 columns of
    data up to 2^21 stay finite in Float32"""
    rng = np.random.default_rng(n + 2)
    for s in (1, 2, 7, 32):
        Xh = wide(rng, (n, s), dt, span=20)
        R = np.triu(rng.choice([-1.0, 1.0], size=(s, s)) * np.exp2(rng.uniform(-3, 0, size=(s, s))) * (1 + rng.random((s, s))), 1)
        R = (R + np.diag(rng.choice([-1.0, 1.0], size=s) * np.exp2(rng.uniform(0, 2, size=s)) * (1 + rng.random(s)))).astype(dt)
        R[np.tril_indices(s, -1)] = np.nan                          # the strict lower triangle is not read
        want = block_rdiv(Xh.copy(), R)
        assert np.all(np.isfinite(want))
        Rf = np.asfortranarray(R)
        for offset in (False, True):
            X = Blk(pkg, ctx, Xh, offset)
            rc = pkg.lib().mik_block_rdiv(ctx.handle, code(pkg, dt), n, s, Rf.ctypes.data_as(_vp), s, _vp(X.ptr), X.ld)
            assert rc == 0, pkg.lib().mik_last_error(ctx.handle)
            assert np.array_equal(X.get(), want), (n, s, offset)
    X = pkg.HipMatrix(n, 40, dt, ctx)
    R = np.asfortranarray(np.eye(40, dtype=dt))
    assert pkg.lib().mik_block_rdiv(ctx.handle, code(pkg, dt), n, 33, R.ctypes.data_as(_vp), 40, _vp(X.buf.ptr), X.ld) == 5


# ---- mik_block_update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 4097, 1_000_003])
def test_block_update_equals_the_composition_of_rotations(pkg, ctx, dt, n):
    rng = np.random.default_rng(n + 3)
    shapes = [(4, 3, 3)] if n == 1_000_003 else [(1, 0, 0), (4, 4, 0), (4, 3, 3), (8, 1, 1), (32, 32, 32), (32, 5, 5)]
    for (sx, b1, b2) in shapes:
        Xh, Rh, Ph = wide(rng, (n, sx), dt, 20), wide(rng, (n, max(b1, 1)), dt, 20), wide(rng, (n, max(b2, 1)), dt, 20)
        V = wide(rng, (sx + b1 + b2, sx), dt, 20)
        xo, po = block_update(sx, b1, b2, Xh, Rh, Ph, V)
        sentinel = np.full((n, sx), 7.0, dt)
        for offset in ((False,) if n == 1_000_003 else (False, True)):
            X, R, P = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Rh, offset), Blk(pkg, ctx, Ph, offset)
            Xo, Po = Blk(pkg, ctx, sentinel, offset), Blk(pkg, ctx, sentinel, offset)
            assert update_raw(pkg, ctx, n, sx, b1, b2, X, R, P, V, Xo, Po) == 0, pkg.lib().mik_last_error(ctx.handle)
            assert np.array_equal(Xo.get(), xo), (n, sx, b1, b2, offset, "Xout")
            assert np.array_equal(Po.get(), po if b1 else sentinel), (n, sx, b1, b2, offset, "Pout")       # b1 == 0: Pout untouched


def test_block_update_refusals(pkg, ctx):
    n, dt = 100, np.float64
    rng = np.random.default_rng(4)
    M = Blk(pkg, ctx, wide(rng, (n, 40), dt), False)
    O1, O2 = Blk(pkg, ctx, np.zeros((n, 40), dt), False), Blk(pkg, ctx, np.zeros((n, 40), dt), False)
    V = np.ones((100, 40), dt)

    class At:                                                   # columns j .. of a block
        def __init__(self, B, j):
            self.ptr, self.ld, self.dt = B.col(j).ptr, B.ld, B.dt

    X, R, P = At(M, 0), At(M, 4), At(M, 8)
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, O2) == 0
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], At(M, 3), O2) == 1          # Xout overlaps X
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(M, 7)) == 1          # Pout overlaps R
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(M, 11)) == 1         # Pout overlaps P
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(O1, 2)) == 1         # the outputs overlap each other
    assert update_raw(pkg, ctx, n, 4, 0, 0, X, R, P, V[:4, :4], O1, At(M, 0)) == 0           # b1 == 0: Pout is not written, so it may be anything
    assert update_raw(pkg, ctx, n, 4, 5, 0, X, R, P, V[:9, :4], O1, O2) == 5                 # b1 > sx
    assert update_raw(pkg, ctx, n, 33, 0, 0, X, R, P, V[:33, :33], O1, O2) == 5              # wider than 32
    assert update_raw(pkg, ctx, n, 4, 0, 2, X, R, P, V[:6, :4], O1, O2) == 1                 # P without R


# ---- the driver: device against double, bit for bit ---------------------------------------------------------------------------------
def lap12(pkg, dt):
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(12, 3, dtype=dt, index_base=0)
    return sp.csc_matrix((nz, rv, cp), shape=(n, n))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("generalized", [False, True])
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("jacobi", [False, True])
def test_device_run_equals_the_double_bit_for_bit(pkg, orc, ctx, dt, generalized, largest, jacobi):
    S = lap12(pkg, dt)
    n = S.shape[0]
    X0 = np.random.default_rng(6).random((n, 4)).astype(dt)
    rd, rh = both(pkg, orc, ctx, dt, S, spd_b(n, dt) if generalized else None, largest, (X0,), jacobi, maxiter=25)
    assert isinstance(rd.X, pkg.HipMatrix) and rd.iterations == rh.iterations and rd.iterations >= 3
    same_trace(rd.trace, rh.trace)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms) and rd.converged == rh.converged
    assert np.array_equal(rd.X.to_numpy(), rh.X.to_numpy())


@pytest.mark.parametrize("dt", DTYPES)
def test_device_batches_equal_the_double_bit_for_bit(pkg, orc, ctx, dt):
    """nev = 6 in batches of 4: the shrinking last batch, the constraint's update"""
    S = lap12(pkg, dt)
    n = S.shape[0]
    X0 = np.random.default_rng(7).random((n, 4)).astype(dt)
    rd, rh = both(pkg, orc, ctx, dt, S, spd_b(n, dt), False, (X0, 6), True, maxiter=20)
    assert len(rd.lam) == 6 and np.array_equal(rd.iterations, rh.iterations) and len(rd.trace) == len(rh.trace)
    for ta, tb in zip(rd.trace, rh.trace):
        same_trace(ta, tb)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms)
    assert np.array_equal(rd.X.to_numpy(), rh.X.to_numpy())


# ---- the driver against the reference's own bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,dims", [(20, 2), (12, 3)])
def test_residual_below_the_tolerance_on_the_laplacians(pkg, ctx, dt, N, dims):
    """test/lobpcg.jl:72-84 on the device: |A X - X diag(lam)| <= tol column by column (checked in float64 on the host)"""
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, dims, dtype=dt, index_base=0)
    S = sp.csc_matrix((nz, rv, cp), shape=(n, n))
    A = pkg.HipCSR.from_scipy(S, ctx)
    tol = import_module(pkg.__name__ + ".lobpcg").default_tolerance(dt)
    d = pkg.HipVector.from_numpy(S.diagonal().astype(dt), ctx)
    for largest, P in ((True, None), (False, pkg.JacobiPrec(d))):
        X0 = np.random.default_rng(8).random((n, 2)).astype(dt)
        r = pkg.lobpcg(A, largest, X0, P=P, tol=tol, maxiter=2000)
        X = r.X.to_numpy().astype(np.float64)
        res = np.linalg.norm(S.astype(np.float64) @ X - X * r.lam.astype(np.float64)[None, :], axis=0)
        print(f"lobpcg {np.dtype(dt).name} laplace {N}^{dims} largest={largest}: {r.iterations} iterations, residuals {res}, tol {tol:.3e}")
        assert r.converged and r.iterations < 2000
        assert np.all(res <= tol)


def test_no_device_allocation_inside_the_iteration_loop(pkg, ctx, monkeypatch):
    S = lap12(pkg, np.float64)
    n = S.shape[0]
    A, B = pkg.HipCSR.from_scipy(S, ctx), pkg.HipCSR.from_scipy(spd_b(n, np.float64), ctx)
    P = pkg.JacobiPrec(pkg.HipVector.from_numpy(S.diagonal(), ctx))
    Cm = np.random.default_rng(9).random((n, 2))
    L = pkg.lib()
    real = L.mik_malloc
    count = [0]

    def counting(*args):
        count[0] += 1
        return real(*args)

    monkeypatch.setattr(L, "mik_malloc", counting)
    it = pkg.LOBPCGIterator(A, B, False, np.random.default_rng(10).random((n, 4)), None, P, Cm)
    seen = []
    step = it.step

    def watched(tol, log):
        seen.append(count[0])
        return step(tol, log)

    it.step = watched
    pkg.lobpcg_(it, maxiter=12, not_zeros=True)
    seen.append(count[0])
    monkeypatch.undo()
    assert count[0] > 0 and len(seen) > 5
    assert len(set(seen)) == 1, seen
