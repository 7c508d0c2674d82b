"""Complex element types on the device.  Every L1 / L2 comparison is bit for bit against the C restatement of the
orders (tests/complex_ref/complex_ref.c); the entries that are by definition real sweeps over the 2 n interleaved reals (norm, copy, sub,
fill, the real-scalar scale) are compared with the real entry on the same memory.  The solvers run the complex test sets of
test/cg.jl:27-47,99-121 and test/gmres.jl:16-57,76-98 and must agree bit for bit -- x, every residual, the counts -- with the numpy double
of tests/complex_host.py running the same Python."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import complex_host as ch
from complex_host import ref  # noqa: F401  (fixture)
from conftest import KN

pytestmark = pytest.mark.gpu

CT = [np.complex128, np.complex64]
_vp = C.c_void_p


def seg(ctx, T):
    w, l = ctx.reduce_shape(T)
    assert w == 16 // np.dtype(T).itemsize
    return 256 * w * l


def rnd(rng, T, n):
    rt = ch.real_of(T)
    return (rng.standard_normal(n).astype(rt) + 1j * rng.standard_normal(n).astype(rt)).astype(T)


def real_view(pkg, v):
    """the same device memory as a vector of 2 n reals"""
    return pkg.HipVector.wrap(v.ptr, 2 * v.n, ch.real_of(v.dtype), v.ctx, owner=v)


# ---------------------------------------------------------------------------------------------
# vector entries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("which", ["1", "S-1", "S", "S+1", "1024S", "1024S+1"])
def test_vector_entries(pkg, ctx, ref, T, which):
    S = seg(ctx, T)
    n = {"1": 1, "S-1": S - 1, "S": S, "S+1": S + 1, "1024S": 1024 * S, "1024S+1": 1024 * S + 1}[which]      # the last pair: the level-2 switch
    shape = ctx.reduce_shape(T)
    rng = np.random.default_rng(n)
    xh, yh = rnd(rng, T, n), rnd(rng, T, n)
    V = lambda a: pkg.HipVector.from_numpy(a, ctx)
    x, y = V(xh), V(yh)
    # dot: one complex scalar, the tree for re and the tree for im
    d = pkg.dot(x, y)
    assert d.dtype == np.dtype(T) and d == ref.dot(xh, yh, shape)
    # the axpy family with a complex scalar
    alpha = T(0.75 - 1.25j)
    for name in ("axpy", "xpby", "scal"):
        dev, want = V(yh), yh.copy()
        if name == "axpy":
            dev.axpy_(alpha, x); ref.axpy(alpha, xh, want)
        elif name == "xpby":
            dev.xpby_(x, alpha); ref.xpby(xh, alpha, want)
        else:
            dev.scal_(alpha); ref.scal(alpha, want)
        assert np.array_equal(dev.to_numpy(), want), name
    # by definition the real sweeps over the 2 n interleaved reals: same bits as the real entry on the same memory
    rt = ch.real_of(T).type
    nx = pkg.norm(x)
    assert nx.dtype == ch.real_of(T) and nx == pkg.norm(real_view(pkg, x)) and nx == ref.nrm2(xh, shape)
    a, b = V(yh), V(yh)
    a.sub_(x); real_view(pkg, b).sub_(real_view(pkg, x))
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    a, b = V(yh), V(yh)
    a.scal_(rt(0.3)); real_view(pkg, b).scal_(rt(0.3))
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    a, b = V(yh), V(yh)
    a.xpby_(x, rt(0.3)); real_view(pkg, b).xpby_(real_view(pkg, x), rt(0.3))                        # the real beta of src/cg.jl:51
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    a, b = V(yh), V(yh)
    a.axpy_(rt(-0.7), x); real_view(pkg, b).axpy_(rt(-0.7), real_view(pkg, x))
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    a, b = V(yh), V(yh)
    a.copyto_(x); real_view(pkg, b).copyto_(real_view(pkg, x))
    assert np.array_equal(a.to_numpy(), xh) and np.array_equal(b.to_numpy(), xh)
    a, b = V(yh), V(yh)
    a.fill_(T(1.5 + 1.5j)); real_view(pkg, b).fill_(rt(1.5))
    assert np.array_equal(a.to_numpy(), b.to_numpy())
    a.fill_(T(2 - 3j))
    assert np.array_equal(a.to_numpy(), np.full(n, T(2 - 3j)))


@pytest.mark.parametrize("T", CT)
def test_norm_outside_the_safe_range_and_unaligned_vectors(pkg, ctx, ref, T):
    S = seg(ctx, T)
    n, shape = S + 1, ctx.reduce_shape(T)
    rng = np.random.default_rng(5)
    tiny = (rnd(rng, T, n) * ch.real_of(T).type(1e-200 if T == np.complex128 else 1e-30)).astype(T)       # every square underflows
    x = pkg.HipVector.from_numpy(tiny, ctx)
    nx = pkg.norm(x)
    assert nx > 0 and nx == pkg.norm(real_view(pkg, x)) and nx == ref.nrm2(tiny, shape)
    # vectors that start 8 bytes into an allocation take the element-wise loads: same bits
    xh, yh = rnd(rng, T, n), rnd(rng, T, n)
    es = np.dtype(T).itemsize
    bx, by = pkg.HipVector(n + 1, T, ctx), pkg.HipVector(n + 1, T, ctx)
    ux = pkg.HipVector.wrap(bx.ptr + 8, n, T, ctx, owner=bx).copy_from_host(xh)
    uy = pkg.HipVector.wrap(by.ptr + 8, n, T, ctx, owner=by).copy_from_host(yh)
    assert es in (8, 16) and ux.ptr % 16 == 8
    assert pkg.dot(ux, uy) == ref.dot(xh, yh, shape)
    want = yh.copy()
    ref.axpy(T(1 - 2j), xh, want)
    uy.axpy_(T(1 - 2j), ux)
    assert np.array_equal(uy.to_numpy(), want)
    ref.xpby(xh, T(0.5 + 3j), want)
    uy.xpby_(ux, T(0.5 + 3j))
    assert np.array_equal(uy.to_numpy(), want)
    ref.scal(T(-0.25 + 1.5j), want)
    uy.scal_(T(-0.25 + 1.5j))
    assert np.array_equal(uy.to_numpy(), want)
    uy.fill_(T(2 - 3j))                                                  # re != im: the complex fill, not the real one over 2 n
    assert np.array_equal(uy.to_numpy(), np.full(n, T(2 - 3j)))


# ---------------------------------------------------------------------------------------------
# SpMV
# ---------------------------------------------------------------------------------------------
def spmv_matrix(T, n_rows=300, n_cols=1500, seed=3):
    """an empty row, rows of 1, 256, 257, 1024 and 1025 entries among short random ones; 300 rows (not a multiple of 256); rectangular"""
    rng = np.random.default_rng(seed)
    special = {0: 0, 5: 1, 17: 256, 130: 257, 255: 1024, 256: 1025, 299: 257}
    rows, cols, vals = [], [], []
    for r in range(n_rows):
        ln = special.get(r, int(rng.integers(1, 9)))
        c = np.sort(rng.choice(n_cols, ln, replace=False))
        rows += [r] * ln
        cols += list(c)
        vals.append(rnd(rng, T, ln))
    return sp.csr_matrix((np.concatenate(vals), (rows, cols)), shape=(n_rows, n_cols))


@pytest.mark.parametrize("T", CT)
def test_spmv_row_orders_and_uploads(pkg, ctx, ref, T):
    M = spmv_matrix(T)
    M.sort_indices()
    assert (ctx.spmv_long_row(), ctx.spmv_long_segment(), ctx.spmv_long_group()) == (256, 1024, 4)
    rng = np.random.default_rng(9)
    xh = rnd(rng, T, M.shape[1])
    want = ref.spmv(M.indptr.astype(np.int32), M.indices.astype(np.int32), np.ascontiguousarray(M.data), xh, M.shape[0])
    assert want[0] == 0 and not np.isnan(want).any()
    x = pkg.HipVector.from_numpy(xh, ctx)
    Mc = M.tocsc()
    Mc.sort_indices()
    ops = []
    for m, is_csc in ((M, False), (Mc, True)):
        for base in (0, 1):
            for it in (np.int64, np.int32):
                ops.append(pkg.HipCSR(m.shape[0], m.shape[1], (m.indptr + base).astype(it), (m.indices + base).astype(it), m.data, index_base=base,
                                      is_csc=is_csc, ctx=ctx))
    for A in ops:
        y = pkg.HipVector(M.shape[0], T, ctx).fill_(T(np.nan))
        assert np.array_equal(pkg.mul_(y, A, x).to_numpy(), want)
    A = ops[0]
    # the operator queries: it runs on its CSR arrays and says so
    assert A.layout() == pkg.HipCSR.LAYOUTS[0] and A.set_layout("auto") is A and A.layout() == pkg.HipCSR.LAYOUTS[0]
    assert A.compact() is False
    assert A.spmv_kernel().startswith("k_spmv_complex")
    nr, nc, nnz, dt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    assert pkg.lib().mik_csr_info(A.handle, C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(dt)) == 0
    assert (nr.value, nc.value, nnz.value, dt.value) == (M.shape[0], M.shape[1], M.nnz, pkg._lib.dtype_code(T))
    es = np.dtype(T).itemsize
    assert A.spmv_stored_bytes() >= M.nnz * (es + 4) + (M.shape[0] + 1) * 4 + (M.shape[0] + M.shape[1]) * es
    # a CSR upload whose rows are not sorted by column lands in the same order
    perm_idx, perm_val = M.indices.copy(), M.data.copy()
    for r in range(M.shape[0]):
        lo, hi = M.indptr[r], M.indptr[r + 1]
        perm_idx[lo:hi], perm_val[lo:hi] = perm_idx[lo:hi][::-1].copy(), perm_val[lo:hi][::-1].copy()
    B = pkg.HipCSR(M.shape[0], M.shape[1], M.indptr.astype(np.int64), perm_idx.astype(np.int64), perm_val, index_base=0, is_csc=False, ctx=ctx)
    assert np.array_equal((B @ x).to_numpy(), want)
    # x and y 8 bytes into their allocations
    bx, by = pkg.HipVector(M.shape[1] + 1, T, ctx), pkg.HipVector(M.shape[0] + 1, T, ctx)
    ux = pkg.HipVector.wrap(bx.ptr + 8, M.shape[1], T, ctx, owner=bx).copy_from_host(xh)
    uy = pkg.HipVector.wrap(by.ptr + 8, M.shape[0], T, ctx, owner=by)
    assert np.array_equal(pkg.mul_(uy, A, ux).to_numpy(), want)


@pytest.mark.parametrize("T", CT)
def test_spmv_grid_stride_on_a_small_machine(pkg, ctx, ref, T):
    """planned for 8 compute units the row-block kernel has 64 workgroups: 16,384 rows per pass, so 16,700 rows take a second, ragged pass"""
    n = 64 * 256 + 316
    rng = np.random.default_rng(21)
    ln = rng.integers(0, 4, n)
    rows = np.repeat(np.arange(n), ln)
    cols = (rows + rng.integers(-3, 4, rows.size)) % n
    M = sp.csr_matrix((rnd(rng, T, rows.size), (rows, cols)), shape=(n, n))      # duplicates are summed by scipy
    M.sort_indices()
    xh = rnd(rng, T, n)
    want = ref.spmv(M.indptr.astype(np.int32), M.indices.astype(np.int32), np.ascontiguousarray(M.data), xh, n)
    A = pkg.HipCSR(n, n, M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data, index_base=0, is_csc=False, ctx=ctx)
    x = pkg.HipVector.from_numpy(xh, ctx)
    full = (A @ x).to_numpy()
    ctx.set_tuning(KN.MACHINE, 8 | (1 << 16))
    try:
        small = (A @ x).to_numpy()
    finally:
        ctx.set_tuning(KN.MACHINE, 0)
    assert np.array_equal(full, want) and np.array_equal(small, want)


# ---------------------------------------------------------------------------------------------
# Modified Gram-Schmidt and gemv_n
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("k", [1, 2, 31])
@pytest.mark.parametrize("size", ["S+1", "several"])
def test_mgs_and_gemv_n(pkg, ctx, ref, T, k, size):
    S = seg(ctx, T)
    n = S + 1 if size == "S+1" else 5 * S + 3
    shape = ctx.reduce_shape(T)
    rng = np.random.default_rng(100 * k + n)
    V = pkg.HipMatrix(n, k, T, ctx)
    Vh = np.zeros(V.ld * k, T)
    for j in range(k):
        col = rnd(rng, T, n) / ch.real_of(T).type(np.sqrt(2 * n))
        Vh[j * V.ld: j * V.ld + n] = col
        V.col(j).copy_from_host(col)
    wh = rnd(rng, T, n)
    w = pkg.HipVector.from_numpy(wh, ctx)
    h = np.zeros(k, T)
    nrm = pkg.orthogonalize_and_normalize_(V, k, w, h, pkg.ModifiedGramSchmidt())
    want_w = wh.copy()
    want_h, want_nrm = ref.mgs(Vh, V.ld, k, want_w, shape)
    assert nrm.dtype == ch.real_of(T) and nrm == want_nrm
    assert np.array_equal(h, want_h) and np.array_equal(w.to_numpy(), want_w)
    for method in (pkg.ClassicalGramSchmidt(), pkg.DGKS()):
        with pytest.raises(pkg.MikError, match=type(method).__name__) as e:
            pkg.orthogonalize_and_normalize_(V, k, w, h, method)
        assert e.value.code == 5                                            # MIK_ERR_NOTIMPL
    c, yh, alpha = rnd(rng, T, k), rnd(rng, T, n), T(0.5 + 2j)
    y = pkg.HipVector.from_numpy(yh, ctx)
    pkg.gemv_n_(y, V, k, c, alpha)
    want_y = yh.copy()
    ref.gemv_n(Vh, V.ld, k, c, alpha, want_y)
    assert np.array_equal(y.to_numpy(), want_y)


# ---------------------------------------------------------------------------------------------
# solvers: the reference's complex test sets, device against the numpy double
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backends(pkg, ctx, ref):
    return ch.DeviceBackend(pkg, ctx), ch.HostBackend(pkg, ref)


@pytest.mark.parametrize("T", CT)
def test_cg_complex_full_system(backends, T):
    dev, host = (ch.cg_full(be, T) for be in backends)
    ch.check_cg_full(dev)
    ch.same(dev, host)


@pytest.mark.parametrize("T", CT)
@pytest.mark.parametrize("solver", ["cg", "gmres"])
def test_termination_criterion(backends, T, solver):
    dev, host = (ch.termination(be, T, solver) for be in backends)
    ch.check_termination(dev)
    ch.same(dev, host)


@pytest.mark.parametrize("T,sparse", [(np.complex128, False), (np.complex64, False), (np.complex128, True)])
def test_gmres_complex_sets(backends, T, sparse):
    dev, host = (ch.gmres_sets(be, T, sparse) for be in backends)
    ch.check_gmres_sets(dev)
    ch.same(dev, host)


def hermitian_laplacian(pkg, T, n):
    """the leading n x n block of the 3-D Laplacian fixture (a principal submatrix of a positive definite matrix), its diagonal shifted by 1,
    plus i K with K real and skew-symmetric on the same pattern: Hermitian, strictly diagonally dominant, so positive definite"""
    N = int(np.ceil(n ** (1 / 3)))
    while N ** 3 < n:
        N += 1
    m, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3)
    L = sp.csc_matrix((nzval, rowval - 1, colptr - 1), shape=(m, m)).tocsr()[:n, :n].tocoo()
    val = L.data.astype(np.complex128)
    val[L.row == L.col] += 1.0
    val[L.row < L.col] += 0.1j
    val[L.row > L.col] -= 0.1j
    return sp.csr_matrix((val.astype(T), (L.row, L.col)), shape=(n, n))


@pytest.mark.parametrize("T", CT)
def test_hermitian_laplacian_cg_and_gmres(pkg, ctx, backends, T):
    n = seg(ctx, T) + 1
    M = hermitian_laplacian(pkg, T, n)
    assert abs(M - M.conj().T).max() == 0
    b = rnd(np.random.default_rng(2), T, n)
    reltol = np.sqrt(np.finfo(ch.real_of(T)).eps)
    res = []
    for be in backends:
        A, bv = be.operator(M), be.vector(b)
        x1, h1 = pkg.cg_(be.vector(np.zeros(n, T)), A, bv, initially_zero=True, maxiter=80, log=True, ops=be.ops)
        x2, h2 = pkg.gmres_(be.vector(np.zeros(n, T)), A, bv, initially_zero=True, restart=5, maxiter=80, log=True, ops=be.ops)
        res.append(dict(x1=x1.to_numpy(), h1=ch._hist(h1), x2=x2.to_numpy(), h2=ch._hist(h2)))
    dev, host = res
    Md, bd = M.astype(np.complex128), b.astype(np.complex128)
    # the stopping test is on the recurrence / implicit residual; the true one may differ from it by the rounding of the steps taken: at
    # most eps ||A|| ||x|| per step (||A||_inf <= 7 + 6 |1 + 0.1 i| < 14 here)
    eps = np.finfo(ch.real_of(T)).eps
    for x, h in ((dev["x1"], dev["h1"]), (dev["x2"], dev["h2"])):
        gap = h["iters"] * eps * 14 * np.linalg.norm(x) / np.linalg.norm(bd)
        assert h["conv"] and np.linalg.norm(Md @ x - bd) / np.linalg.norm(bd) <= reltol + gap
    assert np.all(np.diff(dev["h2"]["res"]) <= 0.0)
    ch.same(dev, host)
    # the public entries without `ops`, and a LinearOperator callback: the same iterates
    A, bv = backends[0].operator(M), backends[0].vector(b)
    x3, h3 = pkg.cg(A, bv, maxiter=80, log=True)
    assert np.array_equal(x3.to_numpy(), dev["x1"]) and np.array_equal(np.array(h3["resnorm"]), dev["h1"]["res"])
    x4, h4 = pkg.gmres(pkg.LinearOperator(n, T, lambda y, x: pkg.mul_(y, A, x), ctx), bv, restart=5, maxiter=80, log=True)
    assert np.array_equal(x4.to_numpy(), dev["x2"]) and h4.mvps == dev["h2"]["mvps"]
    with pytest.raises(TypeError, match="JacobiPrec.*complex"):
        pkg.cg(A, bv, Pl=pkg.JacobiPrec(bv))
    # the fused handles refuse a complex operator (mik_cg_create / mik_gmres_create: MIK_ERR_NOTIMPL)
    x0 = bv.zero()
    with pytest.raises(pkg.MikError) as e:
        pkg.CGIterable(A, x0, bv, pkg.CGStateVariables(x0.zero(), x0.similar(), x0.similar()), pkg.Identity(), abstol=0.0, reltol=1e-8, maxiter=3,
                       initially_zero=True)
    assert e.value.code == 5
    with pytest.raises(pkg.MikError) as e:
        pkg.GMRESIterable(x0, A, bv, abstol=0.0, reltol=1e-8, restart=3, maxiter=3, initially_zero=True, orth_meth=pkg.ModifiedGramSchmidt())
    assert e.value.code == 5


def test_real_path_is_untouched_by_a_complex_solve(pkg, ctx):
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(16, 3)
    A = pkg.HipCSR(n, n, colptr, rowval, nzval, index_base=1, ctx=ctx)
    b = pkg.HipVector.from_numpy(pkg.fixtures.hashed_rhs(n), ctx)

    def real_run():
        x, h = pkg.cg(A, b, maxiter=10, log=True)
        return A.spmv_kernel(), np.array(h["resnorm"]), x.to_numpy()
    before = real_run()
    T = np.complex128
    M = hermitian_laplacian(pkg, T, 600)
    Ac = ch.DeviceBackend(pkg, ctx).operator(M)
    bc = pkg.HipVector.from_numpy(rnd(np.random.default_rng(4), T, 600), ctx)
    _x, hc = pkg.cg(Ac, bc, log=True)
    _x, hg = pkg.gmres(Ac, bc, restart=5, log=True)
    assert hc.isconverged and hg.isconverged
    after = real_run()
    assert before[0] == after[0] and len(before[1]) == 10 and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
