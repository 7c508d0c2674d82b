"""jacobi / gauss_seidel / sor / ssor on the device (iterativesolvers.jl_amd/stationary.py over the mik_stationary entries), bit for
bit against tests/stationary_ref/stationary_ref.c -- the reference's CSC column loops restated in C."""
import numpy as np
import pytest
import scipy.sparse as sp

import stationary_host as sh
from stationary_fixtures import check_methods as _check_methods, dev as _dev       # shared with tests/test_gpu_stationary_paths.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("stationary_ref_gpu"))


def _mats(pkg, ctx, dtype):
    lap = lambda N, d: sh.Mat.from_csc(*pkg.fixtures.laplace_matrix(N, d, dtype))
    n, cp, rv, nz, _ = pkg.fixtures.advection_dominated(8, 100.0)
    long_row = ctx.spmv_long_row()
    return {"lap1": lap(300, 1), "lap2": lap(24, 2), "lap3": lap(12, 3),
            "adv": sh.Mat.from_csc(n, cp, rv, nz.astype(dtype)),
            "sprand": sh.Mat(sh.sprand_dominant(500, 0.01, 1234322, dtype), dtype),
            "arrow": sh.Mat(sh.arrow(3000, long_row + 40, dtype), dtype),
            "arrow_cut": sh.Mat(sh.arrow(3 * ctx.spmv_long_segment() + 500, 3 * ctx.spmv_long_segment() + 100, dtype), dtype),
            "tridiag": sh.Mat(sh.tridiag(2000, dtype), dtype)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_methods_bit_for_bit(pkg, ctx, ref, dtype):
    rng = np.random.default_rng(42)
    for name, M in _mats(pkg, ctx, dtype).items():
        A = _dev(pkg, M)
        S = pkg.StationaryOperator(A)
        info = S.info()
        if name == "tridiag":           # one row per level: a single one-workgroup launch per sweep
            assert info["levels_forward"] == info["levels_backward"] == 2000 and info["launches_forward"] == 1
        if name.startswith("arrow"):
            assert M.n and A.nnz > 0
        try:
            _check_methods(pkg, ref, M, A, 1.2, 3, rng)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


def test_int32_uploads_and_both_omega_types(pkg, ctx, ref):
    """SparseMatrixCSC{T, Int32} (test/stationary.jl:21 runs Ti in (Int64, Int32)); Float32 data with omega Float64 and Float32"""
    rng = np.random.default_rng(7)
    for dtype in (np.float64, np.float32):
        M = sh.Mat(sh.sprand_dominant(400, 0.02, 99, dtype), dtype)
        A = _dev(pkg, M, i32=True)
        for omega in (1.2, np.float32(1.2), 1):
            _check_methods(pkg, ref, M, A, omega, 2, rng)


def test_sor_odd_and_even_maxiter_swap(pkg, ctx, ref):
    """sor! returns iterable.x (:360): after an odd count the internal buffer, the caller's x then holding iterate k - 1"""
    M = sh.Mat.from_csc(*pkg.fixtures.laplace_matrix(10, 3))
    A = _dev(pkg, M)
    b = np.linspace(-1, 1, M.n)
    for k in (2, 3):
        x = pkg.HipVector.from_numpy(np.zeros(M.n))
        r = pkg.sor_(x, A, pkg.HipVector.from_numpy(b), 1.3, maxiter=k)
        xr, rr, which = ref.sor(M, b, np.zeros(M.n), 1.3, k)
        assert (r is x) == (which == 0) == (k % 2 == 0)
        assert np.array_equal(r.to_numpy(), rr) and np.array_equal(x.to_numpy(), xr)
    assert np.array_equal(x.to_numpy(), ref.sor(M, b, np.zeros(M.n), 1.3, 2)[1])


def test_jacobi_iterable_doctest_two_right_hand_sides(pkg, ctx):
    """docs/src/iterators.md:34-70 on the device: the four norms Julia printed"""
    A = sp.diags([-np.ones(3), 2 * np.ones(4), -np.ones(3)], [-1, 0, 1], format="csc")
    Ad = pkg.HipCSR.from_scipy(A)
    b1, b2 = np.array([1.0, 2, 3, 4]), np.array([-1.0, 1, -1, 1])
    x = pkg.HipVector.from_numpy(np.array([0.0, -1, 1, 0]))
    it = pkg.jacobi_iterable(x, Ad, pkg.HipVector.from_numpy(b1), maxiter=2)
    assert it.maxiter == 2 and it.next.n == 4

    def rel(b):
        xs = x.to_numpy()
        y = [0.0] * 4
        for col in range(4):                                   # SparseArrays' column scatter
            for k in range(A.indptr[col], A.indptr[col + 1]):
                y[A.indices[k]] += A.data[k] * xs[col]
        r = b - np.array(y)
        return float(np.sqrt(sum(float(v) * float(v) for v in r)) / np.sqrt(sum(float(v) * float(v) for v in b)))

    assert rel(b1) == 1.2909944487358056
    assert sum(1 for _ in it) == 2
    assert rel(b1) == 0.8228507357554791
    it.b.copyto_(pkg.HipVector.from_numpy(b2))
    assert rel(b2) == 2.6368778887161235
    assert sum(1 for _ in it) == 2
    assert rel(b2) == 1.610815496107484


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_building_blocks_with_aliasing(pkg, ctx, ref, dtype):
    rng = np.random.default_rng(5)
    M = sh.Mat(sh.sprand_dominant(700, 0.01, 3, dtype), dtype)
    ref.diag(M)
    A = _dev(pkg, M)
    S = pkg.StationaryOperator(A)
    V = lambda a: pkg.HipVector.from_numpy(a)
    x, y, b = (rng.standard_normal(M.n).astype(dtype) for _ in range(3))
    assert np.array_equal(S.diag_ldiv_(V(np.zeros(M.n, dtype)), V(x)).to_numpy(), ref.ldiv(M, x))
    xv = V(x)
    assert np.array_equal(S.diag_ldiv_(xv, xv).to_numpy(), ref.ldiv(M, x))             # y may alias x
    for a, be in ((1.0, 0.0), (1.0, 1.0), (2.0, 3.0), (-1.0, 1.0)):
        assert np.array_equal(S.offdiag_mul_(a, V(x), be, V(y)).to_numpy(), ref.offdiag_mul(M, a, x, be, y)), (a, be)
    for upper in (True, False):
        xv = V(x)
        assert np.array_equal(S.gs_multiply_(upper, -1.0, xv, 1.0, V(b), xv).to_numpy(), ref.gs_mul(M, upper, -1.0, x, 1.0, b)), upper   # z === x
        assert np.array_equal(S.gs_multiply_(upper, 2.0, V(x), 3.0, V(b), V(y)).to_numpy(), ref.gs_mul(M, upper, 2.0, x, 3.0, b, y)), upper
        sub = S.backward_sub_ if upper else S.forward_sub_
        assert np.array_equal(sub(V(x)).to_numpy(), ref.sub(M, upper, x)), upper
        for omega in (1.2, np.float32(0.8)):
            assert np.array_equal(sub(V(x), omega, V(y)).to_numpy(), ref.sub(M, upper, x, omega, y)), (upper, omega)


def test_same_results_whatever_the_spmv_layout(pkg, ctx, ref):
    M = sh.Mat.from_csc(*pkg.fixtures.laplace_matrix(16, 3))
    b = np.cos(np.arange(M.n, dtype=np.float64))
    out = []
    for layout in ("auto", "csr"):
        A = _dev(pkg, M).set_layout(layout)
        x = pkg.HipVector.from_numpy(np.zeros(M.n))
        out.append(pkg.ssor_(x, A, pkg.HipVector.from_numpy(b), 1.5, maxiter=2).to_numpy())
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], ref.ssor(M, b, np.zeros(M.n), 1.5, 2)[0])


def test_singular_exception_with_the_column(pkg, ctx):
    cases = [(np.array([[0.0, 1.0], [1.0, 0.0]]), 1),                               # test/stationary.jl:65-80
             (np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 1.0, 1.0]]), 2)]               # missing diagonal
    for z in (0.0, -0.0):                                                              # explicitly stored 0.0 and -0.0
        A = sp.csc_matrix((np.array([2.0, 1.0, 3.0, 1.0, 4.0]), (np.array([0, 1, 2, 2, 1]), np.array([0, 1, 2, 1, 2]))), shape=(3, 3))
        A.sort_indices()
        A.data[A.indptr[2] + list(A.indices[A.indptr[2]:A.indptr[3]]).index(2)] = z
        cases.append((A, 3))
    for A, col in cases:
        A = sp.csc_matrix(A)
        Ad = pkg.HipCSR.from_scipy(A)
        b = pkg.HipVector.from_numpy(np.ones(A.shape[0]))
        for solver in (pkg.jacobi, pkg.gauss_seidel, lambda A, b: pkg.sor(A, b, 0.5), lambda A, b: pkg.ssor(A, b, 0.5)):
            with pytest.raises(np.linalg.LinAlgError) as ei:
                solver(Ad, b)
            assert isinstance(ei.value, pkg.SingularException) and ei.value.col == col and f"SingularException({col})" in str(ei.value)


def test_rectangular_and_compacted_operators_are_refused(pkg, ctx):
    A = sp.random(6, 4, density=0.5, random_state=1, format="csc") + sp.eye(6, 4, format="csc")
    with pytest.raises(pkg.MikError) as ei:
        pkg.StationaryOperator(pkg.HipCSR.from_scipy(A))
    assert ei.value.code == 3
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(16, 3)
    L = pkg.HipCSR(n, n, cp, rv, nz)
    assert L.compact()
    with pytest.raises(pkg.MikError) as ei:
        pkg.StationaryOperator(L)
    assert ei.value.code == 5


def test_gauss_seidel_and_ssor_at_256_cubed(pkg, ctx, ref):
    """the size scripts/stationary_bench.py times is the size that is checked: 2 iterations each"""
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(256, 3)
    M = sh.Mat.from_csc(n, cp, rv, nz)
    A = pkg.HipCSR(n, n, cp, rv, nz)
    del cp, rv
    S = pkg.StationaryOperator(A)
    info = S.info()
    assert info["levels_forward"] == info["levels_backward"] == 3 * 256 - 2
    b = pkg.fixtures.hashed_rhs(n)
    bd = pkg.HipVector.from_numpy(b)
    x = pkg.HipVector(n).fill_(0)
    it = pkg.GaussSeidelIterable(S, x, bd, 2)
    for _ in it:
        pass
    assert np.array_equal(x.to_numpy(), ref.gauss_seidel(M, b, np.zeros(n), 2)[0])
    x.fill_(0)
    it = pkg.SSORIterable(S, 1.5, x, x.similar(), bd, 2)
    for _ in it:
        pass
    assert np.array_equal(x.to_numpy(), ref.ssor(M, b, np.zeros(n), 1.5, 2)[0])
