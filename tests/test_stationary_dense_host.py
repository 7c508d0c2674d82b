"""The dense stationary methods (src/stationary.jl) without a GPU: the C checker tests/stationary_ref/stationary_dense_ref.c (the
reference's column loops) held bit for bit to the per-row forms the device kernels implement, written as explicit numpy chains; the
checker against the assertions of the reference's own dense tests; and the Python layer of stationary_dense.py on a numpy double of its
operator."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import stationary_dense_host as dh
from host_double import FakeVector
from stationary_dense_double import DoubleOperator

OMEGAS = (1.25, np.float32(0.7), 1)             # Float64, Float32, Int


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("stationary_dense_ref"))


def _case(n, dtype, seed=3):
    rng = np.random.default_rng(seed)
    A = dh.dominant(n, dtype, seed)
    assert n < 2 or not np.array_equal(A, A.T)
    return A, rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)


# ---- 1: the checker equals the per-row forms, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_checker_equals_the_row_forms_bit_for_bit(ref, n, dtype):
    A, b, x0 = _case(n, dtype)
    iters = 3 if n < 65 else 2
    # Jacobi
    x, nxt = x0, None
    for _ in range(iters):
        x, nxt = dh.rows_jacobi(A, b, x)
    xr, nr, s = ref.jacobi(A, b, x0, iters)
    assert s == 0 and np.array_equal(xr, x) and np.array_equal(nr, nxt)
    # Gauss-Seidel
    x = x0
    for _ in range(iters):
        x, _t = dh.rows_forward(A, b, x)
    xr, s = ref.gauss_seidel(A, b, x0, iters)
    assert s == 0 and np.array_equal(xr, x)
    for omega in OMEGAS:
        # SOR: tmp keeps the accumulators the divisions read
        x = x0
        for _ in range(iters):
            x, t = dh.rows_forward(A, b, x, omega)
        xr, tr, s = ref.sor(A, b, x0, omega, iters)
        assert s == 0 and np.array_equal(xr, x) and np.array_equal(tr, t), omega
        # SSOR: the backward half is row-parallel on the forward half's x, both parts descending
        x = x0
        for _ in range(iters):
            x, _t = dh.rows_forward(A, b, x, omega)
            x, t = dh.rows_backward(A, b, x, omega)
        xr, tr, s = ref.ssor(A, b, x0, omega, iters)
        assert s == 0 and np.array_equal(xr, x) and np.array_equal(tr, t), omega


def test_the_backward_half_is_not_a_triangular_solve(ref):
    """:254-260 subtracts column col before it updates x[col]: a backward substitution with the NEW x gives other numbers"""
    A, b, x0 = _case(6, np.float64)
    x1, _ = dh.rows_forward(A, b, x0, 1.25)
    solve = x1.copy()
    for r in range(5, -1, -1):
        acc = dh._chain(b[r], A, r, range(r - 1, -1, -1), x1)
        acc = dh._chain(acc, A, r, range(5, r, -1), solve)
        solve[r] = dh._relax(np.float64, x1[r], acc / A[r, r], 1.25)
    xr, _, _ = ref.ssor(A, b, x0, 1.25, 1)
    assert np.array_equal(xr, dh.rows_backward(A, b, x1, 1.25)[0]) and not np.array_equal(xr, solve)


def test_float64_omega_on_float32_data_widens_and_differs_from_float32_omega(ref):
    A, b, x0 = _case(40, np.float32)
    w = 1.2
    wide_x = ref.sor(A, b, x0, w, 3)[0]
    narrow_x = ref.sor(A, b, x0, np.float32(w), 3)[0]
    assert not np.array_equal(wide_x, narrow_x)
    assert np.array_equal(ref.sor(A, b, x0, 1, 2)[0], ref.sor(A, b, x0, np.float32(1), 2)[0])      # an Int omega stays in the element type


def test_a_padded_leading_dimension_changes_nothing(ref):
    A, b, x0 = _case(65, np.float64)
    assert np.array_equal(ref.ssor(A, b, x0, 1.25, 2)[0], ref.ssor(A, b, x0, 1.25, 2, ld=128)[0])
    assert np.array_equal(ref.jacobi(A, b, x0, 2)[0], ref.jacobi(A, b, x0, 2, ld=128)[0])


# ---- 2: what the reference's dense tests assert ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_solvers_converge_to_the_direct_solution_on_a_strictly_diagonally_dominant_system(ref, dtype):
    """test/stationary.jl: the dense methods on a strictly diagonally dominant matrix reach A \\ b"""
    n = 10
    A, b, x0 = _case(n, dtype, seed=11)
    exact = np.linalg.solve(A.astype(np.float64), b.astype(np.float64))
    tol = math.sqrt(np.finfo(dtype).eps)
    for x in (np.zeros(n, dtype), x0):
        for got in (ref.jacobi(A, b, x, 20 * n)[0], ref.gauss_seidel(A, b, x, 20 * n)[0], ref.sor(A, b, x, 0.9, 20 * n)[0],
                    ref.ssor(A, b, x, 0.9, 20 * n)[0]):
            assert np.linalg.norm(got - exact) <= tol * np.linalg.norm(exact)


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_check_diag_reports_the_first_zero_one_based(ref, zero):
    for dtype in (np.float64, np.float32):
        for pos in (0, 3, 6):
            A = dh.dominant(7, dtype)
            A[pos, pos] = zero
            A[6, 6] = zero                      # a later zero is not the one reported
            assert ref.check_diag(A) == pos + 1
            assert ref.jacobi(A, np.ones(7), np.zeros(7), 1)[2] == pos + 1 and ref.ssor(A, np.ones(7), np.zeros(7), 1.0, 1)[2] == pos + 1
    assert ref.check_diag(dh.dominant(7, np.float64)) == 0


# ---- 3: the Python layer on the numpy double -------------------------------------------------------------------------------------
def _V(a):
    return FakeVector(np.array(a))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_public_names_run_exactly_maxiter_iterations(pkg, ref, dtype):
    A, b, x0 = _case(12, dtype)
    for k in (0, 1, 4):
        O = DoubleOperator(pkg, ref, A)
        x = _V(x0)
        assert pkg.jacobi_(x, O, _V(b), maxiter=k) is x and O.calls == ["jacobi"] * k
        assert np.array_equal(x.a, ref.jacobi(A, b, x0, k)[0])
        x = _V(x0)
        assert pkg.gauss_seidel_(x, O, _V(b), maxiter=k) is x and np.array_equal(x.a, ref.gauss_seidel(A, b, x0, k)[0])
        x = _V(x0)
        assert pkg.sor_(x, O, _V(b), 1.25, maxiter=k) is x and np.array_equal(x.a, ref.sor(A, b, x0, 1.25, k)[0])      # in place: no swap
        x = _V(x0)
        assert pkg.ssor_(x, O, _V(b), 1.25, maxiter=k) is x and np.array_equal(x.a, ref.ssor(A, b, x0, 1.25, k)[0])
    O = DoubleOperator(pkg, ref, A)                 # the default is 10 iterations from zeros
    z = np.zeros(12, dtype)
    assert np.array_equal(pkg.jacobi(O, _V(b)).a, ref.jacobi(A, b, z, 10)[0]) and O.calls == ["jacobi"] * 10
    assert np.array_equal(pkg.gauss_seidel(O, _V(b)).a, ref.gauss_seidel(A, b, z, 10)[0])
    assert np.array_equal(pkg.sor(O, _V(b), 0.7).a, ref.sor(A, b, z, 0.7, 10)[0])
    assert np.array_equal(pkg.ssor(O, _V(b), 0.7).a, ref.ssor(A, b, z, 0.7, 10)[0])


def test_iterable_protocol_fields_and_the_state_of_next_and_tmp(pkg, ref):
    A, b, x0 = _case(9, np.float64)
    O = DoubleOperator(pkg, ref, A)
    it = pkg.jacobi_iterable(_V(x0), O, _V(b), maxiter=3)
    assert isinstance(it, pkg.DenseJacobiIterable) and it.A is O and it.maxiter == 3 and it.next.n == 9
    assert it.start() == 1 and not it.done(3) and it.done(4)
    assert it.iterate() == (None, 2) and it.iterate(2) == (None, 3) and it.iterate(4) is None and O.calls == ["jacobi"] * 2
    xr, nr, _ = ref.jacobi(A, b, x0, 2)
    assert np.array_equal(it.x.a, xr) and np.array_equal(it.next.a, nr)              # next keeps the undivided values
    assert np.array_equal(it.next.a / np.diag(A), it.x.a)
    assert sum(1 for _ in it) == 3                                                   # a for loop restarts at start(): maxiter more steps
    g = pkg.gauss_seidel_iterable(_V(x0), O, _V(b), maxiter=2)
    assert isinstance(g, pkg.DenseGaussSeidelIterable) and not hasattr(g, "tmp") and sum(1 for _ in g) == 2
    for build, cls, fn in ((pkg.sor_iterable, pkg.DenseSORIterable, ref.sor), (pkg.ssor_iterable, pkg.DenseSSORIterable, ref.ssor)):
        s = build(_V(x0), O, _V(b), 1.25, maxiter=2)
        assert isinstance(s, cls) and s.omega == 1.25 and s.maxiter == 2 and s.tmp is not s.x
        assert sum(1 for _ in s) == 2
        xr, tr, _ = fn(A, b, x0, 1.25, 2)
        assert np.array_equal(s.x.a, xr) and np.array_equal(s.tmp.a, tr)
    it.b.copyto_(_V(-b))                                                            # the right-hand side is read at every step
    before = it.x.a.copy()
    it.iterate(1)
    assert np.array_equal(it.x.a, ref.jacobi(A, -b, before, 1)[0])


def test_omega_keeps_julias_types(pkg, ref):
    A, b, x0 = _case(20, np.float32)
    O = DoubleOperator(pkg, ref, A)
    expect = {1.25: np.float64, np.float64(1.25): np.float64, np.float32(0.7): np.float32, 1: np.float32, np.int64(1): np.float32}
    for omega, S in expect.items():
        x = _V(x0)
        pkg.ssor_(x, O, _V(b), omega, maxiter=2)
        assert O.scalar[1] == S and type(O.scalar[0]) is S and O.scalar[0] == S(omega), omega
        r = x0
        for _ in range(2):
            r, _t = dh.rows_forward(A, b, r, omega)
            r, _t = dh.rows_backward(A, b, r, omega)
        assert np.array_equal(x.a, r), omega
    O64 = DoubleOperator(pkg, ref, A.astype(np.float64))
    pkg.sor_(_V(x0.astype(np.float64)), O64, _V(b.astype(np.float64)), np.float32(0.7), maxiter=1)
    assert O64.scalar == (np.float64(np.float32(0.7)), np.dtype(np.float64))        # a Float32 omega on Float64 data is promoted exactly
    with pytest.raises(TypeError):
        pkg.sor_(_V(x0), O, _V(b), 1 + 2j, maxiter=1)


def test_dispatch_on_the_operator(pkg, ref, monkeypatch):
    """a HipCSR still reaches stationary.py, anything that is neither a HipCSR, a HipMatrix nor a dense operator is refused"""
    sparse, dense = pkg.stationary, pkg.stationary_dense
    seen = []
    for name in ("jacobi_iterable", "gauss_seidel_iterable", "sor_iterable", "ssor_iterable", "jacobi", "gauss_seidel", "sor", "ssor"):
        monkeypatch.setattr(sparse, name, lambda *a, _n=name, **k: seen.append((_n, a, k)) or _n)
    A = pkg.HipCSR.__new__(pkg.HipCSR)              # no device: only its type is looked at
    A.handle = None
    A.ctx = None
    x, b = object(), object()
    assert dense.jacobi_iterable(x, A, b, maxiter=4) == "jacobi_iterable" and seen[-1] == ("jacobi_iterable", (x, A, b), {"maxiter": 4})
    assert dense.gauss_seidel_iterable(x, A, b) == "gauss_seidel_iterable" and seen[-1][2] == {"maxiter": 10}
    assert dense.sor_iterable(x, A, b, 1.5, maxiter=2) == "sor_iterable" and seen[-1] == ("sor_iterable", (x, A, b, 1.5), {"maxiter": 2})
    assert dense.ssor_iterable(x, A, b, 1.5) == "ssor_iterable"
    assert pkg.jacobi(A, b, maxiter=3) == "jacobi" and seen[-1] == ("jacobi", (A, b), {"maxiter": 3})
    assert pkg.gauss_seidel(A, b) == "gauss_seidel" and pkg.sor(A, b, 0.5) == "sor" and pkg.ssor(A, b, 0.5, maxiter=1) == "ssor"
    assert pkg.jacobi_iterable is dense.jacobi_iterable and pkg.ssor_ is dense.ssor_
    assert pkg.JacobiIterable is sparse.JacobiIterable and pkg.StationaryOperator is sparse.StationaryOperator
    for bad in (np.eye(3), sp.identity(3, format="csc"), None):
        with pytest.raises(TypeError):
            pkg.jacobi(bad, _V(np.ones(3)))


def test_refusals_of_the_dense_path(pkg, ref):
    with pytest.raises(ValueError, match="DimensionMismatch"):
        DoubleOperator(pkg, ref, np.ones((3, 4)))
    M = pkg.HipMatrix.__new__(pkg.HipMatrix)        # no device: the shape is checked before anything is uploaded
    M.n, M.cols, M.dtype = 3, 4, np.dtype(np.float64)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.DenseStationaryOperator(M)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.jacobi(M, _V(np.ones(3)))
    A, b, x0 = _case(5, np.float64)
    O = DoubleOperator(pkg, ref, A)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.jacobi_(_V(np.ones(4)), O, _V(b), maxiter=1)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.sor_(_V(x0.astype(np.float32)), O, _V(b), 1.0, maxiter=1)
    Z = A.copy()
    Z[2, 2] = -0.0
    with pytest.raises(np.linalg.LinAlgError) as ei:
        DoubleOperator(pkg, ref, Z)
    assert isinstance(ei.value, pkg.SingularException) and ei.value.col == 3 and "SingularException(3)" in str(ei.value)


def test_abi_of_the_dense_entries(pkg):
    L = pkg.lib()
    assert L.mik_abi_version() == 6
    plan = pkg._lib.MikDensePlan(0, 0)
    assert [f[0] for f in plan._fields_] == ["form", "spin_limit"]
    assert (pkg._lib.MIK_DENSE_AUTO, pkg._lib.MIK_DENSE_PANEL, pkg._lib.MIK_DENSE_CHAINED) == (0, 1, 2)
    assert L.mik_dense_jacobi_step(None, None, None, None) == 1 and L.mik_dense_gs_step(None, None, None) == 1      # MIK_ERR_INVALID, no device needed
    assert L.mik_dense_sor_step(None, None, None, None, None, 0) == 1 and L.mik_dense_ssor_step(None, None, None, None, None, 0) == 1
    assert L.mik_dense_stationary_info(None, None, None, None, None, None, None) == 1
    assert L.mik_dense_stationary_destroy(None) == 0
