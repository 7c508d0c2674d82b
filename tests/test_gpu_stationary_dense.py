"""jacobi / gauss_seidel / sor / ssor on a dense device matrix (iterativesolvers.jl_amd/stationary_dense.py over the mik_dense_* entries),
bit for bit against tests/stationary_ref/stationary_dense_ref.c -- the reference's column loops restated in C.  Every comparison is
np.array_equal, for x and next / tmp, after 1 and after 3 iterations."""
import ctypes as C

import numpy as np
import pytest

import stationary_dense_host as dh

pytestmark = pytest.mark.gpu

OMEGAS = (1.25, np.float32(0.7), 1)             # Float64, Float32, Int


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("stationary_dense_ref_gpu"))


@pytest.fixture(scope="module")
def shape(pkg, ctx):
    """(W, R): the panel width and the rows per workgroup, from mik_dense_stationary_info"""
    info = pkg.DenseStationaryOperator(pkg.HipMatrix.from_numpy(np.ones((1, 1)))).info()
    assert info["W"] >= 2 and info["R"] >= 2 and info["form"] == "panel" and not info["gave_up"]
    return info["W"], info["R"]


def _vectors(n, dtype, seed=5):
    rng = np.random.default_rng(seed + n)
    return rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)


def _check(pkg, ref, A, checks=(1, 3), form="auto", omegas=OMEGAS):
    """all four methods on A from a random start: x and next / tmp after each iteration count of `checks`"""
    n, dtype = A.shape[0], A.dtype
    b, x0 = _vectors(n, dtype)
    M = pkg.HipMatrix.from_numpy(A)
    assert M.ld != n or n % 64 == 0
    O = pkg.DenseStationaryOperator(M, form=form)
    info = O.info()
    assert info["launches_forward"] == -(-n // info["W"]) and not info["gave_up"]
    V = pkg.HipVector.from_numpy
    bd = V(b)
    runs = [("jacobi", pkg.DenseJacobiIterable(O, V(x0), V(np.zeros(n, dtype)), bd, max(checks)), lambda k: ref.jacobi(A, b, x0, k)[:2]),
            ("gauss_seidel", pkg.DenseGaussSeidelIterable(O, V(x0), bd, max(checks)), lambda k: ref.gauss_seidel(A, b, x0, k)[:1])]
    for w in omegas:
        runs.append((f"sor {w!r}", pkg.DenseSORIterable(O, V(x0), V(np.zeros(n, dtype)), bd, w, max(checks)), lambda k, w=w: ref.sor(A, b, x0, w, k)[:2]))
        runs.append((f"ssor {w!r}", pkg.DenseSSORIterable(O, V(x0), V(np.zeros(n, dtype)), bd, w, max(checks)), lambda k, w=w: ref.ssor(A, b, x0, w, k)[:2]))
    out = {}
    for name, it, expect in runs:
        iteration = it.start()
        while not it.done(iteration):
            _, iteration = it.iterate(iteration)
            k = iteration - 1
            if k in checks:
                want = expect(k)
                got = [it.x.to_numpy()]
                if len(want) == 2:
                    got.append((it.next if hasattr(it, "next") else it.tmp).to_numpy())
                assert np.isfinite(want[0]).all(), (name, n, k)
                for g, wnt, what in zip(got, want, ("x", "next / tmp")):
                    assert np.array_equal(g, wnt), f"{name}: {what} differs after {k} iteration(s), n = {n}, {dtype}, first at {np.flatnonzero(g != wnt)[:4]}"
                out[(name, k)] = got
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_methods_bit_for_bit_around_the_panel_and_workgroup_sizes(pkg, ctx, ref, shape, dtype):
    W, R = shape
    for n in sorted({1, 2, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3, R - 1, R, R + 1, 2 * R + W + 1}):
        _check(pkg, ref, dh.dominant(n, dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_methods_bit_for_bit_at_2049(pkg, ctx, ref, shape, dtype):
    """several workgroups in the row-owned sweep, a one-row last panel, ld != n"""
    assert 2049 > 4 * shape[1]
    _check(pkg, ref, dh.dominant(2049, dtype))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_non_dominant_matrix_at_two_iterations(pkg, ctx, ref, shape, dtype):
    W, R = shape
    _check(pkg, ref, dh.non_dominant(2 * R + W + 1, dtype), checks=(1, 2))


def test_the_panel_form_requested_through_the_plan_equals_auto(pkg, ctx, ref, shape):
    W, R = shape
    A = dh.dominant(2 * R + W + 1, np.float64)
    a, p = _check(pkg, ref, A, form="auto", omegas=(1.25,)), _check(pkg, ref, A, form="panel", omegas=(1.25,))
    assert a.keys() == p.keys() and all(np.array_equal(u, v) for k in a for u, v in zip(a[k], p[k]))
    with pytest.raises(pkg.MikError) as ei:         # the chained form is not built: refused, never silently replaced
        pkg.DenseStationaryOperator(pkg.HipMatrix.from_numpy(A), form="chained")
    assert ei.value.code == 5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_singular_exception_with_the_one_based_index(pkg, ctx, dtype):
    n = 300
    b = pkg.HipVector.from_numpy(np.ones(n, dtype))
    for zero in (0.0, -0.0):
        for pos in (0, n // 2, n - 1):
            A = dh.dominant(n, dtype)
            A[pos, pos] = zero
            if pos < n - 1:
                A[n - 1, n - 1] = zero              # a later zero is not the one reported
            Ad = pkg.HipMatrix.from_numpy(A)
            for solver in (pkg.jacobi, pkg.gauss_seidel, lambda A, b: pkg.sor(A, b, 0.5), lambda A, b: pkg.ssor(A, b, 0.5)):
                with pytest.raises(np.linalg.LinAlgError) as ei:
                    solver(Ad, b)
                assert isinstance(ei.value, pkg.SingularException) and ei.value.col == pos + 1 and f"SingularException({pos + 1})" in str(ei.value)


def test_caller_buffers_as_views_at_a_non_zero_offset(pkg, ctx, ref, shape):
    W, R = shape
    n = 2 * R + W + 1
    for dtype in (np.float64, np.float32):
        A = dh.dominant(n, dtype)
        b, x0 = _vectors(n, dtype)
        O = pkg.DenseStationaryOperator(pkg.HipMatrix.from_numpy(A))
        big = pkg.HipVector(3 * n + 40, dtype).fill_(7)
        x, bd, tmp = big.view(3, n), big.view(n + 9, n), big.view(2 * n + 21, n)
        x.copy_from_host(x0)
        bd.copy_from_host(b)
        it = pkg.DenseSSORIterable(O, x, tmp, bd, 1.25, 3)
        assert sum(1 for _ in it) == 3
        xr, tr, _ = ref.ssor(A, b, x0, 1.25, 3)
        h = big.to_numpy()
        assert np.array_equal(h[3:3 + n], xr) and np.array_equal(h[2 * n + 21:3 * n + 21], tr) and np.array_equal(h[n + 9:2 * n + 9], b)
        untouched = np.ones(3 * n + 40, bool)
        for o in (3, n + 9, 2 * n + 21):
            untouched[o:o + n] = False
        assert (h[untouched] == 7).all()                                            # nothing was stored outside the three views
        x.copy_from_host(x0)
        nxt = tmp
        it = pkg.DenseJacobiIterable(O, x, nxt, bd, 3)
        assert sum(1 for _ in it) == 3
        xr, nr, _ = ref.jacobi(A, b, x0, 3)
        assert np.array_equal(x.to_numpy(), xr) and np.array_equal(nxt.to_numpy(), nr)
        x.copy_from_host(x0)
        assert pkg.gauss_seidel_(x, O.A, bd, maxiter=3) is x and np.array_equal(x.to_numpy(), ref.gauss_seidel(A, b, x0, 3)[0])


def test_public_names_on_a_hip_matrix_and_the_defaults(pkg, ctx, ref):
    A = dh.dominant(70, np.float64)
    b, _ = _vectors(70, np.float64)
    Ad, bd = pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b)
    z = np.zeros(70)
    assert np.array_equal(pkg.jacobi(Ad, bd).to_numpy(), ref.jacobi(A, b, z, 10)[0])
    assert np.array_equal(pkg.gauss_seidel(Ad, bd, maxiter=4).to_numpy(), ref.gauss_seidel(A, b, z, 4)[0])
    assert np.array_equal(pkg.sor(Ad, bd, 1.1).to_numpy(), ref.sor(A, b, z, 1.1, 10)[0])
    assert np.array_equal(pkg.ssor(Ad, bd, 1.1, maxiter=3).to_numpy(), ref.ssor(A, b, z, 1.1, 3)[0])
    x = pkg.HipVector.from_numpy(z)
    assert pkg.sor_(x, Ad, bd, 1.1, maxiter=3) is x                                 # in place, whatever the count (the sparse sor! swaps)


def test_refusals(pkg, ctx):
    L, lib = pkg.lib(), pkg._lib
    A = pkg.HipMatrix.from_numpy(dh.dominant(10, np.float64))
    h, col = C.c_void_p(), C.c_int64()
    for n, ld in ((10, 9), (0, 64), (-1, 64)):
        assert L.mik_dense_stationary_create(ctx.handle, C.c_void_p(A.buf.ptr), n, ld, lib.MIK_F64, None, C.byref(col), C.byref(h)) == 3
    assert L.mik_dense_stationary_create(ctx.handle, C.c_void_p(A.buf.ptr), 10, A.ld, lib.MIK_F64, None, C.byref(col), C.byref(h)) == 0    # plan may be NULL
    assert L.mik_dense_stationary_destroy(h) == 0
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.DenseStationaryOperator(pkg.HipMatrix(6, 4))
    O = pkg.DenseStationaryOperator(A)
    v = pkg.HipVector(20).fill_(0)
    with pytest.raises(pkg.MikError) as ei:
        O.sor_step_(v.view(0, 10), v.view(5, 10), pkg.HipVector(10).fill_(1), 1.0)   # x and tmp overlap
    assert ei.value.code == 1
    with pytest.raises(pkg.MikError) as ei:
        O.gs_step_(v.view(0, 10), v.view(0, 10))
    assert ei.value.code == 1
    with pytest.raises(ValueError, match="DimensionMismatch"):
        O.gs_step_(v, v.view(0, 10))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        O.gs_step_(pkg.HipVector(10, np.float32), pkg.HipVector(10))
