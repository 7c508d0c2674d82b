"""lobpcg on dense operators without a GPU: the reference's "Small full system" testsets (test/lobpcg.jl:34-71) on the numpy double with a
dense operator whose product is the chunked order of mik_dense_mm (tests/lobpcg_dense_double.py), one case above one chunk against
numpy.linalg.eigh, the type checks of ``lobpcg.DeviceOps`` on stand-ins of the device types, and the launch arithmetic of the block plan
restated (tests/dense_block_host.py) over the shapes of tests/test_gpu_dense_block.py."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import dense_block_host as bh
import dense_operator_host as dh
from lobpcg_dense_double import DenseOperator, device_type_doubles, separated, sym
from lobpcg_double import NumpyOps

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dense_mul_ref"))


def shapes(pkg):
    c, r = C.c_int(), C.c_int()
    assert pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r)) == 0
    return c.value, r.value, bh.block_shape(pkg)


def tol_of(pkg, dt):
    return import_module(pkg.__name__ + ".lobpcg").default_tolerance(dt)


def run(pkg, orc, ref, chunk, A, B, largest, *rest, **kw):
    ops = NumpyOps(orc, A.shape[0], A.dtype)
    Ao = DenseOperator(ref, A, chunk)
    args = (Ao, largest) if B is None else (Ao, DenseOperator(ref, B, chunk), largest)
    return pkg.lobpcg(*args, *rest, ops=ops, **kw)


def max_err(A, B, X, lam):
    """test/lobpcg.jl:19-28: the largest column norm of A X - B X diag(lam), in the element type"""
    BX = X if B is None else B @ X
    Rm = A @ X - BX * lam[None, :]
    return np.max(np.sqrt(np.sum(Rm * Rm, axis=0)))


# ---- 1: test/lobpcg.jl:34-71 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("generalized", [False, True])
def test_small_full_system_on_a_dense_operator(pkg, orc, ref, dt, largest, generalized):
    chunk = shapes(pkg)[0]
    n = 10
    A, B = sym(n, dt, 31), (sym(n, dt, 32) if generalized else None)
    b = np.random.default_rng(33).random((n, 1)).astype(dt)
    tol = tol_of(pkg, dt)
    r = run(pkg, orc, ref, chunk, A, B, largest, b, tol=tol, maxiter=200, log=generalized)
    assert r.converged and r.iterations < 200
    X = r.X.to_numpy()
    if generalized:
        assert max_err(A, B, X, r.lam) <= tol                            # :63
    else:
        assert np.linalg.norm(A @ X - X * r.lam[None, :]) <= tol         # :44
    r2 = run(pkg, orc, ref, chunk, A, B, largest, X, tol=10 * tol, log=True)      # :46-48, :65-67
    assert len(r2.trace) == 1


# ---- 2: above one chunk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("largest", [True, False])
def test_a_block_of_4_above_one_chunk_finds_the_extreme_eigenvalues(pkg, orc, ref, dt, largest):
    chunk = shapes(pkg)[0]
    n = 3 * chunk + 5
    A = separated(n, dt, 34)
    X0 = np.random.default_rng(35).random((n, 4)).astype(dt)
    tol = tol_of(pkg, dt)
    r = run(pkg, orc, ref, chunk, A, None, largest, X0, tol=tol, maxiter=200)
    assert r.converged and max_err(A, None, r.X.to_numpy(), r.lam) <= tol
    mu = np.linalg.eigh(A.astype(np.float64))[0]
    want = mu[::-1][:4] if largest else mu[:4]
    assert np.allclose(r.lam, want, atol=10 * tol)                        # the comparison of tests/test_lobpcg_host.py


# ---- 3: DeviceOps takes HipCSR and HipMatrix, each for A and for B -----------------------------------------------------------------------
def test_device_ops_with_dense_accepts_dense_and_sparse_operators_and_refuses_the_rest(pkg):
    DeviceOps = import_module(pkg.__name__ + ".lobpcg").DeviceOps
    Dense, CSR = device_type_doubles(pkg)
    f64, f32 = np.float64, np.float32
    for A, B in ((Dense(10, 10, f64), None), (Dense(10, 10, f32), Dense(10, 10, f32)), (Dense(10, 10, f64), CSR(10, 10, f64)),
                 (CSR(10, 10, f64), Dense(10, 10, f64)), (CSR(10, 10, f32), None)):
        ops = DeviceOps(A, B, dense=True)
        assert (ops.n, ops.dtype) == (10, np.dtype(A.dtype))
        for M in (A, B):
            if isinstance(M, Dense):
                assert M.reserved == 1                                    # the block workspace is allocated when the iterator is built
    for A, B in ((Dense(10, 9, f64), None), (Dense(10, 10, f64), Dense(10, 9, f64)), (Dense(10, 10, f64), Dense(11, 11, f64)),
                 (Dense(10, 10, f64), Dense(10, 10, f32)), (Dense(10, 10, f64), CSR(10, 10, f32)), (CSR(10, 10, f32), Dense(10, 10, f64))):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            DeviceOps(A, B, dense=True)
        assert all(M.reserved == 0 for M in (A, B) if isinstance(M, Dense))      # refused before anything is allocated
    for A, B in ((lambda y, x: y, None), (Dense(10, 10, f64), lambda y, x: y), (None, None), (np.eye(10), None)):
        with pytest.raises(TypeError, match="HipCSR.*callbacks are not supported"):
            DeviceOps(A, B, dense=True)
        if not isinstance(A, Dense):
            with pytest.raises(TypeError, match="HipCSR.*callbacks are not supported"):
                DeviceOps(A, B)
    # the dense route is asked for: without the keyword a HipMatrix is refused as it was before, for A and for B, and nothing is allocated
    for A, B in ((Dense(10, 10, f64), None), (CSR(10, 10, f64), Dense(10, 10, f64)), (Dense(10, 10, f64), Dense(10, 10, f64))):
        with pytest.raises(TypeError, match="HipCSR.*dense=True"):
            DeviceOps(A, B)
        assert all(M.reserved == 0 for M in (A, B) if isinstance(M, Dense))
    assert DeviceOps(CSR(10, 10, f64), CSR(10, 10, f64)).n == 10


# ---- 4: the launch plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_block_plan_of_every_gpu_shape(pkg, dt):
    C_, R, GW = shapes(pkg)
    assert GW >= 2 and bh.B_MAX % GW == 0 and 1 <= bh.GW_MIN <= GW
    sub = lambda d, keys: tuple(d[k] for k in keys)
    for m, n, b in bh.block_shapes(C_, R, GW, np.dtype(dt).itemsize):
        for wmin in (1, bh.GW_MIN, GW):
            for cus in (dh.SMALL_CUS, 256):
                p, v = bh.model_nb(m, n, b, C_, R, GW, cus, wmin), dh.model_n(m, n, C_, R, cus)
                assert p["groups"] * GW - (GW - p["last_w"] if p["groups"] else 0) + p["vector_cols"] == b      # every column once
                assert p["vector_cols"] < wmin and (p["groups"] == 0 or wmin <= p["last_w"] <= GW)
                assert sub(p, ("gx", "gy", "chunks", "passes")) == sub(v, ("gx", "gy", "cols", "passes"))        # the grid of the vector form
    key = ("groups", "last_w", "vector_cols")
    assert [sub(bh.model_nb(65, 65, b, C_, R, 8, 256, 1), key) for b in (1, 7, 8, 9, 16, 31, 32)] == \
        [(1, 1, 0), (1, 7, 0), (1, 8, 0), (2, 1, 0), (2, 8, 0), (4, 7, 0), (4, 8, 0)]
    assert [sub(bh.model_nb(65, 65, b, C_, R, 8, 256, 2), key) for b in (1, 2, 9, 10)] == [(0, 0, 1), (1, 2, 0), (1, 8, 1), (2, 2, 0)]
    for m, n, gx, gy, nc, passes in dh.CHUNK_STRIDE(C_, R):               # two groups, each walking the chunk loop 2 - 4 times
        p = bh.model_nb(m, n, GW + 1, C_, R, GW, dh.SMALL_CUS, 1)
        assert sub(p, ("groups", "last_w", "gx", "gy", "chunks", "passes")) == (2, 1, gx, gy, nc, passes) and passes >= 2
    for nc in dh.COMBINE_NC:
        assert sub(bh.model_nb(65, nc * C_ - 5, 3, C_, R, GW, 11), ("groups", "last_w", "gy", "chunks", "passes")) == (1, 3, nc, nc, 1)
    assert bh.model_nb(0, 5, 3, C_, R, GW, 256)["groups"] == 0 and bh.model_nb(5, 0, 3, C_, R, GW, 256)["chunks"] == 0
