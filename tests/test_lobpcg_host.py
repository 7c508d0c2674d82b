"""lobpcg (src/lobpcg.jl) without a GPU: the assertions of the reference's test/lobpcg.jl on the numpy double of the device side
(tests/lobpcg_double.py), the a-priori eigenvalue bound against numpy.linalg.eigh, the refusals, and the ABI of the four block entries."""
import os
import re
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from lobpcg_double import HostJacobi, NumpyOps, block_rdiv, block_update, operator

DTYPES = [np.float64, np.float32]
SIZES = [10, 50]
ENTRIES = ("mik_spmm", "mik_block_gram", "mik_block_rdiv", "mik_block_update")


def sym(n, dt, seed):
    """test/lobpcg.jl:38-39 with numpy's generator: ``A = rand(n, n); A = A' + A + 20I``, at every n.  The symmetric part has one eigenvalue
    near n (the mean of the entries is 1) and the rest inside a semicircle of radius 2 sqrt(n / 6) (5.8 at n = 50), so the matrix is
    positive definite with its smallest eigenvalue above 10 and serves as the SPD ``B`` of the generalised cases too -- asserted here,
    because check_bound relies on it.  (A shift that grows with n would squeeze the pencil's eigenvalues closer together than the default
    tolerance of Float32 can tell apart.)"""
    R = np.random.default_rng(seed).random((n, n))
    M = R + R.T + 20 * np.eye(n)
    assert np.linalg.eigvalsh(M)[0] > 10
    return M.astype(dt)


def tol_of(pkg, dt):
    """``pkg.lobpcg`` is the function; its module carries default_tolerance (src/lobpcg.jl:751)"""
    return import_module(pkg.__name__ + ".lobpcg").default_tolerance(dt)


def run(pkg, orc, A, B, largest, *rest, **kw):
    """lobpcg on the double: A, B dense host matrices (every entry stored)"""
    ops = NumpyOps(orc, A.shape[0], A.dtype)
    Ao = operator(orc, sp.csc_matrix(A))
    args = (Ao, largest) if B is None else (Ao, operator(orc, sp.csc_matrix(B)), largest)
    kw.setdefault("maxiter", np.inf)
    return pkg.lobpcg(*args, *rest, ops=ops, **kw)


def max_err(A, B, X, lam):
    """test/lobpcg.jl:19-28: the largest column norm of A X - B X diag(lam), in the element type"""
    BX = X if B is None else B @ X
    R = A @ X - BX * lam[None, :]
    return np.max(np.sqrt(np.sum(R * R, axis=0)))


def dense_eigenvalues(A, B):
    A64 = np.asarray(A, np.float64)
    if B is None:
        return np.linalg.eigh(A64)[0]
    L = np.linalg.cholesky(np.asarray(B, np.float64))
    Li = np.linalg.inv(L)
    return np.linalg.eigh(Li @ A64 @ Li.T)[0]


def check_bound(A, B, r):
    """A Ritz pair with x'Bx = 1 and residual r = A x - lam B x has an eigenvalue within |inv(sqrt(B)) r| <= |r| / sqrt(lambda_min(B)) of lam;
    lambda_min(B) > 10 for the matrices of sym().  lam and the norm are stored in T: 4 eps |lam| for those two roundings."""
    mu = dense_eigenvalues(A, B)
    for lam, res in zip(np.asarray(r.lam, np.float64), np.asarray(r.residual_norms, np.float64)):
        assert np.min(np.abs(mu - lam)) <= res + 4 * np.finfo(A.dtype).eps * abs(lam), (lam, res)


# ---- 1: test/lobpcg.jl:32-71, :248-290 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bs", [1, 2])
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("generalized", [False, True])
def test_small_full_system(pkg, orc, dt, n, bs, largest, generalized):
    A, B = sym(n, dt, 1), (sym(n, dt, 2) if generalized else None)
    X0 = np.random.default_rng(3).random((n, bs)).astype(dt)
    tol = tol_of(pkg, dt)
    r = run(pkg, orc, A, B, largest, X0, tol=tol, log=True, rng=np.random.default_rng(4))
    X = r.X.to_numpy()
    assert r.converged and max_err(A, B, X, r.lam) <= tol
    assert r.lam is r.λ and len(r.trace) == r.iterations and r.tolerance == tol and r.maxiter == np.inf
    assert isinstance(r.trace[0], pkg.LOBPCGState) and r.trace[-1].iteration == r.iterations
    assert np.array_equal(r.trace[-1].ritz_values, r.lam) and np.array_equal(r.trace[-1].residual_norms, r.residual_norms)
    check_bound(A, B, r)
    mu = dense_eigenvalues(A, B)
    want = mu[::-1][:bs] if largest else mu[:bs]
    assert np.allclose(r.lam, want, atol=10 * tol)
    # :46-48 from the exact solution: one iteration
    r2 = run(pkg, orc, A, B, largest, X, tol=10 * tol, log=True)
    assert len(r2.trace) == 1


# ---- 2: :85-117 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("generalized", [False, True])
def test_zero_columns_of_x0_are_replaced(pkg, orc, dt, generalized):
    n = 10
    A, B = sym(n, dt, 5), (sym(n, dt, 6) if generalized else None)
    tol = tol_of(pkg, dt)
    for largest in (True, False):
        r = run(pkg, orc, A, B, largest, np.zeros((n, 1), dt), tol=tol, rng=np.random.default_rng(7))
        assert max_err(A, B, r.X.to_numpy(), r.lam) <= tol
        check_bound(A, B, r)


# ---- 3: :118-181 (no initial solution; the iterator form) and :182-212 (Jacobi) ------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("generalized", [False, True])
def test_nev_only_iterator_form_and_jacobi(pkg, orc, dt, n, generalized):
    A, B = sym(n, dt, 8), (sym(n, dt, 9) if generalized else None)
    tol = tol_of(pkg, dt)
    for largest in (True, False):
        r = run(pkg, orc, A, B, largest, 1, tol=tol, rng=np.random.default_rng(10))
        assert max_err(A, B, r.X.to_numpy(), r.lam) <= tol
        r = run(pkg, orc, A, B, largest, 1, P=HostJacobi(np.diag(A)), tol=tol, rng=np.random.default_rng(10))
        assert max_err(A, B, r.X.to_numpy(), r.lam) <= tol
        check_bound(A, B, r)
        ops = NumpyOps(orc, n, dt)
        Ao, Bo = operator(orc, sp.csc_matrix(A)), (operator(orc, sp.csc_matrix(B)) if generalized else None)
        it = pkg.LOBPCGIterator(Ao, Bo, largest, np.random.default_rng(11).random((n, 1)).astype(dt), ops=ops)
        r = pkg.lobpcg_(it, tol=tol, maxiter=np.inf, log=generalized)
        assert max_err(A, B, r.X.to_numpy(), r.lam) <= tol


# ---- 4: :213-246 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("generalized", [False, True])
def test_constraint(pkg, orc, dt, n, generalized):
    A, B = sym(n, dt, 12), (sym(n, dt, 13) if generalized else None)
    tol = tol_of(pkg, dt)
    for largest in (True, False):
        r1 = run(pkg, orc, A, B, largest, 1, tol=tol, rng=np.random.default_rng(14))
        X1 = r1.X.to_numpy()
        r2 = run(pkg, orc, A, B, largest, 1, C=X1.copy(), tol=tol, rng=np.random.default_rng(15))
        X2 = r2.X.to_numpy()
        assert max_err(A, B, X2, r2.lam) <= tol
        assert abs((X1.T @ (X2 if B is None else B @ X2))[0, 0]) <= 2 * n * tol
        mu = dense_eigenvalues(A, B)
        assert abs(r2.lam[0] - (mu[-2] if largest else mu[1])) <= 10 * tol          # the pair next to the deflated one


# ---- 5: :291-364 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("block_size", [1, 2])
@pytest.mark.parametrize("generalized", [False, True])
def test_nev_3_in_batches(pkg, orc, dt, block_size, generalized):
    n = 10
    A, B = sym(n, dt, 16), (sym(n, dt, 17) if generalized else None)
    tol = tol_of(pkg, dt)
    for largest in (True, False):
        X0 = np.random.default_rng(18).random((n, block_size)).astype(dt)
        r = run(pkg, orc, A, B, largest, X0, 3, tol=tol, log=True, rng=np.random.default_rng(19))
        X = r.X.to_numpy()
        assert X.shape == (n, 3) and len(r.lam) == 3 and np.all(r.converged)
        assert max_err(A, B, X, r.lam) <= tol
        assert np.all(np.abs(X.T @ (X if B is None else B @ X) - np.eye(3)) <= 2 * n * tol)
        assert len(r.iterations) == -(-3 // block_size) and np.all(r.iterations > 0)
        check_bound(A, B, r)
        mu = dense_eigenvalues(A, B)
        assert np.allclose(np.sort(r.lam), np.sort(mu[::-1][:3] if largest else mu[:3]), atol=10 * tol)
        # :324-363 with a constraint: the batches stay orthogonal to it
        r1 = run(pkg, orc, A, B, largest, 1, tol=tol, rng=np.random.default_rng(20))
        X1 = r1.X.to_numpy()
        nev = 2 if generalized else 3
        r2 = run(pkg, orc, A, B, largest, X0, nev, C=X1.copy(), tol=tol, log=True, rng=np.random.default_rng(21))
        X2 = r2.X.to_numpy()
        assert max_err(A, B, X2, r2.lam) <= tol
        BX2 = X2 if B is None else B @ X2
        assert np.all(np.abs(X2.T @ BX2 - np.eye(nev)) <= 2 * n * tol) and np.all(np.abs(X1.T @ BX2) <= 2 * n * tol)


# ---- 6: :72-84 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("largest", [True, False])
def test_sparse_laplacian_20x20(pkg, orc, largest):
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(20, 2, index_base=0)
    S = sp.csc_matrix((nzval, rowval, colptr), shape=(n, n))
    rhs = np.random.default_rng(22).standard_normal((n, 1))
    rhs = rhs / np.linalg.norm(rhs)
    tol = tol_of(pkg, np.float64)
    r = pkg.lobpcg(operator(orc, S), largest, rhs, tol=tol, maxiter=np.inf, ops=NumpyOps(orc, n, np.float64))
    A = S.toarray()
    assert max_err(A, None, r.X.to_numpy(), r.lam) <= tol
    check_bound(A, None, r)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_known_extreme_spectrum(pkg, orc, dt):
    """a permuted diagonal: 3 values well above and 3 well below a cluster in [1, 2)"""
    n = 60
    d = np.concatenate([[30.0, 20.0, 10.0], 1 + np.arange(n - 6) / n, [-10.0, -20.0, -30.0]])
    d = d[np.random.default_rng(23).permutation(n)].astype(dt)
    S = sp.diags(d).tocsc()
    ops = NumpyOps(orc, n, dt)
    X0 = np.random.default_rng(24).random((n, 3)).astype(dt)
    tol = tol_of(pkg, dt)
    hi = pkg.lobpcg(operator(orc, S), True, X0, tol=tol, ops=ops)
    lo = pkg.lobpcg(operator(orc, S), False, X0, tol=tol, ops=ops)
    assert hi.converged and lo.converged
    assert np.allclose(hi.lam, [30, 20, 10], atol=10 * tol) and np.allclose(lo.lam, [-30, -20, -10], atol=10 * tol)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_named_errors(pkg, orc):
    A = sym(10, np.float64, 25)
    with pytest.raises(pkg.LobpcgRefusal, match="not stable"):                    # :834
        run(pkg, orc, A, None, True, np.ones((10, 4)))
    with pytest.raises(pkg.LobpcgRefusal, match="exceeds the row dimension"):     # :833
        run(pkg, orc, A, None, True, np.ones((10, 11)))
    with pytest.raises(pkg.LobpcgRefusal, match="Number of eigenvectors"):        # :933
        run(pkg, orc, A, None, True, np.ones((10, 2)), 11)
    with pytest.raises(pkg.LobpcgRefusal, match="not stable"):                    # :934
        run(pkg, orc, A, None, True, np.ones((10, 4)), 3)
    with pytest.raises(pkg.LobpcgCholeskyError) as e:                              # B not positive definite: a MikError, not numpy's
        run(pkg, orc, A, -np.eye(10), True, np.ones((10, 1)))
    assert isinstance(e.value, pkg.MikError) and not isinstance(e.value, np.linalg.LinAlgError)
    with pytest.raises(TypeError):
        pkg.lobpcg(object(), True, 1)                                              # the device side takes HipCSR only
    assert tol_of(pkg, np.float32) == np.float32(np.finfo(np.float32).eps) ** np.float32(0.3)


# ---- 9: the definitions the double implements, against dense algebra ----------------------------------------------------------------
def test_block_definitions_agree_with_dense_algebra():
    rng = np.random.default_rng(26)
    n, sx, b1, b2 = 37, 5, 3, 2
    X, R, P, V = rng.standard_normal((n, sx)), rng.standard_normal((n, b1)), rng.standard_normal((n, b2)), rng.standard_normal((sx + b1 + b2, sx))
    xo, po = block_update(sx, b1, b2, X, R, P, V)
    assert np.allclose(po, R @ V[sx:sx + b1] + P @ V[sx + b1:]) and np.allclose(xo, X @ V[:sx] + po)
    xo, po = block_update(sx, 0, 0, X, R, P, V[:sx])
    assert po is None and np.allclose(xo, X @ V[:sx])
    U = np.triu(rng.standard_normal((sx, sx))) + 4 * np.eye(sx)
    assert np.allclose(block_rdiv(X.copy(), U), X @ np.linalg.inv(U))


# ---- 10: the operators of tests/test_gpu_lobpcg_paths.py have the properties they were built for -----------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_fixture_operators_of_the_gpu_path_tests(pkg, dt):
    """every builder of tests/lobpcg_fixtures.py asserts its own properties (tile passes, straddling rows, empty rows, thresholds, ...)"""
    import ctypes as C

    import lobpcg_fixtures as fx
    t = C.c_int()
    assert pkg.lib().mik_spmv_long_row(C.byref(t)) == 0 and t.value == 256
    for name, build in fx.SPMM_BUILDERS.items():
        S = build(dt, t.value)
        assert S.dtype == dt and S.has_sorted_indices and np.diff(S.indptr).max() <= t.value, name
    assert len(fx.SPMM_BUILDERS) == 15
    S = fx.irregular_spd(dt, t.value)
    assert S.shape == (1500, 1500) and S.dtype == dt
    assert np.linalg.eigvalsh(S.toarray().astype(np.float64))[0] > 0.5          # Gershgorin, checked


# ---- 11: ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_four_entries_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mik.h")).read()
    L = pkg.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg._lib.SIGNATURES and hasattr(L, name)
    assert L.mik_abi_version() == 6
