"""lobpcg for ComplexF64 / ComplexF32 without a GPU: the C checker of the four complex block entries
(tests/complex_ref/complex_block_ref.c) against independent evaluations, the reference's complex test sets (test/lobpcg.jl:36-344 loop over
ComplexF32 and ComplexF64 too) on the complex double of the device side (tests/complex_lobpcg_host.py), the Hermitian host algebra of
lobpcg.py, and what must not change: real runs and the refusals."""
import math
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as sp

import complex_lobpcg_host as ch
from complex_host import real_of
from complex_lobpcg_host import CTYPES, bref, cref  # noqa: F401  (fixtures)


def lob(pkg):
    return import_module(pkg.__name__ + ".lobpcg")


def tol_of(pkg, T):
    return lob(pkg).default_tolerance(T)


# ---- 1: the checker against exact sums ----------------------------------------------------------------------------------------------
def exact_products(a, b):
    """a * b for two arrays of Python-float-representable numbers as lists of Python floats whose exact sum is the exact sum of the products:
    the rounded product and its error term (both doubles; float32 inputs widen exactly and their products are exact, error 0)"""
    out = []
    for x, y in zip(np.asarray(a, np.float64).tolist(), np.asarray(b, np.float64).tolist()):
        p = x * y
        out.append(p)
        e = Fraction(x) * Fraction(y) - Fraction(p)
        if e:
            ef = float(e)
            assert Fraction(ef) == e                                  # no underflow at these magnitudes: the error term is a double
            out.append(ef)
    return out


def gamma(k, T):
    u = float(np.finfo(real_of(T)).eps) / 2
    return k * u / (1 - k * u)


@pytest.mark.parametrize("T", CTYPES)
def test_checker_gram_within_the_summation_bound_of_the_exact_sum(pkg, bref, T):
    """each component within gamma_(n+1) * sum(|xr yr| + |xi yi|) (im: |xr yi| + |xi yr|) of the exact sum: two rounded products and one add
    per element give gamma_2, any summation order gamma_(n-1)"""
    rng = np.random.default_rng(1)
    shape = ch.reduce_shape(pkg, T)
    for n in (1, 700, 2 * 256 * shape[0] * shape[1] + 5):               # one thread; one ragged segment; three segments
        X, Y = ch.cwide(rng, (n, 3), T, 6), ch.cwide(rng, (n, 2), T, 6)
        G = bref.gram(X, Y, shape)
        for i in range(3):
            for j in range(2):
                xr, xi, yr, yi = X[:, i].real, X[:, i].imag, Y[:, j].real, Y[:, j].imag
                re = math.fsum(exact_products(xr, yr) + exact_products(xi, yi))
                im = math.fsum(exact_products(xr, yi) + exact_products(-xi, yr))
                mr = math.fsum(np.abs(xr.astype(np.float64) * yr).tolist() + np.abs(xi.astype(np.float64) * yi).tolist())
                mi = math.fsum(np.abs(xr.astype(np.float64) * yi).tolist() + np.abs(xi.astype(np.float64) * yr).tolist())
                assert abs(float(G[i, j].real) - re) <= gamma(n + 1, T) * mr, (n, i, j)
                assert abs(float(G[i, j].imag) - im) <= gamma(n + 1, T) * mi, (n, i, j)


@pytest.mark.parametrize("T", CTYPES)
def test_checker_spmm_rows_within_the_summation_bound_of_the_exact_sum(cref, bref, T):
    rng = np.random.default_rng(2)
    S = ch._csr_from_lengths(rng, rng.integers(0, 21, size=40), 50, T)
    A = ch.operator(cref, S)
    X = ch.cwide(rng, (50, 3), T, 6)
    Y = bref.spmm(A, X, 3)
    for r in range(40):
        cols, v = S.indices[S.indptr[r]:S.indptr[r + 1]], S.data[S.indptr[r]:S.indptr[r + 1]]
        for j in range(3):
            x = X[cols, j]
            re = math.fsum(exact_products(v.real, x.real) + exact_products(-v.imag, x.imag))
            im = math.fsum(exact_products(v.real, x.imag) + exact_products(v.imag, x.real))
            mr = math.fsum(np.abs(v.real.astype(np.float64) * x.real).tolist() + np.abs(v.imag.astype(np.float64) * x.imag).tolist())
            mi = math.fsum(np.abs(v.real.astype(np.float64) * x.imag).tolist() + np.abs(v.imag.astype(np.float64) * x.real).tolist())
            k = len(cols) + 1
            assert abs(float(Y[r, j].real) - re) <= gamma(k, T) * mr and abs(float(Y[r, j].imag) - im) <= gamma(k, T) * mi, (r, j)
            if len(cols) == 0:
                assert Y[r, j] == 0 and not np.signbit(Y[r, j].real) and not np.signbit(Y[r, j].imag)      # an empty row: (+0, +0)


# ---- 2: rdiv and update of the checker against a plain loop on (re, im) pairs ---------------------------------------------------------
def py_mul(rt, z, w):
    a, b, c, d = rt(z[0] * w[0]), rt(z[1] * w[1]), rt(z[0] * w[1]), rt(z[1] * w[0])
    return rt(a - b), rt(c + d)


def pairs(M, rt):
    return [[(rt(v.real), rt(v.imag)) for v in row] for row in np.asarray(M)]


def from_pairs(P, T):
    return np.array([[complex(float(re), float(im)) for (re, im) in row] for row in P], np.complex128).astype(T)


def py_rdiv(X, R, T):
    rt = real_of(T).type
    Xp, Rp = pairs(X, rt), pairs(R, rt)
    for row in Xp:
        for i in range(len(Rp)):
            xr, xi = row[i]
            for j in range(i):
                pr, pi = py_mul(rt, row[j], Rp[j][i])
                xr, xi = rt(xr - pr), rt(xi - pi)
            d = Rp[i][i][0]
            row[i] = (rt(xr / d), rt(xi / d))
    return from_pairs(Xp, T)


def py_rot(Wp, Fp, rt):
    out = []
    for row in Wp:
        o = []
        for jj in range(len(Fp[0])):
            acc = py_mul(rt, row[0], Fp[0][jj])
            for c in range(1, len(Fp)):
                pr, pi = py_mul(rt, row[c], Fp[c][jj])
                acc = (rt(acc[0] + pr), rt(acc[1] + pi))
            o.append(acc)
        out.append(o)
    return out


def py_add(A, B, rt):
    return [[(rt(a[0] + b[0]), rt(a[1] + b[1])) for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def py_update(sx, b1, b2, X, R, P, V, T):
    rt = real_of(T).type
    Vp = pairs(V, rt)
    po = None
    if b1:
        po = py_rot(pairs(R[:, :b1], rt), Vp[sx:sx + b1], rt)
        if b2:
            po = py_add(po, py_rot(pairs(P[:, :b2], rt), Vp[sx + b1:sx + b1 + b2], rt), rt)
    xo = py_rot(pairs(X[:, :sx], rt), Vp[:sx], rt)
    if b1:
        xo = py_add(xo, po, rt)
    return from_pairs(xo, T), (from_pairs(po, T) if b1 else None)


def upper_factor(rng, s, T):
    """upper triangular, off-diagonal magnitudes below 2, a real diagonal in 1 .. 8 of either sign; the strict lower triangle is NaN (not read)"""
    R = np.triu(ch.cwide(rng, (s, s), np.complex128, 1), 1)
    R = R + np.diag(rng.choice([-1.0, 1.0], size=s) * np.exp2(rng.uniform(0, 2, size=s)) * (1 + rng.random(s)))
    R[np.tril_indices(s, -1)] = np.nan
    return R.astype(T)


@pytest.mark.parametrize("T", CTYPES)
def test_checker_rdiv_and_update_equal_the_python_loops(bref, T):
    rng = np.random.default_rng(3)
    with np.errstate(all="ignore"):
        for s in (1, 2, 5):
            X, R = ch.cwide(rng, (7, s), T, 8), upper_factor(rng, s, T)
            got = bref.rdiv(X, R)
            assert np.all(np.isfinite(got)) and np.array_equal(got, py_rdiv(X, R, T)), s
        for (sx, b1, b2) in [(1, 0, 0), (2, 2, 0), (3, 3, 2), (5, 4, 5)]:
            X, R, P = ch.cwide(rng, (6, sx), T, 8), ch.cwide(rng, (6, max(b1, 1)), T, 8), ch.cwide(rng, (6, max(b2, 1)), T, 8)
            V = ch.cwide(rng, (sx + b1 + b2, sx), T, 8)
            xo, po = bref.update(sx, b1, b2, X, R, P, V)
            wx, wp = py_update(sx, b1, b2, X, R, P, V, T)
            assert np.array_equal(xo, wx) and (po is None) == (wp is None) and (po is None or np.array_equal(po, wp)), (sx, b1, b2)
    Rbad = upper_factor(rng, 3, T)
    Rbad[1, 1] = Rbad[1, 1] + 1j
    with pytest.raises(ValueError, match="column 1"):
        bref.rdiv(ch.cwide(rng, (4, 3), T), Rbad)
    Rz = upper_factor(rng, 3, T)
    Rz[2, 2] = complex(Rz[2, 2].real, -0.0)                              # a diagonal of -0.0 i is real
    bref.rdiv(ch.cwide(rng, (4, 3), T), Rz)


# ---- 3: the reference's complex test sets on the double -------------------------------------------------------------------------------
def residual_norm(A, B, X, lam):
    """norm(A X - X lam) of the single-pair sets (test/lobpcg.jl:44) resp. max_err, the largest column norm of A X - B X lam (:19-28; the
    block sets use it for both problems, :261, :302) -- one function: with one column they are the same number.  In complex128."""
    A, X, lam = np.asarray(A, np.complex128), np.asarray(X, np.complex128), np.asarray(lam, np.complex128)
    BX = X if B is None else np.asarray(B, np.complex128) @ X
    Rm = A @ X - BX * lam[None, :]
    return np.max(np.linalg.norm(Rm, axis=0))


def pencil_eigenvalues(A, B):
    A = np.asarray(A, np.complex128)
    if B is None:
        return np.linalg.eigvalsh(A)
    Li = np.linalg.inv(np.linalg.cholesky(np.asarray(B, np.complex128)))
    return np.linalg.eigvalsh(Li @ A @ Li.conj().T)


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("generalized", [False, True])
def test_single_eigenvalue_sets(pkg, cref, bref, T, largest, generalized):
    """test/lobpcg.jl:36-70 for a complex T: n = 10, A = A' + A + 20I stored fully, one pair from a random start, then from the solution"""
    n = 10
    A, B = ch.hermitian_dense(n, T, 1), (ch.hermitian_dense(n, T, 2) if generalized else None)
    tol = tol_of(pkg, T)
    assert isinstance(tol, real_of(T).type)
    X0 = ch.crand(np.random.default_rng(3), T, n, 1)
    r = ch.run(pkg, cref, bref, A, B, largest, X0, tol=tol, log=True, maxiter=np.inf, rng=np.random.default_rng(4))
    X = r.X.to_numpy()
    assert r.converged and residual_norm(A, B, X, r.lam) <= tol
    assert r.lam.dtype == np.dtype(T) and np.all(r.lam.imag == 0) and r.residual_norms.dtype == real_of(T)
    assert len(r.trace) == r.iterations and np.array_equal(r.trace[-1].ritz_values, r.lam)
    mu = pencil_eigenvalues(A, B)
    assert abs(r.lam[0].real - (mu[-1] if largest else mu[0])) <= 10 * tol
    r2 = ch.run(pkg, cref, bref, A, B, largest, X, tol=10 * tol, log=True, maxiter=np.inf)       # :46-48: start from the exact solution
    assert len(r2.trace) == 1


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("generalized", [False, True])
def test_zero_initial_guess_sets(pkg, cref, bref, T, generalized):
    """:87-116: a zero column of X0 is replaced by rand(T, n) -- re and im drawn"""
    n = 10
    A, B = ch.hermitian_dense(n, T, 5), (ch.hermitian_dense(n, T, 6) if generalized else None)
    tol = tol_of(pkg, T)
    for largest in (True, False):
        r = ch.run(pkg, cref, bref, A, B, largest, np.zeros((n, 1), T), tol=tol, maxiter=np.inf, rng=np.random.default_rng(7))
        assert residual_norm(A, B, r.X.to_numpy(), r.lam) <= tol
    rng = np.random.default_rng(7)
    want = (rng.random((n, 1)) + 1j * rng.random((n, 1))).astype(T)
    assert np.array_equal(lob(pkg)._rand(np.random.default_rng(7), (n, 1), T).astype(T), want) and np.any(want.imag != 0)


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("generalized", [False, True])
def test_block_set(pkg, cref, bref, T, largest, generalized):
    """nev = 2 in one block, and nev = 3 in batches of 2 (:291-322)"""
    n = 10
    A, B = ch.hermitian_dense(n, T, 8), (ch.hermitian_dense(n, T, 9) if generalized else None)
    tol = tol_of(pkg, T)
    X0 = ch.crand(np.random.default_rng(10), T, n, 2)
    r = ch.run(pkg, cref, bref, A, B, largest, X0, tol=tol, log=True, maxiter=np.inf, rng=np.random.default_rng(11))
    assert r.converged and residual_norm(A, B, r.X.to_numpy(), r.lam) <= tol
    mu = pencil_eigenvalues(A, B)
    assert np.allclose(r.lam.real, mu[::-1][:2] if largest else mu[:2], atol=10 * tol)
    r = ch.run(pkg, cref, bref, A, B, largest, X0, 3, tol=tol, log=True, maxiter=np.inf, rng=np.random.default_rng(12))
    X = r.X.to_numpy().astype(np.complex128)
    assert X.shape == (n, 3) and np.all(r.converged) and residual_norm(A, B, X, r.lam) <= tol
    BX = X if B is None else np.asarray(B, np.complex128) @ X
    assert np.all(np.abs(X.conj().T @ BX - np.eye(3)) <= 2 * n * tol)
    assert np.allclose(np.sort(r.lam.real), np.sort(mu[::-1][:3] if largest else mu[:3]), atol=10 * tol)


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("generalized", [False, True])
def test_constraint_set(pkg, cref, bref, T, generalized):
    """:213-246: the second run stays B-orthogonal to the first pair and finds the next one"""
    n = 10
    A, B = ch.hermitian_dense(n, T, 12), (ch.hermitian_dense(n, T, 13) if generalized else None)
    tol = tol_of(pkg, T)
    for largest in (True, False):
        r1 = ch.run(pkg, cref, bref, A, B, largest, 1, tol=tol, maxiter=np.inf, rng=np.random.default_rng(14))
        X1 = r1.X.to_numpy()
        r2 = ch.run(pkg, cref, bref, A, B, largest, 1, C=X1.copy(), tol=tol, maxiter=np.inf, rng=np.random.default_rng(15))
        X2 = r2.X.to_numpy().astype(np.complex128)
        assert residual_norm(A, B, X2, r2.lam) <= tol
        BX2 = X2 if B is None else np.asarray(B, np.complex128) @ X2
        assert abs((X1.astype(np.complex128).conj().T @ BX2)[0, 0]) <= 2 * n * tol
        mu = pencil_eigenvalues(A, B)
        assert abs(r2.lam[0].real - (mu[-2] if largest else mu[1])) <= 10 * tol


# ---- 4: the Hermitian host algebra ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", CTYPES)
def test_host_helpers_on_complex_input(pkg, T):
    m = lob(pkg)
    rng = np.random.default_rng(16)
    eps = np.finfo(real_of(T)).eps
    M = ch.crand(rng, np.complex128, 6, 6)
    G = (M.conj().T @ M + 6 * np.eye(6)).astype(T)
    junk = np.tril(ch.crand(rng, T, 6, 6), -1)                           # Hermitian(.) reads the upper triangle only
    H = m._hermitian(np.triu(G) + junk + 1j * np.eye(6).astype(T))      # ... and the real part of the diagonal
    assert np.array_equal(H, H.conj().T) and np.array_equal(np.triu(H, 1), np.triu(G, 1)) and np.all(np.diagonal(H).imag == 0)
    R = m._cholesky_upper(np.triu(G) + junk, "G")
    assert R.dtype == np.dtype(T) and np.array_equal(R, np.triu(R)) and np.all(np.diagonal(R).imag == 0) and np.all(np.diagonal(R).real > 0)
    assert np.abs(R.conj().T @ R - G).max() <= 50 * eps * np.abs(G).max()
    b = ch.crand(rng, T, 6, 3)
    x = m._solve_upper_t(R, b)
    assert x.dtype == np.dtype(T) and np.abs(R.conj().T @ x - b).max() <= 100 * eps * np.abs(b).max()
    y = m._solve_upper(R, b)
    assert np.abs(R @ y - b).max() <= 100 * eps * np.abs(b).max()
    with pytest.raises(m.LobpcgCholeskyError):
        m._cholesky_upper(-G, "G")


# ---- 5: what must not change ------------------------------------------------------------------------------------------------------------
def test_real_runs_are_unchanged_by_a_complex_one(pkg, orc, cref, bref):
    from lobpcg_double import NumpyOps, operator

    def real_run(dt):
        R = np.random.default_rng(20).random((10, 10))
        A = (R + R.T + 20 * np.eye(10)).astype(dt)
        X0 = np.random.default_rng(21).random((10, 2)).astype(dt)
        r = pkg.lobpcg(operator(orc, sp.csc_matrix(A)), False, X0, ops=NumpyOps(orc, 10, dt), log=True, maxiter=np.inf, rng=np.random.default_rng(22))
        return r

    before = {dt: real_run(dt) for dt in (np.float64, np.float32)}
    A = ch.hermitian_dense(10, np.complex128, 23)
    ch.run(pkg, cref, bref, A, None, False, ch.crand(np.random.default_rng(24), np.complex128, 10, 2), maxiter=np.inf)
    for dt, a in before.items():
        b = real_run(dt)
        assert a.iterations == b.iterations and len(a.trace) == len(b.trace) and a.iterations > 2
        for sa, sb in zip(a.trace, b.trace):
            assert sa.ritz_values.dtype == np.dtype(dt) and np.array_equal(sa.ritz_values, sb.ritz_values)
            assert sa.residual_norms.dtype == np.dtype(dt) and np.array_equal(sa.residual_norms, sb.residual_norms)
        assert np.array_equal(a.X.to_numpy(), b.X.to_numpy()) and a.lam.dtype == np.dtype(dt)
    # the real host algebra is the code it was: bit for bit against its former spelling
    m = lob(pkg)
    G = np.random.default_rng(25).random((5, 5))
    G = G @ G.T + 5 * np.eye(5)
    U = np.triu(G)
    assert np.array_equal(m._hermitian(G), U + np.triu(G, 1).T)
    Rf = np.ascontiguousarray(np.linalg.cholesky(U + np.triu(G, 1).T).T)
    assert np.array_equal(m._cholesky_upper(G, "G"), Rf)
    b = np.random.default_rng(26).random((5, 2))
    x = b.copy()
    for i in range(5):
        x[i] = (x[i] - Rf[:i, i] @ x[:i]) / Rf[i, i]
    assert np.array_equal(m._solve_upper_t(Rf, b), x)
    assert m.default_tolerance(np.float32) == np.float32(np.finfo(np.float32).eps) ** np.float32(0.3)


@pytest.mark.parametrize("T", CTYPES)
def test_the_unchanged_refusals(pkg, cref, T):
    """a complex HipMatrix (dense=True or not) and JacobiPrec on a complex vector are refused as before; no device is touched"""
    M = object.__new__(pkg.HipMatrix)                                    # the refusals come before anything is read from the device
    M.ctx, M.n, M.cols, M.dtype = None, 12, 12, np.dtype(T)
    with pytest.raises(TypeError, match="needs HipCSR operators"):
        pkg.lobpcg(M, False, 1)
    with pytest.raises(TypeError, match=str(np.dtype(T))):
        pkg.lobpcg(M, False, 1, dense=True)
    from complex_host import NpVector
    y = NpVector(cref, np.ones(4, T))
    with pytest.raises(TypeError, match="JacobiPrec is not offered for complex"):
        pkg.JacobiPrec(NpVector(cref, np.ones(4, T))).ldiv_(y)
