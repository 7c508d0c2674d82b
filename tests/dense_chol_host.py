"""ctypes binding of tests/dense_ref/dense_chol_ref.c (the unblocked loops of cholesky! / ldiv! that state the bit contract of the dense
Cholesky, in all four element types), a plain-numpy BLOCKED restatement of the three-launch device plan, the bitwise comparison
`same_bits`, and the matrices of the dense Cholesky tests -- each failing one with a function that asserts, on the checker, the
condition the fixture exists for.  Test infrastructure only."""
import ctypes as C

import numpy as np

from dense_ref_host import DTYPES, _p, build_ref, first_difference, same_bits  # noqa: F401

_SFX = {"float64": "f64", "float32": "f32", "complex128": "c64", "complex64": "c32"}


def real_of(dtype):
    return np.zeros(0, dtype).real.dtype


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def build(outdir):
    return Ref(build_ref("dense_chol_ref", outdir, "-lm"))


class Ref:
    """Every method works on copies.  `ld` > n embeds A in a taller column-major array whose padding rows are NaN: they must never be read."""

    def __init__(self, lib):
        self.L = lib
        for sfx in _SFX.values():
            getattr(lib, f"dcr_factor_{sfx}").restype = C.c_int64
            getattr(lib, f"dcr_solve_{sfx}").restype = None

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{_SFX[np.dtype(dtype).name]}")

    def factor(self, A, ld=None):
        """(the n x n array after the loops: L in its lower triangle, the strict upper triangle as it came; info: 0 or the 1-based index of
        the first column whose pivot is not positive -- the columns from there on are unspecified)"""
        A = np.asarray(A)
        n = A.shape[0]
        assert A.shape == (n, n) and A.dtype in DTYPES
        ld = n if ld is None else int(ld)
        store = np.full((ld, n), np.nan, A.dtype, order="F")
        store[:n, :] = A
        info = self._fn("dcr_factor", A.dtype)(C.c_int64(n), _p(store), C.c_int64(ld))
        return np.asfortranarray(store[:n, :]), int(info)

    def solve(self, L, b):
        """ldiv!(F, b) from the factor: both chains"""
        L = np.asfortranarray(L)
        x = np.ascontiguousarray(b, L.dtype).copy()
        self._fn("dcr_solve", L.dtype)(C.c_int64(x.size), _p(L), C.c_int64(L.shape[0]), _p(x))
        return x


def lower(M):
    """the lower triangle, the strict upper one zeroed: what a comparison of factors looks at"""
    return np.tril(np.asarray(M))


# ---- the three-launch plan in plain numpy, on separate arrays of real and imaginary parts so that every product, difference and sum is
# ---- one rounded numpy operation (numpy's own complex product makes no promise about that) -------------------------------------------
def _msub(ar, ai, zr, zi, wr, wi):
    """(ar + ai i) - (zr + zi i)(wr + wi i): four rounded products, one rounded difference, one rounded sum, two rounded subtractions"""
    p0, p1, p2, p3 = zr * wr, zi * wi, zr * wi, zi * wr
    return ar - (p0 - p1), ai - (p2 + p3)


def blocked(A, W):
    """(the array with L in its lower triangle, info) of the device plan: per panel [k0, k1) the diagonal block (right-looking inside the
    block, the diagonal treated like any other element), then L21 = A21 L11^-H row by row with k ascending and the division last, then the
    LOWER part of the trailing update with k ascending.  The strict upper triangle is never read or written.  FINITE, positive definite
    input is what the comparison with the checker is for; info is the first failing column as the device records it."""
    A = np.array(A, order="F")
    dtype = A.dtype
    n = A.shape[0]
    R = real_of(dtype)
    re, im = np.array(A.real, R, order="F"), np.array(A.imag, R, order="F")
    info = 0
    with np.errstate(all="ignore"):
        for k0 in range(0, n, W):
            k1 = min(k0 + W, n)
            for j in range(k0, k1):                                           # launch 1: the diagonal block
                d = re[j, j]
                if not d > 0 and info == 0:
                    info = j + 1
                ljj = np.sqrt(d)
                re[j, j], im[j, j] = ljj, R.type(0)
                re[j + 1:k1, j] = re[j + 1:k1, j] / ljj
                im[j + 1:k1, j] = im[j + 1:k1, j] / ljj
                for c in range(j + 1, k1):                                    # rows i >= c of column c, the diagonal among them
                    re[c:k1, c], im[c:k1, c] = _msub(re[c:k1, c], im[c:k1, c], re[c:k1, j], im[c:k1, j], re[c, j], -im[c, j])
            for c in range(k0, k1):                                           # launch 2: the rows below the block
                for k in range(k0, c):
                    re[k1:, c], im[k1:, c] = _msub(re[k1:, c], im[k1:, c], re[k1:, k], im[k1:, k], re[c, k], -im[c, k])
                re[k1:, c] = re[k1:, c] / re[c, c]
                im[k1:, c] = im[k1:, c] / re[c, c]
            for k in range(k0, k1):                                           # launch 3: the lower triangle of the trailing block
                for c in range(k1, n):
                    re[c:, c], im[c:, c] = _msub(re[c:, c], im[c:, c], re[c:, k], im[c:, k], re[c, k], -im[c, k])
    out = np.zeros((n, n), dtype, order="F")
    out.real = re
    if is_complex(dtype):
        out.imag = im
    iu = np.triu_indices(n, 1)
    out[iu] = A[iu]
    return np.asfortranarray(out), info


# ---- test matrices ----------------------------------------------------------------------------------------------------------------
def _gauss(rng, shape, dtype):
    g = rng.standard_normal(shape)
    return g + 1j * rng.standard_normal(shape) if is_complex(dtype) else g


def hpd(n, dtype, seed=0):
    """G^H G + n I in double precision, rounded to `dtype`, exactly Hermitian with a real diagonal"""
    rng = np.random.default_rng(seed + 1000 * n)
    G = _gauss(rng, (n, n), dtype)
    A = (G.conj().T @ G + n * np.eye(n)).astype(dtype)
    A = np.tril(A, -1) + np.tril(A, -1).conj().T + np.diag(np.diag(A).real).astype(dtype)
    return np.asfortranarray(A.astype(dtype))


def vector(n, dtype, seed=3):
    return _gauss(np.random.default_rng(seed + 7 * n), n, dtype).astype(dtype)


def exact(n, dtype, seed=0):
    """(A, L, x, b): L with small integer entries (Gaussian integers in the complex types) in -2..2 below a diagonal from {1, 2, 3},
    A = L L^H, x integer in -4..4 (Gaussian in the complex types), b = A x.  Every intermediate of the factorisation and of both
    substitutions is an integer far below 2^24, every pivot is the square of an integer and every quotient an integer, so everything is
    exact in all four types: the loops must return L and x with equality."""
    rng = np.random.default_rng(seed + 1000 * n)
    cx = is_complex(dtype)

    def ints(shape, lo, hi):
        v = rng.integers(lo, hi + 1, shape).astype(np.float64)
        return v + 1j * rng.integers(lo, hi + 1, shape) if cx else v
    L = np.tril(ints((n, n), -2, 2), -1) + np.diag(rng.integers(1, 4, n).astype(np.float64))
    A = L @ L.conj().T
    x = ints(n, -4, 4)
    b = A @ x
    for M in (A, b, L.conj().T @ x):
        assert np.abs(np.asarray(M).real).max() < 2 ** 24 and np.abs(np.asarray(M).imag).max() < 2 ** 24
        assert np.array_equal(M.astype(dtype).astype(np.complex128 if cx else np.float64), M)
    return np.asfortranarray(A.astype(dtype)), np.asfortranarray(L.astype(dtype)), x.astype(dtype), b.astype(dtype)


FAILURES = ("zero", "negative", "nan")


def failure_columns(n, W):
    """the first column, a mid-panel column, the first column of the second panel, the last column"""
    return (0, W // 2, W, n - 1)


def _spoil(A, L, k, kind):
    """the pivot of column k made exactly 0, negative, or NaN; the columns before k are those of the exact fixture"""
    lkk2 = (L[k, k] * L[k, k]).real
    A[k, k] = {"zero": A[k, k].real - lkk2, "negative": A[k, k].real - lkk2 - 3, "nan": np.nan}[kind]


def failing(n, dtype, k, kind, seed=0):
    """(A, later): the exact fixture with column k failing in the way `kind` names, and -- unless k is the last column -- a LATER column
    `later` that fails too (a negative pivot) and must not be the one reported (None when there is none)"""
    A, L, _, _ = exact(n, dtype, seed)
    later = None if k == n - 1 else min(n - 1, k + 5)
    _spoil(A, L, k, kind)
    if later is not None:
        _spoil(A, L, later, "negative")
    return A, later


def failing_case(ref, n, dtype, k, kind):
    """The conditions the fixture exists for, on the checker: column k is the one reported; with the defect of column k alone taken out
    the later column is reported; the zero pivot is exactly zero in integer arithmetic.  Returns (A, the checker's array, k + 1)."""
    A, later = failing(n, dtype, k, kind)
    out, info = ref.factor(A)
    assert info == k + 1, (k, kind, info)
    E, L, _, _ = exact(n, dtype)
    if later is not None:
        B = E.copy(order="F")
        _spoil(B, L, later, "negative")
        assert ref.factor(B)[1] == later + 1
    if kind == "zero":
        Li = np.asarray(L).astype(np.complex128)
        assert int(round(A[k, k].real)) - sum(int(round(abs(v) ** 2)) for v in Li[k, :k]) == 0
    assert ref.factor(E)[1] == 0
    return A, out, k + 1


def poisoned(A):
    """A with its strict upper triangle NaN (both components in the complex types)"""
    P = np.array(A, order="F")
    P[np.triu_indices(P.shape[0], 1)] = np.nan * (1 + 1j) if is_complex(P.dtype) else np.nan
    return P


def plan_launches(n, W):
    """the launches of one factorisation, restated: per panel the diagonal block, and -- with rows below it -- the panel rows and the
    trailing update"""
    return sum(1 + (2 if min(k0 + W, n) < n else 0) for k0 in range(0, n, W))


def gamma(k, dtype):
    """gamma_k = k u / (1 - k u) with the unit roundoff of the real component type"""
    u = np.finfo(real_of(dtype)).eps / 2
    assert k * u < 1
    return k * u / (1 - k * u)
