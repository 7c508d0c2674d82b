"""ctypes binding of tests/dense_ref/dense_chol_ref.c (the unblocked loops of cholesky! / ldiv! that state the bit contract of the dense
Cholesky, in all four element types), a plain-numpy BLOCKED restatement of the three-launch device plan, the bitwise comparison
`same_bits`, and the matrices of the dense Cholesky tests -- each one that exists for a condition (a failing column, a scale, a poisoned
part that must not be read) with a `*_case` function that asserts that condition on the checker first.  Test infrastructure only."""
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


def poisons(dtype):
    """what an element that must never be read is filled with: NaN, +Inf and the largest finite value (which overflows in a product and
    survives a masked sum that a NaN or an Inf would also spoil)"""
    return (np.nan, np.inf, np.finfo(real_of(dtype)).max)


def poison_of(dtype, p):
    """the element of `dtype` whose every real component is p"""
    return np.dtype(dtype).type(complex(p, p) if is_complex(dtype) else p)


def poisoned(A, p=np.nan):
    """A with its strict upper triangle p (both components in the complex types)"""
    P = np.array(A, order="F")
    P[np.triu_indices(P.shape[0], 1)] = poison_of(P.dtype, p)
    return P


def poisoned_case(ref, A, p):
    """(P, the checker's array of P): the checker's lower triangle and its solve of one b are those of the clean matrix, and the strict
    upper triangle leaves the loops as it came"""
    n = A.shape[0]
    P = poisoned(A, p)
    clean, info = ref.factor(A)
    out, info_p = ref.factor(P)
    assert info == 0 and info_p == 0 and same_bits(lower(out), lower(clean))
    iu = np.triu_indices(n, 1)
    assert same_bits(out[iu], P[iu])
    b = vector(n, A.dtype)
    assert same_bits(ref.solve(out, b), ref.solve(clean, b))
    return P, out


def imag_poisoned(A, p):
    """a complex A with the imaginary part of every diagonal entry set to p; the real parts keep their bits (assigned through .imag:
    real + 1j * nan would poison the real part too)"""
    assert is_complex(A.dtype)
    P = np.array(A, order="F")
    d = np.arange(P.shape[0])
    P.imag[d, d] = p
    assert same_bits(np.ascontiguousarray(P.real), np.ascontiguousarray(A.real))
    return P


def imag_poisoned_case(ref, A, p):
    """(P, the checker's array of the CLEAN matrix): the checker never reads the imaginary part of a diagonal entry, so its whole output
    for P -- every stored diagonal imaginary part +0 among it -- has the bits of its output for A"""
    P = imag_poisoned(A, p)
    out, info = ref.factor(A)
    got, info_p = ref.factor(P)
    assert info == 0 and info_p == 0 and same_bits(got, out)
    R = real_of(A.dtype)
    assert same_bits(np.ascontiguousarray(np.diag(got).imag), np.zeros(A.shape[0], R))
    return P, out


# ---- the widths of a last panel, the waves that report, the scales -----------------------------------------------------------------------
def width_sizes(W):
    """every n whose last panel is m = 1 .. W columns wide, alone (n = m) and behind a full panel (n = W + m), and two sizes with two
    full panels ahead: a full last panel (3 W) and a last panel of 17 columns, one past a batch of 16 (3 W + 17).  2 W is W + m at
    m = W: a full last panel behind a full one."""
    out = sorted({m for m in range(1, W + 1)} | {W + m for m in range(1, W + 1)} | {3 * W, 3 * W + 17})
    assert len(out) == 2 * W + 2 and {n % W for n in out} == set(range(W))
    return out


def report_columns(n, W):
    """Failing columns at the positions 1, 2, 3 (mod 4) of the first panel and of a later one; failure_columns(n, W) holds position 0 of
    both.  If every fourth column of a panel is handled by one of four units, each unit reports in both panels."""
    cols = (1, 2, 3, W - 1, W + 1, W + 2, W + 3, 2 * W - 1)
    assert W % 4 == 0 and cols[-1] < n - 1 and len(set(cols)) == len(cols)
    for panel in (0, 1):
        mine = {k % W % 4 for k in cols if k // W == panel}
        both = mine | {k % W % 4 for k in failure_columns(n, W) if k // W == panel}
        assert mine == {1, 2, 3} and both == {0, 1, 2, 3}
    return cols


def scales(dtype):
    """(every diagonal entry of hpd(n) * s subnormal, most entries subnormal but not the diagonal, near overflow), of the real type"""
    R = real_of(dtype)
    f = np.finfo(R)
    return R.type(f.tiny * 2.0 ** -10), R.type(f.tiny * 2.0 ** -4), R.type(f.max / 2.0 ** 12)


def _components(a):
    return np.concatenate([np.asarray(a.real).ravel(), np.asarray(a.imag).ravel()]) if is_complex(a.dtype) else np.asarray(a).ravel()


def scaled_case(ref, dtype, W, which):
    """(A, the checker's array, b, the checker's solution) for A = hpd(2 W + 1) * scales(dtype)[which] and b = vector * the same scale.
    Everywhere: the factorisation succeeds, L is finite with no zero on or below its diagonal, the solution is finite and non-zero.
    Smallest scale: every diagonal entry of A is subnormal and not zero; a pivot is at most A[j,j], so every argument of sqrt is
    subnormal.  Both small scales: at least half of the non-zero real components of A are subnormal."""
    n = 2 * W + 1
    R = real_of(dtype)
    s = scales(dtype)[which]
    tiny = np.finfo(R).tiny
    A = np.asfortranarray((hpd(n, dtype) * s).astype(dtype))
    assert A.dtype == np.dtype(dtype)
    out, info = ref.factor(A)
    il = np.tril_indices(n)
    assert info == 0 and np.isfinite(lower(out)).all() and (out[il] != 0).all()
    if which == 0:
        d = np.diag(A).real
        assert (d > 0).all() and (d < tiny).all()
        assert (np.diag(out).real <= np.sqrt(d)).all()                      # subtracting products that are >= 0 never raises d; sqrt is monotone
    if which in (0, 1):
        comp = np.abs(_components(A))
        assert 2 * np.count_nonzero((comp != 0) & (comp < tiny)) >= np.count_nonzero(comp)
    b = (vector(n, dtype) * s).astype(dtype)
    assert b.dtype == np.dtype(dtype)
    want = ref.solve(out, b)
    assert np.isfinite(want).all() and (want != 0).all()
    return A, out, b, want


def plan_launches(n, W):
    """the launches of one factorisation, restated: per panel the diagonal block, and -- with rows below it -- the panel rows and the
    trailing update"""
    return sum(1 + (2 if min(k0 + W, n) < n else 0) for k0 in range(0, n, W))


def gamma(k, dtype):
    """gamma_k = k u / (1 - k u) with the unit roundoff of the real component type"""
    u = np.finfo(real_of(dtype)).eps / 2
    assert k * u < 1
    return k * u / (1 - k * u)
