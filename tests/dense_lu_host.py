"""ctypes binding of tests/dense_ref/dense_lu_ref.c (the unblocked loops of lu! / ldiv! that state the bit contract of the dense LU), a
plain-numpy BLOCKED restatement of the same factorisation, the bitwise comparison `same_bits`, and the matrices of the dense LU tests --
each non-finite or scaled one with a `*_case` function that asserts, on the checker, the conditions the fixture exists for.  Test
infrastructure only."""
import ctypes as C

import numpy as np

from dense_ref_host import _p, build_ref, first_difference, same_bits  # noqa: F401

_i64p = C.POINTER(C.c_int64)


def build(outdir):
    return Ref(build_ref("dense_lu_ref", outdir))


class Ref:
    """Every method works on copies.  `ld` > n embeds A in a taller column-major array whose padding rows are NaN: they must never be read."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            getattr(lib, f"dlr_factor_{sfx}").restype = C.c_int64
            getattr(lib, f"dlr_pivots_{sfx}").restype = None
            getattr(lib, f"dlr_solve_{sfx}").restype = None

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")

    def factor(self, A, ld=None):
        """(factors n x n, ipiv 1-based int64, singular: 0 or the 1-based index of the first zero pivot column)"""
        A = np.asarray(A)
        n = A.shape[0]
        assert A.shape == (n, n) and A.dtype in (np.float64, np.float32)
        ld = n if ld is None else int(ld)
        store = np.full((ld, n), np.nan, A.dtype, order="F")
        store[:n, :] = A
        ipiv = np.zeros(n, np.int64)
        s = self._fn("dlr_factor", A.dtype)(C.c_int64(n), _p(store), C.c_int64(ld), ipiv.ctypes.data_as(_i64p))
        return np.asfortranarray(store[:n, :]), ipiv, int(s)

    def pivots(self, ipiv, x):
        x = np.array(x)
        self._fn("dlr_pivots", x.dtype)(C.c_int64(x.size), np.ascontiguousarray(ipiv, np.int64).ctypes.data_as(_i64p), _p(x))
        return x

    def solve(self, LU, ipiv, b):
        """ldiv!(F, b) from the factors: the interchanges, then both chains"""
        LU = np.asfortranarray(LU)
        x = self.pivots(ipiv, np.ascontiguousarray(b, LU.dtype))
        self._fn("dlr_solve", LU.dtype)(C.c_int64(x.size), _p(LU), C.c_int64(LU.shape[0]), _p(x))
        return x


def permutation_of(ipiv):
    """the interchanges as one gather: (P x)[i] = x[perm[i]]"""
    perm = np.arange(len(ipiv))
    for j, p in enumerate(np.asarray(ipiv) - 1):
        perm[j], perm[p] = perm[p], perm[j]
    return perm


# ---- a blocked right-looking plan in plain numpy: panels of W columns, interchanges outside the panel, strip solve, trailing update ------
def blocked(A, W):
    """(factors, ipiv 1-based) of the panel plan.  Every array operation rounds the product and the difference on their own, and every
    element still meets its k in ascending order -- so the result must equal the unblocked loop bit for bit.  FINITE data only:
    np.argmax returns the first NaN of a column, which is not the loop's rule (a NaN below the first searched row never wins there)."""
    A = np.array(A, order="F")
    n = A.shape[0]
    ipiv = np.zeros(n, np.int64)
    for k0 in range(0, n, W):
        k1 = min(k0 + W, n)
        for j in range(k0, k1):                                           # the panel: columns [k0, k1), rows [j, n)
            p = j + int(np.argmax(np.abs(A[j:, j])))                      # the first of the largest
            ipiv[j] = p + 1
            if p != j:
                A[[j, p], k0:k1] = A[[p, j], k0:k1]
            A[j + 1:, j] = A[j + 1:, j] / A[j, j]
            A[j + 1:, j + 1:k1] = A[j + 1:, j + 1:k1] - np.outer(A[j + 1:, j], A[j, j + 1:k1])
        outside = np.r_[0:k0, k1:n]
        for j in range(k0, k1):                                           # the panel's interchanges on the other columns, in order
            p = ipiv[j] - 1
            if p != j:
                A[np.ix_([j, p], outside)] = A[np.ix_([p, j], outside)]
        for k in range(k0, k1):                                           # U12 = L11^-1 A12, k ascending
            A[k + 1:k1, k1:] = A[k + 1:k1, k1:] - np.outer(A[k + 1:k1, k], A[k, k1:])
        for k in range(k0, k1):                                           # A22 -= L21 U12, k ascending
            A[k1:, k1:] = A[k1:, k1:] - np.outer(A[k1:, k], A[k, k1:])
    return A, ipiv


# ---- test matrices ----------------------------------------------------------------------------------------------------------------
def random(n, dtype, seed=0):
    """standard normal entries: a row interchange at almost every step"""
    return np.asfortranarray(np.random.default_rng(seed + 1000 * n).standard_normal((n, n)).astype(dtype))


def vector(n, dtype, seed=3):
    return np.random.default_rng(seed + 7 * n).standard_normal(n).astype(dtype)


def dominant(n, dtype, seed=0):
    """strictly diagonally dominant by COLUMNS (elimination keeps that), mixed signs: ipiv is 1..n"""
    rng = np.random.default_rng(seed + 1000 * n)
    A = rng.uniform(-1.0, 1.0, (n, n))
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, np.where(rng.random(n) < 0.5, -1.0, 1.0) * (np.abs(A).sum(axis=0) + 1.0 + rng.random(n)))
    return np.asfortranarray(A.astype(dtype))


def ties(n, dtype, rows, seed=0):
    """column 0 carries the same largest magnitude, with mixed signs, in `rows`: the first of them must win"""
    rng = np.random.default_rng(seed + 1000 * n)
    A = rng.uniform(-1.0, 1.0, (n, n))
    for q, r in enumerate(rows):
        A[r, 0] = -2.0 if q % 2 == 0 else 2.0
    return np.asfortranarray(A.astype(dtype))


def last_row(n, dtype, seed=0):
    """Every column's pivot sits in the LAST row.  Row i carries +-8 in column i + 1 and the last row in column 0, over entries of
    magnitude <= 0.1: step j brings the row with the 8 of column j up from the last position and sends row j -- whose 8 is in column
    j + 1 -- down to it."""
    rng = np.random.default_rng(seed + 1000 * n)
    A = rng.uniform(-0.1, 0.1, (n, n))
    sign = np.where(rng.random(n) < 0.5, -8.0, 8.0)
    for i in range(n):
        A[i, (i + 1) % n] = sign[i]
    return np.asfortranarray(A.astype(dtype))


def exact(n, dtype, seed=0):
    """(A, L, U, rows, x, b): A[rows[i], :] = (L U)[i, :] with unit-lower L from {0, +-1/2, +-1/4}, U integer in -3..3 above a diagonal
    from {+-4, +-8}; x integer in -4..4, b = A x.  Every intermediate of the elimination and of both substitutions is a multiple of
    1/4 far below 2^24, so it is exact in both types; every pivot is unique (|L| < 1 below the diagonal).  The interchanges must
    therefore reproduce `rows`, the factors L and U, and the solve x -- with equality."""
    rng = np.random.default_rng(seed + 1000 * n)
    L = np.tril(rng.choice([0.0, 0.5, -0.5, 0.25, -0.25], (n, n)), -1) + np.eye(n)
    U = np.triu(rng.integers(-3, 4, (n, n)).astype(np.float64), 1) + np.diag(rng.choice([4.0, -4.0, 8.0, -8.0], n))
    rows = rng.permutation(n)
    A = np.zeros((n, n))
    A[rows, :] = L @ U
    x = rng.integers(-4, 5, n).astype(np.float64)
    b = A @ x
    for M in (A, b):
        assert np.array_equal(M.astype(dtype).astype(np.float64), M)
    return np.asfortranarray(A.astype(dtype)), L.astype(dtype), U.astype(dtype), rows, x.astype(dtype), b.astype(dtype)


def zero_column(n, dtype, k, zero=0.0, seed=0):
    """standard normal with column k set to `zero` (0.0 or -0.0): the pivot column at step k is exactly zero whatever the interchanges were"""
    A = random(n, dtype, seed)
    A[:, k] = zero
    return A


# ---- non-finite, tied and scaled matrices.  Each *_case builds one, runs the checker on it and asserts what the matrix exists for; the
# ---- host tests call them at the nominal shapes, the device tests at the shapes mik_dense_lu_info reports -----------------------------
def lead(n, dtype, c, seed=0):
    """uniform(-1, 1) entries, the rows and the columns below c zeroed, 4.0 on the first c diagonal entries.  Steps 0 .. c - 1 keep the
    identity pivots and leave the trailing block as it is (multiplier 0 / 4, a - 0 * 0), so the search of column c sees exactly what a
    fixture puts there."""
    A = np.random.default_rng(seed + 1000 * n + c).uniform(-1.0, 1.0, (n, n))
    A[:c, :] = 0.0
    A[:, :c] = 0.0
    A[np.arange(c), np.arange(c)] = 4.0
    return np.asfortranarray(A.astype(dtype))


def lead_columns(W):
    """the stand-alone search, the fused search, the last column of a panel, the stand-alone search of a later panel"""
    return (0, 1, W - 1, W)


def nan_hidden_offsets(R):
    """(NaN, largest finite) as offsets from the first searched row.  In a tree that lets a lane's NaN discard what is folded into that lane,
    the NaN hides the 5.0: at lane + 2 in the first steps of the tree, at lane + R / 2 in its first step, as lane 0 of the second
    workgroup (a NaN partial).  In the last case, the control, the NaN hides nothing."""
    return ((1, 3), (R // 2 - 28, R - 28), (R, R + 2), (2, R + 2))


def nan_hidden(n, dtype, c, nan_off, max_off):
    A = lead(n, dtype, c)
    A[c + nan_off, c] = np.nan
    A[c + max_off, c] = 5.0
    return A


def nan_hidden_case(ref, dtype, c, R, nan_off, max_off):
    """(A, factors, ipiv).  The loop skips the NaN and takes the 5.0; the NaN row then stays in every later search, one lane nearer the
    front each time, until it reaches the diagonal at step c + nan_off and makes everything below it NaN."""
    n = c + 2 * R + 7
    A = nan_hidden(n, dtype, c, nan_off, max_off)
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0
    assert np.array_equal(ipiv[:c], np.arange(1, c + 1))
    assert ipiv[c] == c + max_off + 1
    finite = np.isfinite(LU).all(axis=1)
    assert finite[:c + nan_off].all() and finite.sum() >= c + nan_off
    return A, LU, ipiv


def nan_pivot(n, dtype, c, whole_column):
    """a NaN in the first searched row of column c above larger finite values in two workgroups -- or column c NaN from top to bottom"""
    A = lead(n, dtype, c)
    A[c + 3, c] = 5.0
    A[n - 2, c] = -7.0
    if whole_column:
        A[:, c] = np.nan
    else:
        A[c, c] = np.nan
    return A


def nan_pivot_case(ref, dtype, c, R, whole_column):
    """(A, factors, ipiv).  The loop starts with best = NaN, which nothing replaces: row c stays, and this is not a zero pivot.  Every
    row below becomes NaN, so the pivots are the identity from c on."""
    n = c + 2 * R + 7
    A = nan_pivot(n, dtype, c, whole_column)
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0 and ipiv[c] == c + 1 and np.array_equal(ipiv, np.arange(1, n + 1))
    return A, LU, ipiv


def inf_pair(n, dtype, R):
    A = random(n, dtype)
    A[5, 0] = np.inf
    A[R + 3, 0] = -np.inf
    return A


def inf_pair_case(ref, dtype, R):
    """(A, factors, ipiv).  The first of the equal magnitudes wins; Inf / Inf makes row R + 3 NaN, and that row waits in R + 2 further
    searches before it is the first one."""
    n = 2 * R + 7
    A = inf_pair(n, dtype, R)
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0 and ipiv[0] == 6
    nan = np.isnan(LU).any(axis=1)
    assert not nan[:R + 3].any() and nan[R + 3]
    return A, LU, ipiv


def zero_nan(n, dtype, k, nan_off, zero=0.0):
    """column k is `zero` (0.0 or -0.0) except for a NaN nan_off rows below the first searched one"""
    A = lead(n, dtype, k)
    A[:, k] = zero
    A[k + nan_off, k] = np.nan
    return A


def zero_nan_case(ref, dtype, k, n, nan_off, zero):
    """(A, factors, ipiv, the 1-based column the loop reports or 0).  best starts at 0 and a NaN never replaces it: SingularException(k + 1).
    With the NaN in the first searched row best is NaN, which is not zero, and every later pivot is NaN too: no exception."""
    A = zero_nan(n, dtype, k, nan_off, zero)
    LU, ipiv, singular = ref.factor(A)
    assert singular == (k + 1 if nan_off else 0)
    return A, LU, ipiv, singular


def late_tie_rows(c, R):
    """four different workgroups of a search whose first row is c"""
    return (c + R - 1, c + R, c + 2 * R + 3, c + 3 * R + 6)


def late_ties(n, dtype, c, rows):
    """column c carries the same largest magnitude, with alternating signs, in `rows`: the first of them must win"""
    A = lead(n, dtype, c)
    for q, r in enumerate(rows):
        A[r, c] = -2.0 if q % 2 == 0 else 2.0
    return A


def late_ties_case(ref, dtype, c, R, drop=0):
    """(A, factors, ipiv, the tied rows) with the first `drop` of the four rows left out"""
    n = c + 3 * R + 7
    rows = late_tie_rows(c, R)[drop:]
    A = late_ties(n, dtype, c, rows)
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0 and ipiv[c] == rows[0] + 1 and np.isfinite(LU).all()
    return A, LU, ipiv, rows


def scales(dtype):
    """(deep in the subnormal range for most of U, near overflow)"""
    f = np.finfo(dtype)
    return np.dtype(dtype).type(f.tiny * 2.0 ** -4), np.dtype(dtype).type(f.max / 2.0 ** 12)


def scaled(n, dtype, scale):
    A = random(n, dtype) * np.dtype(dtype).type(scale)
    assert A.dtype == np.dtype(dtype)
    return np.asfortranarray(A)


def scaled_case(ref, dtype, W, which):
    """(A, factors, ipiv) for scales(dtype)[which].  Small: the factors are finite, none is zero, the pivots are those of the unscaled
    matrix and at least a quarter of the entries are subnormal (the multipliers are not: quotients of two subnormals).  Large: finite."""
    n = 2 * W + 1
    A = scaled(n, dtype, scales(dtype)[which])
    LU, ipiv, singular = ref.factor(A)
    assert singular == 0 and np.isfinite(LU).all()
    if which == 0:
        assert (LU != 0).all() and np.array_equal(ipiv, ref.factor(random(n, dtype))[1])
        assert 4 * np.count_nonzero(np.abs(LU) < np.finfo(dtype).tiny) >= LU.size
    return A, LU, ipiv
