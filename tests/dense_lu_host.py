"""ctypes binding of tests/dense_ref/dense_lu_ref.c (the unblocked loops of lu! / ldiv! that state the bit contract of the dense LU), a
plain-numpy BLOCKED restatement of the same factorisation, and the matrices of the dense LU tests.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dense_ref", "dense_lu_ref.c")

_vp = C.c_void_p
_i64p = C.POINTER(C.c_int64)


def build(outdir):
    """gcc -O2 -ffp-contract=off (no product is ever fused into a difference) -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "dense_lu_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return Ref(C.CDLL(so))


def _p(a):
    return a.ctypes.data_as(_vp)


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
    element still meets its k in ascending order -- so the result must equal the unblocked loop bit for bit."""
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
