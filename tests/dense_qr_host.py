"""ctypes binding of tests/dense_ref/dense_qr_ref.c (the unblocked loops that state the bit contract of the dense QR: factor, tau, lmul both
ways, solve, thin Q), a plain-numpy BLOCKED restatement of the factorisation with the shape of the reduction written out, the bitwise
comparison `same_bits`, and the matrices of the dense QR tests -- each fixture with a `*_case` function that asserts, on the checker, the
condition the fixture exists for.  Test infrastructure only."""
import ctypes as C

import numpy as np

from dense_ref_host import _p, build_ref, first_difference, same_bits  # noqa: F401

DTYPES = [np.float64, np.float32]
ACC = 256                               # the accumulators of a reduction: a property of the contract, not of a launch


def build(outdir):
    return Ref(build_ref("dense_qr_ref", outdir, "-lm"))


class Ref:
    """Every method works on copies.  `ld` > m embeds A in a taller column-major array whose padding rows are NaN: they must never be read."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            getattr(lib, f"dqr_factor_{sfx}").restype = C.c_int64
            for name in ("lmul", "solve", "thin_q"):
                getattr(lib, f"dqr_{name}_{sfx}").restype = None

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")

    def factor(self, A, ld=None):
        """(factors m x n, tau, zero_diag: 0 or the 1-based index of the first R[k,k] == 0)"""
        A = np.asarray(A)
        m, n = A.shape
        assert m >= n >= 1 and A.dtype in (np.float64, np.float32)
        ld = m if ld is None else int(ld)
        store = np.full((ld, n), np.nan, A.dtype, order="F")
        store[:m, :] = A
        tau = np.zeros(n, A.dtype)
        z = self._fn("dqr_factor", A.dtype)(C.c_int64(m), C.c_int64(n), _p(store), C.c_int64(ld), _p(tau))
        return np.asfortranarray(store[:m, :]), tau, int(z)

    def lmul(self, QR, tau, y, adjoint):
        """Q y (adjoint False) or Q' y on a vector or on every column of a matrix"""
        QR = np.asfortranarray(QR)
        m, n = QR.shape
        Y = np.array(y, QR.dtype, order="F")
        assert Y.shape[0] == m
        for col in (Y.T if Y.ndim == 2 else [Y]):
            c = np.ascontiguousarray(col)
            self._fn("dqr_lmul", QR.dtype)(C.c_int64(m), C.c_int64(n), _p(QR), C.c_int64(m), _p(np.ascontiguousarray(tau, QR.dtype)), C.c_int(int(adjoint)), _p(c))
            col[...] = c
        return Y

    def solve(self, QR, tau, b):
        """F \\ b: the n values, for a vector or per column of a matrix"""
        QR = np.asfortranarray(QR)
        m, n = QR.shape
        B = np.array(b, QR.dtype, order="F")
        assert B.shape[0] == m
        out = np.zeros((n,) + B.shape[1:], QR.dtype, order="F")
        for k, col in enumerate(B.T if B.ndim == 2 else [B]):
            c, x = np.ascontiguousarray(col), np.zeros(n, QR.dtype)
            self._fn("dqr_solve", QR.dtype)(C.c_int64(m), C.c_int64(n), _p(QR), C.c_int64(m), _p(np.ascontiguousarray(tau, QR.dtype)), _p(c), _p(x))
            if B.ndim == 2:
                out[:, k] = x
            else:
                out[:] = x
        return out

    def thin_q(self, QR, tau):
        QR = np.asfortranarray(QR)
        m, n = QR.shape
        Q = np.zeros((m, n), QR.dtype, order="F")
        self._fn("dqr_thin_q", QR.dtype)(C.c_int64(m), C.c_int64(n), _p(QR), C.c_int64(m), _p(np.ascontiguousarray(tau, QR.dtype)), _p(Q), C.c_int64(m))
        return Q


def upper(QR):
    """F.R: the n x n upper triangle, +0 below the diagonal"""
    n = QR.shape[1]
    return np.asfortranarray(np.triu(QR[:n, :]))


# ---- the reduction T and a blocked right-looking plan in plain numpy ---------------------------------------------------------------------
def tree(P, lo):
    """T over the rows [lo, lo + len(P)) of the products P (rows x columns, one reduction per column).  Accumulator i mod 256 takes
    acc = acc + p_i in ascending i: the rows are laid out on their absolute indices, 256 to a line, and the lines are added one after
    another (a slot outside the range holds +0, and an accumulator, which starts at +0, is never -0: adding +0 leaves it as it is).  Then
    each group of 64 is folded by a[l] += a[l + s], s = 32 ... 1, and the four sums are added left to right."""
    P = np.asarray(P)
    rows, cols = P.shape
    lines = (lo + rows + ACC - 1) // ACC
    first = lo // ACC
    grid = np.zeros(((lines - first) * ACC, cols), P.dtype)
    grid[lo - first * ACC:lo - first * ACC + rows] = P
    acc = np.zeros((ACC, cols), P.dtype)
    for q in range(lines - first):
        acc = acc + grid[q * ACC:(q + 1) * ACC]
    a = acc.reshape(4, 64, cols).copy()
    s = 32
    while s:
        a[:, :s] = a[:, :s] + a[:, s:2 * s]
        s //= 2
    return ((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0]


def _reflect(A, j, tau, cols):
    """reflector j of A on the columns `cols` of A, in place"""
    if tau == 0 or len(cols) == 0:
        return
    v = A[j:, j].copy()
    v[0] = 1
    X = A[j:, cols]
    w = tree(v[:, None] * X, j)
    t = tau * w
    A[j:, cols] = X - v[:, None] * t[None, :]


def blocked(A, W):
    """(factors, tau, zero_diag) of the panel plan: per panel of W columns, column after column -- form the reflector, apply it to the panel's
    columns to its right -- then the panel's reflectors, in ascending order, on every column right of the panel.  An element meets its
    reflectors in the unblocked loop's order, so the result must equal it bit for bit."""
    A = np.array(A, order="F")
    m, n = A.shape
    T = A.dtype.type
    tau = np.zeros(n, A.dtype)
    with np.errstate(all="ignore"):
        for k0 in range(0, n, W):
            k1 = min(k0 + W, n)
            for j in range(k0, k1):
                alpha = A[j, j]
                s = tree((A[j + 1:, j] * A[j + 1:, j])[:, None], j + 1)[0] if j + 1 < m else T(0)
                if s == 0:
                    tau[j] = 0
                else:
                    nrm = np.sqrt(alpha * alpha + s)
                    beta = -np.copysign(nrm, alpha)
                    tau[j] = (beta - alpha) / beta
                    A[j + 1:, j] = A[j + 1:, j] / (alpha - beta)
                    A[j, j] = beta
                _reflect(A, j, tau[j], np.arange(j + 1, k1))
            for j in range(k0, k1):
                _reflect(A, j, tau[j], np.arange(k1, n))
    zeros = np.flatnonzero(np.diag(A[:n, :]) == 0)
    return A, tau, int(zeros[0]) + 1 if len(zeros) else 0


def plan_launches(n, W):
    """one launch per column, one trailing update per panel that has columns to its right"""
    return n + (n - 1) // W


# ---- test matrices ------------------------------------------------------------------------------------------------------------------------
def random(m, n, dtype, seed=0):
    return np.asfortranarray(np.random.default_rng(seed + 1000 * m + n).standard_normal((m, n)).astype(dtype))


def vector(m, dtype, seed=3):
    return np.random.default_rng(seed + 7 * m).standard_normal(m).astype(dtype)


def block(m, cols, dtype, seed=5):
    return np.asfortranarray(np.random.default_rng(seed + 7 * m + cols).standard_normal((m, cols)).astype(dtype))


def unit(dtype):
    return np.finfo(dtype).eps / 2


def zero_below(m, n, dtype, cols):
    """the columns `cols` are already zero below their diagonal when their turn comes: rows below row c are zero in column c AND in every
    column left of it that could fill it (a leading block that is upper triangular keeps what it meets untouched below its rows)"""
    A = random(m, n, dtype)
    for c in cols:
        A[c + 1:, c] = 0
    return A


def zero_below_case(ref, m, n, dtype, W):
    """(A, factors, tau): column 0 (every element of column 0 below the diagonal is zero at the first position of the first panel) gives
    tau[0] == 0 and leaves the column as it is.  A later column is zero below its diagonal only if the reflectors before it keep it so:
    columns 0 .. c all upper triangular do.  Mid-panel: c = 2; the first position of the second panel: c = W (needs n > W)."""
    cols = [c for c in range(0, 3)] + ([c for c in range(0, W + 1)] if n > W else [])
    A = zero_below(m, n, dtype, sorted(set(cols)))
    QR, tau, z = ref.factor(A)
    top = max(cols)
    assert (tau[:top + 1] == 0).all() and same_bits(QR[:, :top + 1], A[:, :top + 1])     # skipped: nothing stored, H = I
    assert (tau[top + 1:min(n, m - 1)] != 0).all() and z == 0
    return A, QR, tau


SIGNS = (("positive", 1.5, -1.0), ("negative", -1.5, 1.0), ("minus_zero", -0.0, 1.0), ("plus_zero", 0.0, -1.0))   # (name, alpha, the sign of R[0,0])


def signs(m, n, dtype, which):
    """alpha = A[0,0] positive, negative, -0.0 or +0.0 over non-zero rows below it"""
    A = random(m, n, dtype)
    A[0, 0] = SIGNS[which][1]
    return A


def signs_case(ref, m, n, dtype, which):
    """(A, factors, tau).  beta = -copysign(nrm, alpha): R[0,0] takes the sign opposite to alpha's, also where alpha is a zero, and a zero
    alpha gives tau[0] = (beta - 0) / beta = 1."""
    A = signs(m, n, dtype, which)
    QR, tau, z = ref.factor(A)
    assert z == 0 and np.isfinite(QR).all() and np.sign(QR[0, 0]) == SIGNS[which][2]
    assert tau[0] == 1 if A[0, 0] == 0 else 1 < tau[0] <= 2                 # tau = 1 - alpha / beta, and -1 <= alpha / beta < 0
    return A, QR, tau


def zero_column(m, n, dtype, k, zero=0.0):
    A = random(m, n, dtype)
    A[:, k] = zero
    return A


def zero_column_case(ref, m, n, dtype, k):
    """(A, factors, tau).  Column k stays exactly zero under every reflector (w = 0, t = 0, a - v 0 = a): R[k,k] == 0, tau[k] == 0, and
    the checker reports k + 1."""
    A = zero_column(m, n, dtype, k)
    QR, tau, z = ref.factor(A)
    assert z == k + 1 and tau[k] == 0 and (QR[:, k] == 0).all()
    return A, QR, tau


def scale_exponents(dtype):
    return (400, -400) if np.dtype(dtype) == np.float64 else (50, -50)


def scaled(m, n, dtype, k):
    A = np.ldexp(random(m, n, dtype), k)
    assert A.dtype == np.dtype(dtype)
    return np.asfortranarray(A)


def scaled_case(ref, m, n, dtype, k):
    """(A, factors, tau).  Every operation of the loops commutes with a power of two while nothing overflows or turns subnormal:
    R(2^k A) == 2^k R(A), and tau and v are the same bits."""
    A = scaled(m, n, dtype, k)
    QR, tau, z = ref.factor(A)
    QR1, tau1, z1 = ref.factor(random(m, n, dtype))
    assert z == z1 == 0 and same_bits(tau, tau1)
    assert same_bits(np.tril(QR, -1), np.tril(QR1, -1)) and same_bits(np.triu(QR), np.ldexp(np.triu(QR1), k).astype(dtype))
    return A, QR, tau


def nonfinite(m, n, dtype):
    """one NaN and one Inf, in different columns, away from the first column"""
    A = random(m, n, dtype)
    A[m - 2, 1] = np.nan
    A[min(m - 1, 3), n - 1] = np.inf
    return A


def nonfinite_case(ref, m, n, dtype):
    """(A, factors, tau).  Column 0 is finite and so are its reflector and R[0,0]; the NaN reaches everything reflector 1 touches."""
    assert n >= 3
    A = nonfinite(m, n, dtype)
    QR, tau, z = ref.factor(A)
    assert np.isfinite(QR[:, 0]).all() and np.isfinite(tau[0]) and np.isnan(tau[1]) and np.isnan(QR[1:, 1:]).all()
    return A, QR, tau
