"""What tests/test_complex_lobpcg_host.py and tests/test_gpu_complex_lobpcg.py share: the ctypes binding of tests/complex_ref/complex_block_ref.c
(`BlockRef`), a complex double of ``lobpcg.DeviceOps`` whose block entries call that checker (`CNumpyOps`, with the methods of
tests/lobpcg_double.py), operator doubles on ``complex_host.NpCSR``, and the fixtures of the GPU tests -- every builder asserts the property it
was built for.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from complex_host import NpCSR, NpVector, real_of
from complex_host import build as build_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "complex_ref", "complex_block_ref.c")
_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
CTYPES = (np.complex128, np.complex64)

# constants of csrc/mik_lobpcg_complex.h the fixtures are built around (restated; the GPU tests name them where they depend on them)
CSPMM_TILE = 1024                    # MIK_CSPMM_TILE: entries of a 256-row block staged per pass, the first tile starting at the block's first entry
ROW_BLOCK = 256                      # MIK_BLOCK: rows of a row block


def build(outdir):
    """gcc -std=c99 -O2 -ffp-contract=off -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "complex_block_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    return BlockRef(C.CDLL(so))


@pytest.fixture(scope="session")
def bref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("complex_block_ref"))


@pytest.fixture(scope="session")
def cref(tmp_path_factory):
    """the vector checker of tests/complex_host.py (its own fixture is called `ref`)"""
    return build_ref(tmp_path_factory.mktemp("complex_ref_for_lobpcg"))


def _p(a):
    return a.ctypes.data_as(_vp)


def _f(a, dtype=None):
    """a column-major 2-d array of `dtype`; the leading dimension is its row count"""
    a = np.asfortranarray(a, dtype)
    assert a.ndim == 2
    return a


class BlockRef:
    """The C checker of the four block entries.  Blocks are column-major 2-d arrays (leading dimension = rows)."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("cb_spmm", "cb_gram", "cb_update"):
                getattr(lib, f"{name}_{sfx}").restype = None
            getattr(lib, f"cb_rdiv_{sfx}").restype = C.c_int

    def fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.complex128 else 'f32'}")

    def spmm(self, A, X, b, n_rows=None, long_row=256, segment=1024, group=4):
        """A: an object with rowptr / col / val (int32, int32, complex); X: n_cols x >= b -> Y: n_rows x b"""
        X = _f(X, A.val.dtype)
        Y = np.full((A.n_rows, b), np.nan, A.val.dtype, order="F")
        self.fn("cb_spmm", A.val.dtype)(_i64(A.n_rows), _p(A.rowptr), _p(A.col), _p(A.val), _int(b), _p(X), _i64(X.shape[0]), _p(Y), _i64(max(A.n_rows, 1)),
                                        _int(long_row), _int(segment), _int(group))
        return Y

    def gram(self, X, Y, shape):
        X, Y = _f(X), _f(Y, X.dtype)
        G = np.zeros((X.shape[1], Y.shape[1]), X.dtype, order="F")
        self.fn("cb_gram", X.dtype)(_i64(X.shape[0]), _int(X.shape[1]), _int(Y.shape[1]), _p(X), _i64(max(X.shape[0], 1)), _p(Y), _i64(max(Y.shape[0], 1)),
                                    _int(shape[0]), _int(shape[1]), _p(G), _i64(G.shape[0]))
        return G

    def rdiv(self, X, R):
        """X (a copy) * inv(R); ValueError naming the column when a diagonal entry of R is not real"""
        X = _f(X).copy(order="F")
        R = _f(R, X.dtype)
        rc = self.fn("cb_rdiv", X.dtype)(_i64(X.shape[0]), _int(X.shape[1]), _p(R), _i64(R.shape[0]), _p(X), _i64(max(X.shape[0], 1)))
        if rc:
            raise ValueError(f"column {rc - 1}: the diagonal of R is not real")
        return X

    def update(self, sx, b1, b2, X, R, P, V):
        """(Xout, Pout) of mik_block_update; Pout is None when b1 == 0"""
        X = _f(X)
        dt, n = X.dtype, X.shape[0]
        R = _f(R, dt) if b1 else np.zeros((n, 1), dt, order="F")
        P = _f(P, dt) if b2 else np.zeros((n, 1), dt, order="F")
        V = _f(V, dt)
        Xo, Po = np.full((n, sx), np.nan, dt, order="F"), np.full((n, sx), np.nan, dt, order="F")
        ld = _i64(max(n, 1))
        self.fn("cb_update", dt)(_i64(n), _int(sx), _int(b1), _int(b2), _p(X), ld, _p(R), ld, _p(P), ld, _p(V), _i64(V.shape[0]), _p(Xo), ld, _p(Po), ld)
        return Xo, (Po if b1 else None)


# ---------------------------------------------------------------------------------------------
# the complex double of lobpcg.DeviceOps
# ---------------------------------------------------------------------------------------------
class CMatrix:
    """n x cols column-major host block with the methods lobpcg.py uses of a HipMatrix"""

    def __init__(self, ref, n, cols, dtype):
        self.ref, self.n, self.cols, self.ld, self.dtype = ref, int(n), int(cols), int(n), np.dtype(dtype)
        self.a = np.zeros((self.n, self.cols), self.dtype, order="F")

    def col(self, j):
        return NpVector(self.ref, self.a[:, j])

    def to_numpy(self):
        return np.ascontiguousarray(self.a)


def reduce_shape(pkg, dtype):
    w, l = C.c_int(), C.c_int()
    assert pkg.lib().mik_reduce_shape(pkg._lib.dtype_code(dtype), C.byref(w), C.byref(l)) == 0
    return w.value, l.value


class CNumpyOps:
    """``ops=`` of lobpcg for a complex element type: every block entry is the C checker's, the composed statements are the vector checker's."""

    def __init__(self, pkg, ref, bref, n, dtype):
        self.ref, self.bref = ref, bref
        self.dtype, self.n = np.dtype(dtype), int(n)
        assert self.dtype.kind == "c"
        self.shape = reduce_shape(pkg, self.dtype)

    # -- storage ----------------------------------------------------------------------------------
    def matrix(self, rows, cols):
        return CMatrix(self.ref, rows, max(int(cols), 1), self.dtype)

    def upload(self, M, host, c0=0):
        host = np.asarray(host, self.dtype)
        M.a[:, c0:c0 + host.shape[1]] = host

    def download(self, M, cols):
        return M.a[:, :cols].copy()

    def copy_cols(self, dst, d0, src, s0, count):
        for j in range(count):
            dst.a[:, d0 + j] = src.a[:, s0 + j]

    # -- the four block entries -------------------------------------------------------------------
    def spmm(self, A, X, b, Y):
        Y.a[:, :b] = self.bref.spmm(A, X.a, b)

    def gram(self, X, p, Y, q, x0=0, y0=0):
        if not (p and q):
            return np.zeros((p, q), self.dtype)
        return self.bref.gram(X.a[:, x0:x0 + p], Y.a[:, y0:y0 + q], self.shape)

    def rdiv(self, X, s, R):
        X.a[:, :s] = self.bref.rdiv(X.a[:, :s], np.asarray(R, self.dtype))

    def update(self, sx, b1, b2, X, R, P, V, Xout, Pout):
        xo, po = self.bref.update(sx, b1, b2, X.a[:, :sx], R.a[:, :max(b1, 1)] if R is not None else None,
                                  P.a[:, :max(b2, 1)] if P is not None else None, np.asarray(V, self.dtype))
        Xout.a[:, :sx] = xo
        if po is not None:
            Pout.a[:, :sx] = po

    # -- composed from the vector entries ---------------------------------------------------------
    def residuals(self, AX, BX, lam, R, sx):
        rt = real_of(self.dtype)
        out = np.zeros(sx, rt)
        for j in range(sx):
            r = R.a[:, j]
            r[:] = AX.a[:, j]
            self.ref.axpy(rt.type(-np.real(lam[j])), np.ascontiguousarray(BX.a[:, j]), r)          # real x complex
            out[j] = self.ref.nrm2(r, self.shape)
        return out

    def gather_cols(self, dst, src, mask):
        k = 0
        for j in np.flatnonzero(mask):
            dst.a[:, k] = src.a[:, j]
            k += 1

    def constrain(self, X, sx, Y, sy, tmp):
        flat = Y.a.reshape(-1, order="F")                                   # the block's storage, leading dimension n (a view: Y.a is column-major)
        for j in range(sx):
            self.ref.gemv_n(flat, Y.n, sy, np.ascontiguousarray(tmp[:, j], self.dtype), -1, X.a[:, j])

    def precond(self, P, X, bs, temp):
        if P is None:
            return
        for j in range(bs):
            P.ldiv_(temp.col(j), X.col(j))
            X.a[:, j] = temp.a[:, j]


def operator(ref, M):
    """a host operator double: CSR with ascending columns (M: scipy matrix or dense array, every stored entry kept)"""
    return NpCSR(ref, M)


def full_csr(A):
    """every entry of a dense matrix stored: what a Matrix{T} of the reference's test sets becomes"""
    A = np.asarray(A)
    n, m = A.shape
    return sp.csr_matrix((A.reshape(-1).copy(), np.tile(np.arange(m), n), np.arange(n + 1) * m), shape=(n, m))


def run(pkg, ref, bref, A, B, largest, *rest, **kw):
    """lobpcg on the complex double; A, B: scipy matrices or dense arrays"""
    A = A if sp.issparse(A) else full_csr(A)
    ops = CNumpyOps(pkg, ref, bref, A.shape[0], A.dtype)
    args = (operator(ref, A), largest) if B is None else (operator(ref, A), operator(ref, B if sp.issparse(B) else full_csr(B)), largest)
    return pkg.lobpcg(*args, *rest, ops=ops, **kw)


# ---------------------------------------------------------------------------------------------
# test data
# ---------------------------------------------------------------------------------------------
def crand(rng, T, *shape):
    """rand(T, shape...): re and im uniform in [0, 1)"""
    rt = real_of(T)
    return (rng.random(shape).astype(rt) + 1j * rng.random(shape).astype(rt)).astype(T)


def cwide(rng, shape, T, span=10):
    """mixed signs, magnitudes spanning 2^-span .. 2^span in re and im: a fused multiply-add or another association changes bits"""
    def part():
        return rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-span, span, size=shape)) * (1 + rng.random(shape))
    return (part() + 1j * part()).astype(T)


def hermitian_dense(n, T, seed):
    """test/lobpcg.jl:38-39 for a complex T: ``A = rand(T, n, n); A = A' + A + 20I`` -- Hermitian, diagonal real"""
    R = crand(np.random.default_rng(seed), np.complex128, n, n)
    M = R.conj().T + R + 20 * np.eye(n)
    assert np.array_equal(M, M.conj().T) and np.linalg.eigvalsh(M)[0] > 5
    return M.astype(T)


# ---- the operators of the GPU tests ---------------------------------------------------------------------------------------------------
def _csr_from_lengths(rng, lengths, n_cols, T):
    rows = []
    for r, k in enumerate(lengths):
        rows.append(np.sort(rng.choice(n_cols, size=int(k), replace=False)))
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int64) if indptr[-1] else np.zeros(0, np.int64)
    S = sp.csr_matrix((cwide(rng, int(indptr[-1]), T), indices, indptr), shape=(len(lengths), n_cols))
    assert S.has_sorted_indices
    return S


def tile_passes(S):
    """per 256-row block: tile passes of k_cspmm (the first tile starts at the block's first entry)"""
    p = S.indptr
    return [-(-(int(p[min(r0 + ROW_BLOCK, S.shape[0])]) - int(p[r0])) // CSPMM_TILE) for r0 in range(0, S.shape[0], ROW_BLOCK)]


def straddling_rows(S):
    """rows whose entries lie in two tiles of their block"""
    p, out = S.indptr, 0
    for r in range(S.shape[0]):
        e0 = int(p[r // ROW_BLOCK * ROW_BLOCK])
        if p[r + 1] > p[r] and (int(p[r]) - e0) // CSPMM_TILE != (int(p[r + 1]) - 1 - e0) // CSPMM_TILE:
            out += 1
    return out


def spmm_ragged(T):
    """600 x 600, 1 - 60 entries a row: several tile passes per block, rows that straddle a tile boundary"""
    rng = np.random.default_rng(601)
    S = _csr_from_lengths(rng, rng.integers(1, 61, size=600), 600, T)
    assert max(tile_passes(S)) >= 3 and straddling_rows(S) >= 1
    return S


def spmm_holes(T):
    """the same with a first empty row, a last empty row and 300 consecutive empty rows that contain a whole 256-row block"""
    rng = np.random.default_rng(602)
    lengths = rng.integers(1, 61, size=600)
    lengths[0] = lengths[-1] = 0
    lengths[230:530] = 0
    S = _csr_from_lengths(rng, lengths, 600, T)
    assert tile_passes(S)[1] == 0 and max(tile_passes(S)) >= 3 and straddling_rows(S) >= 1
    assert S.indptr[1] == 0 and S.indptr[-1] == S.indptr[-2]
    return S


def spmm_rect(T):
    rng = np.random.default_rng(603)
    S = _csr_from_lengths(rng, rng.integers(0, 41, size=300), 500, T)
    assert S.shape == (300, 500) and len(tile_passes(S)) == 2
    return S


def spmm_long(T, long_row):
    """one row above the long-row threshold: mik_spmm loops mik_spmv over the columns"""
    rng = np.random.default_rng(604)
    lengths = rng.integers(1, 9, size=400)
    lengths[137] = 300
    assert lengths.max() > long_row
    return _csr_from_lengths(rng, lengths, 400, T)


def unit_diagonal(n, seed):
    return np.exp(2j * np.pi * np.random.default_rng(seed).random(n))


def hermitian_similar(Lr, T, seed):
    """H = D L D^H for a real symmetric sparse L and a unit-modulus diagonal D, formed in complex128 and rounded to T entry by entry: the
    diagonal is L's, the lower triangle the exact conjugate of the upper -- Hermitian, with L's spectrum up to the rounding of D"""
    Lr = sp.coo_matrix(Lr)
    d = unit_diagonal(Lr.shape[0], seed)
    up = Lr.row < Lr.col
    vu = (d[Lr.row[up]] * np.conj(d[Lr.col[up]]) * Lr.data[up]).astype(T)
    dg = Lr.row == Lr.col
    rows = np.concatenate([Lr.row[up], Lr.col[up], Lr.row[dg]])
    cols = np.concatenate([Lr.col[up], Lr.row[up], Lr.col[dg]])
    vals = np.concatenate([vu, np.conj(vu), Lr.data[dg].astype(T)])
    H = sp.csr_matrix((vals, (rows, cols)), shape=Lr.shape)
    H.sort_indices()
    Hd = H.toarray()
    assert H.dtype == np.dtype(T) and np.array_equal(Hd, Hd.conj().T) and H.nnz == Lr.nnz
    return H


def laplace_real(pkg, N, dims):
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(N, dims, index_base=0)
    return sp.csc_matrix((nz, rv, cp), shape=(n, n)).tocsr()


def hermitian_b(n, T, seed):
    """B = D' tridiag(-1, 4, -1) D'^H: Hermitian positive definite (strictly diagonally dominant)"""
    Br = sp.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
    return hermitian_similar(Br, T, seed)


def device_csr(pkg, ctx, S):
    S = sp.csr_matrix(S)
    S.sort_indices()
    return pkg.HipCSR(S.shape[0], S.shape[1], S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data, index_base=0, is_csc=False, ctx=ctx)
