"""ctypes binding of tests/dense_ref/dense_mul_ref.c (the chunked and the serial order of y = A x), the matrices of the dense operator
tests, and what tests/test_gpu_dense_operator.py and tests/test_gpu_dense_operator_launch.py share: the `ref` / `shape` fixtures, device
matrices in raw buffers (`Raw`), the launch-plan query, the launch arithmetic restated (`model_n` / `model_t`), the shapes that reach
the grid-stride loops (`CHUNK_STRIDE`, `BATCH_STRIDE`, `SEGMENT_STRIDE`, `streamed_shape`) and the derived error bounds.  Test
infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ladder import dot_bound

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dense_ref", "dense_mul_ref.c")

_vp = C.c_void_p


def build(outdir):
    """gcc -O2 -ffp-contract=off (no product is ever fused into a sum) -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "dense_mul_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return Ref(C.CDLL(so))


def _p(a):
    return a.ctypes.data_as(_vp)


class Ref:
    """`ld` > m embeds A in a taller column-major array whose padding rows are NaN: they must never be read."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("dmr_mul_chunked", "dmr_mul_serial"):
                getattr(lib, f"{name}_{sfx}").restype = None

    @staticmethod
    def _mat(A, ld=None):
        A = np.asarray(A)
        m, n = A.shape
        ld = max(m, 1) if ld is None else int(ld)
        store = np.full((ld, max(n, 1)), np.nan, A.dtype, order="F")
        store[:m, :n] = A
        return m, n, ld, store

    def _fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")

    def chunked(self, A, x, chunk, ld=None):
        m, n, ld, store = self._mat(A, ld)
        x = np.ascontiguousarray(x, store.dtype)
        assert x.size == n
        y = np.full(m, np.nan, store.dtype)
        self._fn("dmr_mul_chunked", store.dtype)(C.c_int64(m), C.c_int64(n), _p(store), C.c_int64(ld), _p(x), _p(y), C.c_int64(int(chunk)))
        return y

    def serial(self, A, x, ld=None):
        m, n, ld, store = self._mat(A, ld)
        x = np.ascontiguousarray(x, store.dtype)
        assert x.size == n
        y = np.full(m, np.nan, store.dtype)
        self._fn("dmr_mul_serial", store.dtype)(C.c_int64(m), C.c_int64(n), _p(store), C.c_int64(ld), _p(x), _p(y))
        return y


# ---- test matrices: seeded, no zero entries ---------------------------------------------------------------------------------------
def _nonzero(a):
    a = np.array(a)
    a[a == 0] = 0.5
    return a


def rect(m, n, dtype, seed=0):
    """m x n, mixed signs and magnitudes over several binades, no zero entries"""
    rng = np.random.default_rng(seed + 131 * m + n)
    return np.asfortranarray(_nonzero(rng.standard_normal((m, n)) * np.exp2(rng.integers(-3, 4, (m, n)))).astype(dtype))


def vec(n, dtype, seed=0):
    return _nonzero(np.random.default_rng(seed + 7 * n + 1).standard_normal(n)).astype(dtype)


def spd(n, dtype, seed=0):
    """A = R'R + I"""
    R = np.random.default_rng(seed + n).random((n, n))
    return np.asfortranarray(_nonzero(R.T @ R + np.eye(n)).astype(dtype))


def shifted(n, dtype, seed=0):
    """rand + n I: non-symmetric, well conditioned"""
    R = np.random.default_rng(seed + 3 * n).random((n, n))
    return np.asfortranarray(_nonzero(R + n * np.eye(n)).astype(dtype))


def oracle_spmv(orc, A, x):
    """the oracle's mul!(y, A::SparseMatrixCSC, x) (column scatter) on the m x n matrix A with every entry stored"""
    A = np.asarray(A)
    m, n = A.shape
    suf, ct = ("f64", C.c_double) if A.dtype == np.float64 else ("f32", C.c_float)
    cp = np.arange(0, m * n + 1, m, dtype=np.int64)
    rv = np.tile(np.arange(m, dtype=np.int64), n)
    val = np.ascontiguousarray(A.T).reshape(-1).copy()
    xa, out = np.ascontiguousarray(x, A.dtype), np.empty(m, A.dtype)
    getattr(orc.lib(), f"orc_csc_spmv_{suf}")(m, n, cp.ctypes.data_as(C.POINTER(C.c_int64)), rv.ctypes.data_as(C.POINTER(C.c_int64)),
                                             val.ctypes.data_as(C.POINTER(ct)), 0, xa.ctypes.data_as(C.POINTER(ct)), out.ctypes.data_as(C.POINTER(ct)))
    return out


# ---- shared by the GPU test modules ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dense_mul_ref"))


@pytest.fixture(scope="session")
def shape(pkg):
    c, r = C.c_int(), C.c_int()
    assert pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r)) == 0
    assert c.value in (32, 64, 128, 256) and r.value >= 64
    return c.value, r.value


def V(pkg, ctx, a):
    return pkg.HipVector.from_numpy(np.ascontiguousarray(a), ctx)


class Raw:
    """A matrix in a raw device buffer with its own mik_dense handle: leading dimension lda, the first element `off` elements into the
    allocation (off = 1: no column start is 16-byte aligned for Float64, and with an odd lda none but every fourth for Float32 -- the
    scalar-load variant).  The padding rows are NaN: they must never be read."""

    def __init__(self, pkg, ctx, A, lda, off=1):
        self.pkg, self.ctx, self.m, self.n, self.lda, self.off = pkg, ctx, A.shape[0], A.shape[1], int(lda), off
        store = np.full((self.lda, max(self.n, 1)), np.nan, A.dtype, order="F")
        store[:self.m, :self.n] = A
        self.buf = pkg.HipVector(off + store.size, A.dtype, ctx)
        self.buf.copy_from_host(np.concatenate([np.full(off, np.nan, A.dtype), store.reshape(-1, order="F")]))
        self.h = _vp()
        self.rc = pkg.lib().mik_dense_create(ctx.handle, pkg._lib.dtype_code(A.dtype), self.m, self.n, _vp(self.buf.ptr + off * A.dtype.itemsize),
                                             self.lda, C.byref(self.h))

    def narrower(self, n):
        """a second handle over the same device buffer: the first n columns (nothing is uploaded again)"""
        assert 0 <= n <= self.n
        R = Raw.__new__(Raw)
        R.pkg, R.ctx, R.m, R.n, R.lda, R.off, R.buf = self.pkg, self.ctx, self.m, int(n), self.lda, self.off, self.buf
        R.h = _vp()
        R.rc = self.pkg.lib().mik_dense_create(self.ctx.handle, self.pkg._lib.dtype_code(self.buf.dtype), R.m, R.n,
                                               _vp(self.buf.ptr + self.off * self.buf.dtype.itemsize), R.lda, C.byref(R.h))
        return R

    def col(self, j):
        return self.buf.view(self.off + j * self.lda, self.m)

    def mul(self, adjoint, x, y):
        return self.pkg.lib().mik_dense_mul(self.h, int(adjoint), _vp(x.ptr), _vp(y.ptr))

    def close(self):
        if self.h:
            self.pkg.lib().mik_dense_destroy(self.h)
            self.h = None


def matrix(pkg, ctx, A):
    """pkg.HipMatrix.from_numpy in one copy: the padding rows of the leading dimension are zero, as HipMatrix leaves them"""
    A = np.asarray(A)
    M = pkg.HipMatrix(A.shape[0], A.shape[1], A.dtype, ctx)
    M.buf.copy_from_host(padded(A, M.ld, 0).reshape(-1, order="F"))
    return M


class Out:
    """a result vector as a view into a longer buffer filled with 7, 64 elements (odd: 65 -- no 16-byte boundary) from its start; `read`
    returns the view's elements after checking that the 7s on both sides are still there"""

    def __init__(self, pkg, ctx, n, dtype, odd=False):
        self.n, self.front = int(n), 64 + int(bool(odd))
        self.buf = pkg.HipVector(self.front + self.n + 64, dtype, ctx).fill_(7)
        self.y = self.buf.view(self.front, self.n)
        assert (self.y.ptr % 16 != 0) == bool(odd)

    def read(self):
        a = self.buf.to_numpy()
        assert np.array_equal(a[:self.front], np.full(self.front, 7, a.dtype)) and np.array_equal(a[self.front + self.n:], np.full(64, 7, a.dtype))
        self.buf.fill_(7)
        return a[self.front:self.front + self.n].copy()


def at_odd_offset(pkg, ctx, a):
    """the vector a on the device, one element into its allocation: not 16-byte aligned"""
    a = np.ascontiguousarray(a)
    buf = pkg.HipVector(a.size + 1, a.dtype, ctx).fill_(7)
    v = buf.view(1, a.size)
    v.copy_from_host(a)
    assert v.ptr % 16 != 0
    return v


def plan(pkg, handle, adjoint, x, y):
    """mik_dev_dense_plan (include/mik_dev.h): the launch plan of mik_dense_mul(handle, adjoint, x, y) on the handle's context as it is now"""
    vec, streamed = C.c_int(-1), C.c_int(-1)
    gx, gy, cols, nseg = (C.c_int64(-1) for _ in range(4))
    assert pkg.lib().mik_dev_dense_plan(handle, int(adjoint), _vp(x.ptr), _vp(y.ptr), C.byref(vec), C.byref(streamed), C.byref(gx), C.byref(gy),
                                        C.byref(cols), C.byref(nseg)) == 0
    return {"vec": vec.value, "streamed": streamed.value, "gx": gx.value, "gy": gy.value, "cols": cols.value, "nseg": nseg.value}


# ---- the launch arithmetic of csrc/mik_dense_mul.hip, restated: what the CPU suite checks the shape tables against ----------------------
TCOLS = 32                          # columns per batch of the T form (MIK_DM_TCOLS; every T case asserts cols == ceil(n / TCOLS) on the plan)
STREAM_BYTES = 192.0e6              # m * n * itemsize beyond which the streamed variants run (MIK_DM_STREAM_BYTES; both sides are asserted on the plan)
SMALL_MACHINE = 8 | (1 << 16)       # MIK_KNOB_MACHINE: 8 compute units, 1 XCD -- 4 * CUs = 32 workgroups over (gx, gy), mik_max_grid = 256
SMALL_CUS = 8


def _ceil(a, b):
    return -(-a // b)


def model_n(m, n, C_, R, cus):
    nc, gx = _ceil(n, C_), _ceil(m, R)
    gy = min(nc, max(1, min(65535, 4 * cus // gx)))
    return {"gx": gx, "gy": gy, "cols": nc, "nseg": 0, "passes": _ceil(nc, gy)}


def model_t(m, n, S, cus):
    nseg, batches = _ceil(m, S), _ceil(n, TCOLS)
    gx = min(nseg, 32 * cus)
    gy = min(batches, max(1, min(65535, 4 * cus // gx)))
    return {"gx": gx, "gy": gy, "cols": batches, "nseg": nseg, "passes": _ceil(batches, gy), "segment_passes": _ceil(nseg, gx)}


def combine_trips(nc, pf=32):
    """(32-batches, 8-batches, tail) of k_dense_n_combine over the partials 1 .. nc - 1"""
    k = nc - 1
    return k // pf, k % pf // 8, k % 8


COMBINE_NC = (9, 10, 33, 41, 42)    # the 8-batch alone, 8 + tail, the 32-batch alone, 32 + 8, 32 + 8 + tail
COMBINE_TRIPS = ((0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1))


def CHUNK_STRIDE(C_, R):
    """N form planned for 8 compute units: (m, n, gx, gy, nc, passes of the chunk loop)"""
    return [(65, 33 * C_ + 3, 1, 32, 34, 2), (R + 1, 49 * C_ + 1, 2, 16, 50, 4), (33 * R + 1, 2 * C_ + 1, 34, 1, 3, 3)]


def BATCH_STRIDE(S):
    """T form planned for 8 compute units: (m, n, gx, gy, batches, passes of the batch loop)"""
    return [(S - 1, 33 * TCOLS + 5, 1, 32, 34, 2), (S + 1, 2 * 16 * TCOLS + TCOLS + 3, 2, 16, 34, 3)]


def SEGMENT_STRIDE(S):
    """T form planned for 8 compute units: (m, n, gx, gy, batches, segments, passes of the segment loop)"""
    return [((256 + 36) * S + 3, 33, 256, 1, 2, 293, 2)]


def streamed_shape(R, itemsize):
    """the smallest matrix of 2R + 1 rows that the streamed variants take: (m, n); n - 1 columns stay on the cached variants"""
    m = 2 * R + 1
    n = int(STREAM_BYTES // (m * itemsize)) + 1
    assert m * n * itemsize > STREAM_BYTES >= m * (n - 1) * itemsize
    return m, n


def launch_shapes(C_, R, S, itemsize):
    """[(direction, m, n, seed of A, seed of x)] of every grid-stride, combine and streamed case of tests/test_gpu_dense_operator_launch.py"""
    out = [("N", 65, nc * C_ - 5, nc, nc) for nc in COMBINE_NC]
    out += [("N", c[0], c[1], 10 + i, 10 + i) for i, c in enumerate(CHUNK_STRIDE(C_, R))]
    out += [("T", c[0], c[1], 20 + i, 20 + i) for i, c in enumerate(BATCH_STRIDE(S))]
    out += [("T", c[0], c[1], 22, 22) for c in SEGMENT_STRIDE(S)]
    m, n = streamed_shape(R, itemsize)
    return out + [("N", m, n, 30, 30), ("N", m, n - 1, 30, 30), ("T", m, n, 30, 31)]


# ---- data and bounds --------------------------------------------------------------------------------------------------------------
def normal(m, n, dtype, seed=0):
    """m x n in column-major order from one vectorised call, no zero entries"""
    a = np.random.default_rng(1000 + seed).standard_normal((n, m), dtype=dtype)
    a[a == 0] = 0.5
    return a.T


def padded(A, lda, fill=np.nan):
    """A inside a column-major (lda, n) array whose padding rows hold `fill`"""
    store = np.full((int(lda), A.shape[1]), fill, A.dtype, order="F")
    store[:A.shape[0]] = A
    return store


def _wide(dtype):
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def n_bound(A, x, C_):
    """(A x, bound): A x in float64 for Float32 data and in np.longdouble for Float64 data; |y - A x| <= (C + nc) eps (|A| |x|) for the chunked
    order -- a term passes through at most 1 + (C - 1) + (nc - 1) roundings of unit roundoff eps / 2, so the factor leaves a margin of 2"""
    A = np.asarray(A)
    m, n = A.shape
    w = _wide(A.dtype)
    s, a = np.zeros(m, w), np.zeros(m, w)
    for j in range(0, n, 2048):                                # column blocks: the wide copy stays small
        Ab, xb = A[:, j:j + 2048].astype(w), np.asarray(x[j:j + 2048]).astype(w)
        s += Ab @ xb
        a += np.abs(Ab) @ np.abs(xb)
    return s, (C_ + _ceil(n, C_)) * w(np.finfo(A.dtype).eps) * a


def within_n_bound(y, A, x, C_):
    s, bound = n_bound(A, x, C_)
    return bool(np.all(np.abs(y.astype(s.dtype) - s) <= bound))


def exact_cols(A, x, rows=4096):
    """(s, a, err) per column j, as np.longdouble: s = sum_i A[i, j] x[i], a = sum_i |A[i, j] x[i]|, |s - the true sum| <= err.  Float32 data:
    the float64 products are exact; Float64 data: products and sums in np.longdouble.  The sums run over blocks of `rows` rows (at most `rows`
    roundings of the accumulator's eps along any path inside a block, one more per block, one for the product), so
    err = (rows + blocks + 1) eps(accumulator) a -- the argument of ladder.exact_dot, for all columns at once."""
    A = np.asarray(A)
    m, n = A.shape
    w, ld = _wide(A.dtype), np.longdouble
    s, a = np.zeros(n, ld), np.zeros(n, ld)
    for i in range(0, m, rows):
        xb = np.asarray(x[i:i + rows]).astype(w)
        for j in range(0, n, 4096):
            Ab = A[i:i + rows, j:j + 4096].astype(w)
            s[j:j + 4096] += (xb @ Ab).astype(ld)
            a[j:j + 4096] += (np.abs(xb) @ np.abs(Ab)).astype(ld)
    k = rows + _ceil(m, rows) + 1
    a = a * (1 + 2 * k * ld(np.finfo(w).eps))                  # a itself was rounded: make it an upper bound
    return s, a, k * ld(np.finfo(w).eps) * a


def within_t_bound(y, A, x, W, L):
    """ladder.dot_bound for the segment count of these columns, every column"""
    s, a, err = exact_cols(A, x)
    nseg = _ceil(A.shape[0], 256 * W * L)
    return bool(np.all(np.abs(y.astype(np.longdouble) - s) <= dot_bound(W, L, nseg, A.dtype, a, err)))


def tree_cols(orc, A, x, W, L):
    """y[j] = the oracle's tree dot of column j with x"""
    A = np.asarray(A)
    x = np.ascontiguousarray(x)
    return np.array([orc.dot(np.ascontiguousarray(A[:, j]), x, "tree", W, L) for j in range(A.shape[1])], A.dtype)
