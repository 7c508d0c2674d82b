"""What tests/test_complex_host.py and tests/test_gpu_complex.py share: the ctypes binding of tests/complex_ref/complex_ref.c (`Ref`), a
numpy double of the device types whose L1 / L2 operations call that checker (`NpVector`, `NpMatrix`, `NpCSR`, `HostOps`), two backends
that build vectors / operators for the same scenario code (`HostBackend`, `DeviceBackend`), and the complex test sets of the reference
(test/cg.jl:27-47,99-121, test/gmres.jl:16-57,76-98) written once over a backend.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "complex_ref", "complex_ref.c")
_vp = C.c_void_p
_i64 = C.c_int64

CTYPES = (np.complex64, np.complex128)


def real_of(dtype):
    return np.dtype(np.dtype(dtype).type(0).real.dtype)


def build(outdir):
    """gcc -std=c99 -O2 -ffp-contract=off -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "complex_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so, "-lm"])
    return Ref(C.CDLL(so))


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("complex_ref"))


def _p(a):
    return a.ctypes.data_as(_vp)


def _c(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a


class Ref:
    """The C checker.  Complex arrays go in as they are (interleaved re, im); `shape` = (W, L) of mik_reduce_shape."""

    def __init__(self, lib):
        self.L = lib
        for sfx, ct in (("f64", C.c_double), ("f32", C.c_float)):
            for name in ("cr_dot", "cr_axpy", "cr_xpby", "cr_scal", "cr_raxpy", "cr_rxpby", "cr_rscal", "cr_sub", "cr_spmv", "cr_gemv_n"):
                getattr(lib, f"{name}_{sfx}").restype = None
            getattr(lib, f"cr_nrm2_{sfx}").restype = ct
            getattr(lib, f"cr_mgs_{sfx}").restype = ct
            getattr(lib, f"cr_raxpy_{sfx}").argtypes = [_i64, ct, _vp, _vp]
            getattr(lib, f"cr_rxpby_{sfx}").argtypes = [_i64, _vp, ct, _vp]
            getattr(lib, f"cr_rscal_{sfx}").argtypes = [_i64, ct, _vp]

    def fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.complex128 else 'f32'}")

    # every method works in place on the arrays it is given (contiguous, of `dtype`)
    def dot(self, x, y, shape):
        out = np.zeros(1, x.dtype)
        self.fn("cr_dot", x.dtype)(_i64(x.size), _p(x), _p(y), C.c_int(shape[0]), C.c_int(shape[1]), _p(out))
        return out[0]

    def nrm2(self, x, shape):
        return real_of(x.dtype).type(self.fn("cr_nrm2", x.dtype)(_i64(x.size), _p(x), C.c_int(shape[0]), C.c_int(shape[1])))

    def axpy(self, alpha, x, y):
        if np.iscomplexobj(alpha):
            self.fn("cr_axpy", y.dtype)(_i64(y.size), _p(np.asarray([alpha], y.dtype)), _p(x), _p(y))
        else:
            self.fn("cr_raxpy", y.dtype)(_i64(y.size), real_of(y.dtype).type(alpha), _p(x), _p(y))

    def xpby(self, x, beta, y):
        if np.iscomplexobj(beta):
            self.fn("cr_xpby", y.dtype)(_i64(y.size), _p(x), _p(np.asarray([beta], y.dtype)), _p(y))
        else:
            self.fn("cr_rxpby", y.dtype)(_i64(y.size), _p(x), real_of(y.dtype).type(beta), _p(y))

    def scal(self, alpha, x):
        if np.iscomplexobj(alpha):
            self.fn("cr_scal", x.dtype)(_i64(x.size), _p(np.asarray([alpha], x.dtype)), _p(x))
        else:
            self.fn("cr_rscal", x.dtype)(_i64(x.size), real_of(x.dtype).type(alpha), _p(x))

    def sub(self, x, y):
        self.fn("cr_sub", y.dtype)(_i64(y.size), _p(x), _p(y))

    def spmv(self, rowptr, col, val, x, n_rows, long_row=256, segment=1024, group=4):
        y = np.full(n_rows, np.nan, val.dtype)
        self.fn("cr_spmv", val.dtype)(_i64(n_rows), _p(rowptr), _p(col), _p(val), _p(x), _p(y), C.c_int(long_row), C.c_int(segment), C.c_int(group))
        return y

    def mgs(self, V, ld, k, w, shape):
        """V: the basis storage (ld x cols, column-major, flat); w is orthogonalised in place -> (h, nrm)"""
        h = np.zeros(max(k, 1), w.dtype)
        nrm = self.fn("cr_mgs", w.dtype)(_i64(w.size), C.c_int(k), _p(V), _i64(ld), _p(w), _p(h), C.c_int(shape[0]), C.c_int(shape[1]))
        return h[:k], real_of(w.dtype).type(nrm)

    def gemv_n(self, V, ld, k, c, alpha, y):
        self.fn("cr_gemv_n", y.dtype)(_i64(y.size), C.c_int(k), _p(V), _i64(ld), _p(_c(c[:k], y.dtype)), _p(np.asarray([alpha], y.dtype)), _p(y))


# ---------------------------------------------------------------------------------------------
# numpy double of HipVector / HipMatrix / HipCSR: same methods, the arithmetic is the C checker's
# ---------------------------------------------------------------------------------------------
class NpVector:
    def __init__(self, ref, a):
        self.ref, self.a = ref, a                    # `a`: a contiguous 1-d array (possibly a view into a matrix)
        self.n, self.dtype = a.size, a.dtype

    def similar(self):
        return NpVector(self.ref, np.full(self.n, np.nan, self.dtype))

    def zero(self):
        return NpVector(self.ref, np.zeros(self.n, self.dtype))

    def copy(self):
        return NpVector(self.ref, self.a.copy())

    def to_numpy(self):
        return self.a.copy()

    def copy_from_host(self, h):
        self.a[:] = np.asarray(h, self.dtype)
        return self

    def fill_(self, v):
        self.a[:] = self.dtype.type(v)
        return self

    def copyto_(self, src):
        self.a[:] = src.a
        return self

    def axpy_(self, alpha, x):
        self.ref.axpy(alpha, x.a, self.a)
        return self

    def xpby_(self, x, beta):
        self.ref.xpby(x.a, beta, self.a)
        return self

    def sub_(self, x):
        self.ref.sub(x.a, self.a)
        return self

    def scal_(self, alpha):
        self.ref.scal(alpha, self.a)
        return self


class NpMatrix:
    def __init__(self, ref, n, cols, dtype):
        self.ref, self.n, self.cols, self.dtype = ref, n, cols, np.dtype(dtype)
        self.ld = (n + 63) // 64 * 64 or 64
        self.store = np.zeros(self.ld * cols, dtype)

    def col(self, j):
        return NpVector(self.ref, self.store[j * self.ld: j * self.ld + self.n])


class NpCSR:
    """a fully stored or sparse matrix as 0-based CSR with ascending columns (`m`: a dense array or a scipy matrix)"""

    def __init__(self, ref, m):
        import scipy.sparse as sp
        m = sp.csr_matrix(m)
        m.sort_indices()
        self.ref = ref
        self.n_rows, self.n_cols = m.shape
        self.dtype = m.dtype
        self.rowptr, self.col, self.val = m.indptr.astype(np.int32), m.indices.astype(np.int32), np.ascontiguousarray(m.data)

    def size(self, d=None):
        return (self.n_rows, self.n_cols) if d is None else (self.n_rows, self.n_cols)[d - 1]


def dense_csr(A):
    """every entry of a dense matrix stored (zeros included): what a Matrix{T} of the reference's test sets becomes"""
    import scipy.sparse as sp
    A = np.asarray(A)
    n, m = A.shape
    return sp.csr_matrix((A.reshape(-1).copy(), np.tile(np.arange(m), n), np.arange(n + 1) * m), shape=(n, m))


class HostOps:
    """the `ops` of GenericCGIterable / GenericGMRESIterable over the double"""

    def __init__(self, pkg, ref):
        self.pkg, self.ref = pkg, ref

    def shape(self, dtype):
        w, l = C.c_int(), C.c_int()
        assert self.pkg.lib().mik_reduce_shape(self.pkg._lib.dtype_code(dtype), C.byref(w), C.byref(l)) == 0
        return w.value, l.value

    def mul_(self, y, A, x):
        y.a[:] = self.ref.spmv(A.rowptr, A.col, A.val, x.a, A.n_rows)
        return y

    def dot(self, x, y):
        return self.ref.dot(x.a, y.a, self.shape(x.dtype))

    def norm(self, x):
        return self.ref.nrm2(x.a, self.shape(x.dtype))

    def orthogonalize_and_normalize_(self, V, k, w, h, method=None):
        assert method is None or isinstance(method, self.pkg.ModifiedGramSchmidt)
        hh, nrm = self.ref.mgs(V.store, V.ld, k, w.a, self.shape(w.dtype))
        h[:k] = hh
        return nrm

    def gemv_n_(self, y, V, k, c, alpha=1.0):
        self.ref.gemv_n(V.store, V.ld, k, c, alpha, y.a)
        return y

    def hessenberg_ldiv_(self, H, rhs):
        return self.pkg.hessenberg_ldiv_(H, rhs)          # host code of the library on both sides

    def basis(self, x, cols):
        return NpMatrix(self.ref, x.n, cols, x.dtype)


class HostBackend:
    name = "host"

    def __init__(self, pkg, ref):
        self.pkg, self.ref, self.ops = pkg, ref, HostOps(pkg, ref)

    def vector(self, a):
        return NpVector(self.ref, np.ascontiguousarray(a).copy())

    def operator(self, m):
        return NpCSR(self.ref, m)


class DeviceBackend:
    name = "device"
    ops = None

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx = pkg, ctx

    def vector(self, a):
        return self.pkg.HipVector.from_numpy(np.ascontiguousarray(a), self.ctx)

    def operator(self, m):
        import scipy.sparse as sp
        m = sp.csr_matrix(m)
        m.sort_indices()
        return self.pkg.HipCSR(m.shape[0], m.shape[1], m.indptr.astype(np.int64), m.indices.astype(np.int64), m.data, index_base=0, is_csc=False,
                               ctx=self.ctx)


class ExactPrec:
    """lu(A) / cholesky(A) as Pl or Pr (test/gmres.jl:19, test/cg.jl:44): ldiv_(y, x) solves on the host, for either backend"""

    def __init__(self, A):
        self.A = np.asarray(A)

    def ldiv_(self, y, x=None):
        x = y if x is None else x
        return y.copy_from_host(np.linalg.solve(self.A, x.to_numpy()).astype(y.dtype))


# ---------------------------------------------------------------------------------------------
# the complex test sets of the reference, over a backend.  Each returns a dict of host results; `check_*` asserts the reference's
# own conditions on it; two backends that ran the same scenario are compared with `same`.
# ---------------------------------------------------------------------------------------------
def rand_t(rng, T, *shape):
    rt = real_of(T)
    return (rng.random(shape).astype(rt) + 1j * rng.random(shape).astype(rt)).astype(T)


def _hist(ch):
    return dict(iters=ch.iters, mvps=ch.mvps, conv=bool(ch.isconverged), res=np.array(ch["resnorm"]))


def cg_full(be, T, n=10):
    """test/cg.jl:27-47 for a complex T"""
    pkg, rng = be.pkg, np.random.default_rng(1234321)
    rt = real_of(T).type
    A = rand_t(rng, T, n, n)
    A = (A.conj().T @ A + np.eye(n)).astype(T)
    b = rand_t(rng, T, n)
    reltol = np.sqrt(np.finfo(rt).eps)
    Ad, bd = be.operator(dense_csr(A)), be.vector(b)
    out = dict(A=A, b=b, reltol=reltol)
    x, ch = pkg.cg_(be.vector(np.zeros(n, T)), Ad, bd, initially_zero=True, reltol=reltol, maxiter=2 * n, log=True, ops=be.ops)    # :33
    out["x"], out["h"] = x.to_numpy(), _hist(ch)
    x, ch = pkg.cg_(be.vector(np.linalg.solve(A, b).astype(T)), Ad, bd, abstol=2 * n * np.finfo(rt).eps, reltol=rt(0), log=True, ops=be.ops)   # :39
    out["h_exact"] = _hist(ch)
    x, ch = pkg.cg_(be.vector(np.zeros(n, T)), Ad, bd, initially_zero=True, Pl=ExactPrec(A), log=True, ops=be.ops)                 # :45
    out["x_prec"], out["h_prec"] = x.to_numpy(), _hist(ch)
    return out


def check_cg_full(o):
    A, b = o["A"].astype(np.complex128), o["b"].astype(np.complex128)
    assert np.linalg.norm(A @ o["x"] - b) / np.linalg.norm(b) <= o["reltol"] and o["h"]["conv"]           # :35-36
    assert o["h_exact"]["iters"] <= 1 and o["h_exact"]["mvps"] <= 2                                       # :40-41
    assert o["h_prec"]["iters"] <= 2 and o["h_prec"]["mvps"] <= 2                                         # :46-47


def termination(be, T, solver):
    """test/cg.jl:99-121 / test/gmres.jl:76-98 for a complex T; solver: 'cg' or 'gmres'"""
    pkg = be.pkg
    rt = real_of(T).type
    A = np.array([[2, -1, 0], [-1, 2, -1], [0, -1, 2]], T)
    n = 3
    b = np.ones(n, T)
    x0 = np.linalg.solve(A, b).astype(T)
    pert = (rt(10) * np.sqrt(np.finfo(rt).eps) * np.array([(-1) ** i for i in range(1, n + 1)], T)).astype(T)
    Ad, bd = be.operator(dense_csr(A)), be.vector(b)
    run = pkg.cg_ if solver == "cg" else pkg.gmres_
    out = {}
    x, ch = run(be.vector(x0 + pert), Ad, bd, log=True, ops=be.ops)
    out["x"], out["h"] = x.to_numpy(), _hist(ch)
    initial = np.linalg.norm(A @ (x0 + pert) - b)
    x, ch = run(be.vector(x0 + pert), Ad, bd, abstol=2 * initial, reltol=rt(0), log=True, ops=be.ops)
    out["h_abs"] = _hist(ch)
    return out


def check_termination(o):
    assert 2 <= o["h"]["iters"] <= 3 and o["h_abs"]["iters"] == 0


def gmres_sets(be, T, sparse, n=10):
    """test/gmres.jl:16-36 (sparse = False: a fully stored matrix) and :38-57 (sparse = True: sprand(T, n, n, 0.5) + I)"""
    import scipy.sparse as sp
    pkg, rng = be.pkg, np.random.default_rng(1234321 + int(sparse))
    rt = real_of(T).type
    if sparse:
        A = (rand_t(rng, T, n, n) * (rng.random((n, n)) < 0.5) + np.eye(n)).astype(T)
        M = sp.csr_matrix(A)
    else:
        A = (rand_t(rng, T, n, n) + np.eye(n)).astype(T)
        M = dense_csr(A)
    b = rand_t(rng, T, n)
    reltol = np.sqrt(np.finfo(rt).eps)
    Ad, bd, F = be.operator(M), be.vector(b), ExactPrec(A)
    zeros = lambda: be.vector(np.zeros(n, T))
    out = dict(A=A, b=b, reltol=reltol)
    x, ch = pkg.gmres_(zeros(), Ad, bd, initially_zero=True, log=True, restart=3, maxiter=10, reltol=reltol, ops=be.ops)               # :23 / :45
    out["x"], out["h"] = x.to_numpy(), _hist(ch)
    x, ch = pkg.gmres_(zeros(), Ad, bd, initially_zero=True, Pl=F, maxiter=1, restart=1, reltol=reltol, log=True, ops=be.ops)          # :28 / :49
    out["x_pl"], out["h_pl"] = x.to_numpy(), _hist(ch)
    x, ch = pkg.gmres_(zeros(), Ad, bd, initially_zero=True, Pl=pkg.Identity(), Pr=F, maxiter=1, restart=1, reltol=reltol, log=True, ops=be.ops)   # :33 / :54
    out["x_pr"], out["h_pr"] = x.to_numpy(), _hist(ch)
    return out


def check_gmres_sets(o):
    A, b = o["A"].astype(np.complex128), o["b"].astype(np.complex128)
    assert np.all(np.diff(o["h"]["res"]) <= 0.0)                                                          # :25
    assert o["h_pl"]["conv"] and np.linalg.norm(np.linalg.solve(A, A @ o["x_pl"] - b)) / np.linalg.norm(b) <= o["reltol"]   # :29-30
    assert o["h_pr"]["conv"] and np.linalg.norm(A @ o["x_pr"] - b) / np.linalg.norm(b) <= o["reltol"]     # :34-35


def same(a, b):
    """bit-identical results of two backends: x, every residual, iteration counts"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k
