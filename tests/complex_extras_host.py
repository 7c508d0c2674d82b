"""What tests/test_complex_extras_host.py and tests/test_gpu_complex_extras.py share: the ctypes binding of
tests/complex_ref/complex_extras_ref.c (`ExtrasRef`), the routing of the module-level calls of extras.py to the numpy double of
tests/complex_solvers_host.py (`patch`), host and device backends whose operators carry their adjoint (`csr`, `dense`, `linop`), plain
complex128 numpy restatements of qmr, IDR(s) and the power method that share no code with the library (`plain_*`: they say with how much
room a seed meets the reference's conditions), and the complex test sets of test/qmr.jl, test/idrs.jl and test/simple_eigensolvers.jl
written once over a backend.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import complex_dense_host as cdh
import complex_host as ch
import complex_solvers_host as cs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "complex_ref", "complex_extras_ref.c")
_vp = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
KINDS = ("csr", "dense", "linop")


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


class ExtrasRef:
    """The C checker.  Complex arrays go in as they are (interleaved re, im) and are changed in place; `shape` = (W, L) of mik_reduce_shape."""

    def __init__(self, lib):
        self.L = lib
        for sfx in ("f64", "f32"):
            for name in ("ce_axpy2_dot", "ce_scal2", "ce_qmr_update", "ce_adj_mul"):
                getattr(lib, f"{name}_{sfx}").restype = None

    def fn(self, name, dtype):
        return getattr(self.L, f"{name}_{'f64' if np.dtype(dtype) == np.complex128 else 'f32'}")

    def axpy2_dot(self, y, a, x1, b, x2, z, shape):
        """y += a x1 (+ b x2); -> dot(z, y) or None.  Real a, b select the real-scalar form."""
        real_sc = not (np.iscomplexobj(a) or np.iscomplexobj(b))
        sa, sb = np.asarray([a], y.dtype), np.asarray([0 if b is None else b], y.dtype)
        out = np.zeros(1, y.dtype)
        self.fn("ce_axpy2_dot", y.dtype)(_i64(y.size), _int(real_sc), _p(sa), _p(x1), _p(sb), _p(x2), _p(y), _p(z), _int(shape[0]), _int(shape[1]), _p(out))
        return out[0] if z is not None else None

    def scal2(self, a, x, b, y):
        self.fn("ce_scal2", x.dtype)(_i64(x.size), _p(np.asarray([a], x.dtype)), _p(x), _p(np.asarray([b], x.dtype)), _p(y))

    def qmr_update(self, v, neg_h1, p_curr, neg_h0, p_prev, inv, g, x, p_out):
        sc = [np.asarray([0 if s is None else s], x.dtype) for s in (neg_h1, neg_h0, inv, g)]
        self.fn("ce_qmr_update", x.dtype)(_i64(x.size), _p(v), _p(sc[0]), _p(p_curr), _p(sc[1]), _p(p_prev), _p(sc[2]), _p(sc[3]), _p(x), _p(p_out))

    def adj_mul(self, m, x):
        """adjoint(m) x by the column loop over the CSC arrays of m (a scipy matrix)"""
        m = sp.csc_matrix(m)
        m.sort_indices()
        cp, rv, nz = m.indptr.astype(np.int64), m.indices.astype(np.int64), np.ascontiguousarray(m.data)
        y = np.full(m.shape[1], np.nan, m.dtype)
        self.fn("ce_adj_mul", m.dtype)(_i64(m.shape[1]), _p(cp), _p(rv), _p(nz), _p(np.ascontiguousarray(x, m.dtype)), _p(y))
        return y


def build(outdir):
    """gcc -std=c99 -O2 -ffp-contract=off -> a shared object in `outdir`."""
    so = os.path.join(str(outdir), "complex_extras_ref.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so])
    return ExtrasRef(C.CDLL(so))


@pytest.fixture(scope="session")
def eref(tmp_path_factory):
    return build(tmp_path_factory.mktemp("complex_extras_ref"))


# ---------------------------------------------------------------------------------------------
# the numpy double under extras.py
# ---------------------------------------------------------------------------------------------
class NpBlock(ch.NpMatrix):
    """`HipMatrix` as extras.py constructs it: (n, cols, dtype, ctx) and from_numpy(a, ctx)"""
    ctx = None

    def __init__(self, n, cols, dtype=np.float64, ctx=None):
        super().__init__(cs_ref(), n, cols, dtype)

    @staticmethod
    def from_numpy(a, ctx=None):
        a = np.asarray(a)
        m = NpBlock(a.shape[0], a.shape[1], a.dtype)
        for j in range(a.shape[1]):
            m.col(j).a[:] = a[:, j]
        return m


_REF = []


def cs_ref():
    return _REF[0]


class HostLinOp:
    """a LinearMap on the double: `mul(y, x)` on NpVectors"""

    def __init__(self, n, dtype, mul):
        self.n_rows = self.n_cols = n
        self.dtype, self.mul = np.dtype(dtype), mul

    def size(self, d=None):
        return (self.n_rows, self.n_cols) if d is None else self.n_rows


def patch(monkeypatch, pkg, be, eref):
    """route what extras.py calls at module level to the double of `be` (a HostBackend of complex_solvers_host)"""
    ex, ops = pkg.extras, be.ops
    _REF[:] = [be.ref]
    shape = lambda v: ops.shape(v.dtype)

    def mul_(y, A, x):
        return A.mul(y, x) or y if isinstance(A, HostLinOp) else ops.mul_(y, A, x)

    def axpy2_dot(y, a, x1, b, x2, z):
        T = y.dtype.type
        return eref.axpy2_dot(y.a, T(a), x1.a, T(0 if b is None else b), None if x2 is None else x2.a, None if z is None else z.a, shape(y))

    def qmr_update(v, neg_h1, p_curr, neg_h0, p_prev, inv, g, x, p_out):
        T = x.dtype.type
        eref.qmr_update(v.a, T(neg_h1), None if p_curr is None else p_curr.a, T(neg_h0), None if p_prev is None else p_prev.a, T(inv), T(g), x.a, p_out.a)

    monkeypatch.setattr(ch.NpVector, "ctx", None, raising=False)
    for name, f in (("dot", ops.dot), ("norm", ops.norm), ("mul_", mul_), ("HipVector", ch.NpVector), ("HipMatrix", NpBlock),
                    ("zerox", lambda A, b: ch.NpVector(be.ref, np.zeros(A.size(2), b.dtype))),
                    ("gemv_t_", lambda V, k, w, col0=0: ops.gemv_t_(V, k, w, col0)), ("_axpy2_dot", axpy2_dot),
                    ("_scal2", lambda a, x, b, y: eref.scal2(x.dtype.type(a), x.a, x.dtype.type(b), y.a)), ("_qmr_update", qmr_update)):
        monkeypatch.setattr(ex, name, f)


class HostBackend(cs.HostBackend):
    def operator(self, m, kind="csr", idx=np.int64):
        m = sp.csc_matrix(m)
        if kind == "dense":
            return cdh.NpDense(m.toarray())
        A, At = ch.NpCSR(self.ref, m), ch.NpCSR(self.ref, m.conj().T)
        if kind == "linop":
            A, At = (HostLinOp(m.shape[0], m.dtype, lambda y, x, B=B: self.ops.mul_(y, B, x)) for B in (A, At))
        A.adj, At.adj = At, A
        return A


class DeviceBackend(cs.DeviceBackend):
    def operator(self, m, kind="csr", idx=np.int64):
        pkg = self.pkg
        m = sp.csc_matrix(m)
        m.sort_indices()
        if kind == "dense":
            return pkg.HipMatrix.from_numpy(m.toarray(), self.ctx)
        A = pkg.extras.with_adjoint(m.shape[0], m.shape[1], m.indptr.astype(idx), m.indices.astype(idx), m.data, index_base=0, ctx=self.ctx)
        if kind == "linop":
            L, Lt = (pkg.LinearOperator(m.shape[0], m.dtype, lambda y, x, B=B: pkg.mul_(y, B, x), self.ctx) for B in (A, A.adj))
            L.adj, Lt.adj = Lt, L
            return L
        return A


class LuPrec:
    """lu(M) as Pl: ldiv_(y) solves on the host, for either backend (test/idrs.jl:54)"""

    def __init__(self, M):
        self.lu = sla.lu_factor(np.asarray(M, np.complex128))

    def ldiv_(self, y, x=None):
        x = y if x is None else x
        return y.copy_from_host(sla.lu_solve(self.lu, x.to_numpy().astype(np.complex128)).astype(y.dtype))


# ---------------------------------------------------------------------------------------------
# plain numpy restatements in complex128: no library code, no checker, no tree -- what a seed is judged with
# ---------------------------------------------------------------------------------------------
def plain_qmr(A, b, x0, reltol, maxiter, abstol=0.0):
    """src/qmr.jl -> (x, iterations, converged)"""
    A, b, x = (np.asarray(v, np.complex128) for v in (A, b, x0))
    n = len(b)
    z = lambda: np.zeros(n, np.complex128)
    v_prev, v_curr, w_prev = z(), b - A @ x, z()
    res = np.linalg.norm(v_curr)
    v_curr = v_curr / res
    w_curr = v_curr.copy()
    beta_prev = beta_curr = delta = 0j
    g0, H = res + 0j, np.zeros(4, np.complex128)
    c_prev, s_prev, c_curr, s_curr = 1.0, 0j, 1.0, 0j
    p_prev, p_curr = z(), z()
    tol = max(reltol * res, abstol)
    it = 1
    while it <= maxiter and res > tol:
        v_next = A @ v_curr
        alpha = np.vdot(v_next, w_curr)
        v_next = v_next - np.conj(alpha) * v_curr - (np.conj(beta_curr) * v_prev if it > 1 else 0)
        w_next = A.conj().T @ w_curr - alpha * w_curr - (delta * w_prev if it > 1 else 0)
        vw = np.vdot(v_next, w_next)
        delta = np.sqrt(abs(vw)) + 0j
        beta_prev, beta_curr = beta_curr, vw / delta
        v_prev, v_curr, w_prev, w_curr = v_curr, v_next / delta, w_curr, w_next / beta_curr
        H[1], H[2], H[3] = np.conj(beta_prev), np.conj(alpha), delta
        if it > 2:
            H[0], H[1] = s_prev * H[1], c_prev * H[1]
        if it > 1:
            H[1], H[2] = c_curr * H[1] + s_curr * H[2], -np.conj(s_curr) * H[1] + c_curr * H[2]
        c, s, H[2] = cs._plain_givens(H[2], H[3])
        g1, g0 = -np.conj(s) * g0, c * g0
        p = (v_prev - (H[1] * p_curr if it > 1 else 0) - (H[0] * p_prev if it > 2 else 0)) / H[2]
        x = x + g0 * p
        c_prev, s_prev, c_curr, s_curr = c_curr, s_curr, c, s
        p_prev, p_curr, g0 = p_curr, p, g1
        res = abs(g1)
        it += 1
    return x, it - 1, bool(res <= tol)


def plain_idrs(A, b, x0, P, reltol, maxiter, smoothing=False, abstol=0.0, Pl=None):
    """src/idrs.jl -> (x, iterations, converged)"""
    A, b, X, P = (np.asarray(v, np.complex128) for v in (A, b, x0, P))
    solve = (lambda v: v) if Pl is None else (lambda v: np.linalg.solve(np.asarray(Pl, np.complex128), v))
    n, s = P.shape
    R = b - A @ X
    normR = np.linalg.norm(R)
    tol = max(reltol * normR, abstol)
    Xs, Rs = X.copy(), R.copy()
    U, G = np.zeros((n, s), np.complex128), np.zeros((n, s), np.complex128)
    M, f, om = np.eye(s, dtype=np.complex128), np.zeros(s, np.complex128), 1 + 0j
    it, step = 1, 1

    def smooth():
        nonlocal Xs, Rs
        Ts = Rs - R
        gamma = np.vdot(Rs, Ts) / np.vdot(Ts, Ts)
        Rs, Xs = Rs - gamma * Ts, Xs - gamma * (Xs - X)
        return np.linalg.norm(Rs)
    while not (normR < tol or it > maxiter):
        if step <= s:
            if step == 1:
                f = P.conj().T @ R
            k = step - 1
            c = sla.solve_triangular(M[k:, k:], f[k:], lower=True)
            V = solve(R - G[:, k:] @ c)
            U[:, k] = U[:, k:] @ c + om * V
            G[:, k] = A @ U[:, k]
            for i in range(k):
                alpha = np.vdot(P[:, i], G[:, k]) / M[i, i]
                G[:, k] -= alpha * G[:, i]
                U[:, k] -= alpha * U[:, i]
            M[k:, k] = P[:, k:].conj().T @ G[:, k]
            beta = f[k] / M[k, k]
            R = R - beta * G[:, k]
            X = X + beta * U[:, k]
            normR = smooth() if smoothing else np.linalg.norm(R)
            f[k + 1:] -= beta * M[k + 1:, k]
            step += 1
        else:
            V = solve(R)
            Q = A @ V
            ns, nt, ts = np.linalg.norm(R), np.linalg.norm(Q), np.vdot(Q, R)
            rho, om = abs(ts / (nt * ns)), ts / (nt * nt)
            if rho < np.sqrt(2) / 2:
                om = om * (np.sqrt(2) / 2) / rho
            R, X = R - om * Q, X + om * V
            normR = smooth() if smoothing else np.linalg.norm(R)
            step = 1
        it += 1
    return (Xs if smoothing else X), it - 1, bool(0 <= normR < tol)


def plain_powm(mul, x0, tol, maxiter):
    """src/simple.jl:28-47 -> (theta, x, converged)"""
    x = np.asarray(x0, np.complex128)
    theta, res, it = 0j, np.inf, 0
    while not (it > maxiter or res <= tol):
        Ax = mul(x)
        theta = np.vdot(x, Ax)
        res = np.linalg.norm(Ax - theta * x)
        x = Ax / np.linalg.norm(Ax)
        it += 1
    return theta, x, bool(res <= tol)


# ---------------------------------------------------------------------------------------------
# the complex test sets of the reference over a backend; `check_*`: the reference's own conditions on the result; `room_*`: the plain
# restatement on the same inputs meets them with a factor 2 to spare, which is what the seeds are chosen by (on the CPU, the smallest of
# 1 .. 59 that passes for both element types: 10 of them do for qmr, 19 for idrs, one for the power method)
# ---------------------------------------------------------------------------------------------
SEED_QMR = 5
SEED_IDRS = 3
SEED_POWM = 1
S = 8                                                                        # idrs: s = 8, the default

_hist = ch._hist
rand_t = ch.rand_t
same = ch.same
_rel, _reltol = cs._rel, cs._reltol


def _sprand(rng, T, n, density, shift):
    """sprand(T, n, n, density) + shift * I"""
    mask = rng.random((n, n)) < density
    return sp.csc_matrix((rand_t(rng, T, n, n) * mask + shift * np.eye(n)).astype(T))


def qmr_inputs(T, seed=SEED_QMR, n=10):
    rng = np.random.default_rng(seed)
    return dict(A=(rand_t(rng, T, n, n) + n * np.eye(n)).astype(T), b=rand_t(rng, T, n), S=_sprand(rng, T, n, 0.5, n), bs=rand_t(rng, T, n),
                reltol=_reltol(T), n=n)


def qmr_sets(be, T, kind="csr", fused=True, idx=np.int64):
    """test/qmr.jl:15-24 (a fully stored matrix, the default reltol) and :26-34 (sparse, reltol = sqrt(eps)) for a complex T"""
    ex, inp = be.pkg.extras, qmr_inputs(T)
    out = {}
    x, h = ex.qmr(be.operator(ch.dense_csr(inp["A"]), kind, idx), be.vector(inp["b"]), log=True, fused=fused)                       # :20
    out["x1"], out["h1"] = x.to_numpy(), _hist(h)
    x, h = ex.qmr(be.operator(inp["S"], kind, idx), be.vector(inp["bs"]), log=True, reltol=inp["reltol"], fused=fused)              # :31
    out["x2"], out["h2"] = x.to_numpy(), _hist(h)
    return out


def check_qmr_sets(o, T, room=1):
    inp = qmr_inputs(T)
    assert o["h1"]["conv"] and _rel(inp["A"], o["x1"], inp["b"]) <= 10 * inp["reltol"] / room                # :22-23 (reltol there is 10 sqrt(eps))
    assert o["h2"]["conv"] and _rel(inp["S"].toarray(), o["x2"], inp["bs"]) <= 2 * inp["reltol"] / room      # :32-33


def room_qmr(T, seed=SEED_QMR):
    inp = qmr_inputs(T, seed)
    n, z = inp["n"], np.zeros(inp["n"], T)
    x1, _, c1 = plain_qmr(inp["A"], inp["b"], z, inp["reltol"], n)
    x2, _, c2 = plain_qmr(inp["S"].toarray(), inp["bs"], z, inp["reltol"], n)
    assert c1 and c2 and _rel(inp["A"], x1, inp["b"]) <= 10 * inp["reltol"] / 2 and _rel(inp["S"].toarray(), x2, inp["bs"]) <= 2 * inp["reltol"] / 2


def termination(be, T, solver, kind="csr", fused=True):
    """test/qmr.jl:42-66, test/idrs.jl:82-106 for a complex T"""
    ex, inp = be.pkg.extras, cs.tridiag_inputs(T)
    rt = ch.real_of(T).type
    Ad, bd = be.operator(ch.dense_csr(inp["A"]), kind), be.vector(inp["b"])
    if solver == "qmr":
        run = lambda **kw: ex.qmr_(be.vector(inp["start"]), Ad, bd, log=True, fused=fused, **kw)
    else:
        P = rand_t(np.random.default_rng(SEED_IDRS), T, 3, S)
        run = lambda **kw: ex.idrs_(be.vector(inp["start"]), Ad, bd, log=True, fused=fused, P=P, **kw)
    out = {}
    x, h = run()
    out["x"], out["h"] = x.to_numpy(), _hist(h)
    x, h = run(abstol=2 * inp["initial"], reltol=rt(0))
    out["h_abs"] = _hist(h)
    return out


def check_termination(o):
    assert 2 <= o["h"]["iters"] <= 3 and o["h_abs"]["iters"] == 0


def idrs_inputs(T, seed=SEED_IDRS, n=10):
    rng = np.random.default_rng(seed)
    return dict(A=(rand_t(rng, T, n, n) + n * np.eye(n)).astype(T), b=rand_t(rng, T, n), S=_sprand(rng, T, n, 0.5, n), bs=rand_t(rng, T, n),
                P=rand_t(rng, T, n, S), reltol=_reltol(T), n=n)


def idrs_sets(be, T, kind="csr", fused=True, idx=np.int64):
    """test/idrs.jl:15-33 (a fully stored matrix, without and with smoothing) and :35-43 (sparse) for a complex T"""
    ex, inp = be.pkg.extras, idrs_inputs(T)
    out = {}
    Ad, bd = be.operator(ch.dense_csr(inp["A"]), kind, idx), be.vector(inp["b"])
    x, h = ex.idrs(Ad, bd, reltol=inp["reltol"], log=True, P=inp["P"], fused=fused)                                                 # :21
    out["x1"], out["h1"] = x.to_numpy(), _hist(h)
    x, h = ex.idrs(Ad, bd, reltol=inp["reltol"], smoothing=True, log=True, P=inp["P"], fused=fused)                                 # :29
    out["x2"], out["h2"] = x.to_numpy(), _hist(h)
    x, h = ex.idrs(be.operator(inp["S"], kind, idx), be.vector(inp["bs"]), log=True, P=inp["P"], fused=fused)                       # :40
    out["x3"], out["h3"] = x.to_numpy(), _hist(h)
    return out


def check_idrs_sets(o, T, room=1):
    inp = idrs_inputs(T)
    assert o["h1"]["conv"] and _rel(inp["A"], o["x1"], inp["b"]) <= inp["reltol"] / room                     # :23-24
    assert o["h2"]["conv"] and _rel(inp["A"], o["x2"], inp["b"]) <= 2 * inp["reltol"] / room                 # :30-31
    assert o["h3"]["conv"] and _rel(inp["S"].toarray(), o["x3"], inp["bs"]) <= inp["reltol"] / room          # :41-42


def room_idrs(T, seed=SEED_IDRS):
    inp = idrs_inputs(T, seed)
    n, z, tol = inp["n"], np.zeros(inp["n"], T), inp["reltol"]
    x1, _, c1 = plain_idrs(inp["A"], inp["b"], z, inp["P"], tol, n)
    x2, _, c2 = plain_idrs(inp["A"], inp["b"], z, inp["P"], tol, n, smoothing=True)
    x3, _, c3 = plain_idrs(inp["S"].toarray(), inp["bs"], z, inp["P"], tol, n)
    assert c1 and c2 and c3
    assert _rel(inp["A"], x1, inp["b"]) <= tol / 2 and _rel(inp["A"], x2, inp["b"]) <= 2 * tol / 2 and _rel(inp["S"].toarray(), x3, inp["bs"]) <= tol / 2


def idrs_prec_inputs(T, n=1000):
    """test/idrs.jl:45-62: sprand(T, 1000, 1000, 0.1) + 30 I and lu(droptol!(copy(A), 0.1))"""
    rng = np.random.default_rng(SEED_IDRS)
    A = _sprand(rng, T, n, 0.1, 30)
    D = A.toarray()
    D[np.abs(D) <= 0.1] = 0
    return dict(A=A, b=rand_t(rng, T, n), P=rand_t(rng, T, n, S), near=D, reltol=_reltol(T), n=n)


def idrs_prec_sets(be, T, fused=True, idx=np.int64):
    ex, inp = be.pkg.extras, idrs_prec_inputs(T)
    Ad, bd = be.operator(inp["A"], "csr", idx), be.vector(inp["b"])
    out = {}
    x, h = ex.idrs(Ad, bd, log=True, P=inp["P"], fused=fused)                                                                       # :50
    out["x"], out["h"] = x.to_numpy(), _hist(h)
    x, h = ex.idrs(Ad, bd, Pl=LuPrec(inp["near"]), log=True, P=inp["P"], fused=fused)                                               # :55
    out["xp"], out["hp"] = x.to_numpy(), _hist(h)
    return out


def check_idrs_prec_sets(o, T):
    inp = idrs_prec_inputs(T)
    A = inp["A"].astype(np.complex128)
    rel = lambda x: np.linalg.norm(A @ x.astype(np.complex128) - inp["b"]) / np.linalg.norm(inp["b"])
    assert o["h"]["conv"] and rel(o["x"]) <= inp["reltol"] and o["hp"]["conv"] and rel(o["xp"]) <= inp["reltol"]   # :51-52, :56-57
    assert np.linalg.norm(o["x"] - o["xp"]) <= 1e-3 * max(np.linalg.norm(o["x"]), np.linalg.norm(o["xp"]))           # :59 (isapprox on vectors)
    assert o["hp"]["iters"] < 0.5 * o["h"]["iters"]                                                                  # :60


def powm_inputs(T, seed=SEED_POWM, n=10):
    rng = np.random.default_rng(seed)
    B = (rand_t(rng, T, n, n) + np.eye(n)).astype(T)
    A = (B.conj().T @ B).astype(T)                                                                                    # :16-17
    ev = np.linalg.eigvalsh(A.astype(np.complex128))
    tol = 2 * n ** 2 * np.linalg.cond(A.astype(np.complex128)) * np.finfo(ch.real_of(T)).eps                          # :20
    x0 = rand_t(rng, T, n)
    x0 = (x0 / np.linalg.norm(x0)).astype(T)
    idx = n // 2
    sigma = T(0.75 * ev[idx - 1] + 0.25 * ev[idx])                                                                    # :33-34 (1-based idx)
    return dict(A=A, ev=ev, tol=tol, x0=x0, sigma=sigma, target=ev[idx - 1], n=n)


def powm_sets(be, T, kind="csr"):
    """test/simple_eigensolvers.jl:24-48 for a complex T: powm and invpowm with F = lu(A - sigma I) as a linear map"""
    ex, inp = be.pkg.extras, powm_inputs(T)
    n = inp["n"]
    out = {}
    lam, x, h = ex.powm_(be.operator(ch.dense_csr(inp["A"]), kind), be.vector(inp["x0"]), tol=inp["tol"], maxiter=10 * n, log=True)          # :25
    out["lam"], out["x"], out["h"] = np.asarray(lam), x.to_numpy(), _hist(h)
    F = LuPrec(inp["A"].astype(np.complex128) - complex(inp["sigma"]) * np.eye(n))                                    # :39-40
    Fmap = be.linear_map(n, T, lambda y, x: F.ldiv_(y, x))
    lam, x, h = ex.invpowm_(Fmap, be.vector(inp["x0"]), shift=inp["sigma"], tol=inp["tol"], maxiter=10 * n, log=True)                        # :42
    out["ilam"], out["ix"], out["ih"] = np.asarray(lam), x.to_numpy(), _hist(h)
    return out


def _approx(a, b, T):
    return abs(a - b) <= np.sqrt(np.finfo(ch.real_of(T)).eps) * max(abs(a), abs(b))                                   # isapprox's default rtol


def check_powm_sets(o, T, room=1):
    inp = powm_inputs(T)
    A = inp["A"].astype(np.complex128)
    assert _approx(inp["ev"][-1], complex(o["lam"]), T) and np.linalg.norm(A @ o["x"] - complex(o["lam"]) * o["x"]) <= inp["tol"] / room     # :27-28
    assert np.linalg.norm(A @ o["ix"] - complex(o["ilam"]) * o["ix"]) <= inp["tol"] / room and _approx(inp["target"], complex(o["ilam"]), T)  # :45-46


def room_powm(T, seed=SEED_POWM):
    inp = powm_inputs(T, seed)
    A, n = inp["A"].astype(np.complex128), inp["n"]
    th, x, _ = plain_powm(lambda v: A @ v, inp["x0"], inp["tol"], 10 * n)
    Fi = np.linalg.inv(A - complex(inp["sigma"]) * np.eye(n))
    ith, ix, _ = plain_powm(lambda v: Fi @ v, inp["x0"], inp["tol"], 10 * n)
    ilam = complex(inp["sigma"]) + 1 / ith
    check_powm_sets(dict(lam=th, x=x, ilam=ilam, ix=ix), T, room=2)


HostBackend.linear_map = lambda self, n, T, mul: HostLinOp(n, T, mul)
DeviceBackend.linear_map = lambda self, n, T, mul: self.pkg.LinearOperator(n, T, mul, self.ctx)
