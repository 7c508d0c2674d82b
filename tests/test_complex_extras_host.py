"""Complex qmr, IDR(s) and the power method without a GPU: the C restatement of the three QMR sweeps and of the
adjoint product (tests/complex_ref/complex_extras_ref.c) against exact rational results and plain Python loops, and the three solvers of
extras.py on the numpy double of the device types -- the complex test sets of test/qmr.jl, test/idrs.jl and
test/simple_eigensolvers.jl with the reference's own conditions, fused and unfused -- plus what must not move: real runs and the
JacobiPrec refusal."""
from fractions import Fraction
from importlib import import_module

import numpy as np
import pytest
import scipy.sparse as sp

import complex_extras_host as ce
import complex_host as ch
from complex_dense_host import dref  # noqa: F401  (fixture)
from complex_extras_host import eref  # noqa: F401  (fixture)
from complex_host import ref  # noqa: F401  (fixture)
from complex_solvers_host import sref  # noqa: F401  (fixture)

CT = [np.complex128, np.complex64]
SHAPE = (1, 1)                       # segments of 256 elements: n = 300 spans two of them
N = 300


def small_ints(rng, T, *shape):
    """complex values with small integer parts: every product and sum below is exact in either precision"""
    return (rng.integers(-3, 4, shape) + 1j * rng.integers(-3, 4, shape)).astype(T)


def fdot(z, y):
    """sum conj(z) y in exact rationals"""
    re = sum(Fraction(int(a.real)) * Fraction(int(b.real)) + Fraction(int(a.imag)) * Fraction(int(b.imag)) for a, b in zip(z, y))
    im = sum(Fraction(int(a.real)) * Fraction(int(b.imag)) - Fraction(int(a.imag)) * Fraction(int(b.real)) for a, b in zip(z, y))
    return complex(float(re), float(im))


@pytest.fixture
def host(pkg, ref, dref, sref, eref, monkeypatch):
    be = ce.HostBackend(pkg, ref, dref, sref)
    ce.patch(monkeypatch, pkg, be, eref)
    return be


@pytest.mark.parametrize("T", CT)
def test_checker_sweeps_against_exact_results(eref, T):
    rng = np.random.default_rng(7)
    rt = ch.real_of(T).type
    x1, x2, y0, z = (small_ints(rng, T, N) for _ in range(4))
    for a, b in ((T(1 - 2j), T(-1 + 1j)), (rt(2), rt(-3))):             # the complex and the real-scalar form
        for xx2 in (x2, None):
            want = (y0 + a * x1 + (b * x2 if xx2 is not None else 0)).astype(T)
            y = y0.copy()
            d = eref.axpy2_dot(y, a, x1, b, xx2, z, SHAPE)
            assert np.array_equal(y, want) and d == T(fdot(z, want))     # dot(z, y): z is the conjugated argument
            y = y0.copy()
            assert eref.axpy2_dot(y, a, x1, b, xx2, None, SHAPE) is None and np.array_equal(y, want)
    x, y = x1.copy(), y0.copy()
    eref.scal2(T(2 - 1j), x, T(1j), y)
    assert np.array_equal(x, (x1 * T(2 - 1j)).astype(T)) and np.array_equal(y, (y0 * T(1j)).astype(T))
    v, pc, pp, xs = (small_ints(rng, T, N) for _ in range(4))
    h1, h0, inv, g = T(1 - 1j), T(2j), T(-1j), T(1 + 2j)
    for cur, prev in ((None, None), (pc, None), (pc, pp)):              # iterations 1, 2 and >= 3
        want_p = ((v + (h1 * pc if cur is not None else 0) + (h0 * pp if prev is not None else 0)) * inv).astype(T)
        xo, po = xs.copy(), np.zeros(N, T)
        eref.qmr_update(v, h1, cur, h0, prev, inv, g, xo, po)
        assert np.array_equal(po, want_p) and np.array_equal(xo, (xs + g * want_p).astype(T))
    xo, po = xs.copy(), pp.copy()                                        # p_out is p_prev's storage
    eref.qmr_update(v, h1, pc, h0, po, inv, g, xo, po)
    assert np.array_equal(po, want_p) and np.array_equal(xo, (xs + g * want_p).astype(T))


def _cx_mul(T, z, w):
    """(zr wr - zi wi) + (zr wi + zi wr) i, every operation rounded in the component type"""
    rt = ch.real_of(T).type
    zr, zi, wr, wi = rt(z.real), rt(z.imag), rt(w.real), rt(w.imag)
    return rt(rt(zr * wr) - rt(zi * wi)), rt(rt(zr * wi) + rt(zi * wr))


@pytest.mark.parametrize("T", CT)
def test_checker_sweeps_against_plain_python_loops(eref, T):
    """rounded inputs: the orders of operations, element by element"""
    rng = np.random.default_rng(8)
    rt = ch.real_of(T).type
    n = 37
    v, pc, pp, xs, x1, x2, y0 = (ch.rand_t(rng, T, n) - T(0.5 + 0.5j) for _ in range(7))
    h1, h0, inv, g = (T(c) for c in ch.rand_t(rng, T, 4) - T(0.5 + 0.5j))
    xo, po = xs.copy(), np.zeros(n, T)
    eref.qmr_update(v, h1, pc, h0, pp, inv, g, xo, po)
    for i in range(n):
        pr, pi = rt(v[i].real), rt(v[i].imag)
        for h, q in ((h1, pc), (h0, pp)):
            tr, ti = _cx_mul(T, h, q[i])
            pr, pi = rt(pr + tr), rt(pi + ti)
        pr, pi = _cx_mul(T, T(complex(pr, pi)), inv)
        tr, ti = _cx_mul(T, g, T(complex(pr, pi)))
        assert po[i] == T(complex(pr, pi)) and xo[i] == T(complex(rt(xs[i].real + tr), rt(xs[i].imag + ti)))
    y, xa, xb = y0.copy(), x1.copy(), x2.copy()
    eref.axpy2_dot(y, h1, x1, h0, x2, None, SHAPE)
    eref.scal2(inv, xa, g, xb)
    for i in range(n):
        tr, ti = _cx_mul(T, h1, x1[i])
        yr, yi = rt(y0[i].real + tr), rt(y0[i].imag + ti)
        tr, ti = _cx_mul(T, h0, x2[i])
        assert y[i] == T(complex(rt(yr + tr), rt(yi + ti)))
        assert xa[i] == T(complex(*_cx_mul(T, x1[i], inv))) and xb[i] == T(complex(*_cx_mul(T, x2[i], g)))


@pytest.mark.parametrize("T", CT)
def test_checker_dot_is_the_complex_dot_tree(eref, ref, T):
    """the reduction of the fused sweep restates the tree of the complex mik_dot: the same bits as tests/complex_ref/complex_ref.c, at a
    size past one level-2 batch of the smallest shape"""
    rng = np.random.default_rng(9)
    n = 256 * 1025 + 3
    x1, y, z = (ch.rand_t(rng, T, n) - T(0.5 + 0.5j) for _ in range(3))
    d = eref.axpy2_dot(y, T(0.5 - 1j), x1, None, None, z, SHAPE)
    assert d == ref.dot(z, y, SHAPE)


@pytest.mark.parametrize("T", CT)
def test_adjoint_product_is_the_column_loop(eref, ref, T):
    """adjoint(A) x: the checker's loop over the columns of A against exact sums, and the CSR arrays with_adjoint uploads for it (the
    same three arrays, values conjugated) through the SpMV checker: the same bits"""
    rng = np.random.default_rng(10)
    m, n = 23, 17
    D = small_ints(rng, T, m, n) * (rng.random((m, n)) < 0.4)
    D[:, 5] = 0                                                          # an empty column of A: an empty row of the adjoint
    M = sp.csc_matrix(D.astype(T))
    x = small_ints(rng, T, m)
    got = eref.adj_mul(M, x)
    assert np.array_equal(got, np.array([fdot(D[:, j], x) for j in range(n)], T))
    xr = ch.rand_t(rng, T, m)
    Mr = sp.csc_matrix((ch.rand_t(rng, T, m, n) * (rng.random((m, n)) < 0.4)).astype(T))
    Mr.sort_indices()
    up = ref.spmv(Mr.indptr.astype(np.int32), Mr.indices.astype(np.int32), np.conj(Mr.data), xr, n)      # what A.adj holds
    assert np.array_equal(eref.adj_mul(Mr, xr), up)


@pytest.mark.parametrize("T", CT)
def test_seeds_leave_room(T):
    ce.room_qmr(T)
    ce.room_idrs(T)
    ce.room_powm(T)


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("T", CT)
def test_qmr_sets_on_the_double(host, T, kind):
    fused = ce.qmr_sets(host, T, kind, fused=True)
    ce.check_qmr_sets(fused, T)
    ce.same(fused, ce.qmr_sets(host, T, kind, fused=False))
    t = ce.termination(host, T, "qmr", kind)
    ce.check_termination(t)
    ce.same(t, ce.termination(host, T, "qmr", kind, fused=False))


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("T", CT)
def test_idrs_sets_on_the_double(host, T, kind):
    fused = ce.idrs_sets(host, T, kind, fused=True)
    ce.check_idrs_sets(fused, T)
    ce.same(fused, ce.idrs_sets(host, T, kind, fused=False))
    t = ce.termination(host, T, "idrs", kind)
    ce.check_termination(t)
    ce.same(t, ce.termination(host, T, "idrs", kind, fused=False))


def test_idrs_with_a_preconditioner_on_the_double(host):
    """test/idrs.jl:45-62 (ComplexF64, n = 1000)"""
    o = ce.idrs_prec_sets(host, np.complex128)
    ce.check_idrs_prec_sets(o, np.complex128)


@pytest.mark.parametrize("kind", ce.KINDS)
@pytest.mark.parametrize("T", CT)
def test_power_method_sets_on_the_double(host, T, kind):
    ce.check_powm_sets(ce.powm_sets(host, T, kind), T)


def test_complex_idrs_never_creates_the_real_handle_and_tolerances_are_real(host):
    inp = ce.idrs_inputs(np.complex64)
    ex = host.pkg.extras
    it = ex.idrs_iterable_(None, host.vector(np.zeros(inp["n"], np.complex64)), host.operator(inp["S"]), host.vector(inp["bs"]), ce.S, None, 0.0, inp["reltol"], 10,
                           P=inp["P"])
    assert it._step is None and it.tol.dtype == np.float32 and it.normR.dtype == np.float32 and it.omega.dtype == np.complex64
    q = ex.qmr_iterable_(host.vector(np.zeros(inp["n"], np.complex64)), host.operator(inp["S"]), host.vector(inp["bs"]))
    assert q.tol.dtype == np.float32 and q.resnorm.dtype == np.float32 and q.lanczos.delta.dtype == np.complex64
    p = ex.powm_iterable_(host.operator(inp["S"]), host.vector(inp["bs"]))
    assert p.tol.dtype == np.float32 and p.residual == np.finfo(np.float32).max and p.tol == np.float32(np.finfo(np.float32).eps * inp["n"] ** 3)


def test_jacobi_prec_on_complex_is_still_refused(host):
    pkg, inp = host.pkg, ce.idrs_inputs(np.complex128)
    d = host.vector(np.ones(inp["n"], np.complex128))
    with pytest.raises(TypeError, match="JacobiPrec is not offered for complex element types"):
        pkg.extras.idrs(host.operator(inp["S"]), host.vector(inp["bs"]), Pl=pkg.JacobiPrec(d), P=inp["P"])


def _real_runs(pkg, orc, monkeypatch):
    """qmr, idrs and powm_ in Float64 on the real host double of tests/host_double.py -> every bit they return"""
    from host_double import FakeOperator, FakeVector, patch
    ex = import_module(pkg.__name__ + ".extras")
    with monkeypatch.context() as mp:
        patch(mp, ex, orc)
        mp.setattr(ex, "givens_algorithm", lambda f, g, dt=np.float64: orc.givens(f, g, dt))
        mp.setattr(ex, "zerox", lambda A, b: FakeVector(np.zeros(A.size(2), b.dtype)))
        rng = np.random.default_rng(41)
        n = 40
        Sm = (sp.random(n, n, density=0.2, random_state=rng, format="csc") + 4 * sp.identity(n)).tocsc()
        b, P = rng.standard_normal(n), rng.random((n, 4))
        A = FakeOperator(orc, Sm)
        x, h = ex.qmr(A, FakeVector(b), maxiter=60, log=True)
        out = [x.to_numpy(), np.array(h["resnorm"])]
        x, h = ex.idrs(A, FakeVector(b), s=4, P=P, log=True, fused=False)
        out += [x.to_numpy(), np.array(h["resnorm"])]
        lam, x, h = ex.powm_(A, FakeVector(b / np.linalg.norm(b)), maxiter=30, log=True)
        out += [np.asarray(lam), x.to_numpy(), np.array(h["resnorm"])]
    return out


def test_real_runs_do_not_move_around_a_complex_solve(pkg, orc, ref, dref, sref, eref, monkeypatch):
    before = _real_runs(pkg, orc, monkeypatch)
    assert all(a.dtype == np.float64 for a in before)
    with monkeypatch.context() as mp:
        be = ce.HostBackend(pkg, ref, dref, sref)
        ce.patch(mp, pkg, be, eref)
        ce.check_qmr_sets(ce.qmr_sets(be, np.complex128), np.complex128)
    after = _real_runs(pkg, orc, monkeypatch)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
