"""The checker of the dense QR tests (tests/dense_ref/dense_qr_ref.c, the bit contract restated as unblocked loops) against what needs no
device: a blocked numpy restatement of the device plan, an a-priori error bound, the scale invariance the contract promises, the fixtures'
own preconditions, and -- on a device-free double of the library -- the refusals of iterativesolvers.jl_amd/dense_qr.py."""
import ctypes as C
import types

import numpy as np
import pytest

import dense_qr_host as qh

DTYPES = qh.DTYPES
W = 32                                  # the panel width the kernels are written for today; the claims below hold at any W


@pytest.fixture(autouse=True)
def feature(pkg):
    """the checker states the contract of pkg.qr: without the feature nothing here has a subject"""
    assert callable(getattr(pkg, "qr", None)) and callable(getattr(pkg, "qr_", None)) and callable(getattr(pkg, "ldiv", None))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return qh.build(tmp_path_factory.mktemp("dense_qr_ref"))


def test_tree_is_the_checkers_reduction(ref):
    """the numpy reduction against the checker's, through the one place the checker exposes it: w of a reflector on a column.  A single
    column whose tau is 1 and whose v is all ones below the diagonal turns a into a - sum(a): the sum is T."""
    for dtype in DTYPES:
        for m in (1, 2, 63, 64, 65, 255, 256, 257, 513, 700):
            a = qh.vector(m, dtype)
            QR = np.ones((m, 1), dtype, order="F")
            got = ref.lmul(QR, np.ones(1, dtype), a, True)
            w = qh.tree(a[:, None], 0)[0]
            assert qh.same_bits(got, (a - w).astype(dtype)), (dtype, m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [1, 3, 8, W])
def test_the_blocked_plan_has_the_bits_of_the_unblocked_loop(ref, dtype, w):
    for m, n in ((1, 1), (2, 1), (5, 5), (10, 6), (w + 3, w + 1), (3 * w + 5, 2 * w + 1), (2 * w + 1, 2 * w + 1), (257, 3), (300, w + 1), (600, 40)):
        A = qh.random(m, n, dtype)
        QR, tau, z = ref.factor(A)
        got, tau_b, z_b = qh.blocked(A, w)
        assert z == z_b == 0 and got.dtype == tau_b.dtype == np.dtype(dtype)
        assert qh.same_bits(got, QR) and qh.same_bits(tau_b, tau), (m, n, w, qh.first_difference(got, QR))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_checker_is_a_qr(ref, dtype):
    """||A - Q R||_F <= m n u ||A||_F and ||Q'Q - I||_F <= m n u: the form of Higham's theorem 19.4 (Accuracy and Stability) with the
    constant 1; evaluated in float64.  Precision itself is held by the bit tests; this only says the loops are a QR at all."""
    u = qh.unit(dtype)
    for m, n in ((10, 6), (65, 65), (300, 33), (600, 40)):
        A = qh.random(m, n, dtype)
        QR, tau, z = ref.factor(A)
        Q, R = ref.thin_q(QR, tau).astype(np.float64), qh.upper(QR).astype(np.float64)
        r1 = np.linalg.norm(A.astype(np.float64) - Q @ R) / (u * np.linalg.norm(A.astype(np.float64)))
        r2 = np.linalg.norm(Q.T @ Q - np.eye(n)) / u
        assert z == 0 and r1 <= m * n and r2 <= m * n, f"{m} x {n} {np.dtype(dtype)}: ||A - QR|| = {r1:.2f} u ||A||, ||Q'Q - I|| = {r2:.2f} u (bound {m * n} u)"
        # lmul both ways against the thin Q, and the solve against the normal equations' answer: loose, in float64
        y = qh.vector(m, dtype)
        qty = ref.lmul(QR, tau, y, True).astype(np.float64)
        assert np.linalg.norm(qty[:n] - Q.T @ y) <= m * n * u * np.linalg.norm(y)
        assert np.linalg.norm(ref.lmul(QR, tau, qty.astype(dtype), False).astype(np.float64) - y) <= 2 * m * n * u * np.linalg.norm(y)
        x = ref.solve(QR, tau, y).astype(np.float64)
        want = np.linalg.lstsq(A.astype(np.float64), y.astype(np.float64), rcond=None)[0]
        assert np.linalg.norm(x - want) <= m * n * u * np.linalg.cond(A.astype(np.float64)) ** 2 * np.linalg.norm(want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_invariance(ref, dtype):
    for k in qh.scale_exponents(dtype):
        for m, n in ((10, 6), (2 * W + 1, W + 1), (300, 5)):
            qh.scaled_case(ref, m, n, dtype, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixtures_hold_their_preconditions(ref, dtype):
    for m, n in ((10, 6), (W + 9, W + 3)):
        A, QR, tau = qh.zero_below_case(ref, m, n, dtype, W)
        assert qh.same_bits(qh.blocked(A, W)[0], QR)                        # the tau == 0 skip, in the plan too
        for which in range(len(qh.SIGNS)):
            A, QR, tau = qh.signs_case(ref, m, n, dtype, which)
            assert qh.same_bits(qh.blocked(A, W)[0], QR)
        for k in (0, 2, n - 1):
            A, QR, tau = qh.zero_column_case(ref, m, n, dtype, k)
            assert qh.blocked(A, W)[2] == k + 1 and qh.same_bits(qh.blocked(A, W)[0], QR)
        A, QR, tau = qh.nonfinite_case(ref, m, n, dtype)
        got, tau_b, _ = qh.blocked(A, W)
        assert qh.same_bits(got, QR) and qh.same_bits(tau_b, tau)           # NaN in the same places
    A = qh.random(5, 5, dtype)                                              # square: the last column has no row below it
    QR, tau, z = ref.factor(A)
    assert tau[4] == 0 and z == 0
    A[:, 4] = 0
    assert ref.factor(A)[2] == 5                                            # ... and a zero there is R[5,5] == 0


def test_padding_is_never_read(ref):
    for dtype in DTYPES:
        A = qh.random(70, 40, dtype)
        assert qh.same_bits(ref.factor(A, ld=96)[0], ref.factor(A)[0])


def test_plan_launches():
    assert [qh.plan_launches(n, 32) for n in (1, 32, 33, 64, 65, 100)] == [1, 32, 34, 65, 67, 103]


# ---- refusals on a device-free double of the library ----------------------------------------------------------------------------------------
class FakeLib:
    """mik_dense_qr_* as the header states them, with no device"""

    def __init__(self, zero_diag=0):
        self.zero_diag = zero_diag
        self.created, self.calls, self.destroyed = [], [], 0

    def mik_dense_qr_create(self, ctx, A, m, n, ld, dtype, plan, col, out):
        self.created.append((m, n, ld, dtype, None if plan is None else plan._obj.value))
        col._obj.value = self.zero_diag
        out._obj.value = 0xC0FFEE
        return 0

    def mik_dense_qr_tau(self, h, tau):
        return 0

    def mik_dense_qr_destroy(self, h):
        self.destroyed += 1
        return 0

    def mik_last_error(self, ctx):
        return b"fake"

    def __getattr__(self, name):
        if not name.startswith("mik_dense_qr_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _double(cls, **fields):
    obj = object.__new__(cls)
    obj.__dict__.update(fields)
    return obj


def _matrix(pkg, n, cols, dtype):
    ctx = types.SimpleNamespace(handle=C.c_void_p(1))
    return _double(pkg.HipMatrix, n=n, cols=cols, ld=max(n, 1), dtype=np.dtype(dtype), ctx=ctx, buf=types.SimpleNamespace(ptr=4096))


def _vector(pkg, n, dtype):
    return _double(pkg.HipVector, n=n, dtype=np.dtype(dtype), ptr=8192, _owns=False, ctx=types.SimpleNamespace(handle=None))


def test_refusals_without_a_device(pkg, monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    for factor in (pkg.qr, pkg.qr_, pkg.ldiv):
        for bad in (np.eye(3), None, "A"):
            with pytest.raises(TypeError, match="HipMatrix"):
                factor(bad) if factor is not pkg.ldiv else factor(bad, None)
    for factor in (pkg.qr, pkg.qr_):
        with pytest.raises(ValueError, match="DimensionMismatch.*wide"):
            factor(_matrix(pkg, 4, 6, np.float64))
        for dtype in (np.complex128, np.complex64):
            with pytest.raises(TypeError, match=str(np.dtype(dtype))):
                factor(_matrix(pkg, 6, 4, dtype))
    with pytest.raises(ValueError, match="DimensionMismatch.*wide"):
        pkg.ldiv(_matrix(pkg, 4, 6, np.float64), _vector(pkg, 4, np.float64))
    assert fake.created == []                                               # refused before the library is reached
    for dtype in DTYPES:
        F = pkg.qr_(_matrix(pkg, 7, 5, dtype), resident_rows=3)
        assert (F.m, F.n, F.dtype, F.zero_diag) == (7, 5, np.dtype(dtype), 0) and fake.created[-1][4] == 3 and F.tau.shape == (5,)
        b, x = _vector(pkg, 7, dtype), _vector(pkg, 5, dtype)
        assert F.ldiv_(x, b) is x and F.ldiv_(b) is b and F.lmul_Q_(b) is b and F.lmul_Qt_(b) is b
        other = np.float32 if dtype != np.float32 else np.float64
        for call in (lambda: F.ldiv_(b, b.__class__), lambda: F.ldiv_(x, x), lambda: F.ldiv_(b, x), lambda: F.ldiv_(x, _vector(pkg, 7, other)),
                     lambda: F.ldiv_(_vector(pkg, 5, other), b), lambda: F.lmul_Q_(x), lambda: F.lmul_Qt_(_vector(pkg, 7, other)), lambda: F.solve(x),
                     lambda: F.ldiv_(x, _matrix(pkg, 7, 2, dtype)), lambda: F.lmul_Q_(np.zeros(7, dtype)), lambda: F.ldiv_(x, b, cols=1)):
            with pytest.raises(ValueError, match="DimensionMismatch"):
                call()
        del F
    assert fake.destroyed == 2 and fake.created[0][4] == 3
    F = pkg.qr_(_matrix(pkg, 7, 5, np.float64))
    assert fake.created[-1][4] is None                                      # no plan: NULL
    F.handle = None


def test_zero_diagonal_refuses_to_solve_without_a_device(pkg, monkeypatch):
    fake = FakeLib(zero_diag=3)
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    F = pkg.qr_(_matrix(pkg, 7, 5, np.float64))                             # qr! does not throw
    assert F.zero_diag == 3
    b, x = _vector(pkg, 7, np.float64), _vector(pkg, 5, np.float64)
    for call in (lambda: F.ldiv_(x, b), lambda: F.ldiv_(b), lambda: F.ldiv_(_matrix(pkg, 5, 2, np.float64), _matrix(pkg, 7, 2, np.float64))):
        with pytest.raises(pkg.SingularException) as ei:
            call()
        assert ei.value.col == 3 and "SingularException(3)" in str(ei.value)
    assert not [c for c in fake.calls if "solve" in c]                      # refused before the library is reached
    assert F.lmul_Q_(b) is b and F.lmul_Qt_(b) is b and fake.calls == ["mik_dense_qr_lmul"] * 2          # the products still work
    F.handle = None


def test_precond_binding_takes_a_square_qr_only(pkg, monkeypatch):
    """_Bound.precond checks the shape, n and dtype where the callback is bound: the callback itself never sees a length"""
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    F = pkg.qr_(_matrix(pkg, 5, 5, np.float64))
    for n, dtype in ((6, np.float64), (5, np.float32)):
        with pytest.raises(ValueError, match="DimensionMismatch.*qr"):
            pkg.api._Bound.precond(types.SimpleNamespace(n=n, dtype=np.dtype(dtype), keep=[]), F)
    T = pkg.qr_(_matrix(pkg, 7, 5, np.float64))
    with pytest.raises(ValueError, match="DimensionMismatch.*qr.*7 x 5"):
        pkg.api._Bound.precond(types.SimpleNamespace(n=5, dtype=np.dtype(np.float64), keep=[]), T)
    F.handle = T.handle = None
