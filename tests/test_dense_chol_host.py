"""The checker of the dense Cholesky tests (tests/dense_ref/dense_chol_ref.c, the bit contract restated as unblocked loops in all four
element types) against what needs no device: the exactly representable fixture, a blocked numpy restatement of the three-launch device
plan, an a-priori backward error bound, the failure fixtures, and -- on a device-free double of the library -- the refusals and
check=False of iterativesolvers.jl_amd/dense_chol.py."""
import ctypes as C
import types

import numpy as np
import pytest

import dense_chol_host as ch

DTYPES = ch.DTYPES
W = 64                                  # the panel width the kernels are written for today; the claims below hold at any W


@pytest.fixture(autouse=True)
def feature(pkg):
    """the checker states the contract of pkg.cholesky: without the feature nothing here has a subject"""
    assert callable(getattr(pkg, "cholesky", None)) and callable(getattr(pkg, "cholesky_", None)) and hasattr(pkg.lib(), "mik_dense_chol_create")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("dense_chol_ref"))


def test_same_bits():
    for dtype in DTYPES:
        a = np.array([1.0, -0.0, 0.0, np.nan, np.inf, -np.inf], dtype)
        assert ch.same_bits(a, a.copy()) and ch.first_difference(a, a.copy()) == []
        for i, v in ((1, 0.0), (2, -0.0), (3, 1.0), (0, np.nan), (4, -np.inf)):
            b = a.copy()
            b[i] = v
            assert not ch.same_bits(a, b), (dtype, i, v)
        assert not ch.same_bits(a, a[:5])
    z = np.array([1 + 2j, complex(3.0, -0.0)], np.complex128)
    w = z.copy()
    w[1] = complex(3.0, 0.0)
    assert np.array_equal(z, w) and not ch.same_bits(z, w)                  # the sign of a zero imaginary part, which == does not see
    assert not ch.same_bits(z, z.astype(np.complex64)) and not ch.same_bits(np.arange(3), np.arange(3))


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_on_the_exact_fixture(ref, dtype):
    """the anchor that shares no code with anything: the factor is L, the solve returns x, with equality"""
    for n in (1, 2, 7, 65, 130):
        A, L, x, b = ch.exact(n, dtype)
        out, info = ref.factor(A)
        assert info == 0 and out.dtype == np.dtype(dtype)
        assert np.array_equal(ch.lower(out), L), n
        assert ch.same_bits(np.diag(out).imag.astype(ch.real_of(dtype)), np.zeros(n, ch.real_of(dtype)))       # +0, not -0
        assert np.array_equal(out[np.triu_indices(n, 1)], A[np.triu_indices(n, 1)])                            # never written
        assert np.array_equal(ref.solve(out, b), x), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_checker_reads_the_lower_triangle_and_the_real_diagonal_only(ref, dtype):
    n = 70
    A = ch.hpd(n, dtype)
    out, info = ref.factor(A)
    P = ch.poisoned(A)
    if ch.is_complex(dtype):
        P.imag[np.arange(n), np.arange(n)] = np.nan                         # the imaginary parts of the diagonal are not read either
    got, info_p = ref.factor(P, ld=96)                                      # ... nor the padding rows
    assert info == 0 and info_p == 0 and np.isfinite(ch.lower(out)).all()
    assert ch.same_bits(ch.lower(got), ch.lower(out))
    b = ch.vector(n, dtype)
    assert ch.same_bits(ref.solve(got, b), ref.solve(out, b))               # the solve does not read them either


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [4, 8])
def test_the_blocked_plan_has_the_bits_of_the_unblocked_loop(ref, dtype, w):
    """diagonal block, rows below it, lower trailing update: k stays ascending per element, and the diagonal treated like any other
    element of the trailing update subtracts exactly lr lr + li li.  This is the claim the device plan rests on."""
    for n in (w - 1, w, w + 1, 2 * w + 1, 5 * w + 3):
        A = ch.hpd(n, dtype)
        out, info = ref.factor(A)
        got, info_b = ch.blocked(A, w)
        assert info == 0 and info_b == 0 and got.dtype == np.dtype(dtype)
        assert ch.same_bits(got, out), (n, w, ch.first_difference(got, out))


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
def test_blocked_plan_at_the_device_width(ref, dtype):
    for n in (W - 1, W, W + 1, 2 * W + 1):
        A = ch.hpd(n, dtype)
        assert ch.same_bits(ch.blocked(A, W)[0], ref.factor(A)[0]), n


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
def test_backward_error_within_the_a_priori_bound(ref, dtype):
    """Each real component of A - L L^H stays within gamma_{4 (n + 1)} (|L| |L^H|), |.| the modulus.  Higham (Accuracy and Stability,
    theorem 10.3) has gamma_{n + 1} for the real loop: a chain of at most n terms, each with one rounded product and one rounded
    subtraction, closed by a division or a square root.  In a complex multiply-subtract a component of a term sees THREE roundings -- the
    product, the sum or difference of the two products, the subtraction -- and the magnitude it is relative to, |zr wr| + |zi wi| or
    |zr wi| + |zi wr|, is at most |z| |w| (Cauchy-Schwarz); the closing division is one more rounding.  That gives gamma_{3 (n + 1)}; the
    four is a generous count of the real roundings per complex multiply-subtract, derived and not tuned -- anyone tightening it must give
    the derivation.  Evaluated in float64 from the checker's factor."""
    for n in (W + 1, 130):
        A = ch.hpd(n, dtype)
        out, info = ref.factor(A)
        assert info == 0
        wide = np.complex128 if ch.is_complex(dtype) else np.float64
        L = ch.lower(out).astype(wide)
        Ah = np.tril(A.astype(wide))
        delta = np.tril(L @ L.conj().T) - Ah
        resid = np.maximum(np.abs(delta.real), np.abs(delta.imag))
        bound = ch.gamma(4 * (n + 1), dtype) * (np.abs(L) @ np.abs(L).conj().T)
        assert (resid <= np.tril(bound)).all(), (n, float((resid / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ch.FAILURES)
def test_checker_reports_the_first_failing_column(ref, dtype, kind):
    n = 130
    for k in ch.failure_columns(n, W):
        A, out, info = ch.failing_case(ref, n, dtype, k, kind)
        L = ch.exact(n, dtype)[1]
        assert np.array_equal(ch.lower(out)[:, :k], L[:, :k])               # the columns before the failure are complete
        assert ch.blocked(A, W)[1] == info                                  # the plan records the same column, whatever runs after it


def test_plan_launches():
    assert [ch.plan_launches(n, 64) for n in (1, 64, 65, 128, 129, 323)] == [1, 1, 4, 4, 7, 16]


# ---- the fixtures of tests/test_gpu_dense_chol_edges.py: each builder's own preconditions, once per element type at W ---------------------
def test_width_sizes_visit_every_width_of_a_last_panel():
    sizes = ch.width_sizes(W)
    assert sizes == sorted(set(sizes)) and len(sizes) == 2 * W + 2
    assert {n for n in sizes if n <= W} == set(range(1, W + 1)) and {n - W for n in sizes if W < n <= 2 * W} == set(range(1, W + 1))
    for m in (15, 16, 17, 31, 32, 33):                                      # one short of, at and one past a batch of 16 and a chunk of 32
        assert m in sizes and W + m in sizes
    assert 2 * W in sizes and 3 * W in sizes and 3 * W + 17 in sizes
    assert [ch.plan_launches(n, W) for n in (2 * W, 3 * W, 3 * W + 17)] == [4, 7, 10]


@pytest.mark.parametrize("dtype", DTYPES)
def test_report_columns_fail_where_they_say(ref, dtype):
    n = 130
    cols = ch.report_columns(n, W)
    assert cols == (1, 2, 3, 63, 65, 66, 67, 127) and not set(cols) & set(ch.failure_columns(n, W))
    L = ch.exact(n, dtype)[1]
    for k in cols:
        A, out, info = ch.failing_case(ref, n, dtype, k, "negative")
        assert info == k + 1 and np.array_equal(ch.lower(out)[:, :k], L[:, :k])
        assert ch.blocked(A, W)[1] == info


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_scaled_case_holds_its_preconditions(ref, dtype, which):
    s = ch.scales(dtype)
    f = np.finfo(ch.real_of(dtype))
    assert all(v.dtype == ch.real_of(dtype) for v in s) and 0 < s[0] < s[1] < f.tiny and f.max / 2 ** 13 < s[2] < f.max
    A, out, b, want = ch.scaled_case(ref, dtype, W, which)
    assert A.shape == (2 * W + 1, 2 * W + 1) and A.flags.f_contiguous and out.dtype == A.dtype == b.dtype == want.dtype == np.dtype(dtype)
    if which == 1:                                                          # here the diagonal is normal: most of the rest is not
        assert (np.diag(A).real >= f.tiny).all()
    if which < 2:                                                           # flushing the subnormal operands alone already changes the factor
        flushed = A.copy(order="F")
        for part in ((flushed.real, flushed.imag) if ch.is_complex(dtype) else (flushed,)):
            part[np.abs(part) < f.tiny] = 0
        got, info = ref.factor(flushed)
        assert info != 0 or not ch.same_bits(ch.lower(got), ch.lower(out))


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
def test_blocked_plan_at_the_smallest_scale(ref, dtype):
    """the plan's claim -- an element meets its k in the loop's order -- does not lean on the magnitudes: subnormal operands, same bits"""
    A, out, _, _ = ch.scaled_case(ref, dtype, W, 0)
    got, info = ch.blocked(A, W)
    assert info == 0 and ch.same_bits(got, out), ch.first_difference(got, out)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_imag_poisoned_diagonal_on_the_checker(ref, dtype):
    n = 2 * W + W + 1
    A = ch.hpd(n, dtype)
    for p in ch.poisons(dtype) + (7,):
        P, out = ch.imag_poisoned_case(ref, A, p)
        d = np.diag(P).imag
        assert (np.isnan(d).all() if np.isnan(p) else (d == p).all()) and ch.same_bits(np.tril(P, -1), np.tril(A, -1))
        b = ch.vector(n, dtype)
        assert ch.same_bits(ref.solve(ref.factor(P)[0], b), ref.solve(out, b))
    with pytest.raises(AssertionError):
        ch.imag_poisoned(ch.hpd(3, np.float64), np.nan)                     # a real matrix has nothing to poison there


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_upper_triangle_on_the_checker(ref, dtype):
    n = 2 * W + W + 1
    A = ch.hpd(n, dtype)
    ps = ch.poisons(dtype)
    assert np.isnan(ps[0]) and np.isinf(ps[1]) and ps[2] == np.finfo(ch.real_of(dtype)).max
    for p in ps:
        P, out = ch.poisoned_case(ref, A, p)
        iu = np.triu_indices(n, 1)
        comp = ch._components(P[iu])
        assert np.isnan(comp).all() if np.isnan(p) else (comp == p).all()
        assert ch.same_bits(np.tril(P), np.tril(A))


# ---- refusals and check=False on a device-free double of the library ---------------------------------------------------------------------
class FakeLib:
    """mik_dense_chol_* as the header states them, with no device: create reports `fail_at` the way `check` asks for"""

    def __init__(self, fail_at=0):
        self.fail_at = fail_at
        self.created, self.solved, self.destroyed = [], 0, 0

    def mik_dense_chol_create(self, ctx, A, n, ld, dtype, check, col, out):
        self.created.append((n, ld, dtype, check))
        col._obj.value = self.fail_at
        if self.fail_at and check:
            return 8
        out._obj.value = 0xC0FFEE
        return 0

    def mik_dense_chol_solve(self, h, y, x):
        self.solved += 1
        return 1 if self.fail_at else 0

    def mik_dense_chol_destroy(self, h):
        self.destroyed += 1
        return 0

    def mik_last_error(self, ctx):
        return b"fake"


def _double(pkg, cls, **fields):
    obj = object.__new__(cls)
    obj.__dict__.update(fields)
    return obj


def _matrix(pkg, n, cols, dtype):
    ctx = types.SimpleNamespace(handle=C.c_void_p(1))
    return _double(pkg, pkg.HipMatrix, n=n, cols=cols, ld=max(n, 1), dtype=np.dtype(dtype), ctx=ctx, buf=types.SimpleNamespace(ptr=4096))


def _vector(pkg, n, dtype):
    return _double(pkg, pkg.HipVector, n=n, dtype=np.dtype(dtype), ptr=8192, _owns=False, ctx=types.SimpleNamespace(handle=None))


def test_refusals_without_a_device(pkg, monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    for factor in (pkg.cholesky, pkg.cholesky_):
        for bad in (np.eye(3), None, "A"):
            with pytest.raises(TypeError, match="HipMatrix"):
                factor(bad)
        with pytest.raises(ValueError, match="DimensionMismatch"):
            factor(_matrix(pkg, 6, 4, np.float64))
    assert fake.created == []                                               # refused before the library is reached
    for dtype in DTYPES:                                                    # all four element types are admitted
        F = pkg.cholesky_(_matrix(pkg, 5, 5, dtype))
        assert F.info == 0 and F.issuccess() and F.uplo == "L" and F.n == 5 and F.dtype == np.dtype(dtype)
        v = _vector(pkg, 5, dtype)
        assert F.ldiv_(v) is v and F.ldiv_(v, _vector(pkg, 5, dtype)) is v
        for bad in (_vector(pkg, 6, dtype), _vector(pkg, 5, np.float32 if dtype != np.float32 else np.float64), np.zeros(5, dtype)):
            for call in (lambda: F.ldiv_(v, bad), lambda: F.ldiv_(bad, v), lambda: F.ldiv_(bad)):
                with pytest.raises(ValueError, match="DimensionMismatch"):
                    call()
        del F                                                               # destroyed while the double is still in place
    assert fake.destroyed == 4
    assert [c[3] for c in fake.created] == [1] * 4 and [c[2] for c in fake.created] == [pkg._lib.dtype_code(np.dtype(d)) for d in DTYPES]


def test_posdef_exception_and_check_false_without_a_device(pkg, monkeypatch):
    assert issubclass(pkg.PosDefException, np.linalg.LinAlgError) and not issubclass(pkg.PosDefException, pkg.SingularException)
    fake = FakeLib(fail_at=7)
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    A = _matrix(pkg, 9, 9, np.complex64)
    with pytest.raises(np.linalg.LinAlgError) as ei:
        pkg.cholesky_(A)
    assert isinstance(ei.value, pkg.PosDefException) and ei.value.k == 7 and "PosDefException(7)" in str(ei.value)
    F = pkg.cholesky_(A, check=False)                                       # never raises for a matrix that is not positive definite
    assert F.factors is A and F.info == 7 and not F.issuccess() and fake.created[-1][3] == 0
    v = _vector(pkg, 9, np.complex64)
    for call in (lambda: F.ldiv_(v), lambda: F.ldiv_(v, _vector(pkg, 9, np.complex64))):
        with pytest.raises(pkg.MikError) as ei:
            call()
        assert ei.value.code == 1 and "PosDefException(7)" in str(ei.value)
    assert fake.solved == 0                                                 # refused before the library is reached
    F.handle = None                                                         # the double's handle must never reach the library


def test_precond_binding_refuses_a_wrong_size_or_type(pkg, monkeypatch):
    """_Bound.precond checks n and dtype where the callback is bound: the callback itself never sees a length"""
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    F = pkg.cholesky_(_matrix(pkg, 5, 5, np.float64))
    bound = types.SimpleNamespace(n=6, dtype=np.dtype(np.float64), keep=[])
    with pytest.raises(ValueError, match="DimensionMismatch.*cholesky"):
        pkg.api._Bound.precond(bound, F)
    bound = types.SimpleNamespace(n=5, dtype=np.dtype(np.float32), keep=[])
    with pytest.raises(ValueError, match="DimensionMismatch.*cholesky"):
        pkg.api._Bound.precond(bound, F)
    F.handle = None
