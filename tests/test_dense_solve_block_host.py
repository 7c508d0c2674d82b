"""Block solves of the dense LU and Cholesky (F.ldiv_(Y, X) on two HipMatrix), the part that needs no device: the block plan restated in
plain Python, the Python argument checks on a device-free double of the library, and that the C checker applied column by column --
what tests/test_gpu_dense_solve_block.py compares the device against -- is what a solve of the whole block computes."""
import ctypes as C
import types

import numpy as np
import pytest

import dense_chol_host as ch
import dense_lu_host as lu
import dense_solve_block_host as sb

W = 64                                  # the panel width the kernels are written for today; the claims below hold at any W
SHAPES = ((2, 32), (1, 32), (8, 32))    # (NB, G) of the real and of the complex types today, and a wider group


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NB,G", SHAPES)
def test_the_widths_visit_a_partial_group_several_groups_and_a_second_pass(NB, G):
    seen = {w: sb.plan(5 * W + 3, w, W, NB, G, 8, False) for w in sb.widths(NB, G)}
    assert set(seen) == {1, 2, NB - 1, NB, NB + 1, 2 * NB + 1, G, G + 1} - {0} and min(seen) == 1 and max(seen) == G + 1
    assert seen[1]["groups"] == [(1, 1)] and seen[NB]["groups"] == [(1, NB)]
    assert seen[NB + 1]["groups"] == [(2, 1)] and seen[2 * NB + 1]["groups"] == [(3, 1)]                 # a last group of one live column
    assert seen[G]["groups"] == [(G // NB, NB)] and seen[G]["passes"] == 1
    assert seen[G + 1]["groups"] == [(G // NB, NB), (1, 1)] and seen[G + 1]["passes"] == 2               # the second pass
    assert (NB == 1) != any(0 < last < NB for p in seen.values() for _, last in p["groups"])             # a partial last group, wherever there can be one


@pytest.mark.parametrize("NB,G", SHAPES)
@pytest.mark.parametrize("gather", (False, True))
def test_a_pass_is_the_launches_of_one_vector_solve(NB, G, gather):
    for n in sb.sizes(W):
        one = sb.vector_launches(n, W, gather)
        assert one == (1 if gather else 0) + 2 * ((n + W - 1) // W)
        for w in sb.widths(NB, G) + [3 * G, 3 * G + 1]:
            p = sb.plan(n, w, W, NB, G, 16, gather)
            assert p["passes"] == (w + G - 1) // G and p["launches"] == p["passes"] * one
            assert p["workspace_bytes"] == n * G * 16                                                     # whatever the width: allocated once
            assert sum((g - 1) * NB + last for g, last in p["groups"]) == w                               # every column is in one group
            assert all(1 <= last <= NB and g <= G // NB for g, last in p["groups"])
    assert sb.plan(5, 0, W, NB, G, 8, gather)["passes"] == 0 and sb.plan(5, -3, W, NB, G, 8, gather)["launches"] == 0
    assert sb.sizes(W) == [1, 2, 63, 64, 65, 129, 323]


# ---- the checker column by column is a solve of the block ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chol_ref(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("dense_chol_ref_block"))


@pytest.fixture(scope="module")
def lu_ref(tmp_path_factory):
    return lu.build(tmp_path_factory.mktemp("dense_lu_ref_block"))


@pytest.mark.parametrize("dtype", ch.DTYPES)
def test_a_blocked_cholesky_solve_of_two_columns_is_two_checker_solves(chol_ref, dtype):
    n = 37
    L, info = chol_ref.factor(ch.hpd(n, dtype))
    assert info == 0
    B = sb.rhs(n, 2, dtype)
    want = sb.per_column(lambda b: chol_ref.solve(L, b), B)
    assert np.isfinite(want).all()
    got = sb.chol_solve_block(L, B)
    assert ch.same_bits(got, want), ch.first_difference(got, want)
    B[5, 1] = np.nan                                                        # one poisoned column leaves the other one's bits alone
    got, want = sb.chol_solve_block(L, B), sb.per_column(lambda b: chol_ref.solve(L, b), B)
    assert ch.same_bits(got, want) and np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1]).any()


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_a_blocked_lu_solve_of_two_columns_is_two_checker_solves(lu_ref, dtype):
    n = 37
    LU, ipiv, singular = lu_ref.factor(lu.random(n, dtype))
    perm = lu.permutation_of(ipiv)
    assert singular == 0 and np.count_nonzero(perm != np.arange(n)) > n // 2
    B = sb.rhs(n, 2, dtype)
    want = sb.per_column(lambda b: lu_ref.solve(LU, ipiv, b), B)
    assert np.isfinite(want).all()
    got = sb.lu_solve_block(LU, perm, B)
    assert lu.same_bits(got, want), lu.first_difference(got, want)


# ---- the Python argument checks on a device-free double of the library ------------------------------------------------------------------
class FakeLib:
    """the create / solve / solve_block / block_plan / destroy entries of both factorisations as the headers state them, with no device"""

    def __init__(self, fail_at=0):
        self.fail_at = fail_at
        self.vector, self.block = [], []

    def _create(self, col, out):
        col._obj.value = self.fail_at
        out._obj.value = 0xC0FFEE
        return 0

    def mik_dense_chol_create(self, ctx, A, n, ld, dtype, check, col, out):
        return self._create(col, out)

    def mik_dense_lu_create(self, ctx, A, n, ld, dtype, col, out):
        return self._create(col, out)

    def mik_dense_lu_ipiv(self, h, ipiv):
        return 0

    def _solve(self, h, y, x):
        self.vector.append((y.value, x.value))
        return 0

    def _solve_block(self, h, Y, ldy, X, ldx, nrhs):
        self.block.append((Y.value, ldy, X.value, ldx, nrhs))
        return 0

    def _plan(self, h, nrhs, nb, g, passes, launches, nbytes):
        for ref, v in zip((nb, g, passes, launches, nbytes), (8, 32, -(-nrhs // 32), 7 * -(-nrhs // 32), 4096)):
            ref._obj.value = v
        return 0

    mik_dense_chol_solve = mik_dense_lu_solve = _solve
    mik_dense_chol_solve_block = mik_dense_lu_solve_block = _solve_block
    mik_dev_dense_chol_block_plan = mik_dev_dense_lu_block_plan = _plan

    def mik_dense_chol_destroy(self, h):
        return 0

    mik_dense_lu_destroy = mik_dense_chol_destroy

    def mik_last_error(self, ctx):
        return b"fake"


def _double(cls, **fields):
    obj = object.__new__(cls)
    obj.__dict__.update(fields)
    return obj


def _matrix(pkg, n, cols, dtype, ld=None, ptr=4096):
    ctx = types.SimpleNamespace(handle=C.c_void_p(1))
    return _double(pkg.HipMatrix, n=n, cols=cols, ld=ld or max(n, 1), dtype=np.dtype(dtype), ctx=ctx, buf=types.SimpleNamespace(ptr=ptr))


def _vector(pkg, n, dtype):
    return _double(pkg.HipVector, n=n, dtype=np.dtype(dtype), ptr=8192, _owns=False, ctx=types.SimpleNamespace(handle=None))


FACTORS = (("cholesky_", np.complex64), ("cholesky_", np.float64), ("lu_", np.float32))


@pytest.mark.parametrize("factor,dtype", FACTORS)
def test_block_ldiv_reaches_the_block_entry_with_both_leading_dimensions(pkg, monkeypatch, factor, dtype):
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    if factor == "lu_":
        monkeypatch.setattr(pkg.dense_lu, "lib", lambda: fake)
    F = getattr(pkg, factor)(_matrix(pkg, 5, 5, dtype))
    Y, X = _matrix(pkg, 5, 9, dtype, ld=64, ptr=1 << 20), _matrix(pkg, 5, 7, dtype, ld=128, ptr=2 << 20)
    assert F.ldiv_(Y, X) is Y and fake.block[-1] == (1 << 20, 64, 2 << 20, 128, 7)                       # all of X
    assert F.ldiv_(Y, X, cols=3) is Y and fake.block[-1] == (1 << 20, 64, 2 << 20, 128, 3)               # its leading columns
    assert F.ldiv_(Y, cols=9) is Y and fake.block[-1] == (1 << 20, 64, 1 << 20, 64, 9)                   # ldiv!(F, Y)
    assert F.ldiv_(Y) is Y and fake.block[-1][4] == 9 and fake.vector == []
    v = _vector(pkg, 5, dtype)
    assert F.ldiv_(v) is v and fake.vector == [(8192, 8192)] and len(fake.block) == 4                    # vectors keep the vector entry
    assert F.block_plan(33) == {"NB": 8, "G": 32, "passes": 2, "launches": 14, "workspace_bytes": 4096}
    F.handle = None


@pytest.mark.parametrize("factor,dtype", FACTORS)
def test_block_ldiv_refusals_without_a_device(pkg, monkeypatch, factor, dtype):
    fake = FakeLib()
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    if factor == "lu_":
        monkeypatch.setattr(pkg.dense_lu, "lib", lambda: fake)
    F = getattr(pkg, factor)(_matrix(pkg, 5, 5, dtype))
    other = np.float32 if np.dtype(dtype) != np.float32 else np.float64
    Y, X, v = _matrix(pkg, 5, 4, dtype), _matrix(pkg, 5, 6, dtype), _vector(pkg, 5, dtype)
    calls = [lambda: F.ldiv_(Y, v), lambda: F.ldiv_(v, X),                                               # a vector and a matrix
             lambda: F.ldiv_(_matrix(pkg, 6, 6, dtype), X), lambda: F.ldiv_(X, _matrix(pkg, 4, 6, dtype)), lambda: F.ldiv_(_matrix(pkg, 6, 6, dtype)),    # rows
             lambda: F.solve(_matrix(pkg, 6, 2, dtype)),
             lambda: F.ldiv_(_matrix(pkg, 5, 6, other), X), lambda: F.ldiv_(X, _matrix(pkg, 5, 6, other)), lambda: F.solve(_matrix(pkg, 5, 2, other)),    # dtype
             lambda: F.ldiv_(Y, X), lambda: F.ldiv_(Y, X, cols=5), lambda: F.ldiv_(X, Y, cols=5),        # too few columns in Y, or in X
             lambda: F.ldiv_(X, X, cols=0), lambda: F.ldiv_(X, cols=-1), lambda: F.ldiv_(X, X, cols=7),
             lambda: F.ldiv_(X, np.zeros((5, 6), dtype)), lambda: F.ldiv_(v, v, cols=1)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            call()
    assert fake.block == [] and fake.vector == []                                                         # refused before the library is reached
    assert F.ldiv_(X, Y, cols=4) is X and F.ldiv_(Y, X, cols=4) is Y and len(fake.block) == 2
    F.handle = None


def test_a_failed_cholesky_refuses_a_block_before_the_library(pkg, monkeypatch):
    fake = FakeLib(fail_at=3)
    monkeypatch.setattr(pkg.dense_factor, "lib", lambda: fake)
    F = pkg.cholesky_(_matrix(pkg, 5, 5, np.float64), check=False)
    assert F.info == 3
    X = _matrix(pkg, 5, 2, np.float64)
    for call in (lambda: F.ldiv_(X), lambda: F.ldiv_(X, _matrix(pkg, 5, 2, np.float64, ptr=1 << 20))):
        with pytest.raises(pkg.MikError) as ei:
            call()
        assert ei.value.code == 1 and "PosDefException(3)" in str(ei.value)
    assert fake.block == []
    F.handle = None


def test_lobpcg_gives_a_dense_factor_one_block_call_and_everything_else_one_call_per_column(pkg):
    """DeviceOps.precond: a DenseFactor solves the first bs columns of the block in place in one call; any other object with ldiv_ keeps
    the per-column path (a solve into temp, a copy back)"""
    lob = __import__(pkg.__name__ + ".lobpcg", fromlist=["DeviceOps"])
    calls = []

    class Col:
        def __init__(self, j):
            self.j = j

        def copyto_(self, src):
            calls.append(("copy", self.j, src.j))

    class Block:
        def col(self, j):
            return Col(j)

    class Routed(pkg.dense_factor.DenseFactor):
        def ldiv_(self, y, x=None, cols=None):
            calls.append(("block", y, x, cols))

    class PerColumn:
        def ldiv_(self, y, x):
            calls.append(("vector", y.j, x.j))

    ops = object.__new__(lob.DeviceOps)
    X, temp = Block(), Block()
    routed = object.__new__(Routed)
    ops.precond(routed, X, 3, temp)
    assert calls == [("block", X, None, 3)]
    del calls[:]
    assert routed.block_min_cols >= 1
    ops.precond(routed, X, routed.block_min_cols - 1, temp)                 # narrower than the measured break-even: the per-column path
    assert [c[0] for c in calls] == ["block", "copy"] * (routed.block_min_cols - 1)
    del calls[:]
    ops.precond(PerColumn(), X, 2, temp)
    assert calls == [("vector", 0, 0), ("copy", 0, 0), ("vector", 1, 1), ("copy", 1, 1)]
