"""F.ldiv_(Y, X) / F.solve(B) on a block of right-hand sides (two HipMatrix) for lu(A) and cholesky(A) on a dense device matrix
(mik_dense_lu_solve_block / mik_dense_chol_solve_block): column j of the result has exactly the bits of the vector solve of column j.
The checkers are tests/dense_ref/dense_lu_ref.c and dense_chol_ref.c applied column by column; every comparison of device values with
them, and with F.ldiv_(y, x) on a column, is same_bits (NaN positions, and the bits everywhere else).  Every shape comes from the
library: W from F.info() / F.plan(), NB, G, passes and launches from F.block_plan."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dense_chol_host as ch
import dense_lu_host as lu
import dense_solve_block_host as sb

pytestmark = pytest.mark.gpu

POISON = -7.25                          # what memory that must not be written is filled with (both components in the complex types)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return {"lu": lu.build(tmp_path_factory.mktemp("dense_lu_ref_block_gpu")), "chol": ch.build(tmp_path_factory.mktemp("dense_chol_ref_block_gpu"))}


# ---- a factorisation on the device and on the checker ------------------------------------------------------------------------------------
class Case:
    """A, its device factorisation F, and `solve`: the checker's ldiv! of one column from the checker's own factors"""

    def __init__(self, pkg, refs, kind, A):
        self.kind, self.A, self.n, self.dtype = kind, A, A.shape[0], A.dtype
        M = pkg.HipMatrix.from_numpy(A)
        if kind == "lu":
            LU, ipiv, singular = refs["lu"].factor(A)
            assert singular == 0
            self.F, self.perm = pkg.lu(M), lu.permutation_of(ipiv)
            self.W, self.vector_launches = self.F.info()["W"], self.F.info()["launches_solve"]
            self.solve = lambda b: refs["lu"].solve(LU, ipiv, b)
        else:
            L, info = refs["chol"].factor(A)
            assert info == 0
            self.F = pkg.cholesky(M)
            self.W, self.vector_launches = self.F.plan()["W"], self.F.plan()["launches_solve"]
            self.solve = lambda b: refs["chol"].solve(L, b)


FIXTURES = [("lu", "dominant", np.float64), ("lu", "dominant", np.float32), ("lu", "random", np.float64), ("lu", "random", np.float32)] + \
           [("chol", "hpd", d) for d in ch.DTYPES]
_MATRIX = {"dominant": lu.dominant, "random": lu.random, "hpd": ch.hpd}


def panel_width(pkg, kind, dtype):
    F = (pkg.lu if kind == "lu" else pkg.cholesky)(pkg.HipMatrix.from_numpy(np.ones((1, 1), dtype)))
    return (F.info() if kind == "lu" else F.plan())["W"]


def poison_of(dtype):
    return ch.poison_of(dtype, POISON)


def device_block(pkg, host, ld):
    """a HipMatrix of host's shape on a leading dimension of its own (ld > n), its padding rows POISON"""
    n, cols = host.shape
    assert ld > n
    M = pkg.HipMatrix(n, cols, host.dtype)
    M.ld, M.buf = ld, pkg.HipVector(ld * cols, host.dtype, M.ctx)
    M.buf.copy_from_host(sb.padded(host, ld, poison_of(host.dtype)).ravel(order="F"))
    return M


def read(M):
    """every element of M's buffer, padding rows included, as an ld x cols array"""
    return M.buf.to_numpy().reshape((M.ld, M.cols), order="F")


def lds(n):
    """(ld of X, ld of Y): different, both larger than n"""
    base = (n + 63) // 64 * 64
    return base + 128, base + 64


def check_plan(case, w):
    """the plan of w columns on this handle: asserted first, against its restatement in plain Python"""
    p = case.F.block_plan(w)
    want = sb.plan(case.n, w, case.W, p["NB"], p["G"], np.dtype(case.dtype).itemsize, case.kind == "lu")
    assert p == sb.reported(want), (case.n, w, p, want)
    assert p["passes"] == -(-w // p["G"]) and p["launches"] == p["passes"] * case.vector_launches
    return p


@pytest.mark.parametrize("kind,fixture,dtype", FIXTURES)
def test_every_size_and_width_bit_for_bit(pkg, ctx, refs, kind, fixture, dtype):
    """Per size one block of G + 1 columns, its checker solutions and its vector solves once; per width a fresh poisoned Y of G + 3 columns on
    another leading dimension: the leading columns have the checker's bits and the vector solve's, every other element keeps its poison."""
    for n in sb.sizes(panel_width(pkg, kind, dtype)):
        case = Case(pkg, refs, kind, _MATRIX[fixture](n, dtype))
        F = case.F
        first = F.block_plan(1)
        NB, G = first["NB"], first["G"]
        assert 1 <= NB <= G and G % NB == 0 and first["workspace_bytes"] == n * G * np.dtype(dtype).itemsize
        bytes_before = (F.info() if kind == "lu" else F.plan())["bytes"]
        B = sb.rhs(n, G + 1, dtype)
        want = sb.per_column(case.solve, B)
        assert np.isfinite(want).all()
        ldx, ldy = lds(n)
        X = device_block(pkg, B, ldx)
        x_before = read(X)
        vec = np.zeros_like(want)
        y = pkg.HipVector(n, dtype)
        for j in range(G + 1):                                                 # F.ldiv_(y, x) on every column
            F.ldiv_(y, X.col(j))
            vec[:, j] = y.to_numpy()
        assert ch.same_bits(vec, want), (n, ch.first_difference(vec, want))
        blank = np.full((n, G + 3), poison_of(dtype), dtype, order="F")
        for w in sb.widths(NB, G):
            check_plan(case, w)
            Y = device_block(pkg, blank, ldy)
            assert F.ldiv_(Y, X, cols=w) is Y
            got = read(Y)
            assert ch.same_bits(got[:n, :w], want[:, :w]), (n, w, ch.first_difference(got[:n, :w], want[:, :w]))
            assert ch.same_bits(got[:n, :w], vec[:, :w])
            assert (got[n:, :] == poison_of(dtype)).all() and (got[:, w:] == poison_of(dtype)).all(), (n, w)      # padding rows, columns from cols on
        assert ch.same_bits(read(X), x_before)                                 # X is untouched in the two-argument form
        for w in (NB + 1, G + 1):                                              # in place: ldiv!(F, X) on the leading w columns
            Z = device_block(pkg, B, ldx)
            assert F.ldiv_(Z, cols=w) is Z
            got = read(Z)
            assert ch.same_bits(got[:n, :w], want[:, :w]), (n, w, ch.first_difference(got[:n, :w], want[:, :w]))
            assert ch.same_bits(got[:n, w:], B[:, w:]) and (got[n:, :] == poison_of(dtype)).all()
        S = F.solve(pkg.HipMatrix.from_numpy(B[:, :NB + 1]))                   # F \ B: a new matrix
        assert isinstance(S, pkg.HipMatrix) and (S.n, S.cols) == (n, NB + 1) and ch.same_bits(S.to_numpy(), want[:, :NB + 1])
        assert (F.info() if kind == "lu" else F.plan())["bytes"] == bytes_before       # what the _info entries report is unchanged


@pytest.mark.parametrize("kind,fixture,dtype", FIXTURES[2:])
def test_non_finite_right_hand_sides_stay_in_their_columns(pkg, ctx, refs, kind, fixture, dtype):
    n = 2 * panel_width(pkg, kind, dtype) + 1
    case = Case(pkg, refs, kind, _MATRIX[fixture](n, dtype))
    NB = case.F.block_plan(1)["NB"]
    w = 2 * NB + 5                                                             # three groups at least, clean columns in every one
    check_plan(case, w)
    B = sb.rhs(n, w, dtype)
    clean = sb.per_column(case.solve, B)
    bad = {1: (n - 1, np.nan), NB + 1: (0, np.inf), w - 1: (n // 2, -np.inf)}                              # single columns, in different groups
    assert len(bad) == 3 and len({j // NB for j in bad}) == 3
    for j, (i, v) in bad.items():
        B[i, j] = v
    want = sb.per_column(case.solve, B)
    for j in range(w):
        assert np.isfinite(want[:, j]).all() == (j not in bad), j
        assert j in bad or ch.same_bits(want[:, j], clean[:, j])
    for in_place in (False, True):
        X = device_block(pkg, B, lds(n)[0])
        Y = X if in_place else device_block(pkg, np.zeros((n, w), dtype, order="F"), lds(n)[1])
        case.F.ldiv_(Y, X)
        got = read(Y)[:n, :]
        assert ch.same_bits(got, want), ch.first_difference(got, want)       # NaN positions in the poisoned columns, the bits in all others


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
@pytest.mark.parametrize("fixture", ("ties", "last_row"))
def test_lu_with_interchanges_far_from_the_identity(pkg, ctx, refs, fixture, dtype):
    W = panel_width(pkg, "lu", dtype)
    n = 2 * W + 1
    A = lu.ties(n, dtype, (3, W + 1, n - 1)) if fixture == "ties" else lu.last_row(n, dtype)
    case = Case(pkg, refs, "lu", A)
    assert np.count_nonzero(case.perm != np.arange(n)) > n // 2
    assert np.array_equal(lu.permutation_of(case.F.ipiv), case.perm)
    G = case.F.block_plan(1)["G"]
    B = sb.rhs(n, G + 1, dtype)
    want = sb.per_column(case.solve, B)
    assert np.isfinite(want).all()
    for w in (case.F.block_plan(1)["NB"] + 1, G + 1):
        check_plan(case, w)
        X = device_block(pkg, B, lds(n)[0])
        Y = device_block(pkg, np.zeros((n, G + 1), dtype, order="F"), lds(n)[1])
        case.F.ldiv_(Y, X, cols=w)
        assert ch.same_bits(read(Y)[:n, :w], want[:, :w]) and ch.same_bits(read(X)[:n, :], B)                # out of place
        case.F.ldiv_(X, cols=w)                                                # in place: the pass is gathered before anything is stored
        got = read(X)[:n, :]
        assert ch.same_bits(got[:, :w], want[:, :w]) and ch.same_bits(got[:, w:], B[:, w:])


# ---- refusals: a named message, no launch, nothing touched -------------------------------------------------------------------------------
def _vp(M, elements=0):
    return C.c_void_p(M.buf.ptr + elements * M.dtype.itemsize)


@pytest.mark.parametrize("kind", ("lu", "chol"))
def test_refusals_leave_everything_as_it_was(pkg, ctx, refs, kind):
    L = pkg.lib()
    dtype, n = np.float64, 70
    case = Case(pkg, refs, kind, ch.hpd(n, dtype))
    F = case.F
    entry = getattr(L, f"mik_dense_{kind}_solve_block")
    B = sb.rhs(n, 6, dtype)
    X, Y = device_block(pkg, B, 192), device_block(pkg, B, 128)
    factors = F.factors.buf.to_numpy()
    x0, y0 = read(X), read(Y)

    def refused(code, text, *args):
        assert entry(F.handle, *args) == code
        assert text in L.mik_last_error(ctx.handle).decode(), L.mik_last_error(ctx.handle).decode()

    refused(3, "nrhs", _vp(Y), Y.ld, _vp(X), X.ld, 0)
    refused(3, "nrhs", _vp(Y), Y.ld, _vp(X), X.ld, -2)
    refused(3, "ldy", _vp(Y), n - 1, _vp(X), X.ld, 2)
    refused(3, "ldx", _vp(Y), Y.ld, _vp(X), n - 1, 2)
    refused(1, "overlap", _vp(X), X.ld, _vp(X), X.ld + 1, 2)                   # the same pointer on another leading dimension
    refused(1, "overlap", _vp(X, 5), X.ld, _vp(X), X.ld, 2)                    # shifted by five elements
    refused(1, "overlap", _vp(X, X.ld), X.ld, _vp(X), X.ld, 3)                 # shifted by a column
    refused(1, "factors", _vp(F.factors), F.factors.ld, _vp(X), X.ld, 2)
    refused(1, "factors", _vp(Y), Y.ld, _vp(F.factors, 3), F.factors.ld, 2)
    assert entry(F.handle, None, Y.ld, _vp(X), X.ld, 2) == 1 and entry(None, _vp(Y), Y.ld, _vp(X), X.ld, 2) == 1
    wide = pkg.HipMatrix(n, 4, np.float32)
    for call in (lambda: F.ldiv_(Y, pkg.HipVector(n, dtype)), lambda: F.ldiv_(pkg.HipVector(n, dtype), X),       # a vector and a matrix
                 lambda: F.ldiv_(pkg.HipMatrix(n + 1, 6, dtype), X), lambda: F.ldiv_(Y, pkg.HipMatrix(n - 1, 6, dtype)), lambda: F.solve(pkg.HipMatrix(n + 1, 2, dtype)),
                 lambda: F.ldiv_(wide, X), lambda: F.ldiv_(Y, wide), lambda: F.solve(wide),
                 lambda: F.ldiv_(pkg.HipMatrix(n, 5, dtype), X), lambda: F.ldiv_(Y, X, cols=7), lambda: F.ldiv_(Y, X, cols=0)):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            call()
    sub = pkg.HipMatrix(n, 2, dtype)                                           # two columns inside X's buffer, one column along: an overlap that is not equality
    sub.ld, sub.buf = X.ld, X.buf.view(X.ld, X.ld + n)
    with pytest.raises(pkg.MikError) as ei:
        F.ldiv_(sub, X, cols=2)
    assert ei.value.code == 1 and "overlap" in str(ei.value)
    assert ch.same_bits(read(X), x0) and ch.same_bits(read(Y), y0) and ch.same_bits(F.factors.buf.to_numpy(), factors)
    F.ldiv_(Y, X)                                                              # and the handle still solves
    assert ch.same_bits(read(Y)[:n, :], sb.per_column(case.solve, B))


def test_a_failed_cholesky_refuses_a_block(pkg, ctx, refs):
    L = pkg.lib()
    n, dtype = 70, np.complex128
    A, _, info = ch.failing_case(refs["chol"], n, dtype, 5, "negative")
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A), check=False)
    assert F.info == info != 0
    B = sb.rhs(n, 3, dtype)
    X = device_block(pkg, B, 128)
    before = read(X)
    with pytest.raises(pkg.MikError) as ei:
        F.ldiv_(X)
    assert ei.value.code == 1 and f"PosDefException({info})" in str(ei.value)
    assert L.mik_dense_chol_solve_block(F.handle, _vp(X), X.ld, _vp(X), X.ld, 3) == 1                          # the C entry refuses it too
    assert "PosDefException" in L.mik_last_error(ctx.handle).decode()
    assert ch.same_bits(read(X), before)


# ---- lobpcg: one block call on the active columns has the bits of one vector solve and one copy per column --------------------------------
class VectorOnly:
    """the same factorisation behind an object that offers ldiv_(y, x) on vectors only: lobpcg's per-column path"""

    def __init__(self, F):
        self.F, self.calls = F, 0

    def ldiv_(self, y, x):
        self.calls += 1
        return self.F.ldiv_(y, x)


@pytest.mark.parametrize("dtype", (np.float64, np.complex128))
def test_lobpcg_with_cholesky_as_p_routed_and_per_column(pkg, ctx, dtype, monkeypatch):
    n = 2 * panel_width(pkg, "chol", dtype) + 1
    A = ch.hpd(n, dtype)
    op = pkg.HipCSR.from_scipy(sp.csr_matrix(A), ctx)
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
    blocks = []
    inner = pkg.DenseCholesky.ldiv_

    def counted(self, y, x=None, cols=None):
        if isinstance(y, pkg.HipMatrix):
            blocks.append(cols)
        return inner(self, y, x, cols)
    monkeypatch.setattr(pkg.DenseCholesky, "ldiv_", counted)
    for width in (3, F.block_plan(1)["NB"] + 1):
        X0 = sb.rhs(n, width, dtype, seed=5)
        del blocks[:]
        routed = pkg.lobpcg(op, False, X0, P=F, tol=1e-300, maxiter=6, log=True)
        assert blocks and max(blocks) == width and all(F.block_min_cols <= b <= width for b in blocks)         # one block call per application
        slow = VectorOnly(F)
        n_blocks = len(blocks)
        per_column = pkg.lobpcg(op, False, X0, P=slow, tol=1e-300, maxiter=6, log=True)
        assert slow.calls >= width and len(blocks) == n_blocks                 # the wrapper took the per-column path
        assert routed.iterations == per_column.iterations and len(routed.trace) == len(per_column.trace) > 1
        assert np.array_equal(routed.lam, per_column.lam) and np.array_equal(routed.residual_norms, per_column.residual_norms)
        for a, b in zip(routed.trace, per_column.trace):
            assert np.array_equal(a.residual_norms, b.residual_norms) and np.array_equal(a.ritz_values, b.ritz_values)
        assert np.array_equal(routed.X.to_numpy(), per_column.X.to_numpy())
