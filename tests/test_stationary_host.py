"""The CPU checker of the stationary methods: tests/stationary_ref/stationary_ref.c (the reference's CSC column loops restated in
C) against numbers Julia printed (docs/src/iterators.md), against the assertions of test/stationary.jl, and against an independent
sequential ROW-view restatement in numpy, bit for bit -- also on the operators of tests/stationary_fixtures.py, whose prescribed level
widths and launch plans are asserted here first.  No GPU."""
import math

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import stationary_fixtures as fx
import stationary_host as sh


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("stationary_ref"))


def _spmv_csc(M, x):
    """SparseArrays' mul!(y, A, x): y .= 0, then the column scatter y[rowval[k]] += nzval[k] * x[col]"""
    y = [M.dtype.type(0)] * M.n
    for col in range(M.n):
        for k in range(M.cp[col], M.cp[col + 1]):
            y[M.rv[k]] = y[M.rv[k]] + M.nz[k] * M.dtype.type(x[col])
    return np.array(y, M.dtype)


def _norm(v):
    """BLAS nrm2 of a 4-vector of moderate values: sqrt of the sequential sum of squares"""
    s = 0.0
    for a in v:
        s += float(a) * float(a)
    return math.sqrt(s)


def test_reproduces_the_jacobi_iterable_doctest_of_docs_iterators_md(ref):
    """docs/src/iterators.md:34-70: the four residual norms Julia printed for jacobi_iterable, maxiter = 2, two right-hand sides"""
    A = sp.diags([-np.ones(3), 2 * np.ones(4), -np.ones(3)], [-1, 0, 1], format="csc")
    M = sh.Mat(A)
    b1, b2 = np.array([1.0, 2, 3, 4]), np.array([-1.0, 1, -1, 1])
    x = np.array([0.0, -1, 1, 0])
    rel = lambda b, x: _norm(b - _spmv_csc(M, x)) / _norm(b)
    assert rel(b1, x) == 1.2909944487358056
    x, s = ref.jacobi(M, b1, x, maxiter=2)
    assert s == 0 and rel(b1, x) == 0.8228507357554791
    assert rel(b2, x) == 2.6368778887161235
    x, s = ref.jacobi(M, b2, x, maxiter=2)
    assert s == 0 and rel(b2, x) == 1.610815496107484


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_solvers_converge_on_diagonally_dominant_matrices(ref, dtype):
    """test/stationary.jl:20-48: every method, maxiter = 2n, on sprand(T, n, n, 4/n) + 2n I reaches norm(b - A x)/norm(b) <= sqrt(eps(T))"""
    n = 10
    rng = np.random.default_rng(1234322)
    A = sh.sprand_dominant(n, 4 / n, 7, dtype)
    M = sh.Mat(A, dtype)
    b = rng.random(n).astype(dtype)
    x0 = rng.random(n).astype(dtype)
    tol = math.sqrt(np.finfo(dtype).eps)
    Ad = A.astype(np.float64)
    res = lambda x: np.linalg.norm(b - Ad @ x.astype(np.float64)) / np.linalg.norm(b)
    for x in (np.zeros(n, dtype), x0):
        assert res(ref.jacobi(M, b, x, maxiter=2 * n)[0]) <= tol
        assert res(ref.gauss_seidel(M, b, x, maxiter=2 * n)[0]) <= tol
        assert res(ref.sor(M, b, x, 1.2, maxiter=2 * n)[1]) <= tol
        assert res(ref.ssor(M, b, x, 1.2, maxiter=2 * n)[0]) <= tol


def test_gauss_seidel_and_sor_with_omega_one_coincide(ref):
    """test/stationary.jl:51-63 (here even bit for bit: omega = 1 makes x/d + 0*y)"""
    A = sh.sprand_dominant(10, 0.4, 11) - 16 * sp.identity(10)       # sprand(10, 10, 4/10) + 4I
    M = sh.Mat(A.tocsc())
    b = A @ np.ones(10)
    for k in range(1, 6):
        xg, _ = ref.gauss_seidel(M, b, np.zeros(10), maxiter=k)
        _, xs, _ = ref.sor(M, b, np.zeros(10), 1.0, maxiter=k)
        assert np.allclose(xg, xs) and np.array_equal(xg, xs)


def test_singular_diagonals_throw_with_the_first_column(ref):
    """test/stationary.jl:65-80 and DiagonalIndices :14-19: missing, zero and -0.0 diagonals"""
    for A, col in ((sp.csc_matrix(np.array([[0.0, 1.0], [1.0, 0.0]])), 1),
                   (sp.csc_matrix(np.array([[0.0, 0, 0], [0, 1, 0], [0, 0, 1]])), 1),
                   (sp.csc_matrix(np.array([[1.0, 0, 0], [0, 1, 2], [0, 3, 0]])), 3)):
        M = sh.Mat(A)
        assert ref.diag(M) == col
        assert ref.jacobi(M, np.ones(A.shape[0]), np.zeros(A.shape[0]))[1] == col
        assert ref.sor(M, np.ones(A.shape[0]), np.zeros(A.shape[0]), 0.5)[2] == col
    for z in (0.0, -0.0):                   # explicitly stored zeros: iszero(-0.0) is true
        A = sp.csc_matrix((np.array([2.0, z, 3.0]), (np.array([0, 1, 2]), np.array([0, 1, 2]))), shape=(3, 3))
        A.data[1] = z
        M = sh.Mat(A)
        assert M.nz.size == 3 and ref.diag(M) == 2


def test_building_blocks_against_dense_linear_algebra(ref):
    """test/stationary.jl:82-201: ldiv!, forward / backward substitution (plain and with update), OffDiagonal mul! for
    (alpha, beta) = (1, 0), (1, 1), (2, 3), and both gauss_seidel_multiply! forms"""
    rng = np.random.default_rng(3)
    A = sh.sprand_dominant(10, 0.3, 21) - 10 * sp.identity(10)        # sprand(10, 10, .3) + 10I
    M = sh.Mat(A.tocsc())
    Ad = A.toarray()
    assert ref.diag(M) == 0 and np.array_equal(M.nz[M.diag], np.diag(Ad))
    assert np.allclose(ref.ldiv(M, np.ones(10)), 1 / np.diag(Ad))
    x = rng.random(10)
    assert np.allclose(ref.sub(M, False, x), sla.solve_triangular(np.tril(Ad), x, lower=True))
    assert np.allclose(ref.sub(M, True, x), sla.solve_triangular(np.triu(Ad), x, lower=False))
    B = rng.random((3, 3)) + 10 * np.eye(3)
    MB = sh.Mat(sp.csc_matrix(B))
    ref.diag(MB)
    x3, y3 = rng.random(3), np.ones(3)
    # the reference writes the relaxed step with alpha = 2, beta = 3 directly (:128-148); here beta = one(T) - omega is what the
    # iterables pass, so check the formula with omega = 2 (beta = -1) against the hand expansion
    z = x3.copy()
    z[0] = 2 * z[0] / B[0, 0] + -1 * y3[0]
    z[1] = 2 * (z[1] - B[1, 0] * z[0]) / B[1, 1] + -1 * y3[1]
    z[2] = 2 * (z[2] - B[2, 0] * z[0] - B[2, 1] * z[1]) / B[2, 2] + -1 * y3[2]
    assert np.allclose(ref.sub(MB, False, x3, 2.0, y3), z)
    z = x3.copy()
    z[2] = 2 * z[2] / B[2, 2] + -1 * y3[2]
    z[1] = 2 * (z[1] - B[1, 2] * z[2]) / B[1, 1] + -1 * y3[1]
    z[0] = 2 * (z[0] - B[0, 1] * z[1] - B[0, 2] * z[2]) / B[0, 0] + -1 * y3[0]
    assert np.allclose(ref.sub(MB, True, x3, 2.0, y3), z)
    O = Ad - np.diag(np.diag(Ad))
    for a, b in ((1.0, 0.0), (1.0, 1.0), (2.0, 3.0)):
        x = rng.random(10)
        assert np.allclose(ref.offdiag_mul(M, a, x, b, np.ones(10)), a * (O @ x) + b * np.ones(10))
    x, b = rng.random(10), rng.random(10)
    assert np.allclose(ref.gs_mul(M, True, -1.0, x, 1.0, b), b - np.triu(Ad, 1) @ x)
    assert np.allclose(ref.gs_mul(M, False, -1.0, x, 1.0, b), b - np.tril(Ad, -1) @ x)


# ---- an independent restatement in the ROW view (the device's formulation), sequential numpy scalars ---------------------------
class RowView:
    def __init__(self, A, dtype):
        c = sp.csr_matrix(A.astype(dtype))
        c.sort_indices()
        self.T = np.dtype(dtype).type
        self.n = c.shape[0]
        self.rows = [(c.indices[c.indptr[i]:c.indptr[i + 1]].tolist(), [self.T(v) for v in c.data[c.indptr[i]:c.indptr[i + 1]]]) for i in range(self.n)]
        self.d = [v[cols.index(i)] for i, (cols, v) in enumerate(self.rows)]

    def offdiag(self, a, x, b, y):             # y[i] = 0 | y | b*y, then += A[i,j]*(a*x[j]) over j != i ascending
        T, out = self.T, []
        for i, (cols, vals) in enumerate(self.rows):
            acc = T(0) if b == 0 else (y[i] if b == 1 else T(b) * y[i])
            for j, v in zip(cols, vals):
                if j != i:
                    acc = acc + v * (T(a) * x[j])
            out.append(acc)
        return out

    def gs(self, upper, a, x, b, y):           # upper: j > i ascending; lower: j < i descending; old x throughout
        T, out = self.T, []
        for i, (cols, vals) in enumerate(self.rows):
            acc = T(b) * y[i]
            terms = [(j, v) for j, v in zip(cols, vals) if (j > i if upper else j < i)]
            for j, v in (terms if upper else terms[::-1]):
                acc = acc + v * (T(a) * x[j])
            out.append(acc)
        return out

    def sub(self, upper, x, S=None, a=None, b=None, y=None):
        x = list(x)
        order = range(self.n - 1, -1, -1) if upper else range(self.n)
        for i in order:
            cols, vals = self.rows[i]
            terms = [(j, v) for j, v in zip(cols, vals) if (j > i if upper else j < i)]
            acc = x[i]
            for j, v in (terms[::-1] if upper else terms):
                acc = acc - v * x[j]
            x[i] = acc / self.d[i] if S is None else self.T(S(a) * S(acc) / S(self.d[i]) + S(b) * S(y[i]))
        return x


def _np_method(R, method, b, x, omega, k, S):
    T = R.T
    b, x = [T(v) for v in b], [T(v) for v in x]
    a, be = (S(omega), S(S(1) - S(omega))) if S is not None else (None, None)
    nxt = [T(0)] * R.n
    for _ in range(k):
        if method == "jacobi":
            nxt = R.offdiag(-1, x, 1, list(b))
            x = [nxt[i] / R.d[i] for i in range(R.n)]
        elif method == "gs":
            x = R.sub(False, R.gs(True, -1, x, 1, b))
        elif method == "sor":
            nxt = R.sub(False, R.gs(True, -1, x, 1, b), S, a, be, x)
            x, nxt = nxt, x
        else:
            tmp = R.sub(False, R.gs(True, -1, x, 1, b), S, a, be, x)
            x = R.sub(True, R.gs(False, -1, tmp, 1, b), S, a, be, tmp)
    return np.array(x, T)


@pytest.mark.parametrize("dtype,omega", [(np.float64, 1.2), (np.float32, 1.2), (np.float32, np.float32(1.2)), (np.float64, np.float32(0.7))])
def test_row_view_restatement_agrees_bit_for_bit(ref, dtype, omega):
    """the device sums rows in the order the column loops deliver them (include/mik.h): a sequential row-view restatement of that
    claim must give the C column-loop restatement's bits, for all four methods, both dtypes, omega as Float64 and Float32"""
    rng = np.random.default_rng(17)
    for A in (sh.sprand_dominant(40, 0.12, 5, dtype), sh.arrow(30, 12, dtype), sh.tridiag(25, dtype)):
        M = sh.Mat(A, dtype)
        R = RowView(A, dtype)
        b = rng.standard_normal(M.n).astype(dtype)
        x0 = rng.standard_normal(M.n).astype(dtype)
        S = np.float32 if sh.omega32(omega, dtype) else np.float64        # the type alpha*x/d + beta*y is evaluated in
        for k in (1, 3):
            assert np.array_equal(ref.jacobi(M, b, x0, k)[0], _np_method(R, "jacobi", b, x0, omega, k, None))
            assert np.array_equal(ref.gauss_seidel(M, b, x0, k)[0], _np_method(R, "gs", b, x0, omega, k, None))
            assert np.array_equal(ref.sor(M, b, x0, omega, k)[1], _np_method(R, "sor", b, x0, omega, k, S))
            assert np.array_equal(ref.ssor(M, b, x0, omega, k)[0], _np_method(R, "ssor", b, x0, omega, k, S))


# ---- the operators of tests/stationary_fixtures.py: their level structure, then the checker on them -----------------------------------
DTYPES = (np.float64, np.float32)
OMEGAS = [(np.float64, 1.2), (np.float64, np.float32(0.7)), (np.float64, 1), (np.float32, 1.2), (np.float32, np.float32(1.2)), (np.float32, 1)]


def test_level_widths_and_launch_plan_on_cases_worked_by_hand():
    """the two plain-numpy functions every info() expectation rests on"""
    assert fx.level_widths(sh.Mat(sh.tridiag(5))) == ([1] * 5, [1] * 5)
    assert fx.level_widths(sh.Mat(sp.identity(7, format="csc"))) == ([7], [7])
    # rows 0, 1 read nothing below; 2 reads 0; 3 reads 1 and 2; 4 reads 0.  Above: 0 reads 4; 1 reads 2; 2 reads 3; 3, 4 nothing
    A = sp.csc_matrix((np.ones(12), ([0, 1, 2, 3, 4, 2, 3, 3, 4, 0, 1, 2], [0, 1, 2, 3, 4, 0, 1, 2, 0, 4, 2, 3])), shape=(5, 5))
    assert fx.level_widths(sh.Mat(A)) == ([2, 2, 1], [2, 2, 1])          # forward {0, 1}, {2, 4}, {3}; backward {3, 4}, {0, 2}, {1}
    assert fx.level_widths(sh.Mat(sp.csc_matrix((0, 0)))) == ([], [])
    assert fx.launch_plan([]) == []
    assert fx.launch_plan([256]) == [("run", 0, 1, 0, 256)] and fx.launch_plan([257]) == [("wide", 0, 1, 0, 257)]
    assert fx.launch_plan([255, 256, 257, 3, 512, 1, 513, 252]) == [("run", 0, 2, 0, 511), ("wide", 2, 3, 511, 768), ("run", 3, 4, 768, 771),
                                                                     ("wide", 4, 5, 771, 1283), ("run", 5, 6, 1283, 1284),
                                                                     ("wide", 6, 7, 1284, 1797), ("run", 7, 8, 1797, 2049)]
    assert fx.launch_plan([300, 257, 1, 2, 3, 400]) == [("wide", 0, 1, 0, 300), ("wide", 1, 2, 300, 557), ("run", 2, 5, 557, 563), ("wide", 5, 6, 563, 963)]
    assert fx.launch_plan([3, 4, 5], narrow=3) == [("run", 0, 1, 0, 3), ("wide", 1, 2, 3, 7), ("wide", 2, 3, 7, 12)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(fx.FIXTURES))
def test_level_fixtures_have_their_prescribed_widths_and_plans(name, dtype):
    """every builder runs its own assertions; here the widths and the number of wide launches are pinned once more, so that a later edit
    cannot quietly turn a fixture narrow again"""
    M = fx.fixture(name, dtype)
    assert M.dtype == dtype and M.widths == fx.level_widths(M) and sum(M.widths[0]) == sum(M.widths[1]) == M.n < 20000
    want = {"edges": fx.EDGES, "stairs": fx.STAIRS, "hubs": fx.HUBS}.get(name)
    if want is not None:
        assert M.widths == want
    wide = {"edges": (3, 3), "stairs": (4, 3), "hubs": (3, 2), "lap24": (26, 26), "sprand4000": (6, 6)}[name]
    launches = {"edges": (7, 5), "stairs": (6, 5), "hubs": (3, 3), "lap24": (28, 28), "sprand4000": (7, 7)}[name]
    for d in (0, 1):
        plan = M.plans[d]
        assert len(plan) == launches[d] and len(fx.wide_launches(plan)) == wide[d] >= 2
        assert [p[0] for p in plan] == ["wide" if M.widths[d][p[1]] > 256 else "run" for p in plan]
        assert all(p[2] == p[1] + 1 and p[4] - p[3] == M.widths[d][p[1]] > 256 for p in fx.wide_launches(plan))
        assert plan[0][3] == 0 and plan[-1][4] == M.n and all(a[4] == b[3] and a[2] == b[1] for a, b in zip(plan, plan[1:]))
    if name == "lap24":
        assert max(M.widths[0]) == 432 and len(M.widths[0]) == 70
    if name == "sprand4000":
        assert max(M.widths[0]) > 900 and len(M.widths[0]) <= 20
    if name == "hubs":                                                   # the long rows sit inside a wide level, in either direction
        lens = np.bincount(M.rv, minlength=M.n)
        assert all(lens[r] > fx.LONG_ROW for r in M.longs[0] + M.longs[1])
        assert fx.launch_plan(M.widths[0])[2][0] == "wide" and fx.launch_plan(M.widths[1])[2][0] == "wide"


def test_width_lists_cover_every_case_between_them():
    lists = [w for pair in (fx.EDGES, fx.STAIRS, fx.HUBS) for w in pair]
    plans = [fx.launch_plan(w) for w in lists]
    adjacent = lambda w, a, b: any({x, y} == {a, b} for x, y in zip(w, w[1:]))
    assert any(adjacent(w, 255, 256) and adjacent(w, 256, 257) for w in lists)                      # 255 | 256 | 257 next to one another
    assert any(adjacent(w, 255, 256) for w in lists) and any(adjacent(w, 255, 257) for w in lists)
    assert any(512 in w for w in lists) and any(513 in w for w in lists)                           # 256 q and 256 q + 1
    assert any(p[0] == "wide" and p[3] % 256 for plan in plans for p in plan)                      # a wide launch whose p0 is no multiple of 256
    assert sum(1 for plan in plans for p in plan if p[0] == "wide" and p[3] % 256) >= 8
    triples = [(a, b, c) for plan in plans for a, b, c in zip(plan, plan[1:], plan[2:])]
    assert any(a[0] == c[0] == "wide" and b[0] == "run" and b[2] - b[1] >= 3 for a, b, c in triples)    # wide -> a run of >= 3 levels -> wide
    assert any(a[0] == c[0] == "wide" and b[0] == "run" and b[4] - b[3] == 1 for a, b, c in triples)    # a one-row level between two wide ones
    assert any(plan[0][0] == "wide" for plan in plans) and any(plan[-1][0] == "wide" for plan in plans)
    assert any(plan[0][0] == "run" for plan in plans) and any(plan[-1][0] == "run" for plan in plans)
    assert any(plan[0][0] == "run" and plan[0][2] - plan[0][1] >= 2 for plan in plans)
    for lo, up in (fx.EDGES, fx.STAIRS, fx.HUBS):                                                   # forward and backward plans differ
        assert fx.kinds(fx.launch_plan(lo)) != fx.kinds(fx.launch_plan(up)) and sum(lo) == sum(up)
    assert sorted(sum(lo) - 2048 for lo, _ in (fx.EDGES, fx.STAIRS, fx.HUBS)) == [-1, 0, 1]         # n on both sides of a multiple of 256


@pytest.mark.parametrize("dtype,omega", OMEGAS)
@pytest.mark.parametrize("name", list(fx.FIXTURES))
def test_row_view_restatement_agrees_on_the_level_fixtures(ref, name, dtype, omega):
    """the checker checked at the shapes the device is held to in tests/test_gpu_stationary_paths.py: the C column loops against the
    numpy row-view restatement, bit for bit, four methods and the four substitutions alone, omega as Float64, Float32 and Int"""
    M = fx.fixture(name, dtype)
    R = RowView(sp.csc_matrix((M.nz, M.rv, M.cp), shape=(M.n, M.n)), dtype)
    rng = np.random.default_rng(23)
    b = rng.standard_normal(M.n).astype(dtype)
    x0 = rng.standard_normal(M.n).astype(dtype)
    S = np.float32 if sh.omega32(omega, dtype) else np.float64
    k = 2
    assert np.array_equal(ref.jacobi(M, b, x0, k)[0], _np_method(R, "jacobi", b, x0, omega, k, None))
    assert np.array_equal(ref.gauss_seidel(M, b, x0, k)[0], _np_method(R, "gs", b, x0, omega, k, None))
    assert np.array_equal(ref.sor(M, b, x0, omega, k)[1], _np_method(R, "sor", b, x0, omega, k, S))
    x = ref.ssor(M, b, x0, omega, k)[0]
    assert np.array_equal(x, _np_method(R, "ssor", b, x0, omega, k, S)) and np.all(np.isfinite(x))
    ref.diag(M)
    a, be = S(omega), S(S(1) - S(omega))
    for upper in (False, True):
        assert np.array_equal(ref.sub(M, upper, b), np.array(R.sub(upper, b), dtype))
        assert np.array_equal(ref.sub(M, upper, b, omega, x0), np.array(R.sub(upper, b, S, a, be, x0), dtype))


def test_float32_with_float64_omega_rounds_once(ref):
    """sor!(x::Vector{Float32}, A, b, 1.2): alpha*x/d + beta*y in Float64 -- a different result from the all-Float32 evaluation"""
    A = sh.sprand_dominant(60, 0.1, 9, np.float32)
    M = sh.Mat(A, np.float32)
    rng = np.random.default_rng(2)
    b = rng.standard_normal(60).astype(np.float32)
    x64 = ref.ssor(M, b, np.zeros(60, np.float32), 1.2, 4)[0]
    x32 = ref.ssor(M, b, np.zeros(60, np.float32), np.float32(1.2), 4)[0]
    assert x64.dtype == np.float32 and not np.array_equal(x64, x32)


def test_sor_swap_quirk(ref):
    """sor! returns iterable.x: after an odd number of iterations the internal buffer, and the caller's x holds iterate k - 1"""
    A = sh.sprand_dominant(20, 0.2, 4)
    M = sh.Mat(A)
    b = np.arange(20.0)
    x2, r2, w2 = ref.sor(M, b, np.zeros(20), 1.3, 2)
    x3, r3, w3 = ref.sor(M, b, np.zeros(20), 1.3, 3)
    assert w2 == 0 and r2 is x2 and w3 == 1
    assert np.array_equal(x3, x2) and not np.array_equal(r3, x3)
