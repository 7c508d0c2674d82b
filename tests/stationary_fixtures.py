"""Operators built to a prescribed LEVEL STRUCTURE, for the triangular sweeps of the stationary methods (csrc/mik_stationary.h): a level
with more than NARROW = 256 rows is one multi-workgroup launch of k_st_tri_level starting at its level-order position p0, a run of
consecutive narrower levels one launch of the one-workgroup k_st_tri_run.  The matrices of tests/test_gpu_stationary.py have no level wider
than 192 rows (the 256^3 Laplacian apart), so each of their sweeps is a single k_st_tri_run launch; the ones here are built so that the
wide kernel, the switch between the two and plans of several launches do the work.

`level_widths` and `launch_plan` restate the level definition of include/mik.h and the launch rule in plain numpy (on the CSC columns, a
scatter -- the library gathers over rows): they are the expectation for StationaryOperator.info() and share no code with the library.
Every builder asserts the widths and plans it was built for; tests/test_stationary_host.py calls every builder, so those assertions run
without a GPU too.  `dev` and `check_methods` are the helpers the two GPU modules share."""
import functools

import numpy as np
import scipy.sparse as sp

import stationary_host as sh
from conftest import graft

NARROW = 256            # MIK_ST_NARROW
BLOCK = 256             # MIK_ST_BLOCK
LONG_ROW = 256          # mik_spmv_long_row(): longer rows are split off at upload (the GPU module asserts the value)


# ---- the expectation: levels from the definition, launches from the rule -------------------------------------------------------------------
def level_widths(M):
    """(forward widths, backward widths) of a sh.Mat: level of row i = 1 + the largest level of the rows it reads in the strict triangle
    (0 for a row that reads none); forward = strict lower, rows ascending; backward = strict upper, rows descending"""
    out = []
    for cols in (range(M.n), range(M.n - 1, -1, -1)):
        forward = cols.step == 1
        level = np.zeros(M.n, np.int64)
        for j in cols:                                                  # level[j] is final: every column it depends on came before
            rows = M.rv[M.cp[j]:M.cp[j + 1]]
            readers = rows[rows > j] if forward else rows[rows < j]     # the rows that read x[j]
            level[readers] = np.maximum(level[readers], level[j] + 1)
        out.append([int(w) for w in np.bincount(level)] if M.n else [])
    return out[0], out[1]


def launch_plan(widths, narrow=NARROW):
    """[(kind, first level, one past the last level, p0, p1)]: kind "wide" is one level of more than `narrow` rows, kind "run" a maximal run
    of consecutive levels of at most `narrow` rows each; [p0, p1) are the level-order positions the launch covers"""
    start = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    plan, l = [], 0
    while l < len(widths):
        l1 = l + 1
        if widths[l] <= narrow:
            while l1 < len(widths) and widths[l1] <= narrow:
                l1 += 1
        plan.append(("wide" if widths[l] > narrow else "run", l, l1, int(start[l]), int(start[l1])))
        l = l1
    return plan


def wide_launches(plan):
    return [p for p in plan if p[0] == "wide"]


# ---- staged: a matrix with exactly these level widths ----------------------------------------------------------------------------------------
def _triangle(rng, widths, n, long_rows, long_len):
    """strict LOWER pattern (i, j), j < i, whose forward levels have exactly `widths` rows.  Rows 0 .. L-1 are a spine, row l reading row
    l - 1 (level l); the other rows get their levels in random index order, and a row of level l >= 1 reads spine row l - 1 plus those of
    three random earlier rows that have a lower level.  About a quarter of the non-spine rows of level >= 1 read the spine row alone;
    level-0 rows read nothing.  `long_rows` rows of the widest level read `long_len` more rows of lower level."""
    L = len(widths)
    assert sum(widths) == n and min(widths) >= 1
    rest = np.repeat(np.arange(L), np.asarray(widths) - 1)
    level = np.concatenate([np.arange(L), rng.permutation(rest)]).astype(np.int64)
    i = np.arange(L, n)
    i = i[level[i] >= 1]
    ii, jj = [np.arange(1, L), i], [np.arange(0, L - 1), level[i] - 1]
    extra = i[rng.random(i.size) < 0.75]
    for _ in range(3):
        j = (rng.random(extra.size) * extra).astype(np.int64)          # uniform in [0, i)
        keep = level[j] < level[extra]
        ii.append(extra[keep])
        jj.append(j[keep])
    longs = []
    if long_rows:
        lw = int(np.argmax(widths))
        cand = np.flatnonzero(level == lw)
        cand = cand[cand >= L]
        for r in cand[::-1]:                                             # late rows: enough lower-level rows in front of them
            below = np.flatnonzero(level[:r] < lw)
            if below.size >= long_len and len(longs) < long_rows:
                longs.append(int(r))
                ii.append(np.full(long_len, r))
                jj.append(rng.choice(below, size=long_len, replace=False))
        assert len(longs) == long_rows, "no room for the long rows"
    pairs = np.unique(np.stack([np.concatenate(ii), np.concatenate(jj)], axis=1), axis=0)
    assert np.all(pairs[:, 1] < pairs[:, 0])
    return pairs[:, 0], pairs[:, 1], longs


def _offdiag_values(rng, count):
    """mixed signs, magnitudes 2^-24 .. 2^3: a fused multiply-add or another association changes bits"""
    return rng.choice([-1.0, 1.0], size=count) * np.exp2(rng.uniform(-24, 2, size=count)) * (1 + rng.random(count))


def staged(lower_widths, upper_widths, dtype, seed, long_rows=0, long_len=0):
    """a nonsymmetric, strictly row-diagonally-dominant sh.Mat whose forward levels have exactly `lower_widths` rows and whose backward levels
    exactly `upper_widths` rows.  The strict upper triangle is the construction of _triangle on mirrored indices (i -> n - 1 - i) from its
    own widths and its own random stream, so the two level-order permutations interleave row indices differently.  The diagonal is
    +-(2 * the row's absolute off-diagonal sum + 1 + U(0, 1)), computed from the values as rounded to `dtype`: every sweep contracts, so a
    few iterations stay finite in Float32.  M.longs: the rows made long on purpose (lower, upper)."""
    n = int(sum(lower_widths))
    assert n == sum(upper_widths)
    rng = np.random.default_rng(seed)
    li, lj, llong = _triangle(rng, list(lower_widths), n, long_rows, long_len)
    ui, uj, ulong = _triangle(rng, list(upper_widths), n, long_rows, long_len)
    ui, uj, ulong = n - 1 - ui, n - 1 - uj, [n - 1 - r for r in ulong]
    i, j = np.concatenate([li, ui]), np.concatenate([lj, uj])
    v = _offdiag_values(rng, i.size).astype(dtype)
    off = np.bincount(i, weights=np.abs(v.astype(np.float64)), minlength=n)
    d = (rng.choice([-1.0, 1.0], size=n) * (2 * off + 1 + rng.random(n))).astype(dtype)
    A = sp.csc_matrix((np.concatenate([v, d]), (np.concatenate([i, np.arange(n)]), np.concatenate([j, np.arange(n)]))), shape=(n, n), dtype=dtype)
    A.sort_indices()
    assert A.nnz == i.size + n and np.all(A.data != 0) and np.all(np.isfinite(A.data))
    assert np.all(np.abs(d.astype(np.float64)) > 1.9 * off + 0.9) and (A != A.T).nnz > 0
    M = sh.Mat(A, dtype)
    M.longs = (llong, ulong)
    M.widths = level_widths(M)
    assert M.widths == (list(lower_widths), list(upper_widths)), "staged: the level widths are not the prescribed ones"
    # rows with an empty strict triangle on one side (tp[p] == tp[p + 1] in that direction), on both, and diagonals stored first / last
    R = A.tocsr()
    R.sort_indices()
    first, last = R.indices[R.indptr[:-1]], R.indices[R.indptr[1:] - 1]
    rows = np.arange(n)
    lower_empty, upper_empty = first == rows, last == rows
    assert lower_empty.sum() >= lower_widths[0] and upper_empty.sum() >= upper_widths[0]
    assert np.any(lower_empty & ~upper_empty) and np.any(upper_empty & ~lower_empty)
    assert np.any(~lower_empty & (np.diff(R.indptr) == 2))              # level >= 1 rows that read their spine row alone
    return M


# ---- the width lists -------------------------------------------------------------------------------------------------------------------------
# "edges", 2049 = 8 * 256 + 1 rows.
#   forward:  255 | 256 (a narrow run of two, every lane of the run kernel busy in the second) | 257 wide at p0 = 511 | 3 | 512 wide at p0 = 771 |
#             1 (a one-row level between two wide ones) | 513 wide at p0 = 1284 | 252: begins and ends with a narrow run
#   backward: 513 wide | 40, 7, 1 (a run of three) | 300 wide at p0 = 561 | 256, 255 (a run) | 677 wide at p0 = 1372: begins and ends wide
EDGES = ([255, 256, 257, 3, 512, 1, 513, 252], [513, 40, 7, 1, 300, 256, 255, 677])
# "stairs", 2047 = 8 * 256 - 1 rows.
#   forward:  300 wide first | 257 wide at p0 = 300 | 1 | 512 wide at p0 = 558 | 50, 60, 70 (wide -> a run of three -> wide) | 797 wide last
#   backward: 100 (a narrow run of one first) | 513 wide at p0 = 100 | 255 | 257 wide at p0 = 868 | 922 wide
STAIRS = ([300, 257, 1, 512, 50, 60, 70, 797], [100, 513, 255, 257, 922])
# "hubs", 2048 rows: three levels, all wide forward, wide | 20 | wide backward; three rows of the widest level of either direction read 300
# rows of lower levels (more than LONG_ROW entries: split off at upload and read back through the long-row table), so long rows sit INSIDE a
# wide level, not on a one-row-per-level band as in sh.arrow
HUBS = ([600, 700, 748], [1000, 20, 1028])


def edges(dtype):
    M = staged(*EDGES, dtype, seed=101)
    assert M.n == 8 * BLOCK + 1
    return M


def stairs(dtype):
    M = staged(*STAIRS, dtype, seed=102)
    assert M.n == 8 * BLOCK - 1
    return M


def hubs(dtype):
    M = staged(*HUBS, dtype, seed=103, long_rows=3, long_len=300)
    lens = np.bincount(M.rv, minlength=M.n)
    assert M.n == 8 * BLOCK and len(M.longs[0]) == len(M.longs[1]) == 3
    assert all(lens[r] > LONG_ROW for r in M.longs[0] + M.longs[1]) and np.count_nonzero(lens > LONG_ROW) == 6
    return M


def lap24(dtype):
    """laplace_matrix(24, 3), 13 824 rows: the levels are the planes i + j + k = const, the middle ones wider than 256"""
    M = sh.Mat.from_csc(*graft.load_package().fixtures.laplace_matrix(24, 3, dtype))
    M.widths = level_widths(M)
    assert M.n == 13824 and len(M.widths[0]) == len(M.widths[1]) == 70 and max(M.widths[0]) == 432
    return M


def sprand4000(dtype):
    """sprand(4000, 4000, 0.001) + 8000 I: about four entries a row, a dozen levels of up to a thousand rows"""
    M = sh.Mat(sh.sprand_dominant(4000, 0.001, 77, dtype), dtype)
    M.widths = level_widths(M)
    return M


# name -> (builder, forward plan kinds, backward plan kinds): "w" a wide launch, "r" a run.  For the staged operators the plans follow from
# the width lists above; for the natural ones they are what level_widths / launch_plan gave when the fixture was written, pinned here so
# that a later edit cannot quietly turn a fixture narrow again.
FIXTURES = {"edges": (edges, "rwrwrwr", "wrwrw"),
            "stairs": (stairs, "wwrwrw", "rwrww"),
            "hubs": (hubs, "www", "wrw"),
            "lap24": (lap24, "r" + 26 * "w" + "r", "r" + 26 * "w" + "r"),
            "sprand4000": (sprand4000, "wwwwwwr", "wwwwwwr")}
STAGED = ("edges", "stairs", "hubs")


def kinds(plan):
    return "".join(p[0][0] for p in plan)


@functools.lru_cache(maxsize=None)
def fixture(name, dtype):
    """the operator (built once per session and dtype; nobody writes to it), with M.widths and M.plans = (forward, backward)"""
    builder, fwd, bwd = FIXTURES[name]
    M = builder(np.dtype(dtype).type)
    M.plans = tuple(launch_plan(w) for w in M.widths)
    for plan, want in zip(M.plans, (fwd, bwd)):
        assert kinds(plan) == want, (name, kinds(plan), want)
        assert wide_launches(plan), name
    return M


# ---- shared by tests/test_gpu_stationary.py and tests/test_gpu_stationary_paths.py ---------------------------------------------------------------
def dev(pkg, M, i32=False):
    cp, rv = (M.cp.astype(np.int32), M.rv.astype(np.int32)) if i32 else (M.cp, M.rv)
    return pkg.HipCSR(M.n, M.n, cp, rv, M.nz, index_base=0)


def check_methods(pkg, ref, M, A, omega, k, rng):
    T = M.dtype
    b = rng.standard_normal(M.n).astype(T)
    x0 = rng.standard_normal(M.n).astype(T)
    bd = pkg.HipVector.from_numpy(b)
    x = pkg.HipVector.from_numpy(x0)
    assert np.array_equal(pkg.jacobi_(x, A, bd, maxiter=k).to_numpy(), ref.jacobi(M, b, x0, k)[0]), "jacobi"
    x = pkg.HipVector.from_numpy(x0)
    assert np.array_equal(pkg.gauss_seidel_(x, A, bd, maxiter=k).to_numpy(), ref.gauss_seidel(M, b, x0, k)[0]), "gauss_seidel"
    x = pkg.HipVector.from_numpy(x0)
    xr, rr, _ = ref.sor(M, b, x0, omega, k)
    r = pkg.sor_(x, A, bd, omega, maxiter=k)
    assert np.array_equal(r.to_numpy(), rr) and np.array_equal(x.to_numpy(), xr), "sor"
    x = pkg.HipVector.from_numpy(x0)
    assert np.array_equal(pkg.ssor_(x, A, bd, omega, maxiter=k).to_numpy(), ref.ssor(M, b, x0, omega, k)[0]), "ssor"
