"""The four block entries of lobpcg (csrc/mik_lobpcg.h) on the paths tests/test_gpu_lobpcg.py does not reach: more than one LDS tile per
row-block, more than one pass of every grid-stride loop, every template width, both host staging paths, leading dimensions with padding,
and the driver on blocks wider than four.  Every comparison is bit for bit: mik_spmm against mik_spmv column by column AND against the CPU
oracle's spmv, mik_block_gram against mik_dot AND the oracle's tree, mik_block_rdiv / mik_block_update against the numpy loops of
tests/lobpcg_double.py, the driver against the numpy double.  GPU box only (-m gpu).

The operators of section 1 come from tests/lobpcg_fixtures.py, where each asserts the properties it was built for (the CPU suite runs those
assertions too); here each additionally asserts what selects the kernel over the column-by-column fallback: no row longer than
mik_spmv_long_row(), and compact() never called.

Grid-stride loops: the row loops of k_block_rdiv / k_block_update and the segment loop of k_block_gram are capped at sweep_grid_cap = 32
workgroups per compute unit, 8192 on an MI355X.  As tests/test_gpu_large_reductions.py does for the lean finalisers, the launches are
planned for an 8-CU machine (development knob MIK_KNOB_MACHINE: cap = 256) so that small vectors take 2 and 3 passes, the last one ragged;
references are computed with the plan back at 0.  One gram rung runs at the machine's real cap.

The case that launches each template instance (both element types each):

    k_spmm_rowgather<., 1>    test_spmm_the_kernel_itself, b = 1
    k_spmm_rowgather<., 2>    ... b = 2
    k_spmm_rowgather<., 4>    ... b = 3, 4
    k_spmm_rowgather<., 8>    ... b = 5, 8 (one column block), 9, 16 (two), 17 (three, the last one column wide), 32 (four)
    k_block_rdiv<., 4>        test_rdiv_every_width, s = 3, 4;            several row passes: test_rdiv_and_update_over_several_grid_passes, s = 3
    k_block_rdiv<., 8>        ... s = 5, 8
    k_block_rdiv<., 16>       ... s = 9, 16;                              the driver at block 9 and 12
    k_block_rdiv<., 32>       ... s = 17, 31;                             several row passes: s = 17
    k_block_update<., 4>      test_update_every_width, sx = 2;            several row passes: (3, 3, 2)
    k_block_update<., 8>      ... sx = 5, 6
    k_block_update<., 16>     ... sx = 9, 12, 16;                         the driver at block 9 and 12
    k_block_update<., 32>     ... sx = 17, 18, 19, 31;                    several row passes: (17, 5, 4)
    k_block_gram<., true>     every gram test in the aligned placement;   several segment passes: test_gram_over_several_grid_passes
    k_block_gram<., false>    ... in the offset placement (odd leading dimension, pointer 1 element past a 16-byte boundary)

blk_rot_row's unrolled-by-4 loop starts at column 1, so k columns leave (k - 1) % 4 for its tail: the shapes of test_update_every_width give
k = 2, 5, 6, 7, 9, 12, 16, 17, 18, 19, 30, 31 and 1 -- every remainder, with and without a trip of the unrolled loop.  The host staging
(mik_stage_small) switches at 8192 bytes: in Float64 (18, 18, 18) stages 54 x 18 x 8 = 7776 bytes through the pinned area, (19, 19, 19) 8664
bytes from a packed copy; s = 31 / 32 of rdiv sit below / at the switch.  Both are also called with leading dimensions larger than the
matrix, the padding NaN."""
import ctypes as C
import gc
from contextlib import contextmanager

import numpy as np
import pytest
import scipy.sparse as sp

import lobpcg_fixtures as fx
from conftest import KN
from host_double import FakeOperator, FakeVector
from ladder import ladder
from lobpcg_double import block_rdiv, block_update
from lobpcg_gpu_util import DTYPES, Blk, both, code, dots, gram_raw, same_trace, spd_b, update_raw, wide

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
SENTINEL = -7.5
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
SMALL_MACHINE = 8 | (1 << 16)           # compute units | XCDs << 16: sweep_grid_cap = 256
PLACEMENTS = (False, True)


@pytest.fixture(autouse=True)
def long_row_shape(orc, ctx):
    """the oracle's spmv with the device's rule for long rows (none of the operators here has one: asserted per operator)"""
    orc.set_long_row(ctx.spmv_long_row(), ctx.spmv_long_segment(), ctx.spmv_long_group())
    yield
    orc.set_long_row(0)
    gc.collect()


@contextmanager
def small_machine(ctx):
    ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
    try:
        cap = ctx.info()["sweep_grid_cap"]
        assert cap == 256
        yield cap
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


# ==============================================================================================
# 1. mik_spmm where k_spmm_rowgather does the work
# ==============================================================================================
def oracle_spmv(orc, S, X):
    """the oracle's column scatter of the same matrix, column by column of X"""
    S = S.tocsc()
    S.sort_indices()
    if S.shape[0] == S.shape[1]:
        A = orc.CSC(S.shape[0], S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.copy(), 0)
        return np.stack([orc.spmv(A, np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])], axis=1)
    A = FakeOperator(orc, S)                                                    # the same oracle entry with n_rows != n_cols
    return np.stack([A.mul(FakeVector(np.zeros(S.shape[0], S.dtype)), FakeVector(X[:, j])).a for j in range(X.shape[1])], axis=1)


def spmm_raw(pkg, ctx, A, b, X, Y):
    rc = pkg.lib().mik_spmm(ctx.handle, A.handle, b, _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld)
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)


def check_spmm(pkg, ctx, name, A, Xh, wants):
    """every width, both placements, Y and all padding pre-filled with a sentinel; `wants`: the references, each n_rows x 32"""
    n_rows, n_cols, dt = A.n_rows, A.n_cols, Xh.dtype
    for b in WIDTHS:
        for offset in PLACEMENTS:
            X = Blk(pkg, ctx, Xh[:, :b], offset, fill=SENTINEL)
            Y = Blk(pkg, ctx, np.full((n_rows, b), SENTINEL, dt), offset, fill=SENTINEL)
            assert (X.n, Y.n) == (n_cols, n_rows) and X.ld >= n_cols and Y.ld >= n_rows
            spmm_raw(pkg, ctx, A, b, X, Y)
            got = Y.get()
            for which, want in wants.items():
                assert np.array_equal(got, want[:, :b]), (name, b, offset, which)
            assert np.all(Y.padding() == SENTINEL) and (Y.padding().size > 0 or not offset), (name, b, offset, "padding of Y")
            assert np.array_equal(X.get(), Xh[:, :b]) and np.all(X.padding() == SENTINEL), (name, b, offset, "X")


def references(pkg, orc, ctx, A, S, Xh):
    """mik_spmv column by column (the definition of mik_spmm), and the oracle"""
    Xd = Blk(pkg, ctx, Xh, False)
    dev = np.stack([pkg.mul_(pkg.HipVector(A.n_rows, Xh.dtype, ctx), A, Xd.col(j)).to_numpy() for j in range(Xh.shape[1])], axis=1)
    return {"mik_spmv": dev, "oracle": oracle_spmv(orc, S, Xh)}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(fx.SPMM_BUILDERS))
def test_spmm_the_kernel_itself(pkg, orc, ctx, dt, name):
    S = fx.SPMM_BUILDERS[name](dt, ctx.spmv_long_row())
    assert np.diff(S.indptr).max() <= ctx.spmv_long_row()
    A = fx.upload(pkg, ctx, S)                                                  # never compacted
    Xh = wide(np.random.default_rng(41), (S.shape[1], 32), dt)
    check_spmm(pkg, ctx, name, A, Xh, references(pkg, orc, ctx, A, S, Xh))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("layout", ["csr", "auto"])
def test_spmm_laplace_12_cubed_on_either_layout(pkg, orc, ctx, dt, layout):
    """mik_spmm reads the CSR arrays whatever layout mik_spmv runs on; the reference mul_ runs on the forced / the default (sliced) layout"""
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(12, 3, dtype=dt, index_base=0)
    S = sp.csc_matrix((nz, rv, cp), shape=(n, n))
    assert np.diff(S.tocsr().indptr).max() == 7 <= ctx.spmv_long_row()
    A = pkg.HipCSR(n, n, cp, rv, nz, index_base=0, ctx=ctx)                     # never compacted
    assert A.layout() != "csr-rowblock"                                         # the default is one of the sliced layouts
    A.set_layout(layout)
    assert (A.layout() == "csr-rowblock") == (layout == "csr")
    Xh = wide(np.random.default_rng(42), (n, 32), dt)
    check_spmm(pkg, ctx, f"laplace 12^3 {layout}", A, Xh, references(pkg, orc, ctx, A, S, Xh))


@pytest.mark.parametrize("dt", DTYPES)
def test_spmm_non_finite_values_stay_in_the_rows_that_reference_them(pkg, orc, ctx, dt):
    """slots past a row's end gather X[0, .], columns past the block gather column j0 again: neither may reach a sum.  X[0, :] = Inf,
    X[c, 1] = NaN for a referenced column c, X[n - 1, b - 1] = -Inf; rows that reference none of the three stay finite"""
    S = fx.ragged(dt, ctx.spmv_long_row())
    n = S.shape[1]
    A = fx.upload(pkg, ctx, S)
    refs = np.bincount(S.indices, minlength=n)
    c = int(np.flatnonzero(refs[1:n - 1] >= 5)[0]) + 1
    assert refs[0] > 0 and refs[c] >= 5 and refs[n - 1] > 0 and 0 < c < n - 1
    touched = np.zeros(S.shape[0], bool)
    touched[np.unique(S.tocoo().row[np.isin(S.tocoo().col, [0, c, n - 1])])] = True
    assert 0 < np.count_nonzero(touched) < S.shape[0] // 4
    rng = np.random.default_rng(43)
    for b in (2, 3, 5, 17):
        Xh = wide(rng, (n, b), dt)
        Xh[0, :] = np.inf
        Xh[c, 1] = np.nan
        Xh[n - 1, b - 1] = -np.inf
        with np.errstate(all="ignore"):
            want = oracle_spmv(orc, S, Xh)
        assert np.all(np.isfinite(want[~touched])) and not np.all(np.isfinite(want[touched]))
        for offset in PLACEMENTS:
            X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, np.full((S.shape[0], b), SENTINEL, dt), offset)
            spmm_raw(pkg, ctx, A, b, X, Y)
            got = Y.get()
            assert np.array_equal(got, want, equal_nan=True), (b, offset)
            assert np.all(np.isfinite(got[~touched])) and np.any(~touched & (np.diff(S.indptr) > 0)), (b, offset)


# ==============================================================================================
# 2. every grid-stride loop taken more than once
# ==============================================================================================
def stride_sizes(ctx, dt):
    """[(m, n)]: m = cap + 1 and 2 * cap + 37 segments of the reduction tree, the last one partial and no multiple of W"""
    W, L = ctx.reduce_shape(dt)
    SEG = 256 * W * L
    return W, L, [(m, (m - 1) * SEG + SEG // 2 + 3) for m in (256 + 1, 2 * 256 + 37)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_gram_over_several_grid_passes(pkg, orc, ctx, dt, which):
    """planned for cap = 256: the segment loop (two barriers in its body) runs 2 and 3 times, the last pass with 1 / 37 workgroups"""
    W, L, sizes = stride_sizes(ctx, dt)
    m, n = sizes[which]
    rng = np.random.default_rng(50 + which)
    Xh, Yh = wide(rng, (n, 9), dt), wide(rng, (n, 4), dt)
    cases = [(1, 1), (5, 3), (4, 4), (9, 2)]
    ref_orc = np.array([[orc.dot(np.ascontiguousarray(Xh[:, i]), np.ascontiguousarray(Yh[:, j]), "tree", W, L) for j in range(4)] for i in range(9)], dt)
    win_orc = np.array([[orc.dot(np.ascontiguousarray(Xh[:, i]), np.ascontiguousarray(Xh[:, 2 + j]), "tree", W, L) for j in range(4)] for i in range(4)], dt)
    for offset in PLACEMENTS:
        X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Yh, offset)
        with small_machine(ctx) as cap:
            assert cap < m
            got = [gram_raw(pkg, ctx, X, p, Y, q) for (p, q) in cases]
            win = gram_raw(pkg, ctx, X, 4, X, 4, x0=0, y0=2)                    # overlapping column windows of one block: 0..3 against 2..5
        ref_dev = dots(pkg, X, 9, Y, 4)                                         # the plan is back at 0
        assert np.array_equal(ref_dev, ref_orc), (m, offset, "mik_dot against the oracle")
        for (p, q), G in zip(cases, got):
            assert np.array_equal(G, ref_orc[:p, :q]), (m, p, q, offset, "oracle")
            assert np.array_equal(G, ref_dev[:p, :q]), (m, p, q, offset, "mik_dot")
        assert np.array_equal(win, win_orc) and np.array_equal(win, dots(pkg, X, 4, X, 4, 0, 2)), (m, offset, "windows")


@pytest.mark.parametrize("dt", DTYPES)
def test_gram_one_rung_past_the_real_cap(pkg, orc, ctx, dt):
    """m = sweep_grid_cap + 1 segments as the machine is: the second pass is one workgroup per tile"""
    from test_gpu_large_reductions import base, rungs_of
    W, L, lad = rungs_of(ctx, dt)
    m, n, _ = lad["cap_plus1"]
    assert m == ctx.info()["sweep_grid_cap"] + 1 and lad == ladder(W, L, ctx.info()["sweep_grid_cap"])
    Xh, Yh = np.stack([base(dt, j, n) for j in (0, 1)], axis=1), np.stack([base(dt, j, n) for j in (2, 3, 4)], axis=1)
    X, Y = Blk(pkg, ctx, Xh, False), Blk(pkg, ctx, Yh, False)
    G = gram_raw(pkg, ctx, X, 2, Y, 3)
    want = np.array([[orc.dot(base(dt, i, n), base(dt, 2 + j, n), "tree", W, L) for j in range(3)] for i in range(2)], dt)
    assert np.array_equal(G, want) and np.array_equal(G, dots(pkg, X, 2, Y, 3)), (m, n)


def rdiv_factor(rng, s, dt):
    """as tests/test_gpu_lobpcg.py: off-diagonal magnitudes in 2^-3 .. 2, diagonal in 1 .. 8, the strict lower triangle NaN (never read)"""
    R = np.triu(rng.choice([-1.0, 1.0], size=(s, s)) * np.exp2(rng.uniform(-3, 0, size=(s, s))) * (1 + rng.random((s, s))), 1)
    R = (R + np.diag(rng.choice([-1.0, 1.0], size=s) * np.exp2(rng.uniform(0, 2, size=s)) * (1 + rng.random(s)))).astype(dt)
    R[np.tril_indices(s, -1)] = np.nan
    return R


def rdiv_raw(pkg, ctx, n, s, Rf, X):
    """Rf: Fortran order, its row count is the leading dimension"""
    assert Rf.flags.f_contiguous
    rc = pkg.lib().mik_block_rdiv(ctx.handle, code(pkg, X.dt), n, s, Rf.ctypes.data_as(_vp), Rf.shape[0], _vp(X.ptr), X.ld)
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)


def update_case(rng, n, sx, b1, b2, dt):
    Xh, Rh, Ph = wide(rng, (n, sx), dt, 20), wide(rng, (n, max(b1, 1)), dt, 20), wide(rng, (n, max(b2, 1)), dt, 20)
    return Xh, Rh, Ph, wide(rng, (sx + b1 + b2, sx), dt, 20)


def check_update(pkg, ctx, n, sx, b1, b2, Xh, Rh, Ph, V, xo, po, offset, what, equal_nan=False):
    sentinel = np.full((n, sx), SENTINEL, Xh.dtype)
    X, R, P = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Rh, offset), Blk(pkg, ctx, Ph, offset)
    Xo, Po = Blk(pkg, ctx, sentinel, offset, fill=SENTINEL), Blk(pkg, ctx, sentinel, offset, fill=SENTINEL)
    assert update_raw(pkg, ctx, n, sx, b1, b2, X, R, P, V, Xo, Po) == 0, pkg.lib().mik_last_error(ctx.handle)
    gx, gp = Xo.get(), Po.get()
    assert np.array_equal(gx, xo, equal_nan=equal_nan), (what, "Xout")
    assert np.array_equal(gp, po, equal_nan=equal_nan), (what, "Pout")
    assert np.all(Xo.padding() == SENTINEL) and np.all(Po.padding() == SENTINEL), (what, "padding")
    return gx, gp


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_rdiv_and_update_over_several_grid_passes(pkg, ctx, dt, which):
    """planned for cap = 256 workgroups of 256 rows: the row loops run 2 and 3 times, the last pass 1 row / 37 workgroups and 5 rows"""
    n = (256 * 256 + 1, 2 * 256 * 256 + 37 * 256 + 5)[which]
    rng = np.random.default_rng(60 + which)
    for s in (3, 17):
        Xh, R = wide(rng, (n, s), dt, span=20), rdiv_factor(rng, s, dt)
        want = block_rdiv(Xh.copy(), R)
        assert np.all(np.isfinite(want))
        X = Blk(pkg, ctx, Xh, bool(which), fill=SENTINEL)
        with small_machine(ctx) as cap:
            assert n > cap * 256
            rdiv_raw(pkg, ctx, n, s, np.asfortranarray(R), X)
        assert np.array_equal(X.get(), want) and np.all(X.padding() == SENTINEL), (n, s)
    for (sx, b1, b2) in [(3, 3, 2), (17, 5, 4)]:
        Xh, Rh, Ph, V = update_case(rng, n, sx, b1, b2, dt)
        xo, po = block_update(sx, b1, b2, Xh, Rh, Ph, V)
        with small_machine(ctx):
            check_update(pkg, ctx, n, sx, b1, b2, Xh, Rh, Ph, V, xo, po, bool(which), (n, sx, b1, b2))


# ==============================================================================================
# 3. every template width, both staging paths, padded leading dimensions
# ==============================================================================================
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [255, 4097])
def test_rdiv_every_width(pkg, ctx, dt, n):
    """a column grows by at most a factor 2^2 per earlier column (tests/test_gpu_lobpcg.py), so up to 32 columns of data up to 2^21 stay
    finite in Float32; R is passed tight and as the corner of a 40 x 40 array of NaN"""
    rng = np.random.default_rng(n + 70)
    for s in (3, 4, 5, 8, 9, 16, 17, 31):
        Xh, R = wide(rng, (n, s), dt, span=20), rdiv_factor(rng, s, dt)
        want = block_rdiv(Xh.copy(), R)
        assert np.all(np.isfinite(want))
        R40 = np.full((40, 40), np.nan, dt, order="F")
        R40[:s, :s] = R
        for Rf in (np.asfortranarray(R), R40):
            for offset in PLACEMENTS:
                X = Blk(pkg, ctx, Xh, offset, fill=SENTINEL)
                rdiv_raw(pkg, ctx, n, s, Rf, X)
                assert np.array_equal(X.get(), want), (n, s, Rf.shape[0], offset)
                assert np.all(X.padding() == SENTINEL), (n, s, Rf.shape[0], offset, "padding")


UPDATE_SHAPES = [(2, 2, 2), (5, 5, 2), (6, 6, 6), (9, 9, 9), (12, 7, 6), (16, 16, 16), (17, 2, 1), (18, 18, 18), (19, 19, 19), (31, 31, 30)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [255, 4097])
def test_update_every_width(pkg, ctx, dt, n):
    """V is passed tight and with five rows of NaN below it (ldv > sx + b1 + b2)"""
    rng = np.random.default_rng(n + 71)
    assert {(k - 1) % 4 for s in UPDATE_SHAPES for k in s} == {0, 1, 2, 3}
    for (sx, b1, b2) in UPDATE_SHAPES:
        Xh, Rh, Ph, V = update_case(rng, n, sx, b1, b2, dt)
        xo, po = block_update(sx, b1, b2, Xh, Rh, Ph, V)
        assert np.all(np.isfinite(xo)) and np.all(np.isfinite(po))
        Vpad = np.full((sx + b1 + b2 + 5, sx), np.nan, dt)
        Vpad[:sx + b1 + b2] = V
        for Vin in (V, Vpad):
            for offset in PLACEMENTS:
                check_update(pkg, ctx, n, sx, b1, b2, Xh, Rh, Ph, Vin, xo, po, offset, (n, sx, b1, b2, Vin.shape[0], offset))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [255, 4097])
def test_gram_every_tile_remainder_into_a_padded_result(pkg, ctx, dt, n):
    """ldg = p + 3: the rows of G below p keep their sentinel"""
    rng = np.random.default_rng(n + 72)
    for (p, q) in [(3, 5), (4, 1), (1, 4), (7, 9), (31, 17)]:
        Xh, Yh = wide(rng, (n, p), dt), wide(rng, (n, q), dt)
        for offset in PLACEMENTS:
            X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Yh, offset)
            G = gram_raw(pkg, ctx, X, p, Y, q, ldg=p + 3, fill=SENTINEL)
            assert G.shape == (p + 3, q) and np.array_equal(G[:p], dots(pkg, X, p, Y, q)), (n, p, q, offset)
            assert np.all(G[p:] == SENTINEL), (n, p, q, offset, "padding of G")


@pytest.mark.parametrize("dt", DTYPES)
def test_update_non_finite_rows_stay_in_their_rows(pkg, ctx, dt):
    """a few rows of X / R / P hold Inf and NaN: those rows come out as IEEE arithmetic makes them (the numpy loop), every other row finite"""
    n = 4097
    rng = np.random.default_rng(73)
    for (sx, b1, b2) in [(5, 5, 2), (9, 9, 9), (17, 2, 1)]:
        Xh, Rh, Ph, V = update_case(rng, n, sx, b1, b2, dt)
        Xh[3, 0], Xh[255, sx - 1], Xh[256, 1] = np.inf, np.nan, -np.inf
        Rh[1000, 0], Rh[4096, b1 - 1] = np.nan, np.inf
        Ph[2000, 0], Ph[4096, b2 - 1] = -np.inf, -np.inf
        bad = np.zeros(n, bool)
        bad[[3, 255, 256, 1000, 2000, 4096]] = True
        with np.errstate(all="ignore"):
            xo, po = block_update(sx, b1, b2, Xh, Rh, Ph, V)
        assert np.all(np.isfinite(xo[~bad])) and np.all(np.isfinite(po[~bad])) and not np.any(np.all(np.isfinite(xo[bad]), axis=1))
        for offset in PLACEMENTS:
            gx, gp = check_update(pkg, ctx, n, sx, b1, b2, Xh, Rh, Ph, V, xo, po, offset, (sx, b1, b2, offset), equal_nan=True)
            assert np.all(np.isfinite(gx[~bad])) and np.all(np.isfinite(gp[~bad])), (sx, b1, b2, offset)


# ==============================================================================================
# 4. the driver beyond a block of four
# ==============================================================================================
_SPD = {}


def spd_operator(ctx, dt):
    """tests/lobpcg_fixtures.irregular_spd, once per element type (as CSC, the form lobpcg_gpu_util.both uploads; symmetric)"""
    dt = np.dtype(dt)
    if dt not in _SPD:
        _SPD[dt] = fx.irregular_spd(dt, ctx.spmv_long_row(), n=1500, seed=11).tocsc()
    return _SPD[dt]


def same_run(pkg, rd, rh):
    assert isinstance(rd.X, pkg.HipMatrix) and rd.iterations == rh.iterations and rd.iterations >= 3
    same_trace(rd.trace, rh.trace)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms) and rd.converged == rh.converged
    assert np.array_equal(rd.X.to_numpy(), rh.X.to_numpy())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("block", [9, 12])
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("jacobi", [False, True])
def test_device_run_with_a_wide_block_equals_the_double(pkg, orc, ctx, dt, block, largest, jacobi):
    """blocks of 9 and 12 columns: mik_spmm with CB = 8 in two column blocks over five tile passes, S = LB = 16, 3 x 3 gram tiles.  Operator
    seed 11 and X0 seed 6 were chosen on the CPU double (tests/lobpcg_double.py) before the first device run: all eight iterations complete
    in both element types, no Cholesky factorisation fails"""
    S = spd_operator(ctx, dt)
    X0 = np.random.default_rng(6).random((S.shape[0], block)).astype(dt)
    rd, rh = both(pkg, orc, ctx, dt, S, None, largest, (X0,), jacobi, maxiter=8)
    assert len(rh.trace) == 8
    same_run(pkg, rd, rh)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("largest", [False, True])
def test_device_generalised_run_with_a_block_of_twelve_equals_the_double(pkg, orc, ctx, dt, largest):
    """A x = lambda B x with the tridiagonal B of spd_b, Jacobi; the seeds (operator 11, X0 6) were chosen on the CPU double as above"""
    S = spd_operator(ctx, dt)
    n = S.shape[0]
    X0 = np.random.default_rng(6).random((n, 12)).astype(dt)
    rd, rh = both(pkg, orc, ctx, dt, S, spd_b(n, dt), largest, (X0,), True, maxiter=8)
    assert len(rh.trace) == 8
    same_run(pkg, rd, rh)


@pytest.mark.parametrize("dt", DTYPES)
def test_device_batches_of_twelve_equal_the_double(pkg, orc, ctx, dt):
    """nev = 20 in batches of 12: the second batch shrinks to 8 columns (S = LB = 8 after 16), the constraint holds 12.  Seeds (operator 11,
    X0 7) chosen on the CPU double as above: both batches run their eight iterations"""
    S = spd_operator(ctx, dt)
    n = S.shape[0]
    X0 = np.random.default_rng(7).random((n, 12)).astype(dt)
    rd, rh = both(pkg, orc, ctx, dt, S, spd_b(n, dt), False, (X0, 20), True, maxiter=8)
    assert len(rd.lam) == 20 and np.array_equal(rd.iterations, rh.iterations) and len(rd.trace) == len(rh.trace) == 2
    for ta, tb in zip(rd.trace, rh.trace):
        assert len(tb) == 8
        same_trace(ta, tb)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms)
    assert np.array_equal(rd.X.to_numpy(), rh.X.to_numpy())
