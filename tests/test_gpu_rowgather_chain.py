"""k_spmv_rowgather (csrc/mik_spmv.h) after its latency chain was shortened: the row bounds, the block bounds, the fused dot's x[r]
and the stop flag come in ONE round trip before the tile DMA, and the first eight gathers of x of every row are issued UNDER the value
stream -- behind a counted wait for the column pieces alone, whose count (the value pieces this wave issued: 0 .. 4 at fp64, 0 .. 2 at fp32)
differs from wave to wave and from pass to pass.  A gather slot that no row of a wave reaches is not issued; the cases hold waves whose rows
all end before slot 7, waves that reach it, and waves without any entry.

Every case runs on the CSR arrays, asserts that k_spmv_rowgather is what runs, and holds mul! -- with and without the fused dot, fp64 and
fp32 -- to the oracle and to k_spmv_rowblock (MIK_KNOB_CSR_KERNEL = 1) bit for bit; the dot(x, y) segment sums are held to
k_spmv_rowblock's.  The shapes are the smallest at which the new code can go wrong: entry counts around every piece boundary, more than one
pass, misaligned block starts, n around one row-block, empty rows and an empty row-block, rows beyond one gather chunk and beyond the
long-row threshold, row-range launches (mik_dev_spmv_run) and the strip map inside cg!."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import KN

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SENTINEL = 7.0                       # what a launch must leave alone


def csr_from_lengths(lens, n_cols, dtype, seed):
    """rows of the given lengths: sorted distinct columns drawn from [0, n_cols), values of both signs away from 0"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n_cols, size=int(l), replace=False)) for l in lens] + [np.empty(0, np.int64)]).astype(np.int64)
    val = (rng.uniform(0.5, 1.5, col.size) * rng.choice([-1.0, 1.0], col.size)).astype(dtype)
    return rowptr, col, val


def spread(total, rows, seed):
    """`total` entries over `rows` rows: as even as possible, the longer rows in seeded places"""
    lens = np.full(rows, total // rows, np.int64)
    lens[np.random.default_rng(seed).permutation(rows)[: total % rows]] += 1
    return lens


def oracle_csc(orc, n, rowptr, col, val):
    M = sp.csr_matrix((val, col, rowptr), shape=(n, n)).tocsc()
    M.sort_indices()
    return orc.CSC(n, M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.copy(), 0)


def run(pkg, dA, dx, fuse_dot=False, rows=(0, -1), skip=None):
    """mik_dev_spmv_run into a y and segment sums filled with SENTINEL: (y, seg)"""
    nb = -(-dA.n_rows // 256)
    y = pkg.HipVector(dA.n_rows, dA.dtype).fill_(SENTINEL)
    seg = pkg.HipVector(nb, dA.dtype).fill_(SENTINEL)
    sb, se = skip if skip else (-1, 0)
    rc = pkg.lib().mik_dev_spmv_run(dA.ctx.handle, dA.handle, C.c_void_p(dx.ptr), C.c_void_p(y.ptr), int(fuse_dot), C.c_void_p(seg.ptr),
                                    rows[0], rows[1], sb, se)
    pkg._lib.check(rc, "mik_dev_spmv_run", dA.ctx.handle)
    return y.to_numpy(), seg.to_numpy()


def upload_csr(pkg, n, rowptr, col, val):
    L = pkg.lib()
    L.mik_set_tuning(KN.LAYOUTS, KN.CSR_ONLY)
    L.mik_set_tuning(KN.CSR_KERNEL, 2)
    dA = pkg.HipCSR(n, n, rowptr, col, val, index_base=0, is_csc=False)
    assert dA.spmv_kernel() == "k_spmv_rowgather"
    return dA


def both_kernels_agree(pkg, orc, n, rowptr, col, val, seed=3):
    """mul! and the fused launch of k_spmv_rowgather against the oracle and k_spmv_rowblock; returns (dA, dx, y, seg) of k_spmv_rowgather"""
    L = pkg.lib()
    dtype = val.dtype
    dA = upload_csr(pkg, n, rowptr, col, val)
    x = np.random.default_rng(seed).standard_normal(n).astype(dtype)
    dx = pkg.HipVector.from_numpy(x)
    want = orc.spmv(oracle_csc(orc, n, rowptr, col, val), x)
    y = pkg.mul_(pkg.HipVector(n, dtype).fill_(SENTINEL), dA, dx).to_numpy()
    yf, seg = run(pkg, dA, dx, fuse_dot=True)
    assert np.array_equal(y, want) and np.array_equal(yf, want)
    L.mik_set_tuning(KN.CSR_KERNEL, 1)
    assert dA.spmv_kernel().startswith("k_spmv_rowblock")
    y1 = pkg.mul_(pkg.HipVector(n, dtype).fill_(SENTINEL), dA, dx).to_numpy()
    y1f, seg1 = run(pkg, dA, dx, fuse_dot=True)
    L.mik_set_tuning(KN.CSR_KERNEL, 2)
    assert dA.spmv_kernel() == "k_spmv_rowgather"
    assert np.array_equal(y, y1) and np.array_equal(yf, y1f) and np.array_equal(seg, seg1)
    return dA, dx, y, seg


@pytest.fixture
def long_rows(orc, ctx):
    orc.set_long_row(ctx.spmv_long_row(), ctx.spmv_long_segment(), ctx.spmv_long_group())
    yield
    orc.set_long_row(0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entries", [0, 1, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049])
def test_piece_counts(pkg, orc, ctx, dtype, entries):
    """one row-block of 256 rows with this many entries: a value piece is 128 (fp32: 256) entries, a column piece 256, and wave w issues
    the pieces w, w + 4, ... that hold an entry -- so the counted wait differs between the waves; 2049 needs a second pass of one entry"""
    n = 256
    rowptr, col, val = csr_from_lengths(spread(entries, n, entries), n, dtype, 100 + entries)
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_one_pass(pkg, orc, ctx, dtype):
    """600 rows of 20 entries: 5120 entries in the first row-block, three passes, and 2048 = 102 * 20 + 8 cuts a row at both tile boundaries"""
    n = 600
    rowptr, col, val = csr_from_lengths(np.full(n, 20), n, dtype, 21)
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pass_ends_at_a_row_end(pkg, orc, ctx, dtype):
    """256 rows of 16 entries: the first pass ends exactly where row 127 does (2048 = 128 * 16), the second where the block does"""
    n = 256
    rowptr, col, val = csr_from_lengths(np.full(n, 16), n, dtype, 22)
    assert rowptr[128] == 2048
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_sizes_and_misaligned_block_starts(pkg, orc, ctx, dtype, n):
    """odd row lengths (1, 3, 5, 7 in seeded order), the last row of every full row-block lengthened until the next block starts at an entry
    that is 1, 2, 3 mod 4: kb is then rounded down into the block before, in both streams (n = 257: one such block of one row; n = 1000: three)"""
    lens = np.minimum(np.random.default_rng(n).choice([1, 3, 5, 7], n), n)
    for b in range(1, -(-n // 256)):
        lens[256 * b - 1] += (b - int(lens[: 256 * b].sum())) % 4
    rowptr, col, val = csr_from_lengths(lens, n, dtype, 30 + n)
    assert [int(rowptr[256 * b]) % 4 for b in range(1, -(-n // 256))] == [1, 2, 3][: -(-n // 256) - 1]
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_and_an_empty_row_block(pkg, orc, ctx, dtype):
    """three row-blocks: the first with every third row empty, the second without any entry (y = 0 there, its dot partial 0), the third full"""
    n = 768
    lens = np.full(n, 5)
    lens[0:256:3] = 0
    lens[256:512] = 0
    rowptr, col, val = csr_from_lengths(lens, n, dtype, 41)
    dA, dx, y, seg = both_kernels_agree(pkg, orc, n, rowptr, col, val)
    assert not y[256:512].any() and not y[0:256:3].any() and y[512:].all()
    assert seg[1] == 0 and seg[0] != 0 and seg[2] != 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_longer_than_a_gather_chunk(pkg, orc, ctx, dtype):
    """rows of 0 .. 40 entries in one block and the next: second to fifth chunk of eight, lanes of one wave leaving the loop at different trips"""
    n = 512
    lens = np.random.default_rng(5).integers(0, 41, n)
    lens[[3, 77, 300]] = [8, 9, 16]
    assert lens.max() <= ctx.spmv_long_row()
    rowptr, col, val = csr_from_lengths(lens, n, dtype, 51)
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_beyond_the_long_row_threshold(pkg, orc, ctx, dtype, long_rows):
    """two rows longer than MIK_LONG_ROW among short ones: k_spmv_longrows sums them first, k_spmv_rowgather picks y[r] up (is_long)"""
    n = 2 * ctx.spmv_long_row() + 600
    lens = np.random.default_rng(6).integers(1, 12, n)
    lens[[5, 300]] = [ctx.spmv_long_row() + 1, ctx.spmv_long_row() + 37]
    rowptr, col, val = csr_from_lengths(lens, n, dtype, 61)
    both_kernels_agree(pkg, orc, n, rowptr, col, val)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_ranges_and_skips(pkg, orc, ctx, dtype):
    """rows=(1, 2) and skip=(2, 4) of tests/test_gpu_spmv_plan.py, launched: the rows of the request equal the whole launch's, with their
    segment sums; nothing else is written"""
    A = orc.laplace(12, 3).astype(dtype)                       # n = 1728: 7 row-blocks, the last one short
    n = A.n
    S = A.to_scipy().tocsr()
    S.sort_indices()
    dA, dx, y, seg = both_kernels_agree(pkg, orc, n, S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.astype(dtype))
    blocks = np.arange(n) // 256
    for kw, inside in ((dict(rows=(1, 2)), (blocks >= 1) & (blocks < 3)), (dict(skip=(2, 4)), (blocks < 2) | (blocks >= 4)),
                       (dict(rows=(6, 1)), blocks == 6)):
        for fd in (False, True):
            yr, sr = run(pkg, dA, dx, fuse_dot=fd, **kw)
            assert np.array_equal(yr[inside], y[inside]) and np.all(yr[~inside] == SENTINEL)
            seg_in = np.unique(blocks[inside])
            seg_out = np.setdiff1d(np.arange(7), seg_in)
            assert np.all(sr[seg_out] == SENTINEL)
            assert np.array_equal(sr[seg_in], seg[seg_in]) if fd else np.all(sr == SENTINEL)


def test_strip_map_inside_cg(pkg, orc, ctx):
    """the 48^3 Laplacian (432 row-blocks) on the CSR arrays: 30 steps of cg! with reltol = 0 against the oracle's TREE mode"""
    N = 48
    n, colptr, rowval, nzval = pkg.fixtures.laplace_matrix(N, 3)
    b = pkg.fixtures.hashed_rhs(n)
    A = pkg.HipCSR(n, n, colptr, rowval, nzval, index_base=1).set_layout("csr")
    assert A.spmv_kernel() == "k_spmv_rowgather"
    x, hist = pkg.cg(A, pkg.HipVector.from_numpy(b), log=True, reltol=0.0, maxiter=30)
    xo, ho = orc.cg(orc.CSC(n, colptr, rowval, nzval, 1), b, reltol=0.0, maxiter=30, mode="tree", shape=ctx.cg_shape(np.float64))
    assert hist.iters == ho["iters"] == 30
    assert np.array_equal(hist["resnorm"], ho["resnorm"])
    assert np.array_equal(x.to_numpy(), xo)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_is_stored_behind_a_stop(pkg, orc, ctx, dtype):
    """after iterate_many has stopped on maxiter, one more batch leaves x, r and c as they are"""
    A = orc.laplace(12, 3).astype(dtype)
    dA = pkg.HipCSR(A.n, A.n, A.colptr, A.rowval, A.nzval, index_base=A.index_base).set_layout("csr")
    assert dA.spmv_kernel() == "k_spmv_rowgather"
    b = pkg.HipVector.from_numpy(orc.hashed_rhs(A.n).astype(dtype))
    it = pkg.cg_iterator_(pkg.zerox(dA, b), dA, b, reltol=0.0, initially_zero=True, maxiter=10)
    assert it.iterate_many(0, 25).size == 10
    before = [v.to_numpy() for v in (it.x, it.r, it.c)]
    assert it.iterate_many(10, 25).size == 0
    after = [v.to_numpy() for v in (it.x, it.r, it.c)]
    assert all(np.array_equal(a, c) for a, c in zip(before, after))
