"""Operators that make k_spmm_rowgather (csrc/mik_lobpcg.h) do the work itself, each with the properties it was built for asserted in plain
numpy.  The kernel gives a workgroup BLOCK = 256 rows and streams that row-block's entries through LDS in passes of TILE = 2048
(MIK_SPMV_TILE of csrc/mik_internal.h), starting at kb = rowptr[first row] & ~3; mik_spmm only launches it while no row is longer than
mik_spmv_long_row() (longer rows are split off at upload, and the operator then goes column by column through mik_spmv).

Every builder returns a scipy CSR matrix with sorted column indices and no stored zero: `upload(pkg, ctx, S)` hands its three arrays over as
they are (is_csc=False).  tests/test_lobpcg_host.py calls every builder, so the property assertions run without a GPU too."""
import numpy as np
import scipy.sparse as sp

BLOCK = 256
TILE = 2048


def values(rng, count, dt):
    """mixed signs, magnitudes 2^-10 .. 2^11: with right-hand sides up to 2^31 a row of 256 products stays finite in Float32"""
    return (rng.choice([-1.0, 1.0], size=count) * np.exp2(rng.uniform(-10, 10, size=count)) * (1 + rng.random(count))).astype(dt)


def from_row_lengths(rng, lens, n_cols, dt):
    """row r gets lens[r] distinct columns, ascending"""
    lens = np.asarray(lens, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.sort(rng.choice(n_cols, size=int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int64)
    S = sp.csr_matrix((values(rng, int(rowptr[-1]), dt), col, rowptr), shape=(len(lens), n_cols))
    assert S.has_sorted_indices and np.all(S.data != 0) and np.array_equal(np.diff(S.indptr), lens)
    return S


def block_starts(S):
    return range(0, S.shape[0], BLOCK)


def block_span(S, r0):
    """(kb, kend) of the row-block that starts at row r0: what the tile loop walks over"""
    return int(S.indptr[r0]) & ~3, int(S.indptr[min(r0 + BLOCK, S.shape[0])])


def passes(S, r0):
    kb, kend = block_span(S, r0)
    return -(-(kend - kb) // TILE)


def straddlers(S):
    """rows whose entries lie on both sides of a tile boundary kb + j * TILE, j >= 1, of their row-block"""
    out = []
    for r0 in block_starts(S):
        kb, kend = block_span(S, r0)
        for edge in range(kb + TILE, kend, TILE):
            for r in range(r0, min(r0 + BLOCK, S.shape[0])):
                if S.indptr[r] < edge < S.indptr[r + 1]:
                    out.append(r)
    return out


def check_runs_the_kernel(S, long_row):
    """the half of spmm_impl's condition that depends on the matrix: no split-off long rows"""
    assert S.nnz > 0 and np.diff(S.indptr).max() <= long_row, (np.diff(S.indptr).max(), long_row)
    return S


# ---- the operators --------------------------------------------------------------------------------------------------------------------
RAGGED_EMPTY = [0, 255, 256, 1499] + [301, 302, 303, 511, 512, 767, 1000, 1279, 1280, 1281, 1498]


def ragged(dt, long_row):
    """1500 x 1500: a last row-block of 220 rows, row lengths uniform in 0 .. 60, empty rows at the edges of blocks and of the matrix (and
    runs of them), every row-block several passes long, rows that straddle a tile boundary"""
    rng = np.random.default_rng(31)
    n = 1500
    lens = rng.integers(0, 61, size=n)
    lens[RAGGED_EMPTY] = 0
    S = from_row_lengths(rng, lens, n, dt)
    lens = np.diff(S.indptr)
    assert n % BLOCK == 220 and lens.min() == 0 and lens.max() == 60
    assert all(lens[r] == 0 for r in RAGGED_EMPTY) and np.count_nonzero(lens == 0) >= 14
    assert all(S.indptr[min(r0 + BLOCK, n)] - S.indptr[r0] > TILE for r0 in block_starts(S))
    assert len(set(straddlers(S))) >= 3
    assert any(S.indptr[r0] & 3 for r0 in block_starts(S))                     # some block's aligned start reaches back into the block before
    return check_runs_the_kernel(S, long_row)


def thresholds(dt, long_row, first):
    """300 x 700, every row as long as a row may be without being split off (long_row = 256), row 0 `first` entries: first = 255 makes
    block 0 65 535 entries -- 32 passes, the last one entry short; first = 256 makes it an exact multiple of TILE"""
    rng = np.random.default_rng(32)
    lens = np.full(300, long_row)
    lens[0] = first
    S = from_row_lengths(rng, lens, 700, dt)
    kb, kend = block_span(S, 0)
    assert long_row == 256 and kb == 0 and kend == 255 * 256 + first
    assert (kend - kb) % TILE == {255: TILE - 1, 256: 0}[first] and passes(S, 0) == 32
    assert (int(S.indptr[256]) & 3) == {255: 3, 256: 0}[first]
    return check_runs_the_kernel(S, long_row)


def one_or_two_passes(dt, long_row, nine, lead):
    """a row-block of 256 rows x 8 entries = TILE exactly (nine: one row has 9, so a second pass of a single entry); lead = 1, 2, 3 puts a
    256-row block of 1280 + lead entries in front, so that the aligned start kb pulls `lead` entries of that block into the tile"""
    rng = np.random.default_rng(33 + 4 * nine + lead)
    lens = np.full(BLOCK, 8)
    if nine:
        lens[137] = 9
    if lead:
        head = np.full(BLOCK, 5)
        head[0] += lead
        lens = np.concatenate([head, lens])
    n = len(lens)
    S = from_row_lengths(rng, lens, n, dt)
    r0 = n - BLOCK
    kb, kend = block_span(S, r0)
    assert int(S.indptr[r0]) - kb == lead and kend - kb == TILE + nine + lead
    assert passes(S, r0) == (2 if nine or lead else 1)
    return check_runs_the_kernel(S, long_row)


def rectangular(dt, long_row, n_rows, n_cols):
    """rows of 0 .. 40 entries; the last column is referenced, so X really has n_cols rows"""
    rng = np.random.default_rng(34 + n_rows)
    lens = rng.integers(0, 41, size=n_rows)
    S = from_row_lengths(rng, lens, n_cols, dt)
    assert S.shape == (n_rows, n_cols) and n_rows != n_cols and np.diff(S.indptr).min() == 0 and np.diff(S.indptr).max() == 40
    assert S.indices.max() == n_cols - 1 and S.indices.min() == 0
    assert all(passes(S, r0) >= 2 for r0 in list(block_starts(S))[:-1])
    return check_runs_the_kernel(S, long_row)


def one_by_one(dt, long_row):
    S = sp.csr_matrix(np.array([[-2.5]], dt))
    assert S.shape == (1, 1) and S.nnz == 1
    return check_runs_the_kernel(S, long_row)


def tridiagonal_257(dt, long_row):
    """the last row-block is the single row 256, its start rowptr[256] = 767 not a multiple of 4"""
    rng = np.random.default_rng(35)
    n = 257
    S = sp.diags([values(rng, n - 1, dt), values(rng, n, dt), values(rng, n - 1, dt)], [-1, 0, 1], format="csr", dtype=dt)
    S.sort_indices()
    assert S.shape == (n, n) and S.nnz == 3 * n - 2 and n - BLOCK == 1 and int(S.indptr[256]) & 3 == 3
    return check_runs_the_kernel(S, long_row)


def irregular_spd(dt, long_row, n=1500, seed=11):
    """the driver's operator: rows of 0 .. 39 random off-diagonal entries in (-1, 1), symmetrised with M + M', the diagonal set to the
    row's absolute sum + 1 + U(0, 1): symmetric and strictly diagonally dominant with a positive diagonal, so positive definite; every
    row-block takes five tile passes"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 40, size=n)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([rng.choice(n, size=int(k), replace=False) for k in lens])
    M = sp.csr_matrix((rng.uniform(-1, 1, size=int(rowptr[-1])), col, rowptr), shape=(n, n))
    S = (M + M.T).tolil()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S = S.astype(dt)                                                          # symmetric before, symmetric after
    off = np.asarray(abs(S).sum(axis=1)).ravel().astype(np.float64)
    S = (S + sp.diags((off + 1 + rng.random(n)).astype(dt))).tocsr().astype(dt)
    S.sort_indices()
    assert (S != S.T).nnz == 0
    d = S.diagonal().astype(np.float64)
    assert np.all(d > 0) and np.all(d - (np.asarray(abs(S).sum(axis=1)).ravel() - d) >= 0.5)
    lens = np.diff(S.indptr)
    assert 8 <= lens.min() and lens.max() <= 69
    assert all(passes(S, r0) == 5 for r0 in block_starts(S))
    return check_runs_the_kernel(S, long_row)


SPMM_BUILDERS = {"ragged": ragged,
                 "thresholds 255": lambda dt, lr: thresholds(dt, lr, 255), "thresholds 256": lambda dt, lr: thresholds(dt, lr, 256)}
for _nine in (False, True):
    for _lead in (0, 1, 2, 3):
        SPMM_BUILDERS[f"{2049 if _nine else 2048} entries, lead {_lead}"] = lambda dt, lr, nine=_nine, lead=_lead: one_or_two_passes(dt, lr, nine, lead)
SPMM_BUILDERS.update({"700 x 1300": lambda dt, lr: rectangular(dt, lr, 700, 1300), "1300 x 700": lambda dt, lr: rectangular(dt, lr, 1300, 700),
                      "1 x 1": one_by_one, "tridiagonal 257": tridiagonal_257})
"""name -> builder(dtype, long_row) of the operators mik_spmm is tested on, the Laplacians apart"""


def upload(pkg, ctx, S):
    """the CSR arrays as they are; never compacted, so the kernel's condition `A->col` holds"""
    assert S.has_sorted_indices
    return pkg.HipCSR(S.shape[0], S.shape[1], S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data, index_base=0, is_csc=False, ctx=ctx)
