"""mik_csr_create three ways -- MIK_KNOB_UPLOAD = 0 (the device pipeline of csrc/mik_upload.hip with its device builders), 1 (the host
path) and 2 (the device transpose with the HOST builders of the wide and jagged layouts on a read-back of the device CSR) -- on the
branches the small matrices of test_gpu_upload.py do not reach: three scan levels, rows at the 256-entry limit of the row sort,
duplicates in a long row, CSR input with unsorted or duplicate columns, rectangular CSC input, the wide layout past 256 patterns, jagged
slices past one scan tile and with waves beyond the last slice, invalid input resident on the device, ragged and tiny slices.  All three
must agree on layout(), spmv_kernel(), spmv_stored_bytes() and the bits of mul_; a square sorted CSC must also give the oracle's bits;
what the oracle does not multiply (rectangular, unsorted, duplicates) carries small integers, so every order of summation and every
fused multiply-add is exact and int64 arithmetic is the reference.  No tolerance anywhere.  GPU box only."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import KN

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SDIAC, SDIA, WIDE, JAGGED, CSR = ("slice-offsets+slice-values+row-masks", "sliced-ell+slice-offsets+row-masks", "wide-slice-values+row-masks",
                                  "jagged-slices", "csr-rowblock")


def three_ways(pkg, make, layouts=0):
    """the operator built with MIK_KNOB_UPLOAD = 0 (device), 1 (host) and 2 (device transpose + host builders)"""
    L = pkg.lib()
    ops = []
    L.mik_set_tuning(KN.LAYOUTS, layouts)
    try:
        for setting in (0, 1, 2):
            L.mik_set_tuning(KN.UPLOAD, setting)
            ops.append(make())
    finally:
        L.mik_set_tuning(KN.UPLOAD, 0)
        L.mik_set_tuning(KN.LAYOUTS, 0)
    return ops


def same_operator(pkg, ops, x, want):
    """ops agree on the layout, the kernel, the stored bytes and the bits of A x; want = those bits; returns the layout"""
    dev = ops[0]
    ys = [pkg.mul_(pkg.HipVector(A.n_rows, x.dtype), A, pkg.HipVector.from_numpy(x)).to_numpy() for A in ops]
    for setting, (A, y) in enumerate(zip(ops, ys)):
        assert A.layout() == dev.layout(), setting
        assert A.spmv_kernel() == dev.spmv_kernel(), setting
        assert A.spmv_stored_bytes() == dev.spmv_stored_bytes(), setting
        assert np.array_equal(y, ys[0]), setting
    assert want.dtype == x.dtype and np.array_equal(ys[0], want)
    return dev.layout()


def random_x(n, dtype, seed):
    x = np.random.default_rng(seed).standard_normal(n).astype(dtype)
    assert np.all(x != 0)                                     # an absent slot of a structured layout adds value * 0: x * 0 must not hide a wrong value
    return x


def small_integers(n, seed, hi=8):
    """nonzero integers in -hi + 1 .. hi - 1"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, hi, size=n) * rng.choice([-1, 1], size=n)


def integer_product(n_rows, rows, cols, vals, x, dtype):
    y = np.zeros(n_rows, np.int64)
    np.add.at(y, rows, vals.astype(np.int64) * x.astype(np.int64)[cols])
    assert np.abs(y).max() < 2 ** 24                          # exact in float32, whatever the order and the contraction
    return y.astype(dtype)


def csc_from_entries(n_cols, rows, cols, vals):
    """0-based CSC arrays of the entries as listed: column by column, rows ascending, duplicates in the order given"""
    order = np.lexsort((rows, cols))                          # stable
    ptr = np.zeros(n_cols + 1, np.int64)
    np.add.at(ptr, cols + 1, 1)
    return np.cumsum(ptr), rows[order].astype(np.int64), vals[order]


def csr_from_offsets(n, offsets, coefs):
    """0-based CSR arrays of the n x n operator with coefs[i] on diagonal offsets[i] (ascending): columns ascend within every row"""
    C = np.arange(n)[:, None] + np.asarray(offsets)[None, :]
    keep = (C >= 0) & (C < n)
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return ptr, C[keep].astype(np.int64), np.broadcast_to(np.asarray(coefs), C.shape)[keep].copy()


def square_csc(pkg, orc, S, dtype, x_seed, layouts=0):
    """three-way agreement + the oracle's bits for a scipy matrix handed over as sorted 1-based CSC; returns the layout"""
    A = orc.CSC.from_scipy(S).astype(dtype)
    x = random_x(A.n, dtype, x_seed)
    ops = three_ways(pkg, lambda: pkg.HipCSR(A.n, A.n, A.colptr, A.rowval, A.nzval, index_base=A.index_base), layouts)
    return same_operator(pkg, ops, x, orc.spmv(A, x))


# ---- three scan levels end to end ----------------------------------------------------------------------------------------------------
BIG_N = 2048 ** 2 + 2049                                      # row-pointer scan: 2050 tiles -> 2 tiles -> 1; slot-pointer scan over 16,393 slices: 2 levels


@functools.lru_cache(maxsize=None)
def big_tridiagonal():
    """1-based CSC of the nonsymmetric tridiagonal operator (-1, 2.5, -1.5); read-only, shared by the four cases"""
    j = np.arange(BIG_N, dtype=np.int64)
    rows = np.stack([j - 1, j, j + 1], axis=1)                # column j holds A[j-1, j], A[j, j], A[j+1, j]
    keep = (rows >= 0) & (rows < BIG_N)
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64) + 1
    nzval = np.broadcast_to(np.array([-1.5, 2.5, -1.0]), rows.shape)[keep].copy()
    out = colptr, rows[keep] + 1, nzval
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("coefficients", ["constant", "one_perturbed"])
def test_three_scan_levels_end_to_end(pkg, orc, ctx, coefficients, dtype):
    """a row pointer that is wrong past row 2048^2 (device_exclusive_scan: a level's offsets not added, the scratch of one level laid over
    the next, data[n] from the wrong slot) moves every later row's entries: other bits than the host path's and the oracle's"""
    colptr, rowval, nzval = big_tridiagonal()
    nzval = nzval.astype(dtype)
    if coefficients == "one_perturbed":                       # one diagonal entry beyond 2048^2 rows: per-row value slots (k_up_row_values)
        r = 2048 ** 2 + 5
        k = colptr[r] - 1 + 1
        assert rowval[k] - 1 == r and nzval[k] == 2.5
        nzval[k] = 3.25
    A = orc.CSC(BIG_N, colptr, rowval, nzval, 1)
    x = random_x(BIG_N, dtype, 11)
    ops = three_ways(pkg, lambda: pkg.HipCSR(BIG_N, BIG_N, colptr, rowval, nzval, index_base=1))
    assert same_operator(pkg, ops, x, orc.spmv(A, x)) == (SDIAC if coefficients == "constant" else SDIA)


# ---- the 256-entry limit of the row sort --------------------------------------------------------------------------------------------
def long_row_matrix(lengths, seed):
    """1024 x 1024: a tridiagonal operator in which a few rows hold exactly lengths[i] entries at columns that are not contiguous"""
    n = 1024
    rng = np.random.default_rng(seed)
    D = np.zeros((n, n))
    i = np.arange(n)
    D[i, i] = 4.0
    D[i[1:], i[:-1]] = -1.0
    D[i[:-1], i[1:]] = -1.25
    for q, (r, length) in enumerate(zip((100, 517, 518, 900), lengths)):
        cols = (np.arange(length) * 3 + q) % n if q % 2 == 0 else np.sort(rng.choice(n, size=length, replace=False))
        D[r] = 0.0
        D[r, cols] = rng.standard_normal(length) + 3.0 * np.sign(rng.standard_normal(length))      # never 0
        assert np.count_nonzero(D[r]) == length
    return sp.csc_matrix(D)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_255_and_256_entries_are_sorted_on_the_device(pkg, orc, ctx, dtype):
    """k_up_sort_rows at its limit (`b - a > 256` returns, the insertion sort moves column and value together): a row left in the order
    of the atomic cursor, or the limit one too low, sums in another order than the oracle"""
    S = long_row_matrix((255, 256, 256, 255), 21)
    assert np.diff(S.tocsr().indptr).max() == 256
    assert square_csc(pkg, orc, S, dtype, 22) in (CSR, JAGGED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_of_257_entries_goes_to_the_host_path(pkg, orc, ctx, dtype):
    """`hs.max_row > 256` in upload_device_t hands the matrix back: kept on the device its unsorted 257-entry row would not give the bits
    of the wave-shaped row sum"""
    S = long_row_matrix((255, 256, 257, 255), 23)
    assert np.diff(S.tocsr().indptr).max() == 257
    orc.set_long_row(ctx.spmv_long_row(), ctx.spmv_long_segment(), ctx.spmv_long_group())
    try:
        square_csc(pkg, orc, S, dtype, 24)
    finally:
        orc.set_long_row(0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_in_a_200_entry_row_of_csc_input(pkg, ctx, dtype):
    """the duplicate scan behind the sort in k_up_sort_rows (`st->dup`): a duplicate that is not reported reaches the mask builders, which
    hold one entry per slot, or is dropped; both entries must be added"""
    n = 512
    i = np.arange(n)
    rows = np.concatenate([i, i[1:], i[:-1]])
    cols = np.concatenate([i, i[:-1], i[1:]])
    keep = rows != 77
    rows, cols = rows[keep], cols[keep]
    lc = (np.arange(198) * 5 + 2) % n                         # 198 distinct columns spread over the row, two of them listed twice
    assert np.unique(lc).size == 198
    lc = np.concatenate([lc, lc[[40, 150]]])
    rows, cols = np.concatenate([rows, np.full(200, 77)]), np.concatenate([cols, lc])
    vals = small_integers(rows.size, 31).astype(dtype)
    ptr, idx, val = csc_from_entries(n, rows, cols, vals)
    x = small_integers(n, 32).astype(dtype)
    ops = three_ways(pkg, lambda: pkg.HipCSR(n, n, ptr, idx, val, index_base=0))
    same_operator(pkg, ops, x, integer_product(n, rows, cols, vals, x, dtype))


# ---- CSR input whose columns are not strictly ascending ------------------------------------------------------------------------------
STENCIL5 = ((-30, -1, 0, 1, 30), (-2, -1, 6, -3, 2), SDIAC)                                        # <= 8 offsets per slice
BAND11 = ((-301, -300, -3, -2, -1, 0, 1, 2, 3, 300, 301), (1, -2, 3, -1, 2, 7, -3, 1, -2, 2, -1), WIDE)   # > 8, <= 32: the wide layout


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", ["none", "two_columns_swapped", "one_column_twice"])
@pytest.mark.parametrize("shape", [STENCIL5, BAND11], ids=["stencil5", "band11"])
def test_csr_input_with_unsorted_or_duplicate_columns(pkg, ctx, shape, defect, dtype):
    """CSR input is neither sorted nor searched for duplicates: the order test of k_up_slice_pattern (`q < p`) / k_up_row_masks
    (`q <= prevq`) and the tests of k_up_wide_masks (`q == ns`, slot taken) keep such rows out of the mask forms, on the device as on the
    host; "none" shows that the shape has the structured layout without the defect"""
    n = 1000
    offsets, coefs, structured = shape
    ptr, idx, val = csr_from_offsets(n, offsets, np.asarray(coefs, dtype))
    a = ptr[500]                                              # row 500 is neither the first row of its slice nor short
    if defect == "two_columns_swapped":
        idx[[a + 1, a + 2]] = idx[[a + 2, a + 1]]
        val[[a + 1, a + 2]] = val[[a + 2, a + 1]]
    elif defect == "one_column_twice":                        # the same column and the same value once more, right behind the first
        idx, val = np.insert(idx, a + 2, idx[a + 1]), np.insert(val, a + 2, val[a + 1])
        ptr = ptr.copy()
        ptr[501:] += 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    x = small_integers(n, 41).astype(dtype)
    ops = three_ways(pkg, lambda: pkg.HipCSR(n, n, ptr, idx, val, index_base=0, is_csc=False))
    layout = same_operator(pkg, ops, x, integer_product(n, rows, idx, val, x, dtype))
    # the mask forms sum a row's slots in ascending slot order and hold one entry per slot: only sorted, duplicate-free rows may have them
    assert layout == structured if defect == "none" else layout in (CSR, JAGGED)


# ---- rectangular CSC input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ["wide_banded", "tall_random"])
def test_rectangular_csc_input(pkg, ctx, shape, dtype):
    """k_up_scatter runs over n_cols, k_up_count_rows checks against n_rows, the cursor and the row pointer hold n_rows + 1: any of them
    taking the other dimension loses or misplaces entries of the longer side"""
    rng = np.random.default_rng(51)
    if shape == "wide_banded":                                # 700 x 1900, six constant diagonals: a structured layout
        n_rows, n_cols = 700, 1900
        offsets = np.array([0, 1, 2, 600, 601, 1199])
        rows = np.repeat(np.arange(n_rows), offsets.size)
        cols = (np.arange(n_rows)[:, None] + offsets[None, :]).ravel()
        vals = np.tile(np.array([5, -1, 2, -3, 1, -2]), n_rows).astype(dtype)
    else:                                                     # 1900 x 700, six distinct random columns per row
        n_rows, n_cols = 1900, 700
        rows = np.repeat(np.arange(n_rows), 6)
        cols = np.argsort(rng.random((n_rows, n_cols)), axis=1)[:, :6].ravel()
        vals = small_integers(rows.size, 52).astype(dtype)
    assert cols.min() >= 0 and cols.max() < n_cols
    ptr, idx, val = csc_from_entries(n_cols, rows, cols, vals)
    x = small_integers(n_cols, 53).astype(dtype)
    ops = three_ways(pkg, lambda: pkg.HipCSR(n_rows, n_cols, ptr, idx, val, index_base=0))
    layout = same_operator(pkg, ops, x, integer_product(n_rows, rows, cols, vals, x, dtype))
    if shape == "wide_banded":
        assert layout == SDIAC


# ---- the wide layout at and past 256 distinct slice patterns ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slices", [256, 300])
def test_wide_layout_with_one_pattern_per_slice(pkg, orc, ctx, slices, dtype):
    """build_sdiaw_device_t: 256 patterns are fetched one by one (`desc + rep[i]`), 300 by one copy of all descriptions indexed through
    rep[] (`all[rep[i]]`); a wrong index gives a slice another slice's values"""
    n = slices * 256
    offsets = np.array([-301, -300, -3, -2, -1, 0, 1, 2, 3, 300, 301])
    ptr, idx, _ = csr_from_offsets(n, offsets, np.zeros(offsets.size))
    rows = np.repeat(np.arange(n), np.diff(ptr))
    d = np.searchsorted(offsets, idx - rows)
    val = ((rows // 256) * offsets.size + d + 1) * 2.0 ** -12           # the value of diagonal d in slice b: one pattern per slice; exact in float32
    assert np.unique(val.astype(np.float32)).size == np.unique((rows // 256) * offsets.size + d).size >= slices * (offsets.size - 2)
    S = sp.csr_matrix((val, idx, ptr), shape=(n, n))
    assert square_csc(pkg, orc, S, dtype, 61) == WIDE


# ---- jagged slices: two scan levels over the slice pointer, a last slice of one row, waves beyond the last slice ----------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64 * 4 + 1, 64 * 5 + 1, 64 * 5 + 2, 64 * 5 + 3, 64 * 6 + 1, 64 * 2048 + 65])
def test_jagged_slices_device_builder_equals_host_builder(pkg, orc, ctx, n, dtype):
    """64 * 4 + 1, 64 * 5 + 1 and 64 * 6 + 1 rows are 5, 6 and 7 slices: 3, 2 and 1 waves of the last four-wave workgroup have no slice
    and read the jptr[nsl + 1 ..] copies; 64 * 2048 + 65 rows are 2,050 slices, the last one of one row"""
    rng = np.random.default_rng(n)
    lens = rng.integers(3, 11, size=n)
    stride = 1 if n < 5000 else 997                           # distinct columns within a row: 15 * stride < n
    pick = np.argsort(rng.random((n, 16)), axis=1)[:, :10]
    keep = np.arange(10)[None, :] < lens[:, None]
    rows = np.repeat(np.arange(n), lens)
    cols = ((np.arange(n)[:, None] + pick * stride) % n)[keep]
    S = sp.csr_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(n, n))
    assert S.nnz == rows.size and np.array_equal(np.diff(S.indptr), lens)
    assert square_csc(pkg, orc, S, dtype, 71, layouts=KN.JAGGED_ALWAYS) == JAGGED


# ---- invalid input that lives in device memory ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_csc", [True, False])
def test_invalid_input_resident_on_the_device_is_refused(pkg, orc, ctx, is_csc):
    """k_up_check_ptr / k_up_count_rows / k_up_convert flag it and upload_device_t returns before the scan, the scatter or any kernel that
    indexes with the arrays; nothing is left on the context"""
    import torch
    dev = torch.device("cuda", 0)
    n = 1000
    ptr, idx, val = csr_from_offsets(n, (-1, 0, 1), np.array([-1.0, 2.0, -1.0]))      # symmetric: the same arrays as CSC and as CSR
    bad_idx = idx.copy()
    bad_idx[1500] = n                                         # one past the last row / column
    bad_ptr = ptr.copy()
    bad_ptr[[600, 601]] = bad_ptr[[601, 600]]                 # ends unchanged, not monotone in the middle
    assert bad_ptr[0] == 0 and bad_ptr[-1] == val.size and np.any(np.diff(bad_ptr) < 0)

    def create(p, i):
        tp, ti, tv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (p, i, val))
        torch.cuda.synchronize()
        return pkg.HipCSR.from_device(n, n, val.size, tp.data_ptr(), ti.data_ptr(), tv.data_ptr(), np.float64, index_base=0, is_csc=is_csc)

    L = pkg.lib()
    x = random_x(n, np.float64, 81)
    want = orc.spmv(orc.CSC(n, ptr, idx, val, 0), x)
    for setting in (0, 1, 2):                                 # 1: the device arrays are staged and the host path validates them
        L.mik_set_tuning(KN.UPLOAD, setting)
        try:
            for p, i in ((ptr, bad_idx), (bad_ptr, idx)):
                with pytest.raises(pkg.MikError) as ei:
                    create(p, i)
                assert ei.value.code == 1                     # MIK_ERR_INVALID: refused by the validation, before anything indexes with it
            A = create(ptr, idx)                              # the context is still usable
        finally:
            L.mik_set_tuning(KN.UPLOAD, 0)
        assert np.array_equal(pkg.mul_(pkg.HipVector(n), A, pkg.HipVector.from_numpy(x)).to_numpy(), want)


# ---- ragged and tiny slices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stencil", ["3-point", "27-offset"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_ragged_and_tiny_slices(pkg, orc, ctx, n, stencil, dtype):
    """the `min((b + 1) * 256, n_rows)` row ends of the per-slice kernels (k_up_slice_pattern, k_up_slice_desc, k_up_wide_desc, k_up_stats)
    with a last slice of 1, 63, 64, 65 and 255 rows and with exactly one full slice"""
    offsets = [-1, 0, 1] if stencil == "3-point" else sorted(a + 7 * b + 49 * c for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    present = [(q, o) for q, o in enumerate(offsets) if abs(o) < n]
    S = sp.diags([np.full(n - abs(o), (q + 1) / 32.0) for q, o in present], [o for _, o in present], shape=(n, n), format="csc")
    square_csc(pkg, orc, S, dtype, 91)
