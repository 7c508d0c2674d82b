"""The SpMV launch plan (csrc/mik_core.hip spmv_plan, read through mik_dev_spmv_plan of include/mik_dev.h): which kernel runs, on how many
workgroups, in how many launches.  The expected plans below restate the rules of the launcher as they stood BEFORE the plan existed (the
branch chain of spmv_launch_impl), case by case -- they were written from that code, not from what the plan function returns:

  slice-constant layout   k_spmv_sdiac under MIK_KNOB_SDIA_KERNEL = 1, else k_spmv_sdiab; k_spmv_sdiab2 when the knob is 0, n is even, nothing
                          is skipped, the first row-block is even and the count is even or the range reaches the end.  Grids: slices (pairs of
                          slices for sdiab2) in twos, rounded up to a multiple of 8.  Only sdiab / sdiab2 leave a range out in one launch.
  wide slice-constant     k_spmv_sdiaw2 (grid: pairs of slices) for even n, knob != 3 and a pair-aligned range, else k_spmv_sdiaw (grid: slices)
  CSR                     k_spmv_rowgather without long rows / windows / row permutation (or MIK_KNOB_CSR_KERNEL = 2), else k_spmv_rowblock;
                          rowblock never splits; long rows: merged into the rowblock launch without the fused dot (grid + one workgroup per 4
                          virtual rows), a k_spmv_longrows launch of their own first with it, and always before rowgather
  jagged slices           k_spmv_jds, long rows lead the same launch; the fused dot inside unless long rows exist: then k_rowdot follows
A row longer than the long-row threshold is one virtual row, or one per segment when it is longer than a segment.
Every case also holds mik_spmv_kernel to the whole-launch plan and mul_ to the oracle, bit for bit."""
import collections
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import KN
from test_gpu_irregular import as_oracle_csc, banded_irregular

pytestmark = pytest.mark.gpu

INVALID, NOTIMPL = 1, 5
NO_RANGE = "SpMV over a row-block range is not available for this operator layout"
Plan = collections.namedtuple("Plan", "kernel grid launches pre_longrows post_rowdot")


def plan(pkg, A, x=None, fuse_dot=False, rows=(0, -1), skip=None):
    """mik_dev_spmv_plan: rows = (first row-block, count; < 0: all), or skip = the row-block range left out (mik_spmv_launch_outside)"""
    name, grid, launches, pre, post = C.create_string_buffer(64), C.c_int64(), C.c_int(), C.c_int(), C.c_int()
    sb, se = skip if skip else (-1, 0)
    rc = pkg.lib().mik_dev_spmv_plan(A.handle, None if x is None else C.c_void_p(x.ptr), int(fuse_dot), rows[0], rows[1], sb, se, name, 64,
                                     C.byref(grid), C.byref(launches), C.byref(pre), C.byref(post))
    pkg._lib.check(rc, "mik_dev_spmv_plan", A.ctx.handle)
    return Plan(name.value.decode(), grid.value, launches.value, pre.value, post.value)


def kernel(pkg, A, **kw):
    return plan(pkg, A, **kw).kernel


def refused(pkg, A, **kw):
    with pytest.raises(pkg.MikError) as ei:
        plan(pkg, A, **kw)
    return ei.value.code, str(ei.value)


def whole_launch_agrees(pkg, orc, dA, Ao, x=None):
    """mik_spmv_kernel is the whole-launch plan, and what runs gives the oracle's bits"""
    dtype = Ao.nzval.dtype
    assert dA.spmv_kernel() == kernel(pkg, dA)
    if x is None:
        x = np.random.default_rng(5).standard_normal(Ao.n).astype(dtype)
    y = pkg.mul_(pkg.HipVector(Ao.n, dtype), dA, pkg.HipVector.from_numpy(x)).to_numpy()
    assert np.array_equal(y, orc.spmv(Ao, x))


def upload(pkg, A):
    return pkg.HipCSR(A.n, A.n, A.colptr, A.rowval, A.nzval, index_base=A.index_base)


def virtual_rows(ctx, lens):
    seg = ctx.spmv_long_segment()
    return int(sum(1 if l <= seg else -(-l // seg) for l in lens[lens > ctx.spmv_long_row()]))


@pytest.fixture
def long_rows(orc, ctx):
    """the oracle's row sums take the wave shape of the long rows; call again after changing MIK_KNOB_LONG_SEGMENT"""
    tell = lambda: orc.set_long_row(ctx.spmv_long_row(), ctx.spmv_long_segment(), ctx.spmv_long_group())
    tell()
    yield tell
    orc.set_long_row(0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_slice_constant_layout(pkg, orc, ctx, dtype):
    L = pkg.lib()
    A = orc.laplace(12, 3).astype(dtype)                       # n = 1728: 7 row-blocks
    dA = upload(pkg, A)
    assert dA.layout() == "slice-offsets+slice-values+row-masks"
    assert plan(pkg, dA) == Plan("k_spmv_sdiab2", 8, 1, 0, 0) == plan(pkg, dA, fuse_dot=True)
    assert plan(pkg, dA, rows=(0, 7)) == plan(pkg, dA)
    assert plan(pkg, dA, rows=(0, 2)) == Plan("k_spmv_sdiab2", 8, 1, 0, 0)
    assert plan(pkg, dA, rows=(1, 1)) == Plan("k_spmv_sdiab", 8, 1, 0, 0)          # odd first block
    assert kernel(pkg, dA, rows=(2, 1)) == "k_spmv_sdiab"                          # odd count that does not reach the end
    assert kernel(pkg, dA, rows=(2, 3)) == "k_spmv_sdiab"
    assert kernel(pkg, dA, rows=(2, 5)) == "k_spmv_sdiab2"                         # odd count, reaches the end
    assert plan(pkg, dA, rows=(3, 0)).launches == 0
    assert plan(pkg, dA, skip=(2, 4)) == Plan("k_spmv_sdiab", 8, 1, 0, 0)          # 5 row-blocks around the gap, one launch
    assert plan(pkg, dA, skip=(0, 7)).launches == 0
    for bad in ((5, 3), (-1, 2)):
        code, text = refused(pkg, dA, rows=bad)
        assert code == INVALID and "SpMV row-block range out of bounds" in text
    code, text = refused(pkg, dA, skip=(4, 8))
    assert code == INVALID and "SpMV: bad interior range" in text
    whole_launch_agrees(pkg, orc, dA, A)
    for knob, want in ((1, "k_spmv_sdiac"), (2, "k_spmv_sdiab"), (3, "k_spmv_sdiab")):
        L.mik_set_tuning(KN.SDIA_KERNEL, knob)
        dK = upload(pkg, A)
        assert plan(pkg, dK) == Plan(want, 8, 1, 0, 0) == plan(pkg, dK, fuse_dot=True)
        assert plan(pkg, dK, skip=(2, 4)) == Plan(want, 8, 2 if knob == 1 else 1, 0, 0)   # the flat-load kernel skips nothing: two ranges
        assert kernel(pkg, dK, rows=(2, 5)) == want
        whole_launch_agrees(pkg, orc, dK, A)
        L.mik_set_tuning(KN.SDIA_KERNEL, 0)
    B = orc.laplace(11, 3).astype(dtype)                       # n = 1331, odd: one row per lane; 6 row-blocks
    dB = upload(pkg, B)
    assert plan(pkg, dB) == Plan("k_spmv_sdiab", 8, 1, 0, 0) == plan(pkg, dB, fuse_dot=True)
    whole_launch_agrees(pkg, orc, dB, B)
    # nothing is armed and the fused whole launch is served, but k_spmv_sdiab takes no epilogue: MINRES keeps its projection sweep
    b = pkg.HipVector.from_numpy(orc.hashed_rhs(B.n).astype(dtype))
    it = pkg.minres_iterable_(pkg.HipVector.from_numpy(np.zeros(B.n, dtype)), dB, b, initially_zero=True, maxiter=1)
    assert it.proj_shape() == ctx.reduce_shape(dtype) != ctx.spmv_dot_shape()
    it2 = pkg.minres_iterable_(pkg.HipVector.from_numpy(np.zeros(A.n, dtype)), dA, pkg.HipVector.from_numpy(orc.hashed_rhs(A.n).astype(dtype)),
                               initially_zero=True, maxiter=1)
    assert it2.proj_shape() == ctx.spmv_dot_shape()            # ... and k_spmv_sdiab2 does


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_wide_slice_constant_layout(pkg, orc, ctx, dtype):
    """the 19-diagonal banded operator of test_gpu_layouts.py"""
    L = pkg.lib()
    offs = [0] + [o for d in (1, 2, 3, 7, 50, 51, 200, 333, 900) for o in (d, -d)]
    for n, want, grid in ((3000, "k_spmv_sdiaw2", 6), (3001, "k_spmv_sdiaw", 12)):           # 12 row-blocks
        S = sp.diags([np.full(n - abs(o), 40.0 if o == 0 else -1.0 / (1 + abs(o) % 5)) for o in offs], offs, format="csc")
        A = orc.CSC.from_scipy(S).astype(dtype)
        dA = upload(pkg, A)
        assert dA.layout() == "wide-slice-values+row-masks"
        assert plan(pkg, dA) == Plan(want, grid, 1, 0, 0) == plan(pkg, dA, fuse_dot=True)
        assert plan(pkg, dA, rows=(1, 2)) == Plan("k_spmv_sdiaw", 2, 1, 0, 0)                # odd first row-block
        assert plan(pkg, dA, rows=(2, 3)) == Plan("k_spmv_sdiaw", 3, 1, 0, 0)                # odd count short of the end
        assert plan(pkg, dA, rows=(2, 4)) == (Plan("k_spmv_sdiaw2", 2, 1, 0, 0) if n == 3000 else Plan("k_spmv_sdiaw", 4, 1, 0, 0))
        assert plan(pkg, dA, skip=(4, 6)).launches == 2
        whole_launch_agrees(pkg, orc, dA, A)
        L.mik_set_tuning(KN.SDIA_KERNEL, 3)
        assert plan(pkg, dA) == Plan("k_spmv_sdiaw", 12, 1, 0, 0)
        whole_launch_agrees(pkg, orc, dA, A)
        L.mik_set_tuning(KN.SDIA_KERNEL, 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_csr_kernels(pkg, orc, ctx, dtype):
    L = pkg.lib()
    A = orc.laplace(12, 3).astype(dtype)
    L.mik_set_tuning(KN.LAYOUTS, KN.CSR_ONLY)
    dA = upload(pkg, A)
    assert dA.layout() == "csr-rowblock"
    assert plan(pkg, dA) == Plan("k_spmv_rowgather", 7, 1, 0, 0) == plan(pkg, dA, fuse_dot=True)
    assert plan(pkg, dA, rows=(1, 2)) == Plan("k_spmv_rowgather", 2, 1, 0, 0)
    assert plan(pkg, dA, skip=(2, 4)) == Plan("k_spmv_rowgather", 2, 2, 0, 0)
    whole_launch_agrees(pkg, orc, dA, A)
    L.mik_set_tuning(KN.CSR_KERNEL, 1)
    assert plan(pkg, dA) == Plan("k_spmv_rowblock", 7, 1, 0, 0) == plan(pkg, dA, fuse_dot=True) == plan(pkg, dA, rows=(0, 7))
    code, text = refused(pkg, dA, rows=(1, 2))
    assert code == NOTIMPL and NO_RANGE in text
    assert refused(pkg, dA, skip=(2, 4))[0] == NOTIMPL
    whole_launch_agrees(pkg, orc, dA, A)


def test_csr_kernels_with_long_rows(pkg, orc, ctx, long_rows):
    L = pkg.lib()
    dtype = np.float32
    n, rowptr, colidx, val = pkg.fixtures.irregular_matrix(20000, dtype, long_rows=True)      # 79 row-blocks
    nlb = (virtual_rows(ctx, np.diff(rowptr)) + 3) // 4
    assert nlb > 1
    dA = pkg.HipCSR(n, n, rowptr, colidx, val, index_base=0, is_csc=False)
    Ao = as_oracle_csc(orc, n, rowptr, colidx, val)
    assert plan(pkg, dA) == Plan("k_spmv_rowblock", 79 + nlb, 1, 0, 0)                        # long-row workgroups merged into the launch
    assert plan(pkg, dA, fuse_dot=True) == Plan("k_spmv_rowblock", 79, 2, 1, 0)               # k_spmv_longrows, then the row-blocks
    code, text = refused(pkg, dA, rows=(1, 2))
    assert code == NOTIMPL and NO_RANGE in text
    whole_launch_agrees(pkg, orc, dA, Ao)
    L.mik_set_tuning(KN.CSR_KERNEL, 2)
    assert plan(pkg, dA) == Plan("k_spmv_rowgather", 79, 2, 1, 0) == plan(pkg, dA, fuse_dot=True)
    assert refused(pkg, dA, rows=(1, 2))[0] == NOTIMPL
    whole_launch_agrees(pkg, orc, dA, Ao)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_x_windows(pkg, orc, ctx, dtype):
    """the banded irregular operator of test_gpu_irregular.py: windows of x in LDS need a 16-byte aligned x and MIK_KNOB_LAYOUTS bit 64 clear"""
    L = pkg.lib()
    n = 9000                                                   # 36 row-blocks
    rowptr, cols, val = banded_irregular(n, dtype, 700)
    dA = pkg.HipCSR(n, n, rowptr, cols, val, index_base=0, is_csc=False)
    Ao = as_oracle_csc(orc, n, rowptr, cols, val)
    x = np.random.default_rng(8).standard_normal(n + 1).astype(dtype)
    dx = pkg.HipVector.from_numpy(x)
    aligned, shifted = dx.view(0, n), dx.view(1, n)
    assert aligned.ptr % 16 == 0 and shifted.ptr % 16 != 0
    assert plan(pkg, dA, x=aligned) == Plan("k_spmv_rowblock+xwin", 36, 1, 0, 0) == plan(pkg, dA, x=aligned, fuse_dot=True) == plan(pkg, dA)
    assert plan(pkg, dA, x=shifted) == Plan("k_spmv_rowblock", 36, 1, 0, 0) == plan(pkg, dA, x=shifted, fuse_dot=True)
    assert refused(pkg, dA, rows=(1, 2))[0] == NOTIMPL
    whole_launch_agrees(pkg, orc, dA, Ao, x[:n])
    y = pkg.mul_(pkg.HipVector(n, dtype), dA, shifted).to_numpy()
    assert np.array_equal(y, orc.spmv(Ao, x[1:]))
    L.mik_set_tuning(KN.LAYOUTS, KN.XWIN_UNUSED)
    assert plan(pkg, dA, x=aligned) == Plan("k_spmv_rowblock", 36, 1, 0, 0)
    whole_launch_agrees(pkg, orc, dA, Ao, x[:n])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_jagged_slices(pkg, orc, ctx, dtype, long_rows):
    L = pkg.lib()
    n, rp, ci, vv = pkg.fixtures.fe_matrix((21, 17), 6, dtype)
    nb = -(-n // 256)
    dA = pkg.HipCSR(n, n, rp, ci, vv, index_base=0, is_csc=False)
    assert dA.layout() == "jagged-slices" and np.diff(rp).max() <= ctx.spmv_long_row()
    assert plan(pkg, dA) == Plan("k_spmv_jds", nb, 1, 0, 0) == plan(pkg, dA, fuse_dot=True)   # dot(x, y) inside the launch
    assert plan(pkg, dA, rows=(1, 2)) == Plan("k_spmv_jds", 2, 1, 0, 0)
    whole_launch_agrees(pkg, orc, dA, as_oracle_csc(orc, n, rp, ci, vv))
    # ... with a few dense rows (test_gpu_layouts.py), cut into segments of 300: their workgroups lead the launch, k_rowdot forms the dot
    S = sp.csr_matrix((vv.astype(np.float64), ci, rp), shape=(n, n)).tolil()
    rng = np.random.default_rng(12)
    for row, cnt in ((7, 300), (n // 2, 1500), (n - 3, 257)):
        cols = np.sort(rng.choice(n, size=cnt, replace=False))
        S[row, cols] = rng.standard_normal(cnt) * 0.01
        S[row, row] = 50.0
    S = ((S + S.T).tocsr() * 0.5 + sp.diags(np.full(n, 5.0))).astype(dtype).tocsr()
    S.sort_indices()
    L.mik_set_tuning(KN.LONG_SEGMENT, 300)
    long_rows()
    assert ctx.spmv_long_segment() == 300
    lens = np.diff(S.indptr)
    virt = virtual_rows(ctx, lens)
    assert virt > (lens > ctx.spmv_long_row()).sum() >= 2      # some of the long rows are cut
    dS = pkg.HipCSR(n, n, S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data, index_base=0, is_csc=False)
    assert dS.layout() == "jagged-slices"
    nlb = (virt + 3) // 4
    assert plan(pkg, dS) == Plan("k_spmv_jds", nb + nlb, 1, 0, 0)
    assert plan(pkg, dS, fuse_dot=True) == Plan("k_spmv_jds", nb + nlb, 2, 0, 1)
    assert refused(pkg, dS, rows=(1, 2))[0] == NOTIMPL
    whole_launch_agrees(pkg, orc, dS, orc.CSC.from_scipy(S.tocsc()))
