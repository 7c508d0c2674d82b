"""lobpcg for ComplexF64 / ComplexF32 on the device: the complex instances of mik_spmm, mik_block_gram, mik_block_rdiv
and mik_block_update against the vector entries and the C checker (tests/complex_ref/complex_block_ref.c) bit for bit, and the driver against
the complex double (tests/complex_lobpcg_host.py) bit for bit and against the known spectrum.  Every comparison is np.array_equal."""
import ctypes as C
from contextlib import contextmanager
from importlib import import_module

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import complex_lobpcg_host as ch
from complex_host import real_of
from complex_lobpcg_host import CTYPES, bref, cref  # noqa: F401  (fixtures)
from conftest import KN
from lobpcg_gpu_util import Blk, code, dots, gram_raw, same_trace, update_raw

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
SENTINEL = complex(-7.5, 3.25)
SMALL_MACHINE = 8 | (1 << 16)           # compute units | XCDs << 16: sweep_grid_cap = 256, 64 resident row blocks for k_cspmm
# constants of csrc/mik_lobpcg_complex.h the cases below are chosen around
SPMM_CB = 4                                       # MIK_CSPMM_CB: the widest column block of k_cspmm; instances 1, 2, 4
RDIV_PW = 8                                       # CBlk<R>::RDIV_PW: columns of a panel of k_cblock_rdiv; factor tiles of 4, 8, 16, 32
UPD_LB = {np.complex128: 8, np.complex64: 16}     # CBlk<R>::UPD_LB: output columns of a panel of k_cblock_update; instances 4, 8 (, 16)
STAGE_PINNED = 8192                               # mik_ctx::COEF_BYTES: mik_stage_small goes through the pinned area up to this size


@contextmanager
def small_machine(ctx):
    ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
    try:
        assert ctx.info()["sweep_grid_cap"] == 256
        yield
    finally:
        ctx.set_tuning(KN.MACHINE, 0)


def nan_of(T):
    return np.dtype(T).type(complex(np.nan, np.nan))


def padding_is(B, fill):
    p = B.padding()
    return np.array_equal(p, np.full(p.shape, fill, p.dtype), equal_nan=True)


# ---- mik_spmm -----------------------------------------------------------------------------------------------------------------------
def spmm_raw(pkg, ctx, A, b, X, Y):
    rc = pkg.lib().mik_spmm(ctx.handle, A.handle, b, _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld)
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)


@pytest.mark.parametrize("T", CTYPES)
def test_spmm_equals_spmv_column_by_column_and_the_checker(pkg, ctx, cref, bref, T):
    """b covers every CB instance (1, 2, 4), several column blocks (5 .. 32), a ragged last column block (3) and a one-column last block
    (5, 9, 17); the padding of X and Y is NaN and must survive; offset: the block starts one element (8 bytes for ComplexF32) past a
    16-byte boundary"""
    long_row = ctx.spmv_long_row()
    assert SPMM_CB == 4 and ch.CSPMM_TILE == 1024
    ops = [("ragged", ch.spmm_ragged(T)), ("holes", ch.spmm_holes(T)), ("rect", ch.spmm_rect(T)), ("long row", ch.spmm_long(T, long_row))]
    rng = np.random.default_rng(1)
    for name, S in ops:
        A = ch.device_csr(pkg, ctx, S)
        assert A.spmv_kernel().startswith("k_spmv_complex") and ("long" in A.spmv_kernel()) == (name == "long row")
        Ah = ch.operator(cref, S)
        widths = (1, 2, 3, 4, 5, 8, 9, 17, 32) if name == "ragged" else (3, 9)
        Xfull = ch.cwide(rng, (S.shape[1], 32), T)
        want_all = bref.spmm(Ah, Xfull, 32, long_row=long_row, segment=ctx.spmv_long_segment(), group=ctx.spmv_long_group())
        for b in widths:
            for offset in (False, True):
                X = Blk(pkg, ctx, Xfull[:, :b], offset, fill=nan_of(T))
                Y = Blk(pkg, ctx, np.full((S.shape[0], b), SENTINEL, T), offset, fill=nan_of(T))
                spmm_raw(pkg, ctx, A, b, X, Y)
                got = Y.get()
                by_spmv = np.stack([pkg.mul_(pkg.HipVector(S.shape[0], T, ctx), A, X.col(j)).to_numpy() for j in range(b)], axis=1)
                assert np.array_equal(got, by_spmv), (name, b, offset, "mik_spmv")
                assert np.array_equal(got, want_all[:, :b]), (name, b, offset, "checker")
                assert padding_is(Y, nan_of(T)) and padding_is(X, nan_of(T)), (name, b, offset, "padding")


@pytest.mark.parametrize("T", CTYPES)
def test_spmm_over_several_row_block_passes(pkg, ctx, cref, bref, T):
    """planned for 8 compute units the grid holds 64 row blocks: 150 blocks take three passes, the last one ragged"""
    rng = np.random.default_rng(2)
    n = 150 * ch.ROW_BLOCK - 7
    S = ch._csr_from_lengths(rng, rng.integers(0, 5, size=n), n, T)
    A = ch.device_csr(pkg, ctx, S)
    Xh = ch.cwide(rng, (n, 5), T)
    X, Y = Blk(pkg, ctx, Xh, False), Blk(pkg, ctx, np.full((n, 5), SENTINEL, T), False)
    with small_machine(ctx):
        spmm_raw(pkg, ctx, A, 5, X, Y)
    assert np.array_equal(Y.get(), bref.spmm(ch.operator(cref, S), Xh, 5))


def test_spmm_refusals_hold_for_a_complex_operator(pkg, ctx):
    T = np.complex128
    A = ch.device_csr(pkg, ctx, ch.spmm_rect(T))
    X, Y = pkg.HipMatrix(500, 40, T, ctx), pkg.HipMatrix(500, 40, T, ctx)
    L = pkg.lib()
    assert L.mik_spmm(ctx.handle, A.handle, 33, _vp(X.buf.ptr), X.ld, _vp(Y.buf.ptr), Y.ld) == 5
    assert L.mik_spmm(ctx.handle, A.handle, 4, _vp(X.buf.ptr), X.ld, _vp(X.col(3).ptr), X.ld) == 1           # Y overlaps X
    assert L.mik_spmm(ctx.handle, A.handle, 4, _vp(X.buf.ptr), 499, _vp(Y.buf.ptr), Y.ld) == 1               # ldx < columns of A


# ---- mik_block_gram -----------------------------------------------------------------------------------------------------------------
def check_gram(pkg, ctx, bref, Xh, Yh, p, q, offset, what, shape):
    X, Y = Blk(pkg, ctx, Xh[:, :p], offset), Blk(pkg, ctx, Yh[:, :q], offset)
    G = gram_raw(pkg, ctx, X, p, Y, q)
    assert np.array_equal(G, dots(pkg, X, p, Y, q)), (what, "mik_dot")
    assert np.array_equal(G, bref.gram(Xh[:, :p], Yh[:, :q], shape)), (what, "checker")
    return X


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_block_gram_equals_dot_pair_by_pair_and_the_checker(pkg, ctx, bref, T, n):
    rng = np.random.default_rng(n)
    shape = ctx.reduce_shape(T)
    Xh, Yh = ch.cwide(rng, (n, 32), T), ch.cwide(rng, (n, 32), T)
    for (p, q) in [(1, 1), (4, 4), (5, 3), (32, 32)]:
        for offset in (False, True):                                    # aligned; one element off with an odd leading dimension
            X = check_gram(pkg, ctx, bref, Xh, Yh, p, q, offset, (n, p, q, offset), shape)
            if (p, q) == (4, 4):
                G = gram_raw(pkg, ctx, X, 4, X, 4, ldg=7, fill=SENTINEL)                  # X == Y, a padded ldg
                assert np.array_equal(G[:4], dots(pkg, X, 4, X, 4)) and np.all(G[4:] == SENTINEL), (n, "X == Y", offset)


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("m", [1024, 1025])
def test_block_gram_on_each_side_of_the_level2_switch(pkg, ctx, bref, T, m):
    """m segments over the 2 n reals: n = 524288 | 524289 for ComplexF64, 1048576 | 1048577 for ComplexF32"""
    W, Lr = ctx.reduce_shape(T)
    seg = 256 * W * Lr
    n = 1024 * seg + (m - 1024)
    assert -(-n // seg) == m and n == {np.complex128: 524288, np.complex64: 1048576}[T] + (m - 1024)
    rng = np.random.default_rng(m)
    Xh, Yh = ch.cwide(rng, (n, 2), T), ch.cwide(rng, (n, 2), T)
    check_gram(pkg, ctx, bref, Xh, Yh, 2, 2, False, (m, n), (W, Lr))


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_block_gram_over_several_grid_passes(pkg, ctx, bref, T, which):
    """planned for cap = 256 the segment loop runs 2 and 3 times, the last pass with 1 / 37 workgroups; the reference with the plan back at 0"""
    W, Lr = ctx.reduce_shape(T)
    seg = 256 * W * Lr
    m = (2 * 256 + 1, 2 * 256 + 37)[which]
    n = (m - 1) * seg + 5
    rng = np.random.default_rng(50 + which)
    Xh, Yh = ch.cwide(rng, (n, 5), T), ch.cwide(rng, (n, 3), T)
    for offset in (False, True):
        X, Y = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Yh, offset)
        with small_machine(ctx):
            got = [gram_raw(pkg, ctx, X, p, Y, q) for (p, q) in [(1, 1), (5, 3)]]
        ref_dev = dots(pkg, X, 5, Y, 3)                                  # the plan is back at 0
        assert np.array_equal(ref_dev, bref.gram(Xh, Yh, (W, Lr))), (m, offset, "mik_dot against the checker")
        assert np.array_equal(got[0], ref_dev[:1, :1]) and np.array_equal(got[1], ref_dev), (m, offset)


def test_block_gram_refusals_hold_for_the_complex_codes(pkg, ctx):
    X = pkg.HipMatrix(100, 40, np.complex64, ctx)
    G = np.zeros((40, 40), np.complex64, order="F")
    L, c = pkg.lib(), code(pkg, np.complex64)
    assert L.mik_block_gram(ctx.handle, c, 100, 33, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 40) == 5
    assert L.mik_block_gram(ctx.handle, c, 100, 4, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 3) == 1
    assert L.mik_block_gram(ctx.handle, 7, 100, 4, 2, _vp(X.buf.ptr), X.ld, _vp(X.buf.ptr), X.ld, G.ctypes.data_as(_vp), 40) == 1


# ---- mik_block_rdiv -----------------------------------------------------------------------------------------------------------------
def rdiv_factor(rng, s, T):
    """off-diagonal components in 2^-3 .. 2 (|R[j, i]| < 2.83), a real diagonal in 1 .. 8 of either sign: a column grows by less than a factor
    4 per earlier column, so 32 columns of data up to 2^9 stay finite in Float32; the strict lower triangle is NaN (never read)"""
    def part():
        return rng.choice([-1.0, 1.0], size=(s, s)) * np.exp2(rng.uniform(-3, 0, size=(s, s))) * (1 + rng.random((s, s)))
    R = np.triu(part() + 1j * part(), 1)
    R = R + np.diag(rng.choice([-1.0, 1.0], size=s) * np.exp2(rng.uniform(0, 2, size=s)) * (1 + rng.random(s)))
    R[np.tril_indices(s, -1)] = complex(np.nan, np.nan)
    return R.astype(T)


def rdiv_raw(pkg, ctx, n, s, Rf, X):
    assert Rf.flags.f_contiguous
    return pkg.lib().mik_block_rdiv(ctx.handle, code(pkg, X.dt), n, s, Rf.ctypes.data_as(_vp), Rf.shape[0], _vp(X.ptr), X.ld)


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("n", [1, 255, 256, 4097])
def test_block_rdiv_equals_the_checker(pkg, ctx, bref, T, n):
    """s covers every factor tile (4, 8, 16, 32) and every panel edge of RDIV_PW = 8 columns (8 | 9, 16 | 17, 31 | 32 = a last panel of 7 and 8)"""
    assert RDIV_PW == 8
    rng = np.random.default_rng(n + 2)
    for s in (1, 3, 4, 5, 8, 9, 16, 17, 31, 32):
        Xh, R = ch.cwide(rng, (n, s), T, 8), rdiv_factor(rng, s, T)
        want = bref.rdiv(Xh, R)
        assert np.all(np.isfinite(want))
        big = np.full((40, s), nan_of(T), T, order="F")                  # R as the corner of a taller array of NaN: a padded ldr
        big[:s] = R
        for offset, Rf in ((False, np.asfortranarray(R)), (True, big)):
            X = Blk(pkg, ctx, Xh, offset, fill=SENTINEL)
            assert rdiv_raw(pkg, ctx, n, s, Rf, X) == 0, pkg.lib().mik_last_error(ctx.handle)
            assert np.array_equal(X.get(), want) and padding_is(X, SENTINEL), (n, s, offset)
    X = pkg.HipMatrix(n, 40, T, ctx)
    R = np.asfortranarray(np.eye(40, dtype=T))
    assert pkg.lib().mik_block_rdiv(ctx.handle, code(pkg, T), n, 33, R.ctypes.data_as(_vp), 40, _vp(X.buf.ptr), X.ld) == 5     # MIK_ERR_NOTIMPL


@pytest.mark.parametrize("T", CTYPES)
def test_block_rdiv_refuses_a_diagonal_that_is_not_real(pkg, ctx, T):
    rng = np.random.default_rng(5)
    Xh, R = ch.cwide(rng, (300, 5), T, 8), rdiv_factor(rng, 5, T)
    R[3, 3] = R[3, 3] + T(1e-3j)
    X = Blk(pkg, ctx, Xh, False, fill=SENTINEL)
    assert rdiv_raw(pkg, ctx, 300, 5, np.asfortranarray(R), X) == 1     # MIK_ERR_INVALID, before anything is launched
    assert "column 3" in pkg.lib().mik_last_error(ctx.handle).decode()
    assert np.array_equal(X.get(), Xh) and padding_is(X, SENTINEL)
    R[3, 3] = complex(R[3, 3].real, -0.0)                               # -0.0 i is real
    assert rdiv_raw(pkg, ctx, 300, 5, np.asfortranarray(R), X) == 0


# ---- mik_block_update ---------------------------------------------------------------------------------------------------------------
def update_case(rng, n, sx, b1, b2, T):
    return ch.cwide(rng, (n, sx), T, 8), ch.cwide(rng, (n, max(b1, 1)), T, 8), ch.cwide(rng, (n, max(b2, 1)), T, 8), ch.cwide(rng, (sx + b1 + b2, sx), T, 8)


def check_update(pkg, ctx, bref, n, sx, b1, b2, case, offset, what, tall=0):
    Xh, Rh, Ph, V = case
    xo, po = bref.update(sx, b1, b2, Xh, Rh, Ph, V)
    sentinel = np.full((n, sx), SENTINEL, Xh.dtype)
    X, R, P = Blk(pkg, ctx, Xh, offset), Blk(pkg, ctx, Rh, offset), Blk(pkg, ctx, Ph, offset)
    Xo, Po = Blk(pkg, ctx, sentinel, offset, fill=SENTINEL), Blk(pkg, ctx, sentinel, offset, fill=SENTINEL)
    Vt = np.concatenate([V, np.full((tall, sx), nan_of(Xh.dtype), Xh.dtype)]) if tall else V          # a padded ldv
    assert update_raw(pkg, ctx, n, sx, b1, b2, X, R, P, Vt, Xo, Po) == 0, pkg.lib().mik_last_error(ctx.handle)
    assert np.array_equal(Xo.get(), xo), (what, "Xout")
    assert np.array_equal(Po.get(), po if b1 else sentinel), (what, "Pout")                             # b1 == 0: Pout untouched
    assert padding_is(Xo, SENTINEL) and padding_is(Po, SENTINEL), (what, "padding")


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("n", [1, 255, 4097])
def test_block_update_equals_the_checker(pkg, ctx, bref, T, n):
    """sx covers every instance (4, 8, and 16 for ComplexF32) and every panel edge: 8 | 9, 16 | 17, 32 = 4 resp. 2 full panels"""
    assert UPD_LB[T] in (8, 16)
    rng = np.random.default_rng(n + 3)
    for (sx, b1, b2) in [(1, 0, 0), (2, 2, 0), (3, 3, 2), (5, 5, 5), (9, 4, 9), (16, 16, 16), (17, 5, 4), (32, 32, 32)]:
        case = update_case(rng, n, sx, b1, b2, T)
        for offset in (False, True):
            check_update(pkg, ctx, bref, n, sx, b1, b2, case, offset, (n, sx, b1, b2, offset), tall=3 if offset else 0)


@pytest.mark.parametrize("T", CTYPES)
def test_block_update_both_staging_paths(pkg, ctx, bref, T):
    """V below and above the 8192 bytes up to which mik_stage_small goes through the pinned area"""
    es = np.dtype(T).itemsize
    below, above = {8: (18, 18, 18), 16: (13, 13, 13)}[es], {8: (19, 19, 19), 16: (14, 14, 14)}[es]
    assert 3 * below[0] * below[0] * es <= STAGE_PINNED < 3 * above[0] * above[0] * es
    rng = np.random.default_rng(7)
    for (sx, b1, b2) in (below, above):
        check_update(pkg, ctx, bref, 700, sx, b1, b2, update_case(rng, 700, sx, b1, b2, T), False, (sx, b1, b2))


@pytest.mark.parametrize("T", CTYPES)
def test_rdiv_and_update_over_several_row_passes(pkg, ctx, bref, T):
    """planned for cap = 256 workgroups of 256 rows the row loops run 3 times, the last pass with 37 workgroups and 5 rows"""
    n = 2 * 256 * 256 + 37 * 256 + 5
    rng = np.random.default_rng(60)
    for s in (3, 17):
        Xh, R = ch.cwide(rng, (n, s), T, 8), rdiv_factor(rng, s, T)
        want = bref.rdiv(Xh, R)
        X = Blk(pkg, ctx, Xh, s == 3, fill=SENTINEL)
        with small_machine(ctx):
            assert rdiv_raw(pkg, ctx, n, s, np.asfortranarray(R), X) == 0
        assert np.array_equal(X.get(), want) and padding_is(X, SENTINEL), (n, s)
    for (sx, b1, b2) in [(3, 3, 2), (17, 5, 4)]:
        case = update_case(rng, n, sx, b1, b2, T)
        with small_machine(ctx):
            check_update(pkg, ctx, bref, n, sx, b1, b2, case, sx == 3, (n, sx, b1, b2))


def test_block_update_refusals_hold_for_the_complex_codes(pkg, ctx):
    n, T = 100, np.complex128
    rng = np.random.default_rng(4)
    M = Blk(pkg, ctx, ch.cwide(rng, (n, 40), T), False)
    O1, O2 = Blk(pkg, ctx, np.zeros((n, 40), T), False), Blk(pkg, ctx, np.zeros((n, 40), T), False)
    V = np.ones((100, 40), T)

    class At:                                                   # columns j .. of a block
        def __init__(self, B, j):
            self.ptr, self.ld, self.dt = B.col(j).ptr, B.ld, B.dt

    X, R, P = At(M, 0), At(M, 4), At(M, 8)
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, O2) == 0
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], At(M, 3), O2) == 1          # Xout overlaps X
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(M, 7)) == 1          # Pout overlaps R
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(M, 11)) == 1         # Pout overlaps P
    assert update_raw(pkg, ctx, n, 4, 4, 4, X, R, P, V[:12, :4], O1, At(O1, 2)) == 1         # the outputs overlap each other
    assert update_raw(pkg, ctx, n, 4, 0, 0, X, R, P, V[:4, :4], O1, At(M, 0)) == 0           # b1 == 0: Pout is not written
    assert update_raw(pkg, ctx, n, 4, 5, 0, X, R, P, V[:9, :4], O1, O2) == 5                 # b1 > sx
    assert update_raw(pkg, ctx, n, 33, 0, 0, X, R, P, V[:33, :33], O1, O2) == 5              # wider than 32
    assert update_raw(pkg, ctx, n, 4, 0, 2, X, R, P, V[:6, :4], O1, O2) == 1                 # P without R


# ---- the driver: device against double, bit for bit; against the known spectrum -------------------------------------------------------
_PROBLEMS = {}


def problem(pkg, N, dims, T):
    """H = D L D^H (L the real Laplacian), B = D tridiag(-1, 4, -1) D^H with the same D, so that the pencil (H, B) has the spectrum of the
    real pencil (L, tridiag); and both spectra"""
    key = (N, dims, np.dtype(T))
    if key not in _PROBLEMS:
        Lr = ch.laplace_real(pkg, N, dims)
        n = Lr.shape[0]
        Br = sp.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")
        if (N, dims) not in _PROBLEMS:
            _PROBLEMS[(N, dims)] = (np.linalg.eigvalsh(Lr.toarray()), scipy.linalg.eigh(Lr.toarray(), Br.toarray(), eigvals_only=True))
        _PROBLEMS[key] = (ch.hermitian_similar(Lr, T, 31), ch.hermitian_similar(Br, T, 31), Lr) + _PROBLEMS[(N, dims)]
    return _PROBLEMS[key]


def both(pkg, ctx, cref, bref, H, B, largest, rest, **kw):
    """(device run, run on the complex double) of one lobpcg call"""
    A, Bd = ch.device_csr(pkg, ctx, H), (ch.device_csr(pkg, ctx, B) if B is not None else None)
    args = (A, largest) if Bd is None else (A, Bd, largest)
    rd = pkg.lobpcg(*args, *rest, log=True, rng=np.random.default_rng(5), **kw)
    rh = ch.run(pkg, cref, bref, H, B, largest, *rest, log=True, rng=np.random.default_rng(5), **kw)
    return rd, rh


def same_results(pkg, rd, rh, T):
    assert isinstance(rd.X, pkg.HipMatrix) and rd.X.dtype == np.dtype(T) and rd.lam.dtype == np.dtype(T) and rd.residual_norms.dtype == real_of(T)
    assert np.array_equal(rd.lam, rh.lam) and np.array_equal(rd.residual_norms, rh.residual_norms)
    assert np.array_equal(rd.X.to_numpy(), rh.X.to_numpy())


@pytest.mark.parametrize("T", CTYPES)
@pytest.mark.parametrize("generalized", [False, True])
@pytest.mark.parametrize("largest", [False, True])
def test_device_run_equals_the_double_and_finds_the_spectrum(pkg, ctx, cref, bref, T, generalized, largest):
    H, B, Lr, mu, mu_b = problem(pkg, 20, 2, T)
    n = H.shape[0]
    tol = import_module(pkg.__name__ + ".lobpcg").default_tolerance(T)
    X0 = ch.crand(np.random.default_rng(6), T, n, 4)
    rd, rh = both(pkg, ctx, cref, bref, H, B if generalized else None, largest, (X0,), tol=tol, maxiter=400)
    assert rd.iterations == rh.iterations and rd.iterations >= 3 and rd.converged == rh.converged
    same_trace(rd.trace, rh.trace)
    same_results(pkg, rd, rh, T)
    assert rd.converged and np.all(rd.lam.imag == 0)
    spec = mu_b if generalized else mu
    want = spec[::-1][:4] if largest else spec[:4]
    print(f"complex lobpcg {np.dtype(T).name} generalized={generalized} largest={largest}: {rd.iterations} iterations, "
          f"|lam - mu| = {np.abs(rd.lam.real - want)}, bound {tol * np.abs(mu).max():.3e}")
    assert np.all(np.abs(rd.lam.real - want) <= tol * np.abs(mu).max())


@pytest.mark.parametrize("T", CTYPES)
def test_device_run_on_the_3d_laplacian(pkg, ctx, cref, bref, T):
    H, _, Lr, mu, _ = problem(pkg, 12, 3, T)
    tol = import_module(pkg.__name__ + ".lobpcg").default_tolerance(T)
    X0 = ch.crand(np.random.default_rng(7), T, H.shape[0], 4)
    rd, rh = both(pkg, ctx, cref, bref, H, None, False, (X0,), tol=tol, maxiter=400)
    assert rd.iterations == rh.iterations and rd.converged
    same_trace(rd.trace, rh.trace)
    same_results(pkg, rd, rh, T)
    assert np.all(np.abs(rd.lam.real - mu[:4]) <= tol * np.abs(mu).max())


@pytest.mark.parametrize("T", CTYPES)
def test_device_batches_equal_the_double(pkg, ctx, cref, bref, T):
    """nev = 6 in batches of 4: the shrinking last batch, the constraint's update, complex random refills"""
    H, B, Lr, mu, mu_b = problem(pkg, 20, 2, T)
    tol = import_module(pkg.__name__ + ".lobpcg").default_tolerance(T)
    X0 = ch.crand(np.random.default_rng(8), T, H.shape[0], 4)
    rd, rh = both(pkg, ctx, cref, bref, H, B, True, (X0, 6), tol=tol, maxiter=400)
    assert len(rd.lam) == 6 and np.array_equal(rd.iterations, rh.iterations) and len(rd.trace) == len(rh.trace)
    for ta, tb in zip(rd.trace, rh.trace):
        same_trace(ta, tb)
    same_results(pkg, rd, rh, T)
    assert np.all(rd.converged) and np.all(np.abs(np.sort(rd.lam.real) - mu_b[-6:]) <= tol * np.abs(mu).max())


@pytest.mark.parametrize("T", CTYPES)
def test_device_constrained_run_equals_the_double(pkg, ctx, cref, bref, T):
    """C = the two largest eigenvectors of H to working accuracy: the run finds the next four"""
    H, _, Lr, mu, _ = problem(pkg, 20, 2, T)
    n = H.shape[0]
    tol = import_module(pkg.__name__ + ".lobpcg").default_tolerance(T)
    w, Z = np.linalg.eigh(H.toarray().astype(np.complex128))
    Cm = Z[:, -2:].astype(T)
    X0 = ch.crand(np.random.default_rng(9), T, n, 4)
    rd, rh = both(pkg, ctx, cref, bref, H, None, True, (X0,), C=Cm, tol=tol, maxiter=400)
    assert rd.iterations == rh.iterations and rd.converged
    same_trace(rd.trace, rh.trace)
    same_results(pkg, rd, rh, T)
    assert np.all(np.abs(rd.lam.real - mu[::-1][2:6]) <= tol * np.abs(mu).max())


def test_no_device_allocation_inside_the_iteration_loop(pkg, ctx, monkeypatch):
    T = np.complex128
    H, B, Lr, mu, _ = problem(pkg, 20, 2, T)
    n = H.shape[0]
    A, Bd = ch.device_csr(pkg, ctx, H), ch.device_csr(pkg, ctx, B)
    Cm = ch.crand(np.random.default_rng(10), T, n, 2)
    L = pkg.lib()
    real = L.mik_malloc
    count = [0]

    def counting(*args):
        count[0] += 1
        return real(*args)

    monkeypatch.setattr(L, "mik_malloc", counting)
    it = pkg.LOBPCGIterator(A, Bd, False, ch.crand(np.random.default_rng(11), T, n, 4), None, None, Cm)
    seen = []
    step = it.step

    def watched(tol, log):
        seen.append(count[0])
        return step(tol, log)

    it.step = watched
    pkg.lobpcg_(it, maxiter=12, not_zeros=True)
    seen.append(count[0])
    monkeypatch.undo()
    assert count[0] > 0 and len(seen) > 5
    assert len(set(seen)) == 1, seen


def test_a_real_run_is_the_same_before_and_after_a_complex_one(pkg, ctx):
    n, cp, rv, nz = pkg.fixtures.laplace_matrix(12, 3, index_base=0)
    S = sp.csc_matrix((nz, rv, cp), shape=(n, n))
    A = pkg.HipCSR.from_scipy(S, ctx)

    def real_run():
        X0 = np.random.default_rng(12).random((n, 4))
        r = pkg.lobpcg(A, False, X0, log=True, maxiter=15, rng=np.random.default_rng(13))
        return A.spmv_kernel(), r

    k0, r0 = real_run()
    H = problem(pkg, 20, 2, np.complex64)[0]
    pkg.lobpcg(ch.device_csr(pkg, ctx, H), True, ch.crand(np.random.default_rng(14), np.complex64, H.shape[0], 4), maxiter=10)
    k1, r1 = real_run()
    assert k0 == k1 and r0.iterations == r1.iterations
    same_trace(r0.trace, r1.trace)
    assert r0.lam.dtype == np.float64 and np.array_equal(r0.lam, r1.lam) and np.array_equal(r0.X.to_numpy(), r1.X.to_numpy())
