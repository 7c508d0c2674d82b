"""The four launch helpers of csrc/mik_kernels.h (launch_map, launch_map2, launch_map_pro, launch_map_with) in their 16-byte AND their
element-wise instances, and both callers of every shared scalar statement of csrc/mik_solvers.hip (the consumer-side Pro* functor of
k_map_with, the Fin* functor of a finaliser launch), bit for bit against the oracle's TREE mode.  GPU box only (-m gpu).

Sizes, from the segment the context reports (SEG = 256 * W * L: 1024 fp64 / 2048 fp32 elements):

    one_element      n = 1                          one lane, one element
    second_group     n = 256 * W + 1                the second 16-byte group of the segment holds a single element
    three_segments   n = 2 * SEG + SEG / 2 + 3      the last segment partial and no multiple of W
    two_passes       n = 256 * SEG + SEG / 2 + 3    planned for 8 compute units (development knob MIK_KNOB_MACHINE, grid cap 256, as
                                                    tests/test_gpu_large_reductions.py): two grid-stride passes, the second ragged

Every case runs with 16-byte aligned operands and with every vector the test can place ONE ELEMENT into its allocation (the kernels then
run their VEC = false instances):

    launch_map       axpy_dot_                                   x, y, z shifted
    launch_map2      two cg! steps with a JacobiPrec             x, b, u, r, c and the diagonal shifted: k_map2<., false, OpPcgUpdateR>
    launch_map_pro   orthogonalize_and_normalize_, Modified      w shifted and V a list of shifted vectors (the vector-of-vectors method):
                     Gram-Schmidt, k = 3, MIK_KNOB_GS = 2        k_map_pro<., false, OpMgsPass / OpScal, .>
    launch_map_with  one bicgstabl(2) outer iteration,           x, b and r_shadow shifted.  BiCGStab's blocks rs / us are allocated by the
                     three minres iterations, orc.laplace(n, 1)  iterable itself (16-byte aligned), but its block sweeps update x as well, so
                                                                 a shifted x runs k_map_with<., false, OpBicgU / OpBicgR, .>.  MINRES
                                                                 allocates its Lanczos vectors itself and its orthogonalisation sweep touches
                                                                 nothing else: k_map_with<., false, OpAxpyDot, ProMinresProj> cannot be
                                                                 reached through the Python mirror (the shifted x reaches the tail sweep,
                                                                 k_map<., false, OpMinresUpdate>).

The two solvers run once more under MIK_KNOB_SOLVER_FORM = 1 (separate finaliser launches at every size): the same statements through
k_fin / k_fin_spread instead of k_map_with, compared with the same oracle run wherever the handle reports the same dot shape.

Degenerate sizes are compared as they come: where the oracle stops early or raises (n = 1), the device must do the same."""
import numpy as np
import pytest

from conftest import KN

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SIZES = ["one_element", "second_group", "three_segments", "two_passes"]
OFFS = [0, 1]
SMALL_MACHINE = 8 | (1 << 16)           # compute units | XCDs << 16: sweep_grid_cap = 256
_POOL = {}


def size_of(ctx, dtype, size):
    """(machine plan, n)"""
    W, L = ctx.reduce_shape(dtype)
    SEG = 256 * W * L
    n = {"one_element": 1, "second_group": 256 * W + 1, "three_segments": 2 * SEG + SEG // 2 + 3, "two_passes": 256 * SEG + SEG // 2 + 3}[size]
    if size == "two_passes":
        ctx.set_tuning(KN.MACHINE, SMALL_MACHINE)
        try:
            assert ctx.info()["sweep_grid_cap"] == 256 < (n + SEG - 1) // SEG <= 1024
        finally:
            ctx.set_tuning(KN.MACHINE, 0)
        return SMALL_MACHINE, n
    assert n % SEG % W != 0
    return 0, n


def pool(ctx, dtype, j, n):
    """vector j (0..4) of a fixed pseudo-random pool, generated once per dtype at the largest size"""
    dtype = np.dtype(dtype).type
    if dtype not in _POOL:
        top = size_of(ctx, dtype, "two_passes")[1]
        rng = np.random.default_rng(91)
        _POOL[dtype] = [rng.standard_normal(top, dtype=dtype) for _ in range(5)]
    return _POOL[dtype][j][:n]


def dev(pkg, a, off):
    """a on the device, `off` elements into its allocation"""
    if off == 0:
        return pkg.HipVector.from_numpy(a)
    big = np.full(a.size + off, 7.25, a.dtype)
    big[off:] = a
    return pkg.HipVector.from_numpy(big).view(off, a.size)


def outcome(fn):
    try:
        return fn()
    except np.linalg.LinAlgError:
        return "LinAlgError"


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_launch_map_axpy_dot(pkg, orc, ctx, size, dtype, off):
    W, L = ctx.reduce_shape(dtype)
    plan, n = size_of(ctx, dtype, size)
    x, y, z = (pool(ctx, dtype, j, n) for j in range(3))
    alpha = dtype(-0.7321)
    dx, dy, dz = dev(pkg, x, off), dev(pkg, y, off), dev(pkg, z, off)
    ctx.set_tuning(KN.MACHINE, plan)
    got = pkg.axpy_dot_(alpha, dx, dy, dz)
    ctx.set_tuning(KN.MACHINE, 0)
    y1 = y + alpha * x
    assert np.array_equal(dy.to_numpy(), y1) and got == dtype(orc.dot(z, y1, "tree", W, L))


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_launch_map2_pcg_tail(pkg, orc, ctx, size, dtype, off):
    """|r|^2 and dot(c, r) in one sweep (OpPcgUpdateR): two cg! steps on a diagonal operator with a diagonal Pl"""
    plan, n = size_of(ctx, dtype, size)
    a = np.abs(pool(ctx, dtype, 0, n)) + dtype(1)
    d = np.abs(pool(ctx, dtype, 1, n)) + dtype(1)
    b = pool(ctx, dtype, 2, n)
    ptr, idx = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64)
    dA = pkg.HipCSR(n, n, ptr, idx, a, index_base=0)
    zero = np.zeros(n, dtype)
    x = dev(pkg, zero, off)
    state = pkg.CGStateVariables(dev(pkg, zero, off), dev(pkg, zero, off), dev(pkg, zero, off))
    ctx.set_tuning(KN.MACHINE, plan)
    x, ch = pkg.cg_(x, dA, dev(pkg, b, off), Pl=pkg.JacobiPrec(dev(pkg, d, off)), statevars=state, initially_zero=True, maxiter=2, reltol=0.0, log=True)
    ctx.set_tuning(KN.MACHINE, 0)
    xo, ho = orc.cg(orc.CSC(n, ptr, idx, a, 0), b, maxiter=2, reltol=0.0, jacobi_diag=d, mode="tree", shape=ctx.cg_shape(dtype))
    assert ch.iters == ho["iters"] and (n == 1 or ch.iters == 2)
    assert np.array_equal(ch["resnorm"], np.asarray(ho["resnorm"], dtype=np.float64), equal_nan=True) and np.array_equal(x.to_numpy(), xo, equal_nan=True)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", SIZES)
def test_launch_map_pro_lean_gram_schmidt(pkg, orc, ctx, size, dtype, off):
    """every pass finalises the previous pass's reduction itself (k_map_pro, PRO = 1), the normalisation the last one's (PRO = 2)"""
    W, L = ctx.reduce_shape(dtype)
    plan, n = size_of(ctx, dtype, size)
    V = np.empty((n, 3), dtype, order="F")
    for j in range(3):
        V[:, j] = pool(ctx, dtype, 1 + j, n) * dtype(1 / np.sqrt(n))
    w0 = pool(ctx, dtype, 0, n)
    dV = pkg.HipMatrix.from_numpy(V) if off == 0 else [dev(pkg, np.ascontiguousarray(V[:, j]), off) for j in range(3)]
    dw = dev(pkg, w0, off)
    h = np.zeros(3, dtype)
    ctx.set_tuning(KN.MACHINE, plan)
    ctx.set_tuning(KN.GS, 2)
    nrm = pkg.orthogonalize_and_normalize_(dV, 3, dw, h, pkg.ModifiedGramSchmidt())
    ctx.set_tuning(KN.GS, 0)
    ctx.set_tuning(KN.MACHINE, 0)
    wo, ho, no = orc.orthogonalize(V, w0, method="mgs", mode="tree", W=W, L=L)
    assert np.array_equal(np.array([nrm]), np.array([no]), equal_nan=True) and np.array_equal(h, ho, equal_nan=True)
    assert np.array_equal(dw.to_numpy(), wo, equal_nan=True)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("solver", ["bicgstab2", "minres"])
@pytest.mark.parametrize("size", SIZES)
def test_launch_map_with_and_the_finaliser_launches(pkg, orc, ctx, size, solver, dtype, off):
    """form 0: the block sweeps / the orthogonalisation sweep form beta, alpha, proj themselves (k_map_with, Pro*); form 1: k_fin /
    k_fin_spread store them first (Fin*) -- one outer iteration of bicgstabl(2), three iterations of minres, against the oracle"""
    plan, n = size_of(ctx, dtype, size)
    A = orc.laplace(n, 1).astype(dtype)
    b = orc.hashed_rhs(n).astype(dtype)
    sh = (orc.hashed_rhs(n) + 0.5).astype(dtype)
    shape = ctx.reduce_shape(dtype)
    want = {}
    for form in (0, 1):
        ctx.set_tuning(KN.MACHINE, plan)
        ctx.set_tuning(KN.SOLVER_FORM, form)
        try:
            dA = pkg.HipCSR(n, n, A.colptr, A.rowval, A.nzval, index_base=A.index_base)
            x = dev(pkg, np.zeros(n, dtype), off)
            if solver == "bicgstab2":
                it = pkg.bicgstabl_iterator_(x, dA, dev(pkg, b, off), 2, max_mv_products=4, reltol=0.0, initial_zero=True, r_shadow=dev(pkg, sh, off))
                key = it.dot_shape()
                ref = lambda: orc.bicgstabl(A, b, 2, None, r_shadow=sh, max_mv_products=4, reltol=0.0, mode="tree", shape=shape, dot_shape=key)
            else:
                it = pkg.minres_iterable_(x, dA, dev(pkg, b, off), initially_zero=True, maxiter=3, reltol=0.0)
                key = it.proj_shape()
                ref = lambda: orc.minres(A, b, maxiter=3, reltol=0.0, mode="tree", shape=shape, proj_shape=key)
            got = outcome(lambda: np.array(list(it)))
            xs = x.to_numpy()
        finally:
            ctx.set_tuning(KN.SOLVER_FORM, 0)
            ctx.set_tuning(KN.MACHINE, 0)
        if key not in want:
            want[key] = outcome(ref)
        if isinstance(want[key], str):
            assert isinstance(got, str) and got == want[key], (form, got)
            continue
        xo, ho = want[key]
        assert not isinstance(got, str), (form, got)
        assert n == 1 or got.size == (1 if solver == "bicgstab2" else 3)
        assert np.array_equal(got, ho["resnorm"], equal_nan=True), (form, got, ho["resnorm"])
        assert np.array_equal(xs, xo, equal_nan=True), form
