"""The triangular sweeps of the stationary methods (csrc/mik_stationary.h) past the one-workgroup launch.  Every matrix of
tests/test_gpu_stationary.py short of its 256^3 case has no level wider than 192 rows, so each of its sweeps is ONE k_st_tri_run launch;
the operators here (tests/stationary_fixtures.py, each built to a prescribed list of level widths and asserting it) make k_st_tri_level, the
switch between the two kernels at 256 | 257 rows and plans of several launches do the work:

    edges       forward  255, 256 | 257 | 3 | 512 | 1 | 513 | 252      backward  513 | 40, 7, 1 | 300 | 256, 255 | 677           n = 2049
    stairs      forward  300 | 257 | 1 | 512 | 50, 60, 70 | 797        backward  100 | 513 | 255 | 257 | 922                     n = 2047
    hubs        forward  600 | 700 | 748                               backward  1000 | 20 | 1028; long rows inside wide levels  n = 2048
    lap24       laplace_matrix(24, 3): 70 levels, 26 wide launches between two runs, either direction                           n = 13824
    sprand4000  sprand(4000, 4000, 0.001) + 8000 I: six wide launches and a run, either direction                               n = 4000

Every comparison is np.array_equal against tests/stationary_ref/stationary_ref.c (the reference's CSC column loops), which
tests/test_stationary_host.py holds to an independent row-view restatement on these same operators.  The plan is checked first
(StationaryOperator.info() against level_widths / launch_plan of the fixtures module, which share no code with the library), so that a
wrong plan is reported as a wrong plan.

The case that launches each instance of k_st_tri_level (each also of k_st_tri_run, every fixture having runs):

    <double, double, false>   test_substitutions, Float64, omega None, forward and backward; gauss_seidel_ in test_whole_methods
    <double, double, true>    ... Float64, omega 1.2 / np.float32(0.8) / 1;                 sor_ / ssor_
    <float, float, false>     ... Float32, omega None
    <float, double, true>     ... Float32, omega 1.2 (a Float64 omega: alpha*x/d + beta*y in Float64, one rounding)
    <float, float, true>      ... Float32, omega np.float32(0.8) and 1 (an Int omega is promoted to the element type)"""
import ctypes as C

import numpy as np
import pytest

import stationary_fixtures as fx
import stationary_host as sh

pytestmark = pytest.mark.gpu
_vp = C.c_void_p
DTYPES = (np.float64, np.float32)
NAMES = list(fx.FIXTURES)
OMEGAS = (None, 1.2, np.float32(0.8), 1)
MIK_ERR_INVALID = 1


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return sh.build(tmp_path_factory.mktemp("stationary_ref_paths"))


@pytest.fixture(scope="module")
def op(pkg, ctx):
    """(M, A, S) of a fixture: uploaded and analysed once per module"""
    made = {}

    def get(name, dtype, i32=False):
        key = (name, np.dtype(dtype), i32)
        if key not in made:
            M = fx.fixture(name, dtype)
            A = fx.dev(pkg, M, i32=i32)
            made[key] = (M, A, pkg.StationaryOperator(A))
        return made[key]

    yield get
    made.clear()


def _vectors(M, seed, count):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(M.n).astype(M.dtype) for _ in range(count)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_plan_is_the_expected_one(pkg, ctx, op, name, dtype):
    M, A, S = op(name, dtype)
    assert ctx.spmv_long_row() == fx.LONG_ROW
    info = S.info()
    got = {k: info[k] for k in ("levels_forward", "levels_backward", "launches_forward", "launches_backward")}
    assert got == {"levels_forward": len(M.widths[0]), "levels_backward": len(M.widths[1]),
                   "launches_forward": len(M.plans[0]), "launches_backward": len(M.plans[1])}
    assert min(len(fx.wide_launches(p)) for p in M.plans) >= 2


@pytest.mark.parametrize("omega", OMEGAS, ids=["plain", "float", "float32", "int"])
@pytest.mark.parametrize("upper", (False, True), ids=["forward", "backward"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_substitutions(pkg, ctx, ref, op, name, dtype, upper, omega):
    """forward_sub! / backward_sub!, plain and relaxed, omega a Python float, an np.float32 and an int: with Float32 data the three scalar
    pairings of _relax_scalars"""
    M, A, S = op(name, dtype)
    ref.diag(M)
    x, y = _vectors(M, 11, 2)
    sub = S.backward_sub_ if upper else S.forward_sub_
    xd = pkg.HipVector.from_numpy(x)
    if omega is None:
        assert sub(xd) is xd
        assert np.array_equal(xd.to_numpy(), ref.sub(M, upper, x))
        return
    yd = pkg.HipVector.from_numpy(y)
    assert sub(xd, omega, yd) is xd
    want = ref.sub(M, upper, x, omega, y)
    assert np.array_equal(xd.to_numpy(), want) and np.array_equal(yd.to_numpy(), y)
    assert np.all(np.isfinite(want))


@pytest.mark.parametrize("omega,k", [(1.2, 3), (np.float32(1.2), 2), (1, 2)], ids=["float", "float32", "int"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_whole_methods(pkg, ctx, ref, op, name, dtype, omega, k):
    """jacobi! / gauss_seidel! / sor! (the returned vector and the caller's x) / ssor!"""
    M, A, _ = op(name, dtype)
    fx.check_methods(pkg, ref, M, A, omega, k, np.random.default_rng(42))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", fx.STAGED)
def test_int32_uploads(pkg, ctx, ref, op, name, dtype):
    """SparseMatrixCSC{T, Int32} on wide levels: the same plan and the same bits, methods and substitutions"""
    M, A, S = op(name, dtype, i32=True)
    info = S.info()
    assert (info["levels_forward"], info["launches_forward"], info["levels_backward"], info["launches_backward"]) == \
        (len(M.widths[0]), len(M.plans[0]), len(M.widths[1]), len(M.plans[1]))
    rng = np.random.default_rng(7)
    for omega in (1.2, np.float32(1.2), 1):
        fx.check_methods(pkg, ref, M, A, omega, 2, rng)
    ref.diag(M)
    x, y = _vectors(M, 12, 2)
    V = pkg.HipVector.from_numpy
    for upper in (False, True):
        sub = S.backward_sub_ if upper else S.forward_sub_
        assert np.array_equal(sub(V(x)).to_numpy(), ref.sub(M, upper, x)), upper
        assert np.array_equal(sub(V(x), 1.2, V(y)).to_numpy(), ref.sub(M, upper, x, 1.2, y)), upper


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_results_whatever_the_spmv_layout(pkg, ctx, ref, dtype):
    M = fx.fixture("edges", dtype)
    b, x0 = _vectors(M, 13, 2)
    out = []
    for layout in ("auto", "csr"):
        A = fx.dev(pkg, M).set_layout(layout)
        bd = pkg.HipVector.from_numpy(b)
        out.append([pkg.ssor_(pkg.HipVector.from_numpy(x0), A, bd, 1.5, maxiter=2).to_numpy(),
                    pkg.gauss_seidel_(pkg.HipVector.from_numpy(x0), A, bd, maxiter=2).to_numpy(),
                    pkg.jacobi_(pkg.HipVector.from_numpy(x0), A, bd, maxiter=2).to_numpy()])
    want = [ref.ssor(M, b, x0, 1.5, 2)[0], ref.gauss_seidel(M, b, x0, 2)[0], ref.jacobi(M, b, x0, 2)[0]]
    for a, c, w in zip(out[0], out[1], want):
        assert np.array_equal(a, c) and np.array_equal(a, w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_row_parallel_kernels(pkg, ctx, ref, op, name, dtype):
    """ldiv! (also y === x), mul! on OffDiagonal (beta 0, 1, other), both gauss_seidel_multiply! forms (z === x and not): n on either side
    of a multiple of 256, rows with an empty strict triangle, diagonals stored first and last in their row"""
    M, A, S = op(name, dtype)
    ref.diag(M)
    x, y, b = _vectors(M, 5, 3)
    V = pkg.HipVector.from_numpy
    assert np.array_equal(S.diag_ldiv_(V(np.zeros(M.n, dtype)), V(x)).to_numpy(), ref.ldiv(M, x))
    xv = V(x)
    assert np.array_equal(S.diag_ldiv_(xv, xv).to_numpy(), ref.ldiv(M, x))
    for a, be in ((1.0, 0.0), (1.0, 1.0), (2.0, 3.0), (-1.0, 1.0), (-0.75, -1.5)):
        xv = V(x)
        assert np.array_equal(S.offdiag_mul_(a, xv, be, V(y)).to_numpy(), ref.offdiag_mul(M, a, x, be, y)), (a, be)
        assert np.array_equal(xv.to_numpy(), x)
    nan = np.full(M.n, np.nan, dtype)                                       # beta == 0 is fill!: what y held does not matter
    assert np.array_equal(S.offdiag_mul_(1.5, V(x), 0.0, V(nan)).to_numpy(), ref.offdiag_mul(M, 1.5, x, 0.0, y))
    for upper in (True, False):
        xv = V(x)
        assert np.array_equal(S.gs_multiply_(upper, -1.0, xv, 1.0, V(b), xv).to_numpy(), ref.gs_mul(M, upper, -1.0, x, 1.0, b)), upper   # z === x
        xv = V(x)
        assert np.array_equal(S.gs_multiply_(upper, 2.0, xv, 3.0, V(b), V(y)).to_numpy(), ref.gs_mul(M, upper, 2.0, x, 3.0, b, y)), upper
        assert np.array_equal(xv.to_numpy(), x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_x_untouched(pkg, ctx, ref, op, dtype):
    """mik_forward_sub / mik_backward_sub with y aliasing x, mik_offdiag_mul with x aliasing y, and the relaxed form without alpha, without
    beta or with a scalar_dtype that is neither MIK_F64 nor MIK_F32: MIK_ERR_INVALID, and nothing is launched"""
    M, A, S = op("edges", dtype)
    L = pkg.lib()
    x, y = _vectors(M, 9, 2)
    xd, yd = pkg.HipVector.from_numpy(x), pkg.HipVector.from_numpy(y)
    one = np.ones(1, dtype)
    p1 = one.ctypes.data_as(_vp)
    code = pkg._lib.dtype_code(dtype)
    for fn in (L.mik_forward_sub, L.mik_backward_sub):
        assert fn(S.handle, p1, _vp(xd.ptr), p1, _vp(xd.ptr), code) == MIK_ERR_INVALID                 # y === x
        assert b"alias" in L.mik_last_error(ctx.handle)
        assert fn(S.handle, None, _vp(xd.ptr), p1, _vp(yd.ptr), code) == MIK_ERR_INVALID               # no alpha
        assert fn(S.handle, p1, _vp(xd.ptr), None, _vp(yd.ptr), code) == MIK_ERR_INVALID               # no beta
        for bad in (2, -1, 7):
            assert fn(S.handle, p1, _vp(xd.ptr), p1, _vp(yd.ptr), bad) == MIK_ERR_INVALID              # scalar_dtype
        assert fn(S.handle, p1, None, p1, _vp(yd.ptr), code) == MIK_ERR_INVALID                        # no x
    assert L.mik_offdiag_mul(S.handle, p1, _vp(xd.ptr), p1, _vp(xd.ptr)) == MIK_ERR_INVALID            # x === y
    assert b"alias" in L.mik_last_error(ctx.handle)
    for sub in (S.forward_sub_, S.backward_sub_):                                                      # and through the Python mirror
        with pytest.raises(pkg.MikError) as ei:
            sub(xd, 1.2, xd)
        assert ei.value.code == MIK_ERR_INVALID
    with pytest.raises(pkg.MikError) as ei:
        S.offdiag_mul_(1.0, xd, 1.0, xd)
    assert ei.value.code == MIK_ERR_INVALID
    ctx.synchronize()
    assert np.array_equal(xd.to_numpy(), x) and np.array_equal(yd.to_numpy(), y)
    # the handle still works, and the plain form (y == NULL) needs neither alpha nor beta
    assert L.mik_forward_sub(S.handle, None, _vp(xd.ptr), None, None, code) == 0
    ref.diag(M)
    assert np.array_equal(xd.to_numpy(), ref.sub(M, False, x))
