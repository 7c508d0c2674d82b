"""cholesky(A) / cholesky_(A) / ldiv_ where test_gpu_dense_chol.py's matrices never go: every width of a last panel, a failing column in
every wave of the diagonal block, subnormal and near-overflow magnitudes, poisoned imaginary parts of the diagonal, poisoned upper
triangle and padding, leading dimensions that are no multiple of 64, Inf / NaN / -0.0 in the right-hand side, one handle solving
several right-hand sides, and the library's own callback held to the Python route.  Every comparison with the checker
(tests/dense_ref/dense_chol_ref.c) is dense_chol_host.same_bits: no tolerance anywhere.  Every fixture that exists for a condition comes
from a dense_chol_host.*_case function, which first asserts that condition on the checker; every W, R, T comes from F.plan()."""
import ctypes as C

import numpy as np
import pytest

import dense_chol_host as ch

pytestmark = pytest.mark.gpu

DTYPES = ch.DTYPES
COMPLEX = [d for d in DTYPES if ch.is_complex(d)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ch.build(tmp_path_factory.mktemp("dense_chol_ref_gpu_edges"))


@pytest.fixture(scope="module")
def shapes(pkg, ctx):
    """per element type (W, R, T): panel width, rows per workgroup of the panel kernel, the larger tile edge of the trailing update"""
    out = {}
    for dtype in DTYPES:
        p = pkg.cholesky(pkg.HipMatrix.from_numpy(np.ones((1, 1), dtype))).plan()
        assert p["W"] >= 4 and p["W"] % 4 == 0 and p["R"] >= 2 and p["tile_rows"] >= 2 and p["tile_cols"] >= 2
        out[np.dtype(dtype).name] = (p["W"], p["R"], max(p["tile_rows"], p["tile_cols"]))
    return out


def shape_of(shapes, dtype):
    return shapes[np.dtype(dtype).name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def solve_all_forms(pkg, F, b, want, tag):
    """ldiv_(y, x), ldiv_(x) and solve(b) against the checker's solution; x is untouched in the two-argument form"""
    n, dtype = b.size, b.dtype
    x, y = pkg.HipVector.from_numpy(b), pkg.HipVector(n, dtype).fill_(7)
    assert F.ldiv_(y, x) is y
    got = y.to_numpy()
    assert ch.same_bits(got, want), (tag, "ldiv_(y, x) differs first at", ch.first_difference(got, want))
    assert ch.same_bits(x.to_numpy(), b), (tag, "x was modified")
    assert F.ldiv_(x) is x and ch.same_bits(x.to_numpy(), want), (tag, "ldiv_(x) differs first at", ch.first_difference(x.to_numpy(), want))
    s = F.solve(pkg.HipVector.from_numpy(b)).to_numpy()
    assert ch.same_bits(s, want), (tag, "solve differs first at", ch.first_difference(s, want))


# ---- 1. every width of a last panel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("half", ["n <= W", "n > W"])
def test_every_width_of_the_last_panel(pkg, ctx, ref, shapes, dtype, half):
    """The last panel 1 .. W columns wide, alone and behind a full panel, and behind two: the diagonal block's w < W, the forward panel's
    batches of 16 with their mask, the backward panel's chunks of 32 with their count -- none of which the plan reports, so every width
    is visited."""
    W = shape_of(shapes, dtype)[0]
    sizes = [n for n in ch.width_sizes(W) if (n > W) == (half == "n > W")]
    assert len(sizes) >= W
    for n in sizes:
        A = ch.hpd(n, dtype)
        out, info = ref.factor(A)
        assert info == 0 and np.isfinite(out).all()
        F = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
        assert F.info == 0 and F.plan()["launches_factor"] == ch.plan_launches(n, W), n
        got = F.factors.to_numpy()
        assert ch.same_bits(got, out), f"factor differs, n = {n}, {np.dtype(dtype)}, first at {ch.first_difference(got, out)}"
        iu = np.triu_indices(n, 1)
        assert ch.same_bits(got[iu], A[iu]), f"the strict upper triangle was written, n = {n}, {np.dtype(dtype)}"
        b = ch.vector(n, dtype)
        want = ref.solve(out, b)
        assert np.isfinite(want).all()
        x, y = pkg.HipVector.from_numpy(b), pkg.HipVector(n, dtype).fill_(7)
        F.ldiv_(y, x)
        h = y.to_numpy()
        assert ch.same_bits(h, want), f"ldiv_(y, x) differs, n = {n}, {np.dtype(dtype)}, first at {ch.first_difference(h, want)}"
        F.ldiv_(x)
        h = x.to_numpy()
        assert ch.same_bits(h, want), f"ldiv_(x) differs, n = {n}, {np.dtype(dtype)}, first at {ch.first_difference(h, want)}"


# ---- 2. a failing column in every wave of the diagonal block ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_failure_reported_from_every_position_in_a_panel(pkg, ctx, ref, shapes, dtype):
    """failure_columns sits at position 0 (mod 4) of its panels only; these columns sit at 1, 2 and 3, in the first panel and in a later
    one, each with a later failing column that must not be the one reported."""
    L, lib = pkg.lib(), pkg._lib
    n, W = 130, shape_of(shapes, dtype)[0]
    for k in ch.report_columns(n, W):
        A, out, info = ch.failing_case(ref, n, dtype, k, "negative")
        assert info == k + 1
        for factor in (pkg.cholesky, pkg.cholesky_):
            with pytest.raises(np.linalg.LinAlgError) as ei:
                factor(pkg.HipMatrix.from_numpy(A))
            assert isinstance(ei.value, pkg.PosDefException) and ei.value.k == k + 1, (k, factor.__name__, ei.value.k)
        F = pkg.cholesky(pkg.HipMatrix.from_numpy(A), check=False)
        assert F.info == k + 1 and F.plan()["info"] == k + 1 and not F.issuccess(), (k, F.info)
        got = F.factors.to_numpy()
        assert ch.same_bits(ch.lower(got)[:, :k], ch.lower(out)[:, :k]), (k, ch.first_difference(ch.lower(got)[:, :k], ch.lower(out)[:, :k]))
        h, col = C.c_void_p(), C.c_int64()
        D = pkg.HipMatrix.from_numpy(A)
        assert L.mik_dense_chol_create(ctx.handle, C.c_void_p(D.buf.ptr), n, D.ld, lib.dtype_code(np.dtype(dtype)), 1, C.byref(col), C.byref(h)) == 8, k
        assert col.value == k + 1 and not h.value, (k, col.value)


# ---- 3. scale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_subnormal_and_near_overflow_magnitudes(pkg, ctx, ref, shapes, dtype, which):
    """0: every argument of sqrt is subnormal; 1: most operands of the products and quotients are; 2: near overflow.  A flush of
    subnormals to zero, in an operand or a result, fails 0 and 1."""
    A, out, b, want = ch.scaled_case(ref, dtype, shape_of(shapes, dtype)[0], which)
    tag = (np.dtype(dtype).name, "scale", ch.scales(dtype)[which])
    F = pkg.cholesky(pkg.HipMatrix.from_numpy(A), check=False)
    assert F.info == 0, (tag, "info", F.info)
    got = F.factors.to_numpy()
    assert ch.same_bits(got, out), (tag, "factor differs first at", ch.first_difference(got, out))
    solve_all_forms(pkg, F, b, want, tag)


# ---- 4. what is never read ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", COMPLEX)
def test_imaginary_parts_of_the_diagonal_are_never_read_and_stored_as_zero(pkg, ctx, ref, shapes, dtype):
    W, R, T = shape_of(shapes, dtype)
    n = 2 * R + W + 1
    A = ch.hpd(n, dtype)
    b = ch.vector(n, dtype)
    for p in ch.poisons(dtype) + (7,):
        P, out = ch.imag_poisoned_case(ref, A, p)
        want = ref.solve(out, b)
        M = pkg.HipMatrix.from_numpy(P)
        F = pkg.cholesky_(M)
        got = M.to_numpy()
        assert F.info == 0 and ch.same_bits(ch.lower(got), ch.lower(out)), (p, ch.first_difference(ch.lower(got), ch.lower(out)))
        assert ch.same_bits(np.ascontiguousarray(np.diag(got).imag), np.zeros(n, ch.real_of(dtype))), (p, "a stored diagonal imaginary part is not +0")
        iu = np.triu_indices(n, 1)
        assert np.array_equal(bits(got[iu]), bits(P[iu])), (p, "the strict upper triangle was written")
        solve_all_forms(pkg, F, b, want, ("imag", p))
        G = pkg.cholesky(pkg.HipMatrix.from_numpy(P))                                  # ... and through the copy
        assert ch.same_bits(ch.lower(G.factors.to_numpy()), ch.lower(out)), p


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_upper_triangle_and_padding_rows(pkg, ctx, ref, shapes, dtype):
    """NaN, +Inf and the largest finite value in the strict upper triangle and in the rows [n, ld) of every column (and, in the complex
    types, in the imaginary parts of the diagonal as well): nothing of them reaches the factor or a solve, and not one bit of the upper
    triangle or the padding is written."""
    W, R, T = shape_of(shapes, dtype)
    n = 2 * R + W + 1
    A = ch.hpd(n, dtype)
    b = ch.vector(n, dtype)
    for p in ch.poisons(dtype):
        P, out = ch.poisoned_case(ref, A, p)
        if ch.is_complex(dtype):
            P, again = ch.imag_poisoned_case(ref, P, p)
            assert ch.same_bits(again, out)
        want = ref.solve(out, b)
        M = pkg.HipMatrix(n, n, dtype)
        assert M.ld > n
        host = np.full((M.ld, n), ch.poison_of(dtype, p), dtype, order="F")
        host[:n, :] = P
        M.buf.copy_from_host(host.ravel(order="F"))
        F = pkg.cholesky_(M)
        back = M.buf.to_numpy().reshape((M.ld, n), order="F")
        assert F.info == 0, (p, F.info)
        assert ch.same_bits(ch.lower(back[:n, :]), ch.lower(out)), (p, ch.first_difference(ch.lower(back[:n, :]), ch.lower(out)))
        assert ch.same_bits(np.ascontiguousarray(np.diag(back[:n, :]).imag), np.zeros(n, ch.real_of(dtype))), (p, "diagonal imaginary part")
        iu = np.triu_indices(n, 1)
        assert np.array_equal(bits(back[:n, :][iu]), bits(host[:n, :][iu])), (p, "the strict upper triangle was written")
        assert np.array_equal(bits(back[n:, :]), bits(host[n:, :])), (p, "a padding row was written")
        solve_all_forms(pkg, F, b, want, ("poison", p))


# ---- 5. any leading dimension ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_leading_dimensions_through_the_c_entry(pkg, ctx, ref, shapes, dtype):
    """The C entry takes any ld >= n: ld = n (odd: column starts aligned to the element only), n + 1, 2 n + 3.  The strict upper triangle,
    the padding rows and 64 elements before and after the matrix are poisoned; the vectors sit at odd element offsets between poisoned
    elements.  Not one bit outside the lower triangle and outside y changes."""
    L, lib = pkg.lib(), pkg._lib
    n = shape_of(shapes, dtype)[0] + 1
    A, b = ch.hpd(n, dtype), ch.vector(n, dtype)
    out, info = ref.factor(A)
    assert info == 0
    want = ref.solve(out, b)
    xo, yo = 3, (n + 9) | 1
    il = np.tril_indices(n)
    for ld in (n, n + 1, 2 * n + 3):
        for p in ch.poisons(dtype):
            poison = ch.poison_of(dtype, p)
            host = np.full(64 + ld * n + 64, poison, dtype)
            mat = host[64:64 + ld * n].reshape((ld, n), order="F")                       # a view
            mat[:n, :] = ch.poisoned(A, p)
            inside = np.zeros(host.size, bool)
            inside[64:64 + ld * n].reshape((ld, n), order="F")[il] = True
            assert np.shares_memory(mat, host) and inside.sum() == n * (n + 1) // 2
            vhost = np.full(2 * n + 40, poison, dtype)
            vhost[xo:xo + n] = b
            big, vecs = pkg.HipVector.from_numpy(host), pkg.HipVector.from_numpy(vhost)
            x, y = vecs.view(xo, n), vecs.view(yo, n)
            h, col = C.c_void_p(), C.c_int64(-1)
            assert L.mik_dense_chol_create(ctx.handle, C.c_void_p(big.view(64, ld * n).ptr), n, ld, lib.dtype_code(np.dtype(dtype)), 1, C.byref(col), C.byref(h)) == 0
            try:
                v = [C.c_int64(-1) for _ in range(8)]
                assert col.value == 0 and L.mik_dense_chol_info(h, *[C.byref(q) for q in v]) == 0
                assert L.mik_dense_chol_solve(h, C.c_void_p(y.ptr), C.c_void_p(x.ptr)) == 0
                back, vback = big.to_numpy(), vecs.to_numpy()
            finally:
                assert L.mik_dense_chol_destroy(h) == 0
            tag = (ld, p)
            assert v[7].value == 0 and v[4].value == ch.plan_launches(n, v[0].value) and v[5].value == 2 * -(-n // v[0].value), (tag, [q.value for q in v])
            got = back[64:64 + ld * n].reshape((ld, n), order="F")[:n, :]
            assert ch.same_bits(ch.lower(got), ch.lower(out)), (tag, ch.first_difference(ch.lower(got), ch.lower(out)))
            assert np.array_equal(bits(back).reshape(host.size, -1)[~inside], bits(host).reshape(host.size, -1)[~inside]), tag       # not one bit
            assert ch.same_bits(vback[yo:yo + n], want), (tag, ch.first_difference(vback[yo:yo + n], want))
            vhost[yo:yo + n] = vback[yo:yo + n]
            assert np.array_equal(bits(vback), bits(vhost)), tag                        # x and every poisoned element around both vectors


# ---- 6. Inf, NaN and -0.0 in the right-hand side ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_right_hand_side_on_finite_factors(pkg, ctx, ref, shapes, dtype):
    """+Inf, NaN and -0.0 in b.  The exact fixture's L holds exact zeros, so 0 * Inf arises -- in the checker and on the device alike.  One
    b carries its Inf in the last entry, where only the last row of the forward chain sees it, so the backward chain starts from an Inf."""
    W = shape_of(shapes, dtype)[0]
    mzero = ch.poison_of(dtype, -0.0)
    for name, A in (("exact", ch.exact(130, dtype)[0]), ("hpd", ch.hpd(2 * W + 1, dtype))):
        n = A.shape[0]
        out, info = ref.factor(A)
        assert info == 0 and np.isfinite(out).all()
        F = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
        got = F.factors.to_numpy()
        assert F.info == 0 and ch.same_bits(got, out), (name, ch.first_difference(got, out))
        rhs = {key: ch.vector(n, dtype) for key in ("inf", "nan", "some -0.0", "inf last")}
        rhs["inf"][n // 3] = np.inf
        rhs["nan"][2 * n // 3] = np.nan
        rhs["some -0.0"][::3] = mzero
        rhs["all -0.0"] = np.full(n, mzero, dtype)
        rhs["inf last"][n - 1] = np.inf
        assert np.signbit(rhs["all -0.0"].real).all() and np.signbit(rhs["some -0.0"].real[::3]).all()
        for key, b in rhs.items():
            want = ref.solve(out, b)
            if key == "inf last" and name == "exact":
                assert np.isinf(want[n - 1]) and np.isnan(want).any()                   # Inf - Inf and, with L's exact zeros, 0 * Inf
            if key in ("inf", "nan"):
                assert not np.isfinite(want).all()
            if key == "all -0.0":
                assert (want == 0).all()
            solve_all_forms(pkg, F, b, want, (name, key))


# ---- 7. the handle's workspace ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_handle_solves_one_right_hand_side_after_another(pkg, ctx, ref, shapes, dtype):
    """b1, a different b2, b1 again, with a handle of another size solving in between on the same context: nothing of an earlier solve
    is left in the handle's workspace"""
    W = shape_of(shapes, dtype)[0]
    n, m = 2 * W + 1, W + 5
    outs, Fs = {}, {}
    for k in (n, m):
        A = ch.hpd(k, dtype)
        outs[k], info = ref.factor(A)
        assert info == 0
        Fs[k] = pkg.cholesky(pkg.HipMatrix.from_numpy(A))
        assert Fs[k].ctx is ctx
    b1, b2, c = ch.vector(n, dtype, seed=3), ch.vector(n, dtype, seed=11), ch.vector(m, dtype, seed=5)
    assert not np.array_equal(b1, b2)
    w1, w2, wc = ref.solve(outs[n], b1), ref.solve(outs[n], b2), ref.solve(outs[m], c)
    assert not ch.same_bits(w1, w2)
    for step, (k, b, want) in enumerate(((n, b1, w1), (m, c, wc), (n, b2, w2), (m, c, wc), (n, b1, w1), (n, b1, w1), (n, b2, w2))):
        y = pkg.HipVector(k, dtype).fill_(7)
        Fs[k].ldiv_(y, pkg.HipVector.from_numpy(b))
        got = y.to_numpy()
        assert ch.same_bits(got, want), (step, k, ch.first_difference(got, want))
    x = pkg.HipVector.from_numpy(b2)                                                    # ... and in place after a two-argument solve
    assert ch.same_bits(Fs[n].ldiv_(x).to_numpy(), w2)


# ---- 8. the library callback is the Python route ---------------------------------------------------------------------------------------------
class PlainLdiv:
    """a preconditioner that is NOT a DenseCholesky for the library: only ldiv_(y, x), like any user type"""

    def __init__(self, F):
        self.F = F
        self.calls = 0

    def ldiv_(self, y, x=None):
        self.calls += 1
        return self.F.ldiv_(y, x)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_solvers_reach_the_factorisation_without_a_python_frame(pkg, ctx, shapes, dtype, monkeypatch):
    """G factors a matrix NEAR S, so the solvers take several iterations, each with an application of G: as Pl of cg, as Pl of gmres and
    as Pr of gmres the library's own callback gives the bits of the route through a Python ldiv_."""
    n = 2 * shape_of(shapes, dtype)[0] + 1
    rng = np.random.default_rng(99)
    M = rng.random((n, n))
    S = (M.T @ M / n + np.eye(n)).astype(dtype)
    b = rng.random(n).astype(dtype)
    G = pkg.cholesky(pkg.HipMatrix.from_numpy((S + 0.05 * np.diag(rng.random(n))).astype(dtype)))
    dS, db = pkg.HipMatrix.from_numpy(S), pkg.HipVector.from_numpy(b)
    routes = {"cg Pl": lambda P: pkg.cg(dS, db, Pl=P, maxiter=12, log=True),
              "gmres Pl": lambda P: pkg.gmres(dS, db, Pl=P, restart=8, maxiter=24, log=True),
              "gmres Pr": lambda P: pkg.gmres(dS, db, Pl=pkg.Identity(), Pr=P, restart=8, maxiter=24, log=True)}
    plain = {}
    for key, run in routes.items():
        P = PlainLdiv(G)
        x, h = run(P)
        assert P.calls > 1 and h.iters > 1, (key, P.calls, h.iters)
        plain[key] = (x.to_numpy(), np.array(h["resnorm"]), h.mvps, h.iters)
    calls = {"n": 0}
    inner = pkg.DenseCholesky.ldiv_

    def counted(self, y, x=None):
        calls["n"] += 1
        return inner(self, y, x)
    monkeypatch.setattr(pkg.DenseCholesky, "ldiv_", counted)
    for key, run in routes.items():
        x, h = run(G)
        x1, res1, mvps1, iters1 = plain[key]
        assert calls["n"] == 0, (key, calls["n"])                                       # no Python frame per ldiv!
        assert h.iters == iters1 and h.mvps == mvps1 and np.array_equal(np.array(h["resnorm"]), res1), (key, h.iters, iters1, h.mvps, mvps1)
        assert np.array_equal(x.to_numpy(), x1), key
