"""qr(A) / qr_(A) on a dense device matrix, lmul with Q and Q', solve, Q() and R() (iterativesolvers.jl_amd/dense_qr.py over the
mik_dense_qr_* entries), bit for bit against tests/dense_ref/dense_qr_ref.c -- the contract's unblocked loops restated in C.  Every
comparison of device values with the checker's is dense_qr_host.same_bits (NaN positions, and the bits everywhere else: -0.0 is not +0.0).
Every shape comes from mik_dense_qr_info.  The reference's own statements carry the reference's own bounds."""
import ctypes as C

import numpy as np
import pytest

import dense_qr_host as qh

pytestmark = pytest.mark.gpu

DTYPES = qh.DTYPES


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return qh.build(tmp_path_factory.mktemp("dense_qr_ref_gpu"))


@pytest.fixture(scope="module")
def W(pkg, ctx):
    info = pkg.qr(pkg.HipMatrix.from_numpy(np.ones((1, 1)))).info()
    assert info["W"] >= 4 and info["accumulators"] == qh.ACC and info["resident"] == 1 and info["resident_rows"] >= 1024 and info["launches_solve"] == 2
    return info["W"]


def shapes(W):
    acc = qh.ACC
    s = [(1, 1), (2, 1), (5, 5), (10, 6), (10, 3), (W + 3, W - 1), (W + 3, W), (W + 3, W + 1), (3 * W + 5, 2 * W + 1), (2 * W + 1, 2 * W + 1)]
    for m in (acc - 1, acc, acc + 1, 2 * acc + 1):
        s += [(m, 3), (m, W + 1)]
    return s


def check_against(pkg, ref, A, F, QR, tau, what):
    """factors, tau, lmul both ways (a vector and a block), solve, Q() and R() of the device factorisation F against the checker's"""
    m, n = A.shape
    dtype = A.dtype
    got = F.factors.to_numpy()
    assert qh.same_bits(got, QR), f"factors differ, {what}, first at {qh.first_difference(got, QR)}"
    assert F.tau.dtype == dtype and qh.same_bits(F.tau, tau), (what, qh.first_difference(F.tau, tau))
    y = qh.vector(m, dtype)
    Y = qh.block(m, 3, dtype)
    for adjoint, lmul in ((True, F.lmul_Qt_), (False, F.lmul_Q_)):
        dy = pkg.HipVector.from_numpy(y)
        assert lmul(dy) is dy
        want = ref.lmul(QR, tau, y, adjoint)
        assert qh.same_bits(dy.to_numpy(), want), (what, adjoint, qh.first_difference(dy.to_numpy(), want))
        dY = pkg.HipMatrix.from_numpy(Y)
        assert lmul(dY, cols=2) is dY
        h = dY.to_numpy()
        assert qh.same_bits(h[:, :2], ref.lmul(QR, tau, Y[:, :2], adjoint)) and np.array_equal(h[:, 2], Y[:, 2]), (what, adjoint)
    Q, R = F.Q(), F.R()
    assert (Q.n, Q.cols, R.n, R.cols) == (m, n, n, n)
    assert qh.same_bits(Q.to_numpy(), ref.thin_q(QR, tau)), (what, qh.first_difference(Q.to_numpy(), ref.thin_q(QR, tau)))
    assert qh.same_bits(R.to_numpy(), qh.upper(QR)), what
    if F.zero_diag == 0:
        db = pkg.HipVector.from_numpy(y)
        x = F.solve(db)
        want = ref.solve(QR, tau, y)
        assert x.n == n and qh.same_bits(x.to_numpy(), want), (what, qh.first_difference(x.to_numpy(), want))
        assert np.array_equal(db.to_numpy(), y)                             # b is not modified
        assert F.ldiv_(db) is db and qh.same_bits(db.to_numpy()[:n], want)  # ldiv!(F, b): the first n entries


@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_bit_for_bit(pkg, ctx, ref, W, dtype):
    for m, n in shapes(W):
        A = qh.random(m, n, dtype)
        QR, tau, z = ref.factor(A)
        M = pkg.HipMatrix.from_numpy(A)
        F = pkg.qr(M)
        info = F.info()
        assert (F.m, F.n, F.zero_diag, z) == (m, n, 0, 0) and info["resident"] == 1
        assert info["launches_factor"] == qh.plan_launches(n, W) and info["launches_solve"] == 1 + -(-n // 64), (m, n)
        assert F.factors is not M and np.array_equal(M.to_numpy(), A)       # qr(A) leaves A untouched
        check_against(pkg, ref, A, F, QR, tau, (m, n, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", DTYPES)
def test_streaming_and_resident_forms_give_the_same_bits(pkg, ctx, ref, W, dtype):
    m = 300
    for n in (3, W + 1):
        A = qh.random(m, n, dtype)
        QR, tau, _ = ref.factor(A)
        S = pkg.qr(pkg.HipMatrix.from_numpy(A), resident_rows=m - 1)
        assert S.info()["resident"] == 0 and S.info()["resident_rows"] == m - 1             # m = 300 streams
        check_against(pkg, ref, A, S, QR, tau, (m, n, "streaming"))
        B = qh.block(m, 5, dtype)
        want = ref.solve(QR, tau, B)
        assert qh.same_bits(S.solve(pkg.HipMatrix.from_numpy(B)).to_numpy(), want)
        for F in (pkg.qr(pkg.HipMatrix.from_numpy(A), resident_rows=m), pkg.qr(pkg.HipMatrix.from_numpy(A))):
            assert F.info()["resident"] == 1                                                # at the limit and by default it stays in LDS
            assert qh.same_bits(F.factors.to_numpy(), S.factors.to_numpy()) and qh.same_bits(F.tau, S.tau)
            assert qh.same_bits(F.Q().to_numpy(), S.Q().to_numpy())
    n = 3 * W + 1                       # a trailing update keeps the rows from its panel's first column on: the first streams, the later ones fit
    A = qh.random(m, n, dtype)
    QR, tau, _ = ref.factor(A)
    F = pkg.qr(pkg.HipMatrix.from_numpy(A), resident_rows=m - W)
    assert F.info()["resident"] == 0 and qh.same_bits(F.factors.to_numpy(), QR) and qh.same_bits(F.tau, tau)


def _with_ld(pkg, A, ld, pad):
    """A in a HipMatrix whose leading dimension is `ld`, the padding rows holding `pad`"""
    m, n = A.shape
    M = pkg.HipMatrix(m, n, A.dtype)
    M.ld = ld
    M.buf = pkg.HipVector(ld * n, A.dtype, M.ctx)
    store = np.full((ld, n), pad, A.dtype, order="F")
    store[:m] = A
    M.buf.copy_from_host(store.ravel(order="F"))
    return M


@pytest.mark.parametrize("dtype", DTYPES)
def test_storage_and_in_place(pkg, ctx, ref, W, dtype):
    m, n = 2 * W + 7, W + 3
    A = qh.random(m, n, dtype)
    QR, tau, _ = ref.factor(A)
    for ld in (m, m + 1, m + 37):
        M = _with_ld(pkg, A, ld, np.nan)                                    # NaN padding: it must stay unread
        F = pkg.qr_(M)
        assert F.factors is M                                               # qr!(A): in place
        check_against(pkg, ref, A, F, QR, tau, (m, n, ld))
        pad = M.buf.to_numpy().reshape(n, ld).T[m:]
        assert np.isnan(pad).all()                                          # ... and unwritten
        Yh = qh.block(m, 3, dtype)
        Y = _with_ld(pkg, Yh, m + 5, np.nan)
        F.lmul_Qt_(Y)
        assert qh.same_bits(Y.to_numpy(), ref.lmul(QR, tau, Yh, True)) and np.isnan(Y.buf.to_numpy().reshape(3, m + 5).T[m:]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fixtures_device_against_checker(pkg, ctx, ref, W, dtype):
    m, n = W + 9, W + 3
    cases = [("zero_below", qh.zero_below_case(ref, m, n, dtype, W)), ("nonfinite", qh.nonfinite_case(ref, m, n, dtype))]
    cases += [(qh.SIGNS[w][0], qh.signs_case(ref, m, n, dtype, w)) for w in range(len(qh.SIGNS))]
    cases += [(f"scaled {k}", qh.scaled_case(ref, m, n, dtype, k)) for k in qh.scale_exponents(dtype)]
    for name, (A, QR, tau) in cases:
        F = pkg.qr(pkg.HipMatrix.from_numpy(A))
        assert F.zero_diag == 0, name
        check_against(pkg, ref, A, F, QR, tau, name)                        # NaN in the same places (same_bits)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_column(pkg, ctx, ref, W, dtype):
    m, n = W + 9, W + 3
    for k in (0, W // 2, W, n - 1):
        A, QR, tau = qh.zero_column_case(ref, m, n, dtype, k)
        if k < n - 1:
            A[:, n - 1] = 0                                                 # a later zero is not the one reported
            QR, tau, z = ref.factor(A)
            assert z == k + 1
        F = pkg.qr(pkg.HipMatrix.from_numpy(A))                             # qr succeeds
        assert F.zero_diag == k + 1 and F.info()["zero_diag"] == k + 1
        for b in (pkg.HipVector.from_numpy(qh.vector(m, dtype)), pkg.HipMatrix.from_numpy(qh.block(m, 3, dtype))):
            with pytest.raises(np.linalg.LinAlgError) as ei:
                F.solve(b)
            assert isinstance(ei.value, pkg.SingularException) and ei.value.col == k + 1 and f"SingularException({k + 1})" in str(ei.value)
        x, b = pkg.HipVector(n, dtype), pkg.HipVector(m, dtype).fill_(1)
        assert pkg.lib().mik_dense_qr_solve(F.handle, C.c_void_p(x.ptr), C.c_void_p(b.ptr)) == 8               # the C entry: MIK_ERR_SINGULAR
        assert f"SingularException({k + 1})" in pkg.lib().mik_last_error(ctx.handle).decode()
        check_against(pkg, ref, A, F, QR, tau, ("zero_column", k))          # lmul, Q, R still work


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_solves(pkg, ctx, ref, W, dtype):
    m, n = 2 * W + 7, W + 3
    A = qh.random(m, n, dtype)
    QR, tau, _ = ref.factor(A)
    F = pkg.qr(pkg.HipMatrix.from_numpy(A))
    for cols in (1, 2, 3, 32, 33):
        B = qh.block(m, cols, dtype)
        if cols >= 3:
            B[5, 1] = np.nan                                                # a non-finite column next to finite ones
        want = ref.solve(QR, tau, B)
        assert np.isfinite(want[:, 0]).all() and (cols < 3 or (np.isnan(want[:, 1]).all() and np.isfinite(want[:, 2:]).all()))
        dB = pkg.HipMatrix.from_numpy(B)
        X = F.solve(dB)
        got = X.to_numpy()
        assert (X.n, X.cols) == (n, cols) and qh.same_bits(got, want), (cols, qh.first_difference(got, want))
        assert qh.same_bits(dB.to_numpy(), B)                               # B is not modified
        for k in range(cols):                                               # each column against its vector solve
            assert qh.same_bits(F.solve(pkg.HipVector.from_numpy(B[:, k])).to_numpy(), got[:, k]), (cols, k)
        assert F.ldiv_(dB) is dB                                            # in place: the first n rows become X
        h = dB.to_numpy()
        assert qh.same_bits(h[:n], want)
        Bl, Xl = _with_ld(pkg, B, m + 3, np.nan), _with_ld(pkg, np.zeros((n, cols + 1), dtype), n + 11, 7)      # any ld; cols of a wider X
        F.ldiv_(Xl, Bl, cols=cols)
        full = Xl.buf.to_numpy().reshape(cols + 1, n + 11).T
        assert qh.same_bits(np.asfortranarray(full[:n, :cols]), want) and (full[n:] == 7).all() and (full[:n, cols] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_lsqr_and_lsmr_against_the_backslash(pkg, ctx, dtype):
    """test/lsqr.jl:15-19 and test/lsmr.jl:68-72 with A \\ b on the device: norm(x - A \\ b) <= 4 sqrt(eps) and <= sqrt(eps)"""
    rng = np.random.default_rng(1234321)
    A, b = rng.random((10, 5)).astype(dtype), rng.random(10).astype(dtype)
    dA, db = pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b)
    direct = pkg.ldiv(dA, db).to_numpy().astype(np.float64)
    sq = float(np.sqrt(np.finfo(dtype).eps))
    x, h = pkg.extras.lsqr(dA, db, log=True)
    assert h.isconverged and np.linalg.norm(x.to_numpy().astype(np.float64) - direct) <= 4 * sq
    x, h = pkg.extras.lsmr(dA, db, log=True)
    assert h.isconverged and np.linalg.norm(x.to_numpy().astype(np.float64) - direct) <= sq
    S = rng.random((5, 5)).astype(dtype) + np.eye(5, dtype=dtype)           # square: the backslash is lu
    dS, d5 = pkg.HipMatrix.from_numpy(S), pkg.HipVector.from_numpy(b[:5].copy())
    assert np.array_equal(pkg.ldiv(dS, d5).to_numpy(), pkg.lu(dS).solve(d5).to_numpy())


def test_orthogonalize_with_the_thin_q_as_the_basis(pkg, ctx):
    """test/orthogonalize.jl:17-47 in Float64 with V = qr(A).Q()"""
    T, n, m = np.float64, 10, 3
    rng = np.random.default_rng(1234321)
    V = pkg.qr(pkg.HipMatrix.from_numpy(rng.random((n, m)).astype(T))).Q()
    Vh = V.to_numpy()
    w0 = rng.random(n).astype(T)
    eps = np.finfo(T).eps
    for method in (pkg.DGKS(), pkg.ClassicalGramSchmidt(), pkg.ModifiedGramSchmidt()):
        h, w = np.zeros(m, T), pkg.HipVector.from_numpy(w0)
        nrm = pkg.orthogonalize_and_normalize_(V, m, w, h, method)
        wh = w.to_numpy()
        assert np.isclose(np.linalg.norm(wh), 1.0, rtol=np.sqrt(eps), atol=0)              # norm(w) ≈ 1
        assert np.linalg.norm(Vh.T @ wh) <= 10 * eps                                        # norm(V'w) ≈ 0 atol = 10 eps
        back = nrm * wh + Vh @ h
        assert np.linalg.norm(back - w0) <= np.sqrt(eps) * max(np.linalg.norm(back), np.linalg.norm(w0))    # nrm w + V h ≈ w_original


@pytest.mark.parametrize("dtype", DTYPES)
def test_gmres_with_a_square_qr_as_pl_and_pr(pkg, ctx, W, dtype, monkeypatch):
    """test/gmres.jl:28-35 with F = qr(A), through the library's own callback: no Python frame per application"""
    reltol = float(np.sqrt(np.finfo(dtype).eps))
    calls = {"n": 0}
    inner = pkg.DenseQR.ldiv_

    def counted(self, *a, **k):
        calls["n"] += 1
        return inner(self, *a, **k)
    for n in (10, 2 * W + 1):
        rng = np.random.default_rng(1234321 + n)
        A = (rng.random((n, n)) + np.eye(n)).astype(dtype)
        b = rng.random(n).astype(dtype)
        A64 = A.astype(np.float64)
        dA, db = pkg.HipMatrix.from_numpy(A), pkg.HipVector.from_numpy(b)
        F = pkg.qr(dA)
        with monkeypatch.context() as mp:
            mp.setattr(pkg.DenseQR, "ldiv_", counted)
            x, h = pkg.gmres(dA, db, Pl=F, maxiter=1, restart=1, reltol=reltol, log=True)
            y, g = pkg.gmres(dA, db, Pl=pkg.Identity(), Pr=F, maxiter=1, restart=1, reltol=reltol, log=True)
            assert calls["n"] == 0
        assert h.isconverged and g.isconverged, n
        r = F.solve(pkg.HipVector.from_numpy((A64 @ x.to_numpy() - b).astype(dtype))).to_numpy()            # F \ (A x - b)
        assert np.linalg.norm(r.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)) <= reltol, n
        assert np.linalg.norm(A64 @ y.to_numpy() - b) / np.linalg.norm(b.astype(np.float64)) <= reltol, n


def test_refusals(pkg, ctx):
    L, lib = pkg.lib(), pkg._lib
    vp = C.c_void_p
    for factor in (pkg.qr, pkg.qr_):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            factor(pkg.HipMatrix(4, 6))                                     # m < n
        with pytest.raises(TypeError, match="HipMatrix"):
            factor(np.eye(3))
        for dtype in (np.complex128, np.complex64):
            with pytest.raises(TypeError, match=np.dtype(dtype).name):
                factor(pkg.HipMatrix(6, 4, dtype))
    with pytest.raises(ValueError, match="DimensionMismatch.*wide"):
        pkg.ldiv(pkg.HipMatrix(4, 6), pkg.HipVector(4))
    Ah = qh.random(10, 6, np.float64)
    A = pkg.HipMatrix.from_numpy(Ah)
    h, col = vp(), C.c_int64()
    for code, name in ((lib.MIK_C64, "ComplexF64"), (lib.MIK_C32, "ComplexF32")):      # through the C entry: named, not implemented
        assert L.mik_dense_qr_create(ctx.handle, vp(A.buf.ptr), 10, 6, A.ld, code, None, C.byref(col), C.byref(h)) == 5
        assert name in L.mik_last_error(ctx.handle).decode()
    for m, n, ld in ((6, 10, 64), (10, 6, 9), (10, 0, 64)):
        assert L.mik_dense_qr_create(ctx.handle, vp(A.buf.ptr), m, n, ld, lib.MIK_F64, None, C.byref(col), C.byref(h)) == 3
        assert "mik_dense_qr_create" in L.mik_last_error(ctx.handle).decode()
    assert L.mik_dense_qr_create(ctx.handle, vp(A.buf.ptr), 2 ** 31 - 64, 6, 2 ** 31, lib.MIK_F64, None, C.byref(col), C.byref(h)) == 5
    assert np.array_equal(A.to_numpy(), Ah)                                 # a refused call has not touched the matrix
    F = pkg.qr_(A)
    b, x = pkg.HipVector(10).fill_(1), pkg.HipVector(6)
    for call in (lambda: F.ldiv_(x, pkg.HipVector(11)), lambda: F.ldiv_(pkg.HipVector(7), b), lambda: F.ldiv_(x, pkg.HipVector(10, np.float32)),
                 lambda: F.solve(pkg.HipVector(6)), lambda: F.lmul_Q_(x), lambda: F.lmul_Qt_(pkg.HipMatrix(6, 2)), lambda: F.solve(pkg.HipMatrix(10, 2, np.float32)),
                 lambda: F.ldiv_(pkg.HipMatrix(6, 1), pkg.HipMatrix(10, 2))):
        with pytest.raises(ValueError, match="DimensionMismatch"):
            call()
    big = pkg.HipVector(40).fill_(1)                                        # overlaps: x inside b, a vector or a block in the factors
    for xs, bs, who in ((big.view(3, 6), big.view(0, 10), "mik_dense_qr_solve"), (A.buf.view(0, 6), b, "mik_dense_qr_solve"), (x, A.buf.view(2, 10), "mik_dense_qr_solve")):
        assert L.mik_dense_qr_solve(F.handle, vp(xs.ptr), vp(bs.ptr)) == 1 and who in L.mik_last_error(ctx.handle).decode()
    assert L.mik_dense_qr_lmul(F.handle, 0, vp(A.buf.ptr), A.ld, 1) == 1 and "mik_dense_qr_lmul" in L.mik_last_error(ctx.handle).decode()
    assert L.mik_dense_qr_thin_q(F.handle, vp(A.buf.ptr), A.ld) == 1 and "mik_dense_qr_thin_q" in L.mik_last_error(ctx.handle).decode()
    blk = pkg.HipVector(200).fill_(1)
    assert L.mik_dense_qr_solve_block(F.handle, vp(blk.view(4, 6).ptr), 10, vp(blk.ptr), 10, 2) == 1        # X inside B
    assert L.mik_dense_qr_solve_block(F.handle, vp(blk.ptr), 10, vp(blk.ptr), 12, 2) == 1                   # the same pointer, other ld
    assert "mik_dense_qr_solve_block" in L.mik_last_error(ctx.handle).decode()
    assert L.mik_dense_qr_solve_block(F.handle, vp(blk.ptr), 5, vp(blk.view(100, 20).ptr), 10, 2) == 3      # ldx < n
    with pytest.raises(ValueError, match="DimensionMismatch.*qr"):          # a tall factorisation is no preconditioner
        pkg.gmres(pkg.HipMatrix.from_numpy(np.eye(6)), pkg.HipVector(6).fill_(1), Pl=F)
    assert L.mik_dense_qr_ldiv_fn(F.handle, vp(x.ptr), vp(b.ptr)) == 3
    S = pkg.qr(pkg.HipMatrix.from_numpy(np.eye(6) + 0.1))
    with pytest.raises(ValueError, match="DimensionMismatch"):              # the callback never sees a length: checked where it is bound
        pkg.gmres(pkg.HipMatrix.from_numpy(np.eye(7)), pkg.HipVector(7).fill_(1), Pl=S)
    assert np.isfinite(F.solve(b).to_numpy()).all()
