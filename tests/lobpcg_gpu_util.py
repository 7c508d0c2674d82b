"""What the GPU tests of the lobpcg block entries share (tests/test_gpu_lobpcg.py, tests/test_gpu_lobpcg_paths.py): test data whose bits
move with any other association, device blocks in both placements, raw calls of the entries, and the device run next to the numpy double."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from lobpcg_double import HostJacobi, NumpyOps, operator

_vp = C.c_void_p
DTYPES = [np.float64, np.float32]


def wide(rng, shape, dt, span=30):
    """mixed signs, magnitudes spanning 2^-span .. 2^span: a fused multiply-add or another association changes bits"""
    a = rng.choice([-1.0, 1.0], size=shape) * np.exp2(rng.uniform(-span, span, size=shape)) * (1 + rng.random(shape))
    return a.astype(dt)


class Blk:
    """an n x k device block: aligned (leading dimension n rounded up to 64), or offset by one element with an odd leading dimension > n;
    everything of the buffer outside the columns holds `fill`"""

    def __init__(self, pkg, ctx, host, offset, fill=0.0):
        self.n, self.k = host.shape
        self.dt = np.dtype(host.dtype)
        self.off = 1 if offset else 0
        self.ld = self.n + 3 + (self.n % 2 == 0) if offset else (self.n + 63) // 64 * 64
        self.buf = pkg.HipVector(self.ld * self.k + self.off, self.dt, ctx)
        flat = np.full(self.ld * self.k + self.off, fill, self.dt)
        for j in range(self.k):
            flat[self.off + j * self.ld: self.off + j * self.ld + self.n] = host[:, j]
        self.buf.copy_from_host(flat)
        self.ptr = self.buf.ptr + self.off * self.dt.itemsize

    def col(self, j):
        return self.buf.view(self.off + j * self.ld, self.n)

    def at(self, j):
        """device address of column j"""
        return self.ptr + j * self.ld * self.dt.itemsize

    def get(self):
        flat = self.buf.to_numpy()
        return np.stack([flat[self.off + j * self.ld: self.off + j * self.ld + self.n] for j in range(self.k)], axis=1)

    def padding(self):
        """every element of the buffer that belongs to no column"""
        flat = self.buf.to_numpy()
        keep = np.ones(flat.size, bool)
        for j in range(self.k):
            keep[self.off + j * self.ld: self.off + j * self.ld + self.n] = False
        return flat[keep]


def code(pkg, dt):
    return pkg._lib.dtype_code(dt)


def gram_raw(pkg, ctx, X, p, Y, q, ldg=None, fill=0.0, x0=0, y0=0):
    """G = X[:, x0:x0+p]' * Y[:, y0:y0+q]; with ldg the whole ldg x q host array comes back, pre-filled with `fill`"""
    G = np.full((ldg or p, q), fill, X.dt, order="F")
    rc = pkg.lib().mik_block_gram(ctx.handle, code(pkg, X.dt), X.n, p, q, _vp(X.at(x0)), X.ld, _vp(Y.at(y0)), Y.ld, G.ctypes.data_as(_vp), G.shape[0])
    assert rc == 0, pkg.lib().mik_last_error(ctx.handle)
    return G


def dots(pkg, X, p, Y, q, x0=0, y0=0):
    return np.array([[pkg.dot(X.col(x0 + i), Y.col(y0 + j)) for j in range(q)] for i in range(p)], X.dt)


def update_raw(pkg, ctx, n, sx, b1, b2, X, R, P, V, Xo, Po):
    """V: (sx + b1 + b2) x sx, or taller -- its row count is passed as the leading dimension"""
    Vf = np.asfortranarray(V)
    return pkg.lib().mik_block_update(ctx.handle, code(pkg, X.dt), n, sx, b1, b2, _vp(X.ptr), X.ld, _vp(R.ptr), R.ld, _vp(P.ptr), P.ld,
                                      Vf.ctypes.data_as(_vp), Vf.shape[0], _vp(Xo.ptr), Xo.ld, _vp(Po.ptr), Po.ld)


def spd_b(n, dt):
    """tridiagonal (-1, 4, -1): strictly diagonally dominant, SPD"""
    return sp.diags([-np.ones(n - 1), 4 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csc", dtype=dt)


def both(pkg, orc, ctx, dt, S, Sb, largest, rest, jacobi, **kw):
    """(device run, run on the numpy double) of one lobpcg call"""
    A, B = pkg.HipCSR.from_scipy(S, ctx), (pkg.HipCSR.from_scipy(Sb, ctx) if Sb is not None else None)
    d = S.diagonal().astype(dt)
    dev_args = (A, largest) if B is None else (A, B, largest)
    rd = pkg.lobpcg(*dev_args, *rest, P=pkg.JacobiPrec(pkg.HipVector.from_numpy(d, ctx)) if jacobi else None, log=True,
                    rng=np.random.default_rng(5), **kw)
    return rd, double_run(pkg, orc, dt, S, Sb, largest, rest, jacobi, **kw)


def double_run(pkg, orc, dt, S, Sb, largest, rest, jacobi, **kw):
    """the host half of both(): needs no device"""
    n = S.shape[0]
    d = S.diagonal().astype(dt)
    dbl_args = (operator(orc, S), largest) if Sb is None else (operator(orc, S), operator(orc, Sb), largest)
    return pkg.lobpcg(*dbl_args, *rest, P=HostJacobi(d) if jacobi else None, log=True, rng=np.random.default_rng(5),
                      ops=NumpyOps(orc, n, dt), **kw)


def same_trace(ta, tb):
    assert len(ta) == len(tb), (len(ta), len(tb))
    for a, b in zip(ta, tb):
        assert a.iteration == b.iteration
        assert np.array_equal(a.ritz_values, b.ritz_values), (a.iteration, a.ritz_values, b.ritz_values)
        assert np.array_equal(a.residual_norms, b.residual_norms), (a.iteration, a.residual_norms, b.residual_norms)
