"""What the tests of the block solves of the dense LU and Cholesky (F.ldiv_(Y, X) on two HipMatrix) share: the block plan restated in
plain Python, the sizes and widths a test visits, a numpy restatement of both substitutions on a block of columns (one rounded numpy
operation per rounded operation of the contract, every column side by side), and the checker applied column by column.  Test
infrastructure only."""
import numpy as np

import dense_chol_host as ch


def sizes(W):
    """one row, two, around one panel, a partial third panel, six panels with a short last one"""
    return sorted({1, 2, W - 1, W, W + 1, 2 * W + 1, 5 * W + 3})


def widths(NB, G):
    """one column, two, around one group of NB columns per lane (a partial last group before and after it), several groups, a whole pass,
    and one column into the second pass"""
    return sorted({1, 2, NB - 1, NB, NB + 1, 2 * NB + 1, G, G + 1} - {0})


def vector_launches(n, W, gather):
    """launches of one vector solve: ceil(n / W) each way, and the LU's gather"""
    return (1 if gather else 0) + 2 * -(-n // W)


def plan(n, nrhs, W, NB, G, itemsize, gather):
    """the block plan: passes of at most G columns, each the launches of one vector solve over its groups of NB columns; the workspace is
    n x G elements whatever nrhs is.  `groups` lists, per pass, (groups launched in grid y, live columns of the last group)."""
    assert G % NB == 0
    cols = [min(G, nrhs - c) for c in range(0, max(nrhs, 0), G)]
    return {"NB": NB, "G": G, "passes": len(cols), "launches": len(cols) * vector_launches(n, W, gather), "workspace_bytes": n * G * itemsize,
            "groups": [(-(-c // NB), c - (-(-c // NB) - 1) * NB) for c in cols]}


def reported(p):
    """the keys F.block_plan reports"""
    return {k: p[k] for k in ("NB", "G", "passes", "launches", "workspace_bytes")}


def rhs(n, cols, dtype, seed=11):
    rng = np.random.default_rng(seed + 13 * n + cols)
    B = rng.standard_normal((n, cols))
    if ch.is_complex(dtype):
        B = B + 1j * rng.standard_normal((n, cols))
    return np.asfortranarray(B.astype(dtype))


def padded(B, ld, poison):
    """B in a taller column-major array of ld rows whose padding rows are `poison`"""
    out = np.full((ld, B.shape[1]), poison, B.dtype, order="F")
    out[:B.shape[0], :] = B
    return out


# ---- both substitutions on a block of columns in numpy: separate arrays of real and imaginary parts (dense_chol_host._msub), a row of the
# ---- block per step, so that every column sees the operations of the contract in the contract's order ---------------------------------
def _parts(B):
    R = ch.real_of(B.dtype)
    return np.array(B.real, R), np.array(np.imag(B), R)


def _join(re, im, dtype):
    out = np.zeros(re.shape, dtype)
    out.real = re
    if ch.is_complex(dtype):
        out.imag = im
    return out


def chol_solve_block(L, B):
    """ldiv! of the Cholesky contract on every column of B at once"""
    n = L.shape[0]
    if not ch.is_complex(B.dtype):                                          # real: a product and a difference, no imaginary zeros to sign
        x = np.array(B, L.dtype)
        with np.errstate(all="ignore"):
            for i in range(n):
                acc = x[i].copy()
                for k in range(i):
                    acc = acc - L[i, k] * x[k]
                x[i] = acc / L[i, i]
            for i in range(n - 1, -1, -1):
                acc = x[i].copy()
                for k in range(n - 1, i, -1):
                    acc = acc - L[k, i] * x[k]
                x[i] = acc / L[i, i]
        return x
    lr, li = _parts(np.asarray(L))
    xr, xi = _parts(np.asarray(B))
    with np.errstate(all="ignore"):
        for i in range(n):
            ar, ai = xr[i].copy(), xi[i].copy()
            for k in range(i):
                ar, ai = ch._msub(ar, ai, lr[i, k], li[i, k], xr[k], xi[k])
            xr[i], xi[i] = ar / lr[i, i], ai / lr[i, i]
        for i in range(n - 1, -1, -1):
            ar, ai = xr[i].copy(), xi[i].copy()
            for k in range(n - 1, i, -1):
                ar, ai = ch._msub(ar, ai, lr[k, i], -li[k, i], xr[k], xi[k])
            xr[i], xi[i] = ar / lr[i, i], ai / lr[i, i]
    return _join(xr, xi, B.dtype)


def lu_solve_block(LU, perm, B):
    """ldiv! of the LU contract on every column of B at once: the interchanges as one gather, the unit-lower chain ascending, the upper
    chain descending with the division last"""
    n = LU.shape[0]
    x = np.array(B[perm, :], LU.dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = x[i].copy()
            for k in range(i):
                acc = acc - LU[i, k] * x[k]
            x[i] = acc
        for i in range(n - 1, -1, -1):
            acc = x[i].copy()
            for k in range(n - 1, i, -1):
                acc = acc - LU[i, k] * x[k]
            x[i] = acc / LU[i, i]
    return x


def per_column(solve, B):
    """the checker on every column of B: what the device block solve is compared against"""
    return np.stack([solve(np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])], axis=1)
