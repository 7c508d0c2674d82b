"""device_exclusive_scan of csrc/mik_upload.hip (the row pointer of the CSC -> CSR transpose, the slot pointer of the per-slice-offset
layouts and the slice pointer of the jagged slices all come out of it) through its development entry mik_dev_exclusive_scan, against
numpy.cumsum in int64: one tile, two levels, and the three levels a 256^3 operator takes on every upload (more than 2048^2 elements),
with the carries that only one level sees, and guard words around the array.  GPU box only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048                                   # SCAN_TILE: elements per workgroup
GUARD = 64
SENTINEL = -0x5A5A5A5B
SIZES = [0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE, TILE * (TILE - 1) + 1, TILE ** 2 - 1, TILE ** 2, TILE ** 2 + 1, TILE ** 2 + TILE + 1]
INPUTS = ["random", "one_at_0", "one_at_end", "one_at_top_level"]


def cases():
    for n in SIZES:
        for kind in INPUTS:
            if kind == "one_at_top_level" and n <= TILE ** 2:       # index 2048^2 exists only beyond it
                continue
            if kind in ("one_at_0", "one_at_end") and n == 0:
                continue
            yield pytest.param(n, kind, id=f"{n}-{kind}")


def input_values(n, kind):
    if kind == "random":
        return np.random.default_rng(n + 1).integers(0, 8, size=n, dtype=np.int32)       # totals stay below 2^25
    v = np.zeros(n, np.int32)
    v[{"one_at_0": 0, "one_at_end": n - 1, "one_at_top_level": TILE ** 2}[kind]] = 1
    return v


def scan_on_device(pkg, ctx, values):
    """values (int32, n) -> the n + 1 words mik_dev_exclusive_scan leaves, and the guard words in front of and behind them"""
    L, check, vp = pkg.lib(), pkg._lib.check, C.c_void_p
    n = values.size
    buf = np.full(GUARD + n + 1 + GUARD, SENTINEL, np.int32)          # data[n] starts as a sentinel too: the total must be written
    buf[GUARD:GUARD + n] = values
    p = vp()
    check(L.mik_malloc(ctx.handle, buf.nbytes, C.byref(p)), "mik_malloc", ctx.handle)
    try:
        check(L.mik_memcpy_h2d(ctx.handle, p, buf.ctypes.data_as(vp), buf.nbytes), "mik_memcpy_h2d", ctx.handle)
        check(L.mik_dev_exclusive_scan(ctx.handle, vp(p.value + 4 * GUARD), n), "mik_dev_exclusive_scan", ctx.handle)
        check(L.mik_memcpy_d2h(ctx.handle, buf.ctypes.data_as(vp), p, buf.nbytes), "mik_memcpy_d2h", ctx.handle)
    finally:
        check(L.mik_free(ctx.handle, p), "mik_free", ctx.handle)
    return buf[GUARD:GUARD + n + 1], buf[:GUARD], buf[GUARD + n + 1:]


@pytest.mark.parametrize("n,kind", cases())
def test_exclusive_scan_equals_cumsum(pkg, ctx, n, kind):
    values = input_values(n, kind)
    want = np.zeros(n + 1, np.int64)
    np.cumsum(values, dtype=np.int64, out=want[1:])                    # want[i] = sum of values[:i]; want[n] = the total
    got, front, behind = scan_on_device(pkg, ctx, values)
    assert np.array_equal(front, np.full(GUARD, SENTINEL, np.int32)) and np.array_equal(behind, np.full(GUARD, SENTINEL, np.int32))
    assert got[n] == want[n]
    assert np.array_equal(got.astype(np.int64), want)


def test_exclusive_scan_refuses_what_it_cannot_index(pkg, ctx):
    L = pkg.lib()
    assert L.mik_dev_exclusive_scan(ctx.handle, None, 4) == 1 and L.mik_dev_exclusive_scan(ctx.handle, C.c_void_p(256), -1) == 1      # MIK_ERR_INVALID
    assert L.mik_dev_exclusive_scan(ctx.handle, C.c_void_p(256), 2 ** 31) == 5                                                     # MIK_ERR_NOTIMPL
