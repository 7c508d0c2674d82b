"""The shapes of tests/test_gpu_dense_operator_launch.py without a GPU: the tables of expected grids against the launch arithmetic of
csrc/mik_dense_mul.hip restated in tests/dense_operator_host.py (the GPU tests hold the same tables to mik_dev_dense_plan), and the
references of every shape -- the C restatement of the chunked order, the oracle's tree dot -- inside the error bounds the GPU tests
assert for the device results, so that a bound that a correct result could miss shows here first."""
import ctypes as C

import numpy as np
import pytest

import dense_operator_host as dh

DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return dh.build(tmp_path_factory.mktemp("dense_mul_ref"))


def _shapes(pkg, dtype):
    c, r, w, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert pkg.lib().mik_dense_mul_shape(C.byref(c), C.byref(r)) == 0
    assert pkg.lib().mik_reduce_shape(pkg._lib.dtype_code(dtype), C.byref(w), C.byref(l)) == 0
    return c.value, r.value, w.value, l.value, 256 * w.value * l.value


def _sub(d, keys):
    return tuple(d[k] for k in keys)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_shape_tables_give_the_grids_and_pass_counts_they_state(pkg, dtype):
    C_, R, W, L, S = _shapes(pkg, dtype)
    assert [dh.combine_trips(nc) for nc in dh.COMBINE_NC] == list(dh.COMBINE_TRIPS)
    assert dh.combine_trips(50) == (1, 2, 1)                             # 32 + 8 + 8 + tail: the second chunk-stride shape
    for nc in dh.COMBINE_NC:                                             # one pass on any machine of at least 11 compute units
        assert _sub(dh.model_n(65, nc * C_ - 5, C_, R, 11), ("gx", "gy", "cols", "passes")) == (1, nc, nc, 1)
    for m, n, gx, gy, nc, passes in dh.CHUNK_STRIDE(C_, R):
        assert _sub(dh.model_n(m, n, C_, R, dh.SMALL_CUS), ("gx", "gy", "cols", "passes")) == (gx, gy, nc, passes)
    assert [c[5] for c in dh.CHUNK_STRIDE(C_, R)] == [2, 4, 3]
    for m, n, gx, gy, batches, passes in dh.BATCH_STRIDE(S):
        assert _sub(dh.model_t(m, n, S, dh.SMALL_CUS), ("gx", "gy", "cols", "passes", "segment_passes")) == (gx, gy, batches, passes, 1)
    for m, n, gx, gy, batches, nseg, passes in dh.SEGMENT_STRIDE(S):
        assert _sub(dh.model_t(m, n, S, dh.SMALL_CUS), ("gx", "gy", "cols", "nseg", "passes", "segment_passes")) == (gx, gy, batches, nseg, 2, passes)
    m, n = dh.streamed_shape(R, np.dtype(dtype).itemsize)
    assert m == 2 * R + 1
    if R == 1024:
        assert n == {8: 11714, 4: 23427}[np.dtype(dtype).itemsize]
    assert (dh.SMALL_MACHINE & 0xFFFF, dh.SMALL_MACHINE >> 16) == (dh.SMALL_CUS, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_references_of_every_shape_stay_inside_the_bounds_the_device_is_held_to(pkg, orc, ref, dtype):
    C_, R, W, L, S = _shapes(pkg, dtype)
    for direction, m, n, seed_a, seed_x in dh.launch_shapes(C_, R, S, np.dtype(dtype).itemsize):
        A = dh.normal(m, n, dtype, seed=seed_a)
        if direction == "N":
            x = dh.vec(n, dtype, seed=seed_x)
            assert dh.within_n_bound(ref.chunked(A, x, C_), A, x, C_), (m, n)
        else:
            x = dh.vec(m, dtype, seed=seed_x)
            assert dh.within_t_bound(dh.tree_cols(orc, A, x, W, L), A, x, W, L), (m, n)
