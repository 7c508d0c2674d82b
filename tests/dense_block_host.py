"""What tests/test_gpu_dense_block.py and tests/test_lobpcg_dense_host.py share about the block product Y = A X of a dense device matrix
(mik_dense_mm, csrc/mik_dense_mul.hip): the launch arithmetic of the block plan restated (`model_nb`, next to `model_n` of
tests/dense_operator_host.py), the shape and width tables of the GPU tests, the plan query and the raw call.  Test infrastructure only."""
import ctypes as C

import dense_operator_host as dh

_vp = C.c_void_p
GW_MIN = 2                          # MIK_DM_GW_MIN: a last group narrower than this runs through the vector kernels
B_MAX = 32                          # widest block of mik_dense_mm


def model_nb(m, n, b, C_, R, GW, cus, wmin=GW_MIN):
    """the plan of mik_dense_mm: launches of the block kernel, the width of the last one, the trailing columns left to the vector kernels, the
    grid (the vector form's) and the passes of the chunk loop"""
    if m == 0 or n == 0 or b <= 0:
        return {"groups": 0, "last_w": 0, "vector_cols": 0, "gx": 0, "gy": 0, "chunks": 0, "passes": 0}
    groups, last, vector_cols = dh._ceil(b, GW), b % GW or GW, 0
    if last < wmin:
        vector_cols, groups = last, groups - 1
        last = GW if groups else 0
    v = dh.model_n(m, n, C_, R, cus)
    return {"groups": groups, "last_w": last, "vector_cols": vector_cols, "gx": v["gx"], "gy": v["gy"], "chunks": v["cols"], "passes": v["passes"]}


def bit_shapes(C_, R):
    """(m, n) of the bit tests: one element; below one chunk; one chunk, a row short of one workgroup; a row and a column past both; several of each"""
    return [(1, 1), (65, C_ - 1), (R - 1, C_), (R + 1, C_ + 1), (2 * R + 1, 5 * C_ + 3)]


def widths(GW):
    return [1, 2, 3, GW - 1, GW, GW + 1, 2 * GW, 31, 32]


def block_shapes(C_, R, GW, itemsize):
    """[(m, n, b)] of every case of tests/test_gpu_dense_block.py that asserts a plan"""
    out = [(m, n, b) for m, n in bit_shapes(C_, R) for b in widths(GW)]
    out += [(c[0], c[1], GW + 1) for c in dh.CHUNK_STRIDE(C_, R)]
    out += [(65, nc * C_ - 5, 3) for nc in dh.COMBINE_NC]
    m, n = dh.streamed_shape(R, itemsize)
    return out + [(m, n, GW + 1), (m, n - 1, GW + 1)]


def block_shape(pkg):
    g = C.c_int()
    assert pkg.lib().mik_dense_block_shape(C.byref(g)) == 0
    return g.value


def _ptr(M):
    return M.ptr if hasattr(M, "ptr") else M.buf.ptr


def plan(pkg, handle, b, X, Y):
    """mik_dev_dense_block_plan for the blocks X, Y (a Blk of tests/lobpcg_gpu_util.py or a HipMatrix)"""
    vec, streamed, groups, last_w, vcols = (C.c_int(-1) for _ in range(5))
    gx, gy, chunks, ws = (C.c_int64(-1) for _ in range(4))
    assert pkg.lib().mik_dev_dense_block_plan(handle, int(b), _vp(_ptr(X)), X.ld, _vp(_ptr(Y)), Y.ld, C.byref(vec), C.byref(streamed), C.byref(gx),
                                              C.byref(gy), C.byref(chunks), C.byref(groups), C.byref(last_w), C.byref(vcols), C.byref(ws)) == 0
    return {"vec": vec.value, "streamed": streamed.value, "gx": gx.value, "gy": gy.value, "chunks": chunks.value, "groups": groups.value,
            "last_w": last_w.value, "vector_cols": vcols.value, "workspace_bytes": ws.value}


def mm(pkg, handle, b, X, Y):
    return pkg.lib().mik_dense_mm(handle, int(b), _vp(X.ptr), X.ld, _vp(Y.ptr), Y.ld)


def min_width(pkg, handle, w):
    assert pkg.lib().mik_dev_dense_block_min_width(handle, int(w)) == 0
