"""What the bindings of the C checkers under tests/dense_ref/ share (dense_lu_host.py, dense_chol_host.py): the build of a checker, the
pointer of an array, and the bitwise comparison `same_bits` of device values with the checker's.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [np.float64, np.float32, np.complex128, np.complex64]


def build_ref(name, outdir, *libs):
    """tests/dense_ref/`name`.c with gcc -O2 -ffp-contract=off (no product is ever fused into a difference) -> a shared object in
    `outdir`, loaded."""
    so = os.path.join(str(outdir), name + ".so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "dense_ref", name + ".c"), "-o", so, *libs])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _reals(a):
    """a floating array as it is, a complex one as its (re, im) pairs"""
    return np.ascontiguousarray(np.stack([a.real, a.imag], axis=-1)) if a.dtype.kind == "c" else np.ascontiguousarray(a)


def _differs(got, want):
    """where `same_bits` fails, over the array of real components; None when shape or dtype differ or the dtype is not one of DTYPES"""
    if got.shape != want.shape or got.dtype != want.dtype or got.dtype not in DTYPES:
        return None
    g, w = _reals(got), _reals(want)
    u = np.uint64 if g.dtype == np.float64 else np.uint32
    gn, wn = np.isnan(g), np.isnan(w)
    return (gn != wn) | (~gn & ~wn & (g.view(u) != w.view(u)))


def same_bits(got, want):
    """Same shape and dtype, NaN in exactly the same positions (per component of a complex), and everywhere else equal as unsigned
    integers of the component width, so -0.0 differs from +0.0.  The payload and the sign of a NaN are not compared: an x86 host and
    the device generate different default NaNs, and the contract does not speak of them."""
    d = _differs(np.asarray(got), np.asarray(want))
    return d is not None and not bool(d.any())


def first_difference(got, want):
    """up to four indices (into the array of real components) at which `same_bits` fails, for an assertion message"""
    got, want = np.asarray(got), np.asarray(want)
    d = _differs(got, want)
    return (got.shape, got.dtype, want.shape, want.dtype) if d is None else np.argwhere(d)[:4].tolist()
