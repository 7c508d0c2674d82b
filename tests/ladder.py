"""The size ladder of tests/test_gpu_large_reductions.py and the references that do not share code with the oracle's tree.

Every dot, norm and fused sweep ends in the two-level tree of include/mik.h ("Reduction semantics"): level 1 cuts the vector into
m = ceil(n / SEG) segments of SEG = 256 * W * L elements, level 2 lets thread t of 1024 add the segment sums t, t + 1024, ....  The
code that evaluates it changes form with m (csrc/mik_internal.h level2_sum / block_level2_256, the grid-stride loops of
csrc/mik_kernels.h); `ladder` puts one size on each side of every such switch, always with a partial last segment that is not a
multiple of the vector width W.  Nothing is typed in: W, L come from mik_reduce_shape, cap from mik_ctx_info (sweep_grid_cap); the
level-2 width 1024 is the documented one.

`exact_dot` is the reference the derived error bound is checked against -- on the device result and, in the CPU suite, on the oracle's
tree itself, so that device and oracle cannot be wrong together."""
import math

import numpy as np

LEVEL2 = 1024                      # virtual threads of level 2 (include/mik.h)

RUNGS = ["m1024", "m1025", "batch8_minus1", "batch8_plus500", "cap_plus1", "two_cap_plus37", "batch32_minus524", "batch32_plus517",
         "control_16k"]
THREE = ["m1025", "cap_plus1", "batch32_plus517"]     # the short ladder of the secondary entries: tail loop, ragged grid, 32-deep batch


def segment(W, L):
    return 256 * W * L


def ladder(W, L, cap):
    """{rung: (m, n, regime)} for a tree with segments of 256 * W * L elements and a sweep grid capped at `cap` workgroups"""
    SEG = segment(W, L)
    r = SEG // 2 + 3                                   # partial last segment: neither 0 nor a multiple of W
    assert 0 < r < SEG and (W == 1 or r % W != 0)
    ms = {"m1024": LEVEL2, "m1025": LEVEL2 + 1, "batch8_minus1": 8 * LEVEL2 - 1, "batch8_plus500": 8 * LEVEL2 + 500,
          "cap_plus1": cap + 1, "two_cap_plus37": 2 * cap + 37, "batch32_minus524": 31 * LEVEL2 + 500, "batch32_plus517": 32 * LEVEL2 + 517}
    out = {}
    for name in RUNGS:
        if name == "control_16k":
            m, n = 16 * LEVEL2, 16 * LEVEL2 * SEG      # exact multiple of everything: what the 128^3 / 256^3 solves already cover
        else:
            m = ms[name]
            n = (m - 1) * SEG + r
        assert -(-n // SEG) == m
        out[name] = (m, n, regime(m, cap))
    return out


def regime(m, cap):
    """which forms of the level-2 code and of the sweep's grid-stride loop a vector of m segments runs through"""
    t_lo, t_hi = m // LEVEL2, -(-m // LEVEL2)          # segment sums per level-2 thread: the last threads have t_lo, the first t_hi
    parts = []
    if m <= LEVEL2:
        parts.append("consumer-side finalise (block_level2_256)")
    else:
        def trips(t):
            return f"{t // 32}x32+{t % 32 // 8}x8+{t % 8}"
        parts.append("separate finaliser, level2_sum trips " + (trips(t_hi) if t_lo == t_hi else f"{trips(t_hi)} | {trips(t_lo)} split at thread {m % LEVEL2}"))
    passes = -(-m // cap)
    parts.append(f"grid {min(m, cap)} x {passes} pass{'es' if passes > 1 else ''}" + (f", last pass {m - (passes - 1) * cap} workgroups" if passes > 1 and m % cap else ""))
    return "; ".join(parts)


def depth(W, L, m):
    """D: the largest number of additions along any path of the tree from a product to the result -- W * L in a level-1 thread (from +0),
    6 in its wave tree, 3 over the 4 wave sums, ceil(m / 1024) in a level-2 thread (from +0), 6 in its wave tree, 15 over the 16 wave sums"""
    return W * L + 6 + 3 + -(-m // LEVEL2) + 6 + 15


def gamma(k, dtype):
    e = float(np.finfo(dtype).eps)
    return k * e / (1 - k * e)


def exact_dot(x, y, use_fsum=False):
    """(s, a, err): s = sum x_i y_i and a = sum |x_i y_i| as np.longdouble, |s - the true sum| <= err.

    float32 data: the float64 products are exact (24 + 24 bits).  float64 data: the product is split without error into p + e
    (Veltkamp / Dekker; no FMA involved).  use_fsum: math.fsum adds these exactly (err = one rounding of the result).  Otherwise
    numpy's pairwise sums, for float64 data in np.longdouble (64-bit significand where the platform has one), for float32 data in
    float64: fewer than 64 roundings of relative size eps(accumulator) along any path, so err = 64 * eps(accumulator) * a -- at least
    three decimal orders below the bounds it serves (eps(longdouble) / eps(float64), eps(float64) / eps(float32))."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    ld = np.longdouble
    acc = ld if x.dtype == np.float64 else np.float64
    s, a = ld(0), ld(0)
    terms = []
    step = 1 << 22
    for i in range(0, x.size, step):
        xs, ys = x[i:i + step].astype(np.float64), y[i:i + step].astype(np.float64)
        p = xs * ys
        parts = [p]
        if x.dtype == np.float64:
            def split(v):
                t = 134217729.0 * v                    # 2^27 + 1
                hi = t - (t - v)
                return hi, v - hi
            xh, xl = split(xs)
            yh, yl = split(ys)
            parts.append(((xh * yh - p) + xh * yl + xl * yh) + xl * yl)
        a += ld(np.abs(p).sum())
        if use_fsum:
            terms.extend(parts)
        else:
            for q in parts:
                s += ld(q.astype(acc).sum())
    a = a * (1 + 64 * ld(np.finfo(np.float64).eps))     # a was added up in float64 (pairwise): make it an upper bound
    if use_fsum:
        f = math.fsum(np.concatenate(terms)) if terms else 0.0
        return ld(f), a, ld(abs(f)) * ld(2.0 ** -53)
    return s, a, 64 * ld(np.finfo(acc).eps) * a


def dot_bound(W, L, m, dtype, a, err):
    """|tree - exact| <= gamma_{D+1} * sum |x_i y_i| (+ the reference's own error): one rounding for the product, at most D for the additions"""
    return np.longdouble(gamma(depth(W, L, m) + 1, dtype)) * a + err


def nrm_bound(W, L, m, dtype, s, err):
    """t = tree sum of squares = s (1 + th), |th| <= g = gamma_{D+1}; |sqrt(1 + th) - 1| <= g / 2 * (1 + g); the correctly rounded sqrt adds eps / 2:
    |nrm - sqrt(s)| <= sqrt(s) * (g + eps) / 2 * (1 + g) (+ the reference's error through the square root)"""
    g = np.longdouble(gamma(depth(W, L, m) + 1, dtype))
    e = np.longdouble(np.finfo(dtype).eps)
    root = np.sqrt(s)
    return root * (g + e) / 2 * (1 + g) + (err / (2 * root) if root > 0 else 0) + root * np.longdouble(np.finfo(np.longdouble).eps)
