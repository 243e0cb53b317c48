"""The closed form of the FP8 quantizer's gradient with a learned maxval, in numpy (shared by
golden/gen_golden_learn.py and the learned-range tests).

quantize_to_fp8_ste_MM's gradient is that of the clamp min(max(x, lo), maxval), lo = -maxval (signed) or the
constant 0, with ATen's half-and-half split of a tie:

    grad_x = g wx        wx = 1 inside (lo, maxval), 1/2 on a bound, 0 outside or NaN
    grad_maxval = sum g wm over the row of maxval
        wm = +1 (x > maxval), +1/2 (x == maxval), -1 (x < -maxval), -1/2 (x == -maxval) (signed only), else 0
"""
import numpy as np

U = 2.0 ** -10                 # every term g wm of an exact-sum input is a multiple of U
BUDGET = 2.0 ** 22 * U         # ... and sum |g wm| <= BUDGET per row: any summation order gives the same bits
BOUND = 2.0 ** -23             # |kernel - exact| <= BOUND sum |g wm| (double accumulation, one fp32 rounding)


def weights(x, maxval, sign_bits, per_channel):
    """(wx, wm) float32, x's shape; maxval [rows] if per_channel (rows = x.shape[0]) else [1]."""
    x = np.asarray(x, np.float32)
    mx = np.asarray(maxval, np.float32).reshape([-1] + [1] * (x.ndim - 1)) if per_channel else np.float32(maxval[0])
    lo = -mx if sign_bits == 1 else np.zeros_like(mx)
    with np.errstate(invalid="ignore"):
        twice = ((x > lo) & (x < mx)).astype(np.float32) + ((x >= lo) & (x <= mx)).astype(np.float32)
        h = np.float32(1.0) - twice * np.float32(0.5)
        wm = np.where(x >= mx, h, np.where((x <= lo) & (sign_bits == 1), -h, np.float32(0.0)))
    return twice * np.float32(0.5), wm.astype(np.float32)


def closed_form(x, maxval, g, sign_bits, per_channel):
    """grad_x (float32), the float64 sums of the fp32 terms g wm per row [rows], and sum |g wm| per row."""
    wx, wm = weights(x, maxval, sign_bits, per_channel)
    g = np.asarray(g, np.float32)
    with np.errstate(invalid="ignore"):
        gx = (g * wx).astype(np.float32)
        terms = (g * wm).astype(np.float32).astype(np.float64)
    rows = x.shape[0] if per_channel else 1
    terms = terms.reshape(rows, -1)
    return gx, terms.sum(axis=1), np.abs(terms).sum(axis=1)


def bits(a):
    """The fp32 bit patterns of a, a zero's sign cleared: grad_x is a multiplication (-3 * 0 = -0.0, as the
    quantizer's backward always was), where ATen's max / min backward writes +0.0."""
    return (np.asarray(a, np.float32) + np.float32(0.0)).view(np.int32)


def exact_sum_g(rng, shape, amp=127):
    """An upstream gradient whose terms g wm are multiples of U: integers in [-amp, amp] times 2^-9 (a smaller
    amp keeps a long row inside BUDGET)."""
    return (rng.integers(-amp, amp + 1, size=shape).astype(np.float32) * np.float32(2.0 ** -9)).astype(np.float32)
