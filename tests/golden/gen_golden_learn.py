#!/usr/bin/env python
"""Golden-vector generator for the FP8 quantizer's gradient with a LEARNED maxval (TEST INFRASTRUCTURE ONLY).

Like gen_golden_ste.py it runs only where the reference checkout is mounted, imports the reference UNMODIFIED
(through gen_golden's import shim) and writes a fixture next to itself:

  learn_maxval.npz  per case: the input x, the maxval, the upstream gradient g, (n_bits, mantissa bits, sign
                    bits, per channel), and grad_x / grad_maxval -- what the reference's own autograd gives
                    for quantize_to_fp8_ste_MM(x, maxval).backward(g) with maxval.requires_grad_()
                    (fp8_quantizer.py:97-173: the clamp's gradient, the bias rounded, the scales detached).

Cases: E4M3, E3M4 and E5M2 (mantissa 3, 4, 2), signed and unsigned, per tensor and per channel, 5 x 333 inputs
each (12 cases): about a fifth of the inputs outside the clamp, about 3 % exactly on +maxval or -maxval of their
row (ATen splits the gradient of a max / min tie in half) and, for the unsigned cases, about 3 % exact zeros.

Exact sums: torch's reduction order is not specified, so g is an integer in [-127, 127] times 2^-9; every term
g wm is then a multiple of u = 2^-10 and the generator asserts sum |g wm| <= 2^22 u per row: any summation
order, in fp32 or double, gives the same bits.  It also asserts that the reference's grad_x and grad_maxval
equal the closed form (tests/learn_ranges_ref.py) bit for bit.

Usage:  python tests/golden/gen_golden_learn.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402,F401  (installs the import shim, puts the reference on sys.path)
from quantization.quantizers.fp8_quantizer import quantize_to_fp8_ste_MM  # noqa: E402

import learn_ranges_ref as lr  # noqa: E402

ROWS, INNER = 5, 333


def main():
    rng = np.random.default_rng(20261021)
    data, total = {}, 0
    for name, mbits in (("e4m3", 3), ("e3m4", 4), ("e5m2", 2)):
        for sign_bits in (1, 0):
            for per_channel in (False, True):
                maxval = np.array([0.75, 1.5, 2.5, 4.0, 2.0] if per_channel else [2.0], np.float32)
                mx = np.broadcast_to(maxval.reshape(-1, 1), (ROWS, INNER)) if per_channel else \
                    np.full((ROWS, INNER), maxval[0], np.float32)
                z = rng.standard_normal((ROWS, INNER)).astype(np.float32)
                if sign_bits == 1:  # P(|z| > 1.28) = 0.2
                    x = z * mx / np.float32(1.28)
                else:  # 5 % negative, 16 % of the rest above maxval
                    x = np.abs(z) * mx / np.float32(1.405)
                    x[rng.random((ROWS, INNER)) < 0.05] *= np.float32(-1.0)
                    x[rng.random((ROWS, INNER)) < 0.03] = 0.0
                tie = rng.random((ROWS, INNER)) < 0.03
                side = np.where((rng.random((ROWS, INNER)) < 0.5) & (sign_bits == 1), np.float32(-1.0), np.float32(1.0))
                x = np.where(tie, side * mx, x).astype(np.float32)
                g = lr.exact_sum_g(rng, (ROWS, INNER))
                gx, gm64, budget = lr.closed_form(x, maxval, g, sign_bits, per_channel)
                assert (budget <= lr.BUDGET).all(), budget / lr.U
                xt = torch.from_numpy(x.copy()).requires_grad_(True)
                mt = torch.from_numpy(maxval.copy()).requires_grad_(True)
                y, _ = quantize_to_fp8_ste_MM(xt, 8, mt, torch.tensor([float(mbits)]), sign_bits)
                y.backward(torch.from_numpy(g))
                ref_gx, ref_gm = xt.grad.numpy(), mt.grad.numpy()
                # (the sign of a zero aside: the closed form multiplies, -3 * 0 = -0.0, ATen's backward fills +0.0)
                assert np.array_equal(lr.bits(ref_gx), lr.bits(gx))
                assert ref_gm.shape == maxval.shape
                assert np.array_equal(ref_gm.view(np.int32), gm64.astype(np.float32).view(np.int32))
                key = f"{name}_s{sign_bits}_{'pc' if per_channel else 'pt'}"
                data[key + "/x"] = x
                data[key + "/maxval"] = maxval
                data[key + "/g"] = g
                data[key + "/meta"] = np.array([8, mbits, sign_bits, int(per_channel)], np.int64)
                data[key + "/grad_x"] = ref_gx.astype(np.float32)
                data[key + "/grad_maxval"] = ref_gm.astype(np.float32)
                total += x.size
                wx, wm = lr.weights(x, maxval, sign_bits, per_channel)
                print(key, "outside", float((wx == 0).mean()), "ties", float((wx == 0.5).mean()),
                      "budget / u 2^%.1f" % np.log2(budget.max() / lr.U), "grad_maxval", ref_gm)
    path = os.path.join(HERE, "learn_maxval.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", total, "inputs")


if __name__ == "__main__":
    main()
