#!/usr/bin/env python
"""Golden-vector generator for the FP8 quantizer's straight-through gradient (TEST INFRASTRUCTURE ONLY).

Like gen_golden.py it runs only where the reference checkout is mounted, imports the reference UNMODIFIED
(through gen_golden's import shim) and writes a fixture next to itself:

  ste_quant.npz   per case: the input x, the maxval, (n_bits, mantissa bits, sign bits, per channel), and
                  grad -- d sum(quantize_to_fp8_ste_MM(x)) / dx as the reference's own autograd gives it
                  (fp8_quantizer.py:97-173: the clamp's mask, the rounding straight-through, the scales
                  detached), at fixed maxval.

Cases: E4M3, E3M4 and E5M2 (mantissa 3, 4, 2), signed and unsigned, per tensor and per channel, 4 x 84 = 336
inputs each (12 cases, 4032 inputs): normal values scaled so that about a fifth fall outside the clamp, with
some exact zeros.  No input sits on a clamp bound (|x| == maxval, or x == 0 for an unsigned quantizer -- ATen
splits the gradient of a max / min tie in half): the generator asserts it, so the gradient is a 0 / 1 mask.

Usage:  python tests/golden/gen_golden_ste.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402,F401  (installs the import shim, puts the reference on sys.path)
from quantization.quantizers.fp8_quantizer import quantize_to_fp8_ste_MM  # noqa: E402

ROWS, INNER = 4, 84


def main():
    rng = np.random.default_rng(20261020)
    data, total = {}, 0
    for name, mbits in (("e4m3", 3), ("e3m4", 4), ("e5m2", 2)):
        for sign_bits in (1, 0):
            for per_channel in (False, True):
                x = rng.standard_normal((ROWS, INNER)).astype(np.float32) * np.float32(1.6)
                if sign_bits == 1:
                    x[rng.random((ROWS, INNER)) < 0.05] = 0.0  # (an unsigned quantizer's lower bound is 0: a tie)
                maxval = np.array([2.0], np.float32) if not per_channel else np.array([0.75, 1.5, 2.5, 4.0], np.float32)
                mx = maxval.reshape(-1, 1) if per_channel else maxval
                lo = -mx if sign_bits == 1 else np.zeros_like(mx)
                assert not ((x == mx) | (x == lo)).any()
                xt = torch.from_numpy(x).requires_grad_(True)
                y, _ = quantize_to_fp8_ste_MM(xt, 8, torch.from_numpy(maxval), torch.tensor([float(mbits)]), sign_bits)
                y.sum().backward()
                g = xt.grad.numpy()
                assert set(np.unique(g)) <= {0.0, 1.0}
                key = f"{name}_s{sign_bits}_{'pc' if per_channel else 'pt'}"
                data[key + "/x"] = x
                data[key + "/maxval"] = maxval
                data[key + "/meta"] = np.array([8, mbits, sign_bits, int(per_channel)], np.int64)
                data[key + "/grad"] = g.astype(np.float32)
                data[key + "/y"] = y.detach().numpy()
                total += x.size
                print(key, "passes", int(g.sum()), "of", x.size)
    path = os.path.join(HERE, "ste_quant.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", total, "inputs")


if __name__ == "__main__":
    main()
