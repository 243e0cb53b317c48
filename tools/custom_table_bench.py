#!/usr/bin/env python
"""Op-level time of a custom error table against the built-in one.

    python tools/custom_table_bench.py [--reps 30] [--warmup 5] [--batch 64]

Two layers, each with the built-in E4M3 table and with T_pos[ma][mb] = (ma + 2 mb + 3) % 4 (entries 0..3, a
cruder truncating multiplier's): ResNet-18 layer2 conv2 (128 -> 128 channels, 3x3, 28x28) and MobileNetV2's
3x3 depthwise at 96 channels, 56x56.  HIP events around each launch on the current stream, the median of
--reps launches after --warmup; one JSON line per (layer, table) with the path counters of the timed
launches.  FP8A_LIB_PATH selects another build of libfp8approx.so (the parent commit's, for the A/B).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_POS = [[(ma + 2 * mb + 3) % 4 for mb in range(8)] for ma in range(8)]
LAYERS = [("r18.layer2.conv2", 128, 128, 3, 1, 1, 28, 1), ("mbv2.dw96", 96, 96, 3, 1, 1, 56, 96)]


def grid(rng, shape, bias, zero_frac):
    expo = rng.integers(7, 16, size=shape)
    mant = rng.integers(0, 8, size=shape)
    v = np.ldexp(1.0 + mant / 8.0, expo - bias) * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(shape) < zero_frac] = 0.0
    return torch.from_numpy(v.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.error_tables import get_error_table_NN, load_error_table
    dev = "cuda:0"
    fl = fa.make_flags(with_approx=True, with_s2nn2s_opt=True, quant_btw_mult_accu=True)
    bA, bB = 11, 16
    bR = bA + bB - 17  # every term inside the scaled-e4m3 range (as tools/gemm_bench.py)
    tables = (("builtin", get_error_table_NN(4, 3, False, 3)), ("T_pos", load_error_table(T_POS, 3)))
    rng = np.random.default_rng(0)
    for name, cin, cout, k, s, p, h, groups in LAYERS:
        x = grid(rng, (args.batch, cin, h, h), bA, 0.5).to(dev)
        w = grid(rng, (cout, cin // groups, k, k), bB, 0.0).to(dev)
        bW = torch.full((cout,), bB, dtype=torch.int32, device=dev)
        for tname, tab in tables:
            def run():
                return fa.approx_conv2d(x, w, 4, 3, bA, bW, bR, tab, flags=fl, stride=(s, s), padding=(p, p),
                                        groups=groups)
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            _lib.path_stats(reset=True)
            _lib.fallback_stats(reset=True)
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            ho = (h + 2 * p - k) // s + 1
            macs = args.batch * ho * ho * cout * (cin // groups) * k * k
            med = statistics.median(times)
            print(json.dumps(dict(layer=name, table=tname, batch=args.batch, median_ms=round(med, 4),
                                  min_ms=round(min(times), 4), max_ms=round(max(times), 4), reps=args.reps,
                                  gmacs_per_s=round(macs / med / 1e6, 1),
                                  paths={k_: v for k_, v in _lib.path_stats(reset=True).items() if v},
                                  fallbacks=_lib.fallback_stats(reset=True), lib=os.path.basename(os.path.dirname(
                                      _lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH))), flush=True)


if __name__ == "__main__":
    main()
