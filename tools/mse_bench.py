#!/usr/bin/env python
"""Times the FP8 MSE range search on one GPU.

    python tools/mse_bench.py [--output profiles/mse_measure.json]

Three tensors (the ResNet-18 stem activation at calibration batch 64, a layer4 weight per channel, a
ViT-B/16 fc1 input at batch 64), widths [3] and 1..6: the literal estimator path (one fake
quantization per candidate), the fused estimator path and the bare kernel call, the fused ones with
"mse_group" 0 and 1.  HIP events around each call, warm-up, several repeats; median, min and max.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd import _lib  # noqa: E402
from fp8_quantization_amd.approx_ops import fp8_mse_losses  # noqa: E402
from fp8_quantization_amd.quantization import FPQuantizer, RangeEstimators, mse_search_grid  # noqa: E402

DEV = "cuda:0"


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), reps=reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--output", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    tensors = [
        ("resnet18_stem_act_b64 [64,64,112,112] per tensor",
         lambda: torch.relu(torch.randn(64, 64, 112, 112, device=DEV)), False),
        ("resnet18_layer4_weight [512,512,3,3] per channel", lambda: torch.randn(512, 512, 3, 3, device=DEV) * 0.02, True),
        ("vit_b16_fc1_input_b64 [64,197,768] per tensor", lambda: torch.randn(64, 197, 768, device=DEV), False),
    ]
    out = []
    for name, make, per_channel in tensors:
        x = make()
        grid = mse_search_grid(x, per_channel)
        for wname, msearch, widths in (("M=3", False, [3]), ("M=1..6", True, [1, 2, 3, 4, 5, 6])):
            row = dict(tensor=name, widths=wname, elements=x.numel(), candidates=111 * len(widths))

            def estimator(fused):
                q = FPQuantizer(n_bits=8, per_channel=per_channel, mantissa_bits=3, maxval=None, set_maxval=True,
                                mse_include_mantissa_bits=msearch)
                est = RangeEstimators.MSE.cls(per_channel=per_channel, quantizer=q, fused=fused)

                def run():
                    est.reset()
                    est(x)
                return run
            row["literal_estimator"] = timed(estimator(False), 1, 3 if x.numel() > 2 ** 25 else 5)
            for g in (0, 1):
                old = _lib.set_option("mse_group", g)
                row[f"fused_estimator_group{g}"] = timed(estimator(True), 2, 10)
                row[f"kernel_group{g}"] = timed(lambda: fp8_mse_losses(x, grid, widths, 8, 1, per_channel), 3, 20)
                _lib.set_option("mse_group", old)
            lit = row["literal_estimator"]["median_ms"]
            for g in (0, 1):
                row[f"literal_over_fused_estimator_group{g}"] = lit / row[f"fused_estimator_group{g}"]["median_ms"]
                row[f"elem_cand_per_s_group{g}"] = x.numel() * row["candidates"] / (row[f"kernel_group{g}"]["median_ms"] * 1e-3)
            print(json.dumps(row), flush=True)
            out.append(row)
        del x, grid
        torch.cuda.empty_cache()
    if args.output:
        with open(args.output, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
