#!/usr/bin/env python
"""The fake quantizer's fused training pair (fp8a_fq_train_forward + fp8a_fq_train_backward)
against the composition it replaces, on the same tensors:

    python tools/fq_train_bench.py [--shapes act,stem,weight,dw,vit] [--reps 30] [--warmup 5]

Comparator: the quantizer's recorded forward and backward as they stood before the fused pair -- the quantize
kernel plus the torch expressions that build the one-byte mask, and g * (mask * 0.5) -- plus the torch
expression for grad_maxval.  There was no maxval gradient before, so that expression is the only comparator
there is.  HIP events, median of --reps after --warmup.  Bytes: forward 4 + 4 + 1 per element (x, y, code),
backward 4 + 1 + 4 (g, code, grad_x); the fraction is of 6.3 TB/s, the achievable HBM rate.
One JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12
SHAPES = {
    "act": ((64, 64, 56, 56), False),       # ResNet-18 layer1 activation
    "stem": ((64, 3, 224, 224), False),     # stem input
    "weight": ((512, 512, 3, 3), True),     # per-channel weight
    "dw": ((960, 1, 3, 3), True),           # MobileNetV2 depthwise weight
    "vit": ((12608, 3072), False),          # ViT fc1 activation
}


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
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
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from fp8_quantization_amd.approx_ops import (fp8_fake_quantize, fp8_fake_quantize_backward,
                                                 fp8_fake_quantize_train)
    dev = "cuda:0"
    for name in args.shapes.split(","):
        shape, per_row = SHAPES[name]
        rows = shape[0] if per_row else 1
        x = torch.randn(shape, device=dev)
        g = torch.randn(shape, device=dev)
        mxv = x.reshape(rows, -1).abs().amax(dim=1) * 0.6  # (about a fifth of a normal tensor beyond the clamp)
        mx = mxv.view([-1] + [1] * (x.dim() - 1)) if per_row else mxv
        n = x.numel()
        state = {}

        def fused_fwd():
            state["code"] = fp8_fake_quantize_train(x, mxv, 8, 3, 1, per_row)[2]

        def fused_bwd():
            fp8_fake_quantize_backward(g, state["code"], rows, 1)

        def old_fwd():
            fp8_fake_quantize(x, mxv, 8, 3, 1, per_row)
            lo = -mx
            state["twice"] = ((x > lo) & (x < mx)).to(torch.uint8) + ((x >= lo) & (x <= mx)).to(torch.uint8)

        def old_bwd():
            g * (state["twice"].to(g.dtype) * 0.5)
            lo = -mx
            wm = (x > mx).to(g.dtype) + 0.5 * (x == mx).to(g.dtype) - (x < lo).to(g.dtype) - 0.5 * (x == lo).to(g.dtype)
            (g * wm).reshape(rows, -1).sum(dim=1)

        t = {k: _median_ms(f, args.reps, args.warmup) for k, f in
             (("fused_fwd", fused_fwd), ("fused_bwd", fused_bwd), ("old_fwd", old_fwd), ("old_bwd", old_bwd))}
        rec = dict(shape=name, dims=list(shape), per_row=per_row, elements=n)
        for k, v in t.items():
            rec[k + "_ms"] = round(v, 4)
        for k in ("fused_fwd", "fused_bwd"):
            rate = 9.0 * n / (t[k] * 1e-3)
            rec[k + "_tbs"] = round(rate / 1e12, 3)
            rec[k + "_hbm_fraction"] = round(rate / HBM, 3)
        rec["speedup"] = round((t["old_fwd"] + t["old_bwd"]) / (t["fused_fwd"] + t["fused_bwd"]), 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
