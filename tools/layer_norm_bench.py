#!/usr/bin/env python
"""Times the layer norm block (csrc/layer_norm.h) against the torch ops it replaces, on one GPU.

    python tools/layer_norm_bench.py [--output profiles/layer_norm/layer_norm_bench.json] [--reps 30]

For x [B * 197, 768] (ViT-B/16's token rows), B = 16 and 64, eps = 1e-12, with the input quantizer (8 bits, M = 3,
signed, maxval 4):
  * forward: approx_ops.layer_norm against fp8_fake_quantize and F.layer_norm (two passes, four trips through HBM);
  * backward: approx_ops.layer_norm_backward against the autograd of the recorded FPQuantizer (ste_backward) and
    F.layer_norm forward.
The two sides alternate inside the timed loop; HIP events around each call, warm-up, at least 30 repeats; median, min
and max in ms.  Beside each: the byte floor, passes x tensor bytes at the 6.3 TB/s a float4 copy reaches -- 2 passes
forward (read x, write y), 3 backward (read x and g, write dx).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd.approx_ops import fp8_fake_quantize, layer_norm, layer_norm_backward  # noqa: E402
from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer  # noqa: E402

DEV = "cuda:0"
HBM = 6.3e12  # achievable bytes / s (a float4 copy)
N, EPS = 768, 1e-12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), reps=len(ts))


def rows(reps):
    out = []
    for batch in (16, 64):
        x = torch.randn((batch * 197, N), device=DEV) * 3
        g = torch.randn_like(x)
        gamma, beta = torch.randn(N, device=DEV), torch.randn(N, device=DEV)
        mx = torch.tensor([4.0], device=DEV)
        q = (mx, 8, 3, 1)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        _, mean, rstd, _ = layer_norm(x, gamma, beta, EPS, q)
        fq = FPQuantizer(n_bits=8, mantissa_bits=3, maxval=4.0)
        fq.ste_backward = True
        leaves = [x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()]
        recorded = F.layer_norm(fq(leaves[0]), (N,), leaves[1], leaves[2], EPS)
        calls = dict(
            forward_fused=lambda: layer_norm(x, gamma, beta, EPS, q, out=y),
            forward_torch=lambda: F.layer_norm(fp8_fake_quantize(x, mx, 8, 3)[0], (N,), gamma, beta, EPS),
            backward_fused=lambda: layer_norm_backward(x, g, gamma, mean, rstd, q, out=dx),
            backward_torch=lambda: torch.autograd.grad(recorded, leaves, g, retain_graph=True))
        for fn in list(calls.values()) * 3:
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                ts[k].append(event_ms(fn))
        nbytes = 4 * x.numel()
        row = dict(shape=list(x.shape), tensor_bytes=nbytes, **{k: summary(v) for k, v in ts.items()},
                   forward_floor_ms=2 * nbytes / HBM * 1e3, backward_floor_ms=3 * nbytes / HBM * 1e3)
        for d in ("forward", "backward"):
            row[f"{d}_torch_over_fused"] = row[f"{d}_torch"]["median_ms"] / row[f"{d}_fused"]["median_ms"]
            row[f"{d}_share_of_floor"] = row[f"{d}_floor_ms"] / row[f"{d}_fused"]["median_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
        del x, g, y, dx, leaves, recorded
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--output", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("layer_norm_bench needs a HIP device")
    out = dict(layer_norm=rows(max(30, args.reps)))
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
