#!/usr/bin/env python
"""Times the attention softmax block (csrc/attn_softmax.h) against the torch ops it replaces, on one GPU.

    python tools/attn_softmax_bench.py [--output profiles/attention_softmax/attn_softmax_bench.json] [--reps 30]

For scores [B, 12, 197, 197] (ViT-B/16), B = 16 and 64, with the PV operand's quantizer (8 bits, M = 3, unsigned,
maxval 1):
  * forward: approx_ops.attention_softmax against scores * scale, torch.softmax and fp8_fake_quantize (three passes);
  * backward: approx_ops.attention_softmax_backward against the autograd of the recorded scale, softmax and
    FPQuantizer (ste_backward) forward.
The two sides alternate inside the timed loop; HIP events around each call, warm-up, at least 30 repeats; median, min
and max in ms.  Beside each: the byte floor, passes x tensor bytes at the 6.3 TB/s a float4 copy reaches -- 2 passes
forward (read s, write y), 3 backward (read s and g, write ds).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd.approx_ops import (attention_softmax, attention_softmax_backward,  # noqa: E402
                                             fp8_fake_quantize)
from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer  # noqa: E402

DEV = "cuda:0"
HBM = 6.3e12  # achievable bytes / s (a float4 copy)
SCALE = 64 ** -0.5


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
        s = torch.randn((batch, 12, 197, 197), device=DEV) * 8
        g = torch.randn_like(s)
        mx = torch.tensor([1.0], device=DEV)
        q = (mx, 8, 3, 0)
        y, ds = torch.empty_like(s), torch.empty_like(s)
        fq = FPQuantizer(n_bits=8, mantissa_bits=3, maxval=1.0)
        fq.sign_bits, fq.ste_backward = 0, True
        sg = s.clone().requires_grad_()
        recorded = fq(torch.softmax(sg * SCALE, dim=-1))
        calls = dict(
            forward_fused=lambda: attention_softmax(s, SCALE, q, out=y),
            forward_torch=lambda: fp8_fake_quantize(torch.softmax(s * SCALE, dim=-1), mx, 8, 3, sign_bits=0),
            backward_fused=lambda: attention_softmax_backward(s, g, SCALE, q, out=ds),
            backward_torch=lambda: torch.autograd.grad(recorded, sg, g, retain_graph=True))
        for fn in list(calls.values()) * 3:
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                ts[k].append(event_ms(fn))
        nbytes = 4 * s.numel()
        row = dict(shape=list(s.shape), tensor_bytes=nbytes, **{k: summary(v) for k, v in ts.items()},
                   forward_floor_ms=2 * nbytes / HBM * 1e3, backward_floor_ms=3 * nbytes / HBM * 1e3)
        for d in ("forward", "backward"):
            row[f"{d}_torch_over_fused"] = row[f"{d}_torch"]["median_ms"] / row[f"{d}_fused"]["median_ms"]
            row[f"{d}_share_of_floor"] = row[f"{d}_floor_ms"] / row[f"{d}_fused"]["median_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
        del s, g, y, ds, sg, recorded
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--output", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("attn_softmax_bench needs a HIP device")
    out = dict(attention_softmax=rows(max(30, args.reps)))
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
