#!/usr/bin/env python
"""grad_bmm (fp8a_grad_bmm) against torch's fp32 product on the backward's own shapes, same operands.

    python tools/grad_bench.py [--iters 30] [--warmup 5] [--out FILE.jsonl]

HIP events around each call, median of --iters after --warmup.  Shapes at batch 64: ResNet-18 layer2 conv2
(128 -> 128, 3 x 3, 28 x 28) data and weight gradients, ViT-B/16 fc1 (768 -> 3072, 197 tokens) both products,
and attention's four (12 heads, d = 64).  A is a normal fp32 gradient, B bf16-exact (what a saved FP8 operand
is), so no tile is recomputed (checked).  One JSON line per shape: both medians, their ratio, the TFLOP/s of
the useful fp32 product (2 M N K per item), and the largest |difference| against torch over the largest |value|.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd import _lib  # noqa: E402
from fp8_quantization_amd.approx_ops import grad_bmm  # noqa: E402

DEV = "cuda:0"


def bf16_exact(t):
    return (t.view(torch.int32) & -65536).view(torch.float32)


def med_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def shapes():
    g = torch.Generator(device=DEV).manual_seed(0)

    def rn(*s):
        return torch.randn(s, device=DEV, generator=g)
    Bn, C, Ln, Kg = 64, 128, 784, 1152
    dy, w, cols = rn(Bn, C, Ln), bf16_exact(rn(C, Kg)), bf16_exact(rn(Bn, Ln, Kg))
    yield ("r18.layer2.conv2 dgrad", lambda: grad_bmm(dy.transpose(1, 2), w.unsqueeze(0).expand(Bn, C, Kg)),
           lambda: torch.matmul(dy.transpose(1, 2), w), Bn * Ln * C * Kg)
    yield ("r18.layer2.conv2 wgrad", lambda: grad_bmm(dy.transpose(0, 1), cols, k2=True),
           lambda: torch.einsum("bol,blk->ok", dy, cols), Bn * Ln * C * Kg)
    T, D, F_ = 64 * 197, 768, 3072
    dyl, wl, xl = rn(T, F_), bf16_exact(rn(F_, D)), bf16_exact(rn(T, D))
    yield ("vit.fc1 dX", lambda: grad_bmm(dyl, wl), lambda: torch.matmul(dyl, wl), T * F_ * D)
    yield ("vit.fc1 dW", lambda: grad_bmm(dyl.t(), xl), lambda: torch.matmul(dyl.t(), xl), T * F_ * D)
    B, H, S, d = 64, 12, 197, 64
    ds, dc = rn(B, H, S, S), rn(B, H, S, d)
    q, k, v = (bf16_exact(rn(B, H, S, d)) for _ in range(3))
    p = bf16_exact(rn(B, H, S, S).softmax(-1))
    yield ("attn dQ = dS K", lambda: grad_bmm(ds, k), lambda: torch.matmul(ds, k), B * H * S * S * d)
    yield ("attn dK^T = dS^T Q", lambda: grad_bmm(ds.transpose(-1, -2), q),
           lambda: torch.matmul(ds.transpose(-1, -2), q), B * H * S * S * d)
    yield ("attn dP = dC V^T", lambda: grad_bmm(dc, v.transpose(-1, -2)),
           lambda: torch.matmul(dc, v.transpose(-1, -2)), B * H * S * S * d)
    yield ("attn dV^T = dC^T P", lambda: grad_bmm(dc.transpose(-1, -2), p),
           lambda: torch.matmul(dc.transpose(-1, -2), p), B * H * S * S * d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []
    for name, ours, theirs, macs in shapes():
        _lib.grad_stats(reset=True)
        got, ref = ours(), theirs()
        rec = _lib.grad_stats(reset=True)["recomputed"]
        dev = float((got - ref).abs().max() / ref.abs().max())
        t_ours, t_torch = med_ms(ours, a.iters, a.warmup), med_ms(theirs, a.iters, a.warmup)
        lines.append(dict(shape=name, grad_bmm_ms=t_ours, torch_fp32_ms=t_torch, ratio_vs_torch=t_ours / t_torch,
                          grad_bmm_tflops=2e-9 * macs / t_ours, torch_tflops=2e-9 * macs / t_torch,
                          recomputed_tiles=rec, max_diff_over_max=dev))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
