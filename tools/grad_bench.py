#!/usr/bin/env python
"""grad_bmm (fp8a_grad_bmm) against torch's fp32 product on the backward's own shapes, same operands.

    python tools/grad_bench.py [--iters 30] [--warmup 5] [--split-k 1,2,4,auto] [--out FILE.jsonl]

HIP events around each call, median of --iters after --warmup.  Shapes at batch 64: ResNet-18 layer2 conv2
(128 -> 128, 3 x 3, 28 x 28) data and weight gradients, ViT-B/16 fc1 (768 -> 3072, 197 tokens) both products,
and attention's four (12 heads, d = 64).  A is a normal fp32 gradient, B bf16-exact (what a saved FP8 operand
is), so no tile is recomputed (checked).  One JSON line per shape: both medians, their ratio, the TFLOP/s of
the useful fp32 product (2 M N K per item), and the largest |difference| against torch over the largest |value|.
Without --split-k the run and its lines are as they always were (the eight shapes, split_k = 1).
--split-k: one value or a comma list of grad_bmm's split_k (an int or auto), the sweep of DESIGN.md §3ah: the
shapes then also hold the weight gradients of ResNet-18's conv1 (64 x 147, K = 64 x 12544) and layer4.1.conv2
(512 x 4608, K = 64 x 49), and there is one line per shape and value, with the splits "auto" resolved to, the
product pass's workgroups and the time relative to the latest split_k = 1 of the same shape.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd import _lib  # noqa: E402
from fp8_quantization_amd.approx_ops import grad_bmm, grad_split_auto  # noqa: E402

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


def shapes(sweep=False):
    """(name, grad_bmm call taking split_k, torch's call, MACs, (nb, M, N, K) of the launch); sweep: the two more
    weight gradients"""
    g = torch.Generator(device=DEV).manual_seed(0)

    def rn(*s):
        return torch.randn(s, device=DEV, generator=g)
    Bn, C, Ln, Kg = 64, 128, 784, 1152
    dy, w, cols = rn(Bn, C, Ln), bf16_exact(rn(C, Kg)), bf16_exact(rn(Bn, Ln, Kg))
    yield ("r18.layer2.conv2 dgrad", lambda sk=1: grad_bmm(dy.transpose(1, 2), w.unsqueeze(0).expand(Bn, C, Kg), split_k=sk),
           lambda: torch.matmul(dy.transpose(1, 2), w), Bn * Ln * C * Kg, (Bn, Ln, Kg, C))
    yield ("r18.layer2.conv2 wgrad", lambda sk=1: grad_bmm(dy.transpose(0, 1), cols, k2=True, split_k=sk),
           lambda: torch.einsum("bol,blk->ok", dy, cols), Bn * Ln * C * Kg, (1, C, Kg, Bn * Ln))
    T, D, F_ = 64 * 197, 768, 3072
    dyl, wl, xl = rn(T, F_), bf16_exact(rn(F_, D)), bf16_exact(rn(T, D))
    yield ("vit.fc1 dX", lambda sk=1: grad_bmm(dyl, wl, split_k=sk), lambda: torch.matmul(dyl, wl), T * F_ * D, (1, T, D, F_))
    yield ("vit.fc1 dW", lambda sk=1: grad_bmm(dyl.t(), xl, split_k=sk), lambda: torch.matmul(dyl.t(), xl), T * F_ * D,
           (1, F_, D, T))
    B, H, S, d = 64, 12, 197, 64
    ds, dc = rn(B, H, S, S), rn(B, H, S, d)
    q, k, v = (bf16_exact(rn(B, H, S, d)) for _ in range(3))
    p = bf16_exact(rn(B, H, S, S).softmax(-1))
    yield ("attn dQ = dS K", lambda sk=1: grad_bmm(ds, k, split_k=sk), lambda: torch.matmul(ds, k), B * H * S * S * d,
           (B * H, S, d, S))
    yield ("attn dK^T = dS^T Q", lambda sk=1: grad_bmm(ds.transpose(-1, -2), q, split_k=sk),
           lambda: torch.matmul(ds.transpose(-1, -2), q), B * H * S * S * d, (B * H, S, d, S))
    yield ("attn dP = dC V^T", lambda sk=1: grad_bmm(dc, v.transpose(-1, -2), split_k=sk),
           lambda: torch.matmul(dc, v.transpose(-1, -2)), B * H * S * S * d, (B * H, S, S, d))
    yield ("attn dV^T = dC^T P", lambda sk=1: grad_bmm(dc.transpose(-1, -2), p, split_k=sk),
           lambda: torch.matmul(dc.transpose(-1, -2), p), B * H * S * S * d, (B * H, d, S, S))

    def wgrad(name, cout, kg, ln):  # a convolution's weight gradient at batch 64: [cout x 64 ln] @ [64 ln x kg]
        dyc, colc = rn(Bn, cout, ln), bf16_exact(rn(Bn, ln, kg))
        return (name, lambda sk=1: grad_bmm(dyc.transpose(0, 1), colc, k2=True, split_k=sk),
                lambda: torch.einsum("bol,blk->ok", dyc, colc), Bn * ln * cout * kg, (1, cout, kg, Bn * ln))
    if sweep:
        yield wgrad("r18.conv1 wgrad", 64, 147, 12544)
        yield wgrad("r18.layer4.1.conv2 wgrad", 512, 4608, 49)


def split_list(v):
    out = [x if x == "auto" else int(x) for x in v.split(",")]
    if not out or any(x != "auto" and x < 1 for x in out):
        raise argparse.ArgumentTypeError("a comma list of integers >= 1 and auto")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--split-k", type=split_list, default=None, help="grad_bmm's split_k: one value or a comma list")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []
    for name, ours, theirs, macs, (nb, M, N, K) in shapes(sweep=a.split_k is not None):
        t_torch = t_one = None
        for sk in a.split_k or [1]:
            _lib.grad_stats(reset=True)
            got, ref = ours(sk), theirs()
            st = _lib.grad_stats(reset=True)
            dev = float((got - ref).abs().max() / ref.abs().max())
            del got, ref
            t_ours = med_ms(lambda: ours(sk), a.iters, a.warmup)
            if t_torch is None:
                t_torch = med_ms(theirs, a.iters, a.warmup)
            rec = dict(shape=name, grad_bmm_ms=t_ours, torch_fp32_ms=t_torch, ratio_vs_torch=t_ours / t_torch,
                       grad_bmm_tflops=2e-9 * macs / t_ours, torch_tflops=2e-9 * macs / t_torch,
                       recomputed_tiles=st["recomputed"], max_diff_over_max=dev)
            if a.split_k is not None:
                t_one = t_ours if sk == 1 else t_one
                rec.update(split_k=sk, splits=grad_split_auto(nb, M, N, K, DEV) if sk == "auto" else sk,
                           blocks=st["tiles"], vs_split_1=(t_ours / t_one) if t_one else None)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
