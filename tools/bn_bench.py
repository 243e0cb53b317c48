#!/usr/bin/env python
"""Times the BN re-estimation's training-mode forward and the bn_train kernels on one GPU.

    python tools/bn_bench.py [--output profiles/bn_measure.json] [--reps 20]

  * one re-estimation batch (every BN-fused layer in training mode at momentum 1, as
    bn_reestimate.reestimate_bn_stats runs it) of MobileNetV2 and ResNet-18 at 224 x 224, batch 16
    (the reference's) and 64, with fuse_bn_train on and off -- off is F.batch_norm + the unfused
    activation / quantizer passes, the forward this repository ran before the kernels existed.  The
    two variants alternate inside the timed loop.
  * the kernels alone on the largest activation of each network at batch 64: the statistics call
    (bn_stats_kernel + bn_finalize_kernel; one read of x) and the whole in-place call (+ bn_apply_kernel;
    one more read and one write), against their byte floors at the 6.3 TB/s a float4 copy reaches;
    the apply kernel's own time is the difference of the two calls.
HIP events around each call, warm-up, at least 20 repeats; median, min and max in ms.
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd.approx_ops import bn_train  # noqa: E402
from fp8_quantization_amd.bn_reestimate import bn_fused_layers  # noqa: E402

DEV = "cuda:0"
HBM = 6.3e12  # achievable bytes / s (a float4 copy)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), reps=len(ts))


def build(arch):
    from fp8_quantization_amd.mobilenet_workload import mobilenet_v2_approx
    from fp8_quantization_amd.resnet_workload import resnet18_approx
    torch.manual_seed(0)
    m = (mobilenet_v2_approx if arch == "mobilenet_v2" else resnet18_approx)(bn_stats_batches=1, device=DEV)
    m = m.to(DEV).eval()
    m.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(torch.randn(16, 3, 224, 224, device=DEV))
    m.fix_ranges()
    return m


def model_rows(arch, reps):
    m = build(arch)
    layers = [l for _, l in bn_fused_layers(m)]
    for l in layers:
        l.training, l.momentum = True, 1.0
    rows = []
    for batch in (16, 64):
        x = torch.randn(batch, 3, 224, 224, device=DEV)

        def step(fuse):
            for l in layers:
                l.fuse_bn_train = fuse
            with torch.no_grad():
                m(x)
        for fuse in (True, False, True, False):
            step(fuse)
        torch.cuda.synchronize()
        ts = {True: [], False: []}
        for _ in range(reps):
            for fuse in (True, False):
                ts[fuse].append(event_ms(lambda: step(fuse)))
        row = dict(arch=arch, batch=batch, fused=summary(ts[True]), unfused=summary(ts[False]))
        row["unfused_over_fused"] = row["unfused"]["median_ms"] / row["fused"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def kernel_rows(reps):
    rows = []
    for name, shape in (("mobilenet_v2 features.2 expand [64,96,112,112]", (64, 96, 112, 112)),
                        ("resnet18 stem [64,64,112,112]", (64, 64, 112, 112))):
        x = torch.randn(shape, device=DEV)
        C = shape[1]
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        mx = torch.tensor([4.0], device=DEV)
        calls = dict(
            stats=lambda: bn_train(x, gamma, beta, rm, rv, 1.0, 1e-5, stats_only=True),
            stats_apply=lambda: bn_train(x, gamma, beta, rm, rv, 1.0, 1e-5, activation=nn.ReLU6(), out=x),
            stats_apply_quant=lambda: bn_train(x, gamma, beta, rm, rv, 1.0, 1e-5, activation=nn.ReLU6(),
                                               out_quantizer=(mx, 8, 3, 1), out=x))
        row = dict(tensor=name, elements=x.numel())
        for key, fn in calls.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            row[key] = summary([event_ms(fn) for _ in range(reps)])
        nbytes = 4 * x.numel()
        row["stats_floor_ms"] = nbytes / HBM * 1e3
        row["apply_floor_ms"] = 2 * nbytes / HBM * 1e3
        row["apply_ms"] = row["stats_apply"]["median_ms"] - row["stats"]["median_ms"]
        row["apply_quant_ms"] = row["stats_apply_quant"]["median_ms"] - row["stats"]["median_ms"]
        row["stats_share_of_floor"] = row["stats_floor_ms"] / row["stats"]["median_ms"]
        row["apply_share_of_floor"] = row["apply_floor_ms"] / row["apply_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--output", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--arch", nargs="*", default=["mobilenet_v2", "resnet18"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bn_bench needs a HIP device")
    reps = max(20, args.reps)
    out = dict(kernels=kernel_rows(reps), models=[r for a in args.arch for r in model_rows(a, reps)])
    if args.output:
        os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
        with open(args.output, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
