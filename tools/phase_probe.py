#!/usr/bin/env python
"""Where a gemm_f8mx_kernel workgroup's cycles go, per ResNet-18 layer: before the first barrier (the tile
setup), the K loop, after the K loop's last barrier (the NaN test, the store, the split sum).

    FP8A_LIB_PATH=<a -DFP8A_CLOCK_STAMP=1 build> python tools/phase_probe.py [--batch 1024] [--layers l1.c,..]

Needs a clock-stamp build (tools/gemm_bench.py --build-diag makes one; for the 64-bit index code build the
parent commit of "gemm_f8mx: 32-bit tile setup and store indexing" the same way).  Each layer runs as a ResNet-18 block runs it -- the stem with
BN + ReLU in the store, the 3 x 3 layers with BN + ReLU and the next convolution's word image emitted, the
1 x 1 downsampling layers plain -- on non-negative on-grid activations made on the device.  One line per layer:
workgroups, s_memtime ticks per workgroup and the three shares (fp8a_clock_stats with reset bit 1), and the
time of the whole call (pre-passes included) by HIP events.  The shares are thread 0's view of its workgroup, not executed-instruction counts.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.gemm_bench import RESNET18  # noqa: E402


def grid(gen, shape, E, M, bias, zero_frac, dev, signed):
    emax = 2 ** E - 1
    expo = torch.randint(max(0, emax - 8), emax + 1, shape, generator=gen, device=dev)
    mant = torch.randint(0, 2 ** M, shape, generator=gen, device=dev).float() / 2 ** M
    v = torch.where(expo == 0, torch.ldexp(mant, torch.full_like(expo, 1 - bias)), torch.ldexp(1.0 + mant, expo - bias))
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen, device=dev).float() * 2 - 1)
    v[torch.rand(shape, generator=gen, device=dev) < zero_frac] = 0.0
    return v


def phases(L):
    out = (ctypes.c_uint64 * 3)()
    assert L.fp8a_clock_stats(ctypes.cast(out, ctypes.c_void_p), 2) == 0
    ph = [int(v) for v in out]
    assert L.fp8a_clock_stats(ctypes.cast(out, ctypes.c_void_p), 1) == 0
    return ph, int(out[0]), int(out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", default="")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import bn_act_epilogue, new_word_image
    from fp8_quantization_amd.error_tables import get_error_table_NN
    L = _lib.load()
    dev = "cuda:0"
    E, M = 4, 3
    tab = get_error_table_NN(E, M, False, 3)
    fl = fa.make_flags(with_approx=True, with_s2nn2s_opt=True, quant_btw_mult_accu=True)
    bA, bB = 2 ** (E - 1) + 3, 2 ** (E - 1) + 8
    bR = bA + bB - 17
    gen = torch.Generator(device=dev).manual_seed(0)
    for (name, cin, cout, k, s, p, h) in RESNET18:
        if args.layers and name not in args.layers.split(","):
            continue
        x = grid(gen, (args.batch, cin, h, h), E, M, bA, 0.5, dev, signed=name == "conv1")
        w = grid(gen, (cout, cin, k, k), E, M, bB, 0.0, dev, signed=True)
        bW = torch.full((cout,), bB, dtype=torch.int32, device=dev)
        kw = dict(flags=fl, stride=(s, s), padding=(p, p))
        if k > 1:
            ep = bn_act_epilogue(torch.zeros(cout), torch.ones(cout), torch.ones(cout), torch.zeros(cout), 0.0,
                                 torch.nn.ReLU())
            kw["epilogue"] = (ep[0].to(dev),) + tuple(ep[1:])
        if k == 3:
            ho = (h + 2 * p - k) // s + 1
            img = new_word_image(args.batch, cout, ho, ho, 1, 1, dev)
            nq = (torch.tensor([4.0], device=dev), 8, M, 1)
            kw["chain"] = (None, (img, (1, 1), nq, torch.tensor([bR], dtype=torch.int32, device=dev), M))
        run = lambda: fa.approx_conv2d(x, w, E, M, bA, bW, bR, tab, **kw)  # noqa: E731
        run()
        torch.cuda.synchronize()
        phases(L)
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ph, cyc, wgs = phases(L)
        tot = max(sum(ph), 1)
        ho = (h + 2 * p - k) // s + 1
        print(json.dumps(dict(layer=name, M=args.batch * ho * ho, K=cin * k * k, N=cout, workgroups=wgs // args.reps,
                              ticks_per_wg=round(cyc / max(wgs, 1)), pre_barrier=round(ph[0] / tot, 4),
                              k_loop=round(ph[1] / tot, 4), after=round(ph[2] / tot, 4),
                              pre_ticks=round(ph[0] / max(wgs, 1)), after_ticks=round(ph[2] / max(wgs, 1)),
                              call_ms=round(sorted(ts)[len(ts) // 2], 3),
                              lib=os.path.basename(os.environ.get("FP8A_LIB_PATH", "default")))), flush=True)
        del x, w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
