#!/usr/bin/env python
"""Timings of the batched approx product (fp8a_bmm) at ViT-B/16's attention shapes, and its comparators.

    python tools/bmm_bench.py --mode bmm  [--batch 64]            # fp8a_bmm: QK^T and PV, one launch each
    python tools/bmm_bench.py --mode loop [--batch 8]             # a Python loop of approx_matmul per (image, head)
    FP8A_NO_MX=1 python tools/bmm_bench.py --mode flat            # one approx_matmul, M = batch*heads*S (gemm_fast_kernel)
    python tools/bmm_bench.py --mode vit  [--batch 64] [--runs 3] # ViT-B/16 forward, approx_attention off / on interleaved

S = 197 tokens, 12 heads of d = 64, E4M3 with the built-in table and the default flags (approx, s2n, qbma).
HIP events; median of --iters launches after --warmup.  One JSON line per measurement on stdout and, with
--out FILE, appended to FILE.  `loop` and `flat` use only entry points older than fp8a_bmm, so they also run
against an older build of the library (FP8A_LIB_PATH).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fp8_quantization_amd import _lib  # noqa: E402
from fp8_quantization_amd import approx_ops as ops  # noqa: E402
from fp8_quantization_amd.error_tables import get_error_table_NN  # noqa: E402

DEV = "cuda:0"
S, HEADS, D, E, M = 197, 12, 64, 4, 3


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def grid(shape, maxval, seed):
    """Values on the E4M3 grid of `maxval` (the FP8 fake quantizer's output) and their int bias."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * (maxval / 4)).to(DEV)
    q, bias = ops.fp8_fake_quantize(x, torch.tensor([float(maxval)], device=DEV), 8, M)
    return q, int(bias.reshape(-1)[0].item())


def operands(batch):
    """q, k, v as [B, S, H*d] linear outputs and probs [B, H, S, S], all on their grids."""
    q, bq = grid((batch, S, HEADS * D), 4.0, 1)
    k, bk = grid((batch, S, HEADS * D), 4.0, 2)
    v, bv = grid((batch, S, HEADS * D), 4.0, 3)
    p, _ = grid((batch, HEADS, S, S), 1.0, 4)
    p, bp = ops.fp8_fake_quantize(p.abs(), torch.tensor([1.0], device=DEV), 8, M)
    return q, k, v, p, bq, bk, bv, int(bp.reshape(-1)[0].item())


def heads(t):
    return t.view(t.shape[0], S, HEADS, D).permute(0, 2, 1, 3)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["bmm", "loop", "flat", "vit"], required=True)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--attention", choices=["both", "on", "off"], default="both",
                    help="vit mode: which models run (a kernel trace of one of them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    table = get_error_table_NN(E, M, withComp=False, dnsmp_factor=3)
    flags = ops.make_flags(True, True, True, False)
    base = dict(mode=a.mode, lib=os.path.relpath(_lib.LIB_PATH), no_mx=os.environ.get("FP8A_NO_MX"), warmup=a.warmup,
                iters=a.iters)

    if a.mode == "vit":
        from fp8_quantization_amd.vit_workload import vit_approx_macs_per_image, vit_b16_approx
        batch = a.batch or 64
        g = torch.Generator().manual_seed(1)
        x = torch.randn((batch, 3, 224, 224), generator=g).to(DEV)
        models = {}
        which = {"both": (False, True), "on": (True,), "off": (False,)}[a.attention]
        for on in which:
            m = vit_b16_approx(seed=0, approx_attention=on).to(DEV).eval()
            m.quantized()
            m.estimate_ranges()
            with torch.no_grad():
                m(x[:8])
            m.fix_ranges()
            models[on] = m
        for run in range(a.runs):  # interleaved: off, on, off, on, ...
            for on in which:
                with torch.no_grad():
                    med, best = timed(lambda: models[on](x), 3, 10)
                macs0 = vit_approx_macs_per_image() * batch
                macs1 = vit_approx_macs_per_image(approx_attention=on) * batch
                emit(dict(base, what="vit_b16_forward", approx_attention=on, run=run, batch=batch, ms_median=med,
                          ms_min=best, images_per_s=batch / med * 1e3, gmacs_linears_per_s=macs0 / med * 1e-6,
                          gmacs_with_attention_per_s=macs1 / med * 1e-6), a.out)
        return

    batch = a.batch or (8 if a.mode == "loop" else 64)
    q, k, v, p, bq, bk, bv, bp = operands(batch)
    bR_qk, bR_pv = bq + bk - 2 ** E - 3, bp + bv - 2 ** E - 3  # (the products stay inside the result grid)
    qh, kt, vh = heads(q), heads(k).transpose(-1, -2), heads(v)
    macs = batch * HEADS * S * S * D

    if a.mode == "bmm":
        scores = torch.empty((batch, HEADS, S, S), device=DEV)
        ctx = torch.empty((batch, S, HEADS, D), device=DEV)
        cases = [("qk", lambda: ops.approx_bmm(qh, kt, E, M, bq, bk, bR_qk, table, flags=flags, out=scores)),
                 ("pv", lambda: ops.approx_bmm(p, vh, E, M, bp, bv, bR_pv, table, flags=flags,
                                               out=ctx.permute(0, 2, 1, 3)))]
        _lib.bmm_stats(reset=True)
        for name, fn in cases:
            med, best = timed(fn, a.warmup, a.iters)
            emit(dict(base, what=name, batch=batch, ms_median=med, ms_min=best, gmacs_per_s=macs / med * 1e-6,
                      ms_per_product=med / (batch * HEADS)), a.out)
        emit(dict(base, what="bmm_stats", **_lib.bmm_stats()), a.out)
    elif a.mode == "loop":
        def loop_qk():
            for i in range(batch):
                for h in range(HEADS):
                    ops.approx_matmul(qh[i, h], kt[i, h], E, M, bq, bk, bR_qk, table, flags=flags)

        def loop_pv():
            for i in range(batch):
                for h in range(HEADS):
                    ops.approx_matmul(p[i, h], vh[i, h], E, M, bp, bv, bR_pv, table, flags=flags)
        for name, fn in (("qk", loop_qk), ("pv", loop_pv)):
            med, best = timed(fn, a.warmup, a.iters)
            emit(dict(base, what=name, batch=batch, ms_median=med, ms_min=best, gmacs_per_s=macs / med * 1e-6,
                      ms_per_product=med / (batch * HEADS)), a.out)
    else:  # flat: the same per-term math and tile in one gemm_fast_kernel launch (FP8A_NO_MX=1)
        A = qh.reshape(batch * HEADS * S, D).contiguous()
        B = kt[0, 0].contiguous()
        _lib.path_stats(reset=True)
        med, best = timed(lambda: ops.approx_matmul(A, B, E, M, bq, bk, bR_qk, table, flags=flags), a.warmup, a.iters)
        emit(dict(base, what="flat_qk", batch=batch, M=A.shape[0], N=S, K=D, ms_median=med, ms_min=best,
                  gmacs_per_s=A.shape[0] * S * D / med * 1e-6, paths=_lib.path_stats()), a.out)


if __name__ == "__main__":
    main()
