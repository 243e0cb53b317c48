#!/usr/bin/env python
"""Golden-vector generator for the BN statistics re-estimation (TEST INFRASTRUCTURE ONLY).

Like gen_golden.py it runs only where the reference checkout is mounted, imports the reference
UNMODIFIED (through gen_golden's import shim) and writes a fixture next to itself:

  bn_reestimate.npz   the reference's own reestimate_BN_stats (utils/qat_utils.py:60-108) on its
                      QuantizedMobileNetV2 in G8's construction (gen_golden.gen_g8, case mbv2_e4m3:
                      width 0.25, 32x32, E4M3 approx on, the state and calibration batch recorded in
                      g8_mbv2.npz -- the generator checks that it rebuilt exactly that state), for 2
                      batches of 4 images:
        x0, x1                          the input batches
        layers                          the BN-fused layers' names, in module order
        init_mean/<l>, init_var/<l>     the statistics before re-estimation
        final_mean/<l>, final_var/<l>   ... and after, for every BN layer
        teacher                         three layers: the stem, the first depthwise, the last 1x1
        pre<b>/<l>, out<b>/<l>          their pre-BN tensor (the product) and layer output, batch b
        stat_mean<b>/<l>, stat_var<b>/<l>   the per-batch statistics the layer held after batch b
                                        (momentum 1: torch's fp32 batch mean / unbiased variance)
        mean64<b>/<l>, var64<b>/<l>     float64 two-pass statistics of pre<b> (var64: biased)

Usage:  python tests/golden/gen_golden_bnre.py
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (installs the import shim, puts the reference on sys.path)


def _import_reference():
    # models/__init__.py and utils/__init__.py import modules that need torchvision / click / ignite
    # (absent here): register the packages without running their __init__, give qat_utils the one
    # name it imports from the data loaders, then import the reference modules unmodified
    for pkg in ("models", "utils"):
        if pkg not in sys.modules:
            p = types.ModuleType(pkg)
            p.__path__ = [os.path.join(gg.REF, pkg)]
            sys.modules[pkg] = p
    if "utils.imagenet_dataloaders" not in sys.modules:
        dl = types.ModuleType("utils.imagenet_dataloaders")
        dl.ImageNetDataLoaders = object
        sys.modules["utils.imagenet_dataloaders"] = dl
    from models.mobilenet_v2 import MobileNetV2
    from models.mobilenet_v2_quantized_approx import QuantizedMobileNetV2
    from quantization.quantized_folded_bn import BNFusedHijacker
    from utils.qat_utils import reestimate_BN_stats
    return MobileNetV2, QuantizedMobileNetV2, BNFusedHijacker, reestimate_BN_stats


def main():
    MobileNetV2, QuantizedMobileNetV2, BNFusedHijacker, reestimate_BN_stats = _import_reference()
    g8 = np.load(os.path.join(HERE, "g8_mbv2.npz"))
    E, M = 4, 3
    run_method = dict(approx_flag=True, quantize_after_mult_and_add=False, res_quantizer_flag=True,
                      original_quantize_res=False)
    gg.ac.get_error_table_NN = gg.v9.get_error_table_NN
    torch.manual_seed(88)  # gen_g8's construction, step for step
    fp = MobileNetV2(n_class=10, input_size=32, width_mult=0.25)
    with torch.no_grad():
        for m in fp.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.5, 2.0)
            elif isinstance(m, nn.Linear):
                m.weight.normal_(0, 0.1)
                m.bias.uniform_(-0.1, 0.1)
    qp = gg.qparams_for(E, M, gg.approx_params(E, M, 3, False, True, True, True), dict(run_method))
    with contextlib.redirect_stdout(io.StringIO()):
        model = QuantizedMobileNetV2(fp, input_size=(1, 3, 32, 32), **qp)
    for k, v in model.state_dict().items():
        assert np.array_equal(v.numpy(), g8[f"mbv2_e4m3__state__{k}"]), f"state differs from g8_mbv2.npz: {k}"
    model.eval()
    model.quantized()
    model.estimate_ranges()
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        model(torch.from_numpy(g8["mbv2_e4m3__x_cal"]))
    model.fix_ranges()

    gen = torch.Generator().manual_seed(2024)
    xs = [torch.randn(4, 3, 32, 32, generator=gen) for _ in range(2)]
    layers = [(n, m) for n, m in model.named_modules() if isinstance(m, BNFusedHijacker)]
    dw = next(n for n, m in layers if getattr(m, "groups", 1) > 1)
    teacher = [layers[0][0], dw, [n for n, m in layers if isinstance(m, nn.Conv2d)][-1]]
    out = {"x0": xs[0].numpy(), "x1": xs[1].numpy(), "layers": np.array([n for n, _ in layers]),
           "teacher": np.array(teacher)}
    for n, m in layers:
        out[f"init_mean/{n}"] = m.running_mean.detach().clone().numpy()
        out[f"init_var/{n}"] = m.running_var.detach().clone().numpy()
    batch = {"b": -1}
    hooks = []
    mods = dict(layers)
    for n in teacher:
        mod = mods[n]

        def run_forward(x, weight, bias, offsets=None, _m=mod, _n=n, _f=type(mod).run_forward):
            y = _f(_m, x, weight, bias, offsets)
            if _n == teacher[0]:
                batch["b"] += 1  # the stem runs first in every forward
            pre = y.detach().clone()
            out[f"pre{batch['b']}/{_n}"] = pre.numpy()
            p64 = pre.double().transpose(0, 1).reshape(pre.shape[1], -1)
            mean = p64.mean(1)
            out[f"mean64{batch['b']}/{_n}"] = mean.numpy()
            out[f"var64{batch['b']}/{_n}"] = ((p64 - mean[:, None]) ** 2).mean(1).numpy()
            return y
        mod.run_forward = run_forward

        def hook(m, inp, outp, _n=n):
            b = batch["b"]
            out[f"out{b}/{_n}"] = outp.detach().clone().numpy()
            out[f"stat_mean{b}/{_n}"] = m.running_mean.detach().clone().numpy()
            out[f"stat_var{b}/{_n}"] = m.running_var.detach().clone().numpy()
        hooks.append(mod.register_forward_hook(hook))
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        reestimate_BN_stats(model, [(x, 0) for x in xs], num_batches=2)
    for h in hooks:
        h.remove()
    assert batch["b"] == 1
    assert not model.training and all(not m.training for _, m in layers)
    for n, m in layers:
        out[f"final_mean/{n}"] = m.running_mean.detach().clone().numpy()
        out[f"final_var/{n}"] = m.running_var.detach().clone().numpy()
    path = os.path.join(HERE, "bn_reestimate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(layers), "BN layers; teacher layers", teacher)


if __name__ == "__main__":
    main()
