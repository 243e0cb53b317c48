"""Fine-tune an approx-FP8 model THROUGH the approximate multiplier: SGD steps whose forward is the approx
forward and whose backward is the straight-through estimator (custom_approx_params["ste_backward"]:
quantizer masks, the exact product's gradients on the gradient GEMM fp8a_grad_bmm).

    python -m fp8_quantization_amd.finetune --synthetic 64 --arch resnet18|mobilenet_v2|vit_b16 \
        --steps 10 --lr 1e-3 [--batch-size 64] [--momentum 0.9] [--approx-attention] \
        [--learn-ranges [--range-lr 1e-4]] [--grad-split-k N|auto] [--seed 0]

A driver, not a trainer (no schedule, checkpoints or augmentation): it calibrates and fixes the FP8 ranges as
the validation driver does (imagenet.py: estimate_ranges over --num-est-batches batches, fix_ranges), keeps the
model in eval mode (BN uses its running statistics, dropout is off), and runs SGD on every trainable
parameter.  One JSON line per step: the loss, the step's milliseconds with their forward / backward split and,
inside the backward, the gradient GEMMs and the convolutions' im2col + fold plumbing (HIP events), and the
64 x 64 tiles the gradient GEMM recomputed in fp32 -- 0 as long as every saved operand is on its FP8 grid; a
step that recomputed any makes the exit status 1.
--learn-ranges: the FP8 ranges train too (FPQuantizer.learn_maxval): the model is built with
learn_maxval, learn_ranges() follows the calibration, the maxvals form their own parameter group with
--range-lr (default: --lr), and fix_ranges() follows the last step.  Each record also carries the number
of learned ranges, the quantizers' recorded forward + backward milliseconds and the largest relative change
of any maxval since calibration (without the flag: 0 ranges, the milliseconds, 0.0).  The driver does not
clamp a range: a maxval that is not finite or not positive after a step ends the run with exit status 1.
--grad-split-k: every gradient GEMM of the backward splits its reduction along K into N parts, or into what
approx_ops.grad_split_auto picks per product ("auto"), and adds the parts in a fixed order:
custom_approx_params["grad_split_k"]; default 1, off.  grad_gemm_ms then includes the reduce passes.
Data: --synthetic N random images and labels, or <images-dir>/train as imagenet.py reads it.
"""
import argparse
import json
import os
import sys

import torch

from . import _lib, approx_ops
from .imagenet import NumericImageFolder, SyntheticImages, _loader, build_model


def _split_k(v):
    if v == "auto":
        return v
    try:
        n = int(v)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"an integer >= 1 or auto, not {v!r}")
    return n


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images-dir", default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="N random images instead of a dataset")
    ap.add_argument("--arch", default="resnet18", choices=["resnet18", "resnet50", "mobilenet_v2", "vit_b16"])
    ap.add_argument("--weights", default=None, help="float (torchvision-format) state dict")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--num-est-batches", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--expo-width", type=int, default=4)
    ap.add_argument("--mant-width", type=int, default=3)
    ap.add_argument("--dnsmp-factor", type=int, default=3)
    ap.add_argument("--with-comp", action="store_true")
    ap.add_argument("--approx-attention", action="store_true",
                    help="ViT only: QK^T and PV of every attention through the approx multiplier")
    ap.add_argument("--seed", type=int, default=None, help="seed of the model's initialization and the data order")
    ap.add_argument("--learn-ranges", action="store_true",
                    help="train every FP8 quantizer's maxval as well (its own parameter group)")
    ap.add_argument("--range-lr", type=float, default=None, help="learning rate of the maxvals (default: --lr)")
    ap.add_argument("--grad-split-k", type=_split_k, default=1, metavar="{N,auto}",
                    help="split the gradient GEMMs' reductions along K: a part count, or auto (default 1: off)")
    ap.add_argument("--output", default=None, help="also write the step records (a JSON list) here")
    return ap.parse_args(argv)


def approx_cfg(args):
    cfg = dict(expo_width=args.expo_width, mant_width=args.mant_width, dnsmp_factor=args.dnsmp_factor,
               withComp=args.with_comp, ste_backward=True)
    if args.approx_attention:
        cfg["approx_attention"] = True
    if args.learn_ranges:
        cfg["learn_maxval"] = True
    if getattr(args, "grad_split_k", 1) != 1:
        cfg["grad_split_k"] = args.grad_split_k
    return cfg


def _events_ms(pairs):
    return float(sum(a.elapsed_time(b) for a, b in pairs))


def finetune(model, data, args, dev):
    """Calibrate on the first --num-est-batches batches of `data`, then --steps SGD steps over it (cycled);
    returns the step records."""
    from .distributed import calibrate_on_rank0

    def cal():
        for i, (x, _) in enumerate(_loader(data, args.batch_size, args.num_workers)):
            yield x.to(dev, non_blocking=True)
            if i >= args.num_est_batches - 1:
                break
    calibrate_on_rank0(model, cal())
    model.eval()  # BN on its running statistics, dropout off: only the products, quantizers and affines train
    ranges, cal0 = [], None
    if args.learn_ranges:
        from .distributed import quantizers
        model.learn_ranges()
        ranges = list({id(q.maxval): q.maxval for q in quantizers(model)
                       if isinstance(q.maxval, torch.nn.Parameter)}.values())
        cal0 = torch.cat([p.detach().reshape(-1) for p in ranges]).clone()
    rid = {id(p) for p in ranges}
    groups = [dict(params=[p for p in model.parameters() if p.requires_grad and id(p) not in rid])]
    if ranges:
        groups.append(dict(params=ranges, lr=args.lr if args.range_lr is None else args.range_lr))
    opt = torch.optim.SGD(groups, lr=args.lr, momentum=args.momentum)
    records, step = [], 0
    _lib.grad_stats(reset=True)
    while step < args.steps:
        for x, y in _loader(data, args.batch_size, args.num_workers):
            if step >= args.steps:
                break
            x, y = x.to(dev, non_blocking=True), y.to(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            approx_ops._STE_PROFILE = prof = {}
            opt.zero_grad(set_to_none=True)
            ev[0].record()
            loss = torch.nn.functional.cross_entropy(model(x), y)
            ev[1].record()
            loss.backward()
            ev[2].record()
            opt.step()
            ev[3].record()
            approx_ops._STE_PROFILE = None
            torch.cuda.synchronize()
            st = _lib.grad_stats(reset=True)
            rec = dict(step=step, loss=float(loss.detach()), step_ms=ev[0].elapsed_time(ev[3]),
                       forward_ms=ev[0].elapsed_time(ev[1]), backward_ms=ev[1].elapsed_time(ev[2]),
                       grad_gemm_ms=_events_ms(prof.get("grad_gemm", ())),
                       im2col_fold_ms=_events_ms(prof.get("im2col", ())) + _events_ms(prof.get("fold", ())),
                       grad_gemm_launches=st["launches"], recomputed_tiles=st["recomputed"])
            rec.update(learned_ranges=len(ranges), max_range_change=0.0, bad_ranges=0,
                       quantizer_ms=_events_ms(prof.get("fq_forward", ())) + _events_ms(prof.get("fq_backward", ())))
            if ranges:
                now = torch.cat([p.detach().reshape(-1) for p in ranges])
                rec.update(max_range_change=float(((now - cal0).abs() / cal0.abs()).max()),
                           bad_ranges=int((~(torch.isfinite(now) & (now > 0))).sum()))
            print(json.dumps(rec), flush=True)
            records.append(rec)
            step += 1
            if rec.get("bad_ranges"):
                print(f"step {rec['step']}: {rec['bad_ranges']} learned maxval(s) not finite or not positive "
                      "(lower --range-lr)", file=sys.stderr)
                return records
    if ranges:
        model.fix_ranges()
    return records


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("the approx path needs a HIP device")
    if not args.synthetic and not args.images_dir:
        raise SystemExit("give --synthetic N or --images-dir")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.synthetic:
        data = SyntheticImages(args.synthetic, args.image_size)
    else:
        data = NumericImageFolder(os.path.join(args.images_dir, "train"), args.image_size)
    model = build_model(args.arch, args.weights, approx_cfg(args), args.image_size).to(dev).eval()
    records = finetune(model, data, args, dev)
    if args.output:
        with open(args.output, "w") as f:
            json.dump(records, f, indent=1)
    return 1 if any(r["recomputed_tiles"] or r.get("bad_ranges") for r in records) else 0


if __name__ == "__main__":
    sys.exit(main())
