#!/usr/bin/env python
"""Golden-vector generator for the FP8 MSE range estimator (TEST INFRASTRUCTURE ONLY).

Like gen_golden.py it runs only where the reference checkout is mounted, imports the reference
UNMODIFIED (through gen_golden's import shim) and writes a fixture next to itself:

  mse_cases.npz   per case: the input batches, the reference FP_MSE_Estimator's search_grid, its
                  mses after every batch, the picked mantissa width, the returned maxval, the
                  quantizer's final sign_bits, and ref_dev -- the largest relative deviation of
                  the reference's fp32 mses from a float64 accumulation of the same fp32 terms
                  (range_estimators.py:285-369, fp8_quantizer.py:97-173, 262-287).

Two conditions make a comparison against another implementation airtight; the generator checks
both on the reference alone and redraws a case's seed until they hold (no case is ever dropped):
  * in float64 no candidate's bias argument 2^E - log2(mx) + log2(2 - 2^-M) - 1 lies within 1e-4 of
    a half-integer (the rounded bias cannot depend on the log2 implementation);
  * every arg-min the selection takes -- per channel over the candidates of the winning width, per
    channel over the widths -- has a clear winner: best and runner-up differ relatively by more
    than 10 (ref_dev + B), B = L 2^-24 + 2^-40 the fused kernel's summation bound (L = MSE_L of
    csrc/fq_mse.h).  (Candidates that tie with the winner exactly -- nothing clamped, the same bias:
    the same terms element for element -- tie in any implementation that sums the same terms.)

Usage:  python tests/golden/gen_golden_mse.py
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402,F401  (installs the import shim, puts the reference on sys.path)
from quantization.quantizers.fp8_quantizer import FPQuantizer  # noqa: E402
from quantization.range_estimators import RangeEstimators  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(HERE))


def kernel_bound():
    src = open(os.path.join(ROOT, "fp8_quantization_amd", "csrc", "fq_mse.h")).read()
    v = int(re.search(r"constexpr int MSE_V = (\d+);", src).group(1))
    assert re.search(r"constexpr int MSE_L = MSE_V;", src)
    return v * 2.0 ** -24 + 2.0 ** -40


def draw(name, rng):
    """(batches, per_channel, mantissa search, allow_unsigned) of a case."""
    def rn(*shape, scale=1.0):
        return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))
    if name == "w8x3x3x3":      # per-channel weights, inner 27: shorter than a wave
        return [rn(8, 3, 3, 3, scale=0.2) * torch.linspace(0.5, 3.0, 8).view(8, 1, 1, 1)], True, False, False
    if name == "act2x5x7x7":    # a per-tensor activation, mantissa search
        return [rn(2, 5, 7, 7)], False, True, False
    if name == "pc4x37":        # per channel, mantissa search
        return [rn(4, 37) * torch.tensor([[0.3], [1.0], [4.0], [11.0]])], True, True, False
    if name == "two_batches":   # the second batch exceeds the grid the first one defined
        return [rn(3, 50), rn(3, 50, scale=2.5)], False, False, False
    if name == "unsigned":      # allow_unsigned: a non-negative batch, then a signed one
        return [rn(4, 30).abs(), rn(4, 30)], False, False, True
    if name == "zero_row":      # a row whose largest |x| is 0: maxval 0, NaN losses
        x = rn(3, 20)
        x[1] = 0.0
        return [x], True, False, False
    raise KeyError(name)


CASES = ["w8x3x3x3", "act2x5x7x7", "pc4x37", "two_batches", "unsigned", "zero_row"]


def run_case(name, seed, B):
    rng = np.random.default_rng(seed)
    batches, per_channel, msearch, unsigned = draw(name, rng)
    q = FPQuantizer(n_bits=8, per_channel=per_channel, mantissa_bits=3, maxval=None, set_maxval=True,
                    mse_include_mantissa_bits=msearch, allow_unsigned=unsigned)
    est = RangeEstimators.MSE.cls(per_channel=per_channel, quantizer=q)
    calls = []  # per quantizer forward of one batch: (float64 mean of the fp32 terms, bias argument ok)
    state = {}

    def hook(mod, inp, out):
        x = inp[0]
        terms = ((x - out) ** 2).double()
        dims = list(range(1, x.dim())) if per_channel else list(range(x.dim()))
        calls.append(terms.mean(dims).reshape(-1))
        M = float(torch.clamp(torch.round(mod.mantissa_bits), 1, mod.n_bits - mod.sign_bits))
        E = mod.n_bits - mod.sign_bits - M
        mx = mod.maxval.double().reshape(-1)
        mx = mx[mx > 0]
        arg = 2.0 ** E - torch.log2(mx) + np.log2(2.0 - 2.0 ** -M) - 1.0
        if mx.numel() and float(((arg - torch.floor(arg)) - 0.5).abs().min()) < 1e-4:
            state["half"] = True

    h = q.register_forward_hook(hook)
    out = {}
    acc64 = None
    ref_dev = 0.0
    for b, x in enumerate(batches):
        calls.clear()
        lo, hi = est(x)
        mses = est.mses.clone()
        step = torch.stack(calls).reshape(mses.shape)
        acc64 = step if acc64 is None else acc64 + step
        ok = torch.isfinite(acc64) & (acc64 > 0)
        if ok.any():
            ref_dev = max(ref_dev, float(((mses.double() - acc64).abs() / acc64)[ok].max()))
        out[f"{name}/x{b}"] = x.numpy()
        out[f"{name}/mses{b}"] = mses.numpy()
    h.remove()
    if state.get("half"):
        return None
    # the arg-mins' margins (rows with NaN losses have no arg-min to protect)
    mses = est.mses.double()
    need = 10.0 * (ref_dev + B)

    def clear(v, v64):
        """Per column of v [n][rows]: the entries tied with the minimum are exact ties (equal float64
        sums of their terms too: the same terms, so any fixed summation order ties them as well),
        and every other entry exceeds the minimum by the margin."""
        for r in range(v.shape[1]):
            col, col64 = v[:, r], v64[:, r]
            if not torch.isfinite(col).all():
                continue
            tied = col == col.min()
            if not bool((col64[tied] == col64[tied][0]).all()):
                return False
            rest = col[~tied]
            if rest.numel() and float(((rest - col.min()) / rest).min()) <= need:
                return False
        return True

    mbit_list = [float(m) for m in range(1, 7)] if msearch else [3.0]
    best_m = mbit_list.index(float(q.mantissa_bits))
    if not clear(mses[best_m], acc64[best_m]):
        return None
    if len(mbit_list) > 1 and not clear(mses.min(1)[0], acc64.min(1)[0]):
        return None
    out[f"{name}/search_grid"] = est.search_grid.numpy()
    out[f"{name}/maxval"] = hi.numpy().astype(np.float32)
    out[f"{name}/xmin"] = lo.numpy().astype(np.float32)
    out[f"{name}/meta"] = np.array([len(batches), int(per_channel), int(msearch), int(unsigned),
                                    int(round(float(q.mantissa_bits))), int(q.sign_bits), seed], dtype=np.int64)
    out[f"{name}/ref_dev"] = np.array([ref_dev], dtype=np.float64)
    return out


def main():
    B = kernel_bound()
    data = {}
    for k, name in enumerate(CASES):
        for attempt in range(200):
            seed = 1000 * (k + 1) + attempt
            out = run_case(name, seed, B)
            if out is not None:
                break
        else:
            raise RuntimeError(f"{name}: no seed satisfied the fixture's conditions")
        meta = out[f"{name}/meta"]
        print(f"{name}: seed {seed}, mantissa {meta[4]}, sign_bits {meta[5]}, ref_dev {out[name + '/ref_dev'][0]:.3g}, "
              f"maxval {out[name + '/maxval']}")
        data.update(out)
    path = os.path.join(HERE, "mse_cases.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
