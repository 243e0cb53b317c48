"""Range estimators (reference: quantization/range_estimators.py:56-125, 285-393).

current_minmax (weights, per channel), allminmax (activations, running min/max over every
calibration batch) and running_minmax (EMA): plain torch reductions on the device.

MSE (FP_MSE_Estimator): the grid search over 111 candidate maxvals (times the mantissa widths with
mse_include_mantissa_bits) for the FP8 quantizer's smallest mean squared error.  The losses of all
candidates come from one fused pass over the tensor (approx_ops.fp8_mse_losses, csrc/fq_mse.h);
``fused=False`` runs the reference's literal loop -- one fake quantization per candidate -- over this
project's FPQuantizer instead: the semantic ground truth and the timing baseline.
"""
import enum

import torch
from torch import nn


def _minmax(x, per_channel):
    if per_channel:
        flat = x.reshape(x.shape[0], -1)
        return flat.min(-1)[0].detach(), flat.max(-1)[0].detach()
    return x.min().detach(), x.max().detach()


class _Estimator(nn.Module):
    def __init__(self, per_channel=False, quantizer=None, **kwargs):
        super().__init__()
        self.per_channel = per_channel
        self.quantizer = quantizer
        self.current_xmin = None
        self.current_xmax = None

    def reset(self):
        self.current_xmin = self.current_xmax = None


class CurrentMinMaxEstimator(_Estimator):
    def __init__(self, percentile=None, **kwargs):
        super().__init__(**kwargs)
        if percentile:
            raise NotImplementedError("percentile ranges are not used on the approx path")

    def forward(self, x):
        self.current_xmin, self.current_xmax = _minmax(x, self.per_channel)
        return self.current_xmin, self.current_xmax


class AllMinMaxEstimator(_Estimator):
    def forward(self, x):
        lo, hi = _minmax(x, self.per_channel)
        if self.current_xmin is None:
            self.current_xmin, self.current_xmax = lo, hi
        else:
            self.current_xmin = self.current_xmin.minimum(lo)
            self.current_xmax = self.current_xmax.maximum(hi)
        return self.current_xmin, self.current_xmax


class RunningMinMaxEstimator(_Estimator):
    def __init__(self, momentum=0.9, **kwargs):
        super().__init__(**kwargs)
        self.momentum = momentum

    def forward(self, x):
        lo, hi = _minmax(x, self.per_channel)
        if self.current_xmin is None:
            self.current_xmin, self.current_xmax = lo, hi
        else:
            a = self.momentum
            self.current_xmin = (1 - a) * lo + a * self.current_xmin
            self.current_xmax = (1 - a) * hi + a * self.current_xmax
        return self.current_xmin, self.current_xmax


class OptMethod(enum.Enum):
    grid = 1
    golden_section = 2


MSE_GRID_POINTS = 111  # the reference's grid size, whatever num_candidates says (range_estimators.py:305)


def mse_search_grid(x, per_channel):
    """The reference's candidate maxvals (range_estimators.py:295-308): per channel (or for the whole
    tensor) 111 points of torch.linspace(0.1 mx, 1.2 mx), mx = max(|min|, |max|), built on the host
    in fp32 from mx.item() so the candidates' bits are the reference's.  Returns [111][rows] on x's
    device."""
    flat = x.detach().reshape(x.shape[0], -1) if per_channel else x.detach().reshape(1, -1)
    mxs = torch.max(flat.min(-1)[0].abs(), flat.max(-1)[0].abs()).cpu()
    lsp = [torch.linspace(0.1 * mx.item(), 1.2 * mx.item(), MSE_GRID_POINTS) for mx in mxs]
    return torch.stack(lsp).transpose(0, 1).contiguous().to(x.device)


def mse_select(mses, search_grid, mbit_list):
    """The reference's pick (range_estimators.py:349-369) from the accumulated losses
    mses [n_mbits][n_cand][rows]: the best width per channel, the plurality vote over channels
    (torch.mode), then per channel the arg-min candidate of the winning width.  Returns
    (best_mbits float, maxval [rows]); runs wherever mses lives."""
    best_mbits_per_channel = mses.min(1)[0].argmin(0)
    best_mbit_idx = torch.mode(best_mbits_per_channel).values.item()
    best = mses[best_mbit_idx].argmin(0)
    maxval = search_grid.gather(0, best.reshape(1, -1)).reshape(-1)
    return float(mbit_list[best_mbit_idx]), maxval


class FP_MSE_Estimator(_Estimator):
    def __init__(self, num_candidates=100, opt_method=OptMethod.grid, range_margin=0.5, fused=True, **kwargs):
        super().__init__(**kwargs)
        assert opt_method == OptMethod.grid
        self.num_candidates = num_candidates  # (unused, as in the reference: the grid has 111 points)
        self.range_margin = range_margin
        self.fused = fused
        self.mses = self.search_grid = None

    def reset(self):
        super().reset()
        self.mses = self.search_grid = None

    def _define_search_range(self, x, mbit_list):
        # the FIRST batch defines the grid; later batches accumulate on it (range_estimators.py:302-316)
        if self.search_grid is None:
            assert self.mses is None
            self.search_grid = mse_search_grid(x, self.per_channel)
            self.mses = torch.zeros((len(mbit_list),) + tuple(self.search_grid.shape), dtype=torch.float32,
                                    device=x.device)
        return self.search_grid, self.mses

    def _literal(self, x, search_grid, mses, mbit_list, sign_bits):
        """range_estimators.py:334-347, one fake quantization per (width, candidate)."""
        q = self.quantizer
        meandims = list(range(x.dim()))[1:] if self.per_channel else list(range(x.dim()))
        for m, mbits in enumerate(mbit_list):
            q.mantissa_bits = torch.Tensor([mbits]).to(x.device)
            for i, maxval in enumerate(search_grid):
                q.set_quant_range(sign_bits * -1.0 * maxval, maxval)
                xfp = q(x)
                mses[m, i, :] += ((x - xfp) ** 2).mean(meandims)

    def _fused(self, x, search_grid, mses, mbit_list, sign_bits):
        """The same accumulation from one pass over x.  The quantizer's state moves as the loop moves
        it: every candidate's set_quant_range makes it unsigned under the same condition, and the
        last candidate's maxval stays behind."""
        from ..approx_ops import fp8_mse_losses
        q = self.quantizer
        if q.allow_unsigned and bool((sign_bits * -1.0 * search_grid >= 0).all(-1).any()):
            q.sign_bits = 0
        widths = [int(min(max(round(m), 1), q.n_bits - q.sign_bits)) for m in mbit_list]  # (fp8_quantizer.py:111)
        sse = fp8_mse_losses(x, search_grid, widths, q.n_bits, q.sign_bits, self.per_channel)
        count = x.numel() // search_grid.shape[-1]
        mses += (sse / count).to(torch.float32)
        q.set_quant_range(sign_bits * -1.0 * search_grid[-1], search_grid[-1])

    def forward(self, x):
        q = self.quantizer
        mbit_list = [float(q.mantissa_bits)]
        if q.mse_include_mantissa_bits:
            # highest possible value is n_bits - sign_bits - 1
            mbit_list = [float(m) for m in range(1, q.n_bits - q.sign_bits)]
        x = x.detach()
        search_grid, mses = self._define_search_range(x, mbit_list)
        assert mses.shape[1:] == search_grid.shape, f"{mses.shape}, {search_grid.shape}"
        assert mses.shape[0] == len(mbit_list), f"{mses.shape}, {len(mbit_list)} mantissa widths"
        # (needed here too, for the search range: range_estimators.py:332)
        sign_bits = int(torch.any(x < 0)) if q.allow_unsigned else 1
        # the loop never moves the quantizer's maxval without set_maxval: only the literal path can
        # evaluate "every candidate at the maxval the quantizer happens to hold"
        if self.fused and q.set_maxval:
            self._fused(x, search_grid, mses, mbit_list, sign_bits)
        else:
            self._literal(x, search_grid, mses, mbit_list, sign_bits)
        best_mbits, maxval = mse_select(mses, search_grid, mbit_list)
        q.mantissa_bits = torch.tensor(best_mbits).to(q.mantissa_bits.device)
        maxval = maxval.to(q.maxval.device)
        self.current_xmin, self.current_xmax = sign_bits * -1.0 * maxval, maxval
        return self.current_xmin, self.current_xmax


class _Choice:
    def __init__(self, cls):
        self.cls = cls


class RangeEstimators:
    current_minmax = _Choice(CurrentMinMaxEstimator)
    allminmax = _Choice(AllMinMaxEstimator)
    running_minmax = _Choice(RunningMinMaxEstimator)
    MSE = _Choice(FP_MSE_Estimator)
