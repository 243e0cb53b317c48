"""FP8 fake quantizer (reference: quantization/quantizers/fp8_quantizer.py:97-173, 191-319).

quantize_to_fp8_ste_MM keeps its signature and return value (values, float bias); the
per-element arithmetic is the HIP kernel fp8a_fp8_quantize.  FPQuantizer keeps the
reference's attribute surface: n_bits, mantissa_bits (tensor), maxval (tensor), sign_bits,
custom_bias (set by every forward), set_quant_range / fix_ranges.  mantissa_bits is assignable (the
MSE range estimator stores its winning width there, range_estimators.FP_MSE_Estimator): the integer
width forward hands to the kernels follows the assignment.
"""
import torch
from torch import nn

from ..approx_ops import _ste_timed, fp8_fake_quantize, fp8_fake_quantize_backward, fp8_fake_quantize_train


def quantize_to_fp8_ste_MM(x_float, n_bits, maxval, num_mantissa_bits, sign_bits):
    M = int(torch.clamp(torch.round(torch.as_tensor(num_mantissa_bits, dtype=torch.float32)), 1,
                        n_bits - sign_bits).item()) if isinstance(num_mantissa_bits, torch.Tensor) else \
        int(min(max(round(float(num_mantissa_bits)), 1), n_bits - sign_bits))
    maxval = torch.as_tensor(maxval, dtype=torch.float32, device=x_float.device)
    per_row = maxval.numel() != 1
    return fp8_fake_quantize(x_float, maxval, n_bits, M, sign_bits=sign_bits, per_row=per_row)


class _FakeQuantTrain(torch.autograd.Function):
    """The quantizer's recorded forward with the reference's backward, one kernel pass each way
    (fp8a_fq_train_forward / fp8a_fq_train_backward, csrc/fq_train.h).  quantize_to_fp8_ste_MM
    (fp8_quantizer.py:97-173) is differentiable torch: its bias is rounded, its power-of-two scales are detached
    and its rounding is straight-through, so (g s) / s = g exactly and what remains is the gradient of the clamp
    min(max(x, minval), maxval), minval = -maxval or the constant 0.  With respect to x it passes inside the
    clamp, is zero outside, and -- as ATen's maximum / minimum split a tie -- half at x == minval or
    x == maxval.  With respect to maxval it is the sum of g over the elements the upper bound clamps minus the
    sum over those the signed lower bound clamps, a tie counting half.  Saved: one code byte per element."""

    @staticmethod
    def forward(ctx, x, maxval, q):
        rows = maxval.numel()
        with _ste_timed("fq_forward"):
            res, q.custom_bias, code = fp8_fake_quantize_train(x, maxval, q.n_bits, q._mbits_int,
                                                               sign_bits=q.sign_bits, per_row=rows != 1)
        ctx.save_for_backward(code)
        ctx.fq = (rows, q.sign_bits, maxval.shape)
        return res

    @staticmethod
    def backward(ctx, g):
        (code,) = ctx.saved_tensors
        rows, sign_bits, shape = ctx.fq
        with _ste_timed("fq_backward"):
            gx, gm = fp8_fake_quantize_backward(g, code, rows, sign_bits)
        return (gx if ctx.needs_input_grad[0] else None, gm.view(shape) if ctx.needs_input_grad[1] else None, None)


class FPQuantizer(nn.Module):
    """8-bit floating-point quantizer with a custom exponent bias set by ``maxval``.

    ``ste_backward`` (default off; set by the owning layer from custom_approx_params['ste_backward']): a
    forward that autograd records goes through _FakeQuantTrain, the quantize kernel's values with the
    reference's gradient with respect to x and -- for a learned range -- maxval.

    Learned ranges: built with ``learn_maxval=True``, make_range_trainable() (QuantizationManager.learn_ranges)
    turns ``maxval`` into an nn.Parameter; fix_ranges() turns it back into a plain tensor with the same data.
    While it is a Parameter every range update writes it in place.  Learned mantissa widths stay out: an approx
    layer's error table belongs to one format and the kernels take an integer width."""
    ste_backward = False

    def __init__(self, n_bits=8, per_channel=False, scale_domain=None, mantissa_bits=4, maxval=3,
                 set_maxval=False, learn_maxval=False, learn_mantissa_bits=False, mse_include_mantissa_bits=True,
                 allow_unsigned=False, **kwargs):
        super().__init__()
        self.n_bits = n_bits
        self.per_channel = per_channel
        self.state = None
        self.ebits = n_bits - mantissa_bits - 1
        self.default_bias = 2 ** (self.ebits - 1)
        default_maxval = (2 - 2 ** (-mantissa_bits)) * 2 ** (2 ** self.ebits - 1 - self.default_bias)
        self.maxval = torch.Tensor([maxval if maxval is not None else default_maxval])
        self.mantissa_bits = torch.Tensor([float(mantissa_bits)])
        self.set_maxval = set_maxval
        self.learning_maxval = learn_maxval
        self.learning_mantissa_bits = learn_mantissa_bits
        self.mse_include_mantissa_bits = mse_include_mantissa_bits
        self.allow_unsigned = allow_unsigned
        self.sign_bits = 1
        self.custom_bias = None

    @property
    def mantissa_bits(self):
        return self._mantissa_bits

    @mantissa_bits.setter
    def mantissa_bits(self, value):
        # the reference keeps a float tensor and rounds it in every forward (round_ste_func,
        # fp8_quantizer.py:111); the kernels take an integer width, read once per assignment
        if not isinstance(value, torch.Tensor):
            value = torch.Tensor([float(value)])
        self._mantissa_bits = value
        self._mbits_int = int(round(float(value.detach().reshape(-1)[0])))

    def _make_unsigned(self, x_min):
        if isinstance(x_min, torch.Tensor):
            return self.allow_unsigned and bool(torch.all(x_min >= 0))
        return self.allow_unsigned and x_min >= 0

    @property
    def is_initialized(self):
        # always True, as the reference's FPQuantizer (fp8_quantizer.py:252-254): it starts from a
        # default maxval, so fix_ranges never raises for it (QuantizationManager.fix_ranges)
        return True

    def _assign_maxval(self, value):
        """maxval <- value.  A Parameter keeps its identity (an optimizer holds it; torch refuses a plain
        tensor under its name): it is written in place, under no_grad."""
        if isinstance(self.maxval, nn.Parameter):
            with torch.no_grad():
                value = value.detach().to(dtype=self.maxval.dtype)
                if value.device != self.maxval.device or value.shape != self.maxval.shape:
                    self.maxval.data = value.clone()
                else:
                    self.maxval.copy_(value)
        else:
            self.maxval = value

    def forward(self, x_float):
        if self.maxval.device != x_float.device:
            self._assign_maxval(self.maxval.to(x_float.device))
        mx = self.maxval
        if torch.is_grad_enabled():
            if mx.requires_grad and not self.ste_backward:
                raise RuntimeError("FPQuantizer: maxval is learned but custom_approx_params['ste_backward'] is off: "
                                   "this forward would train nothing (switch ste_backward on, or run under no_grad)")
            if self.ste_backward and (x_float.requires_grad or mx.requires_grad):
                return _FakeQuantTrain.apply(x_float, mx, self)
        res, self.custom_bias = quantize_to_fp8_ste_MM(x_float, self.n_bits, mx.detach() if mx.requires_grad else mx,
                                                       self._mbits_int, self.sign_bits)
        return res

    def set_quant_range(self, x_min, x_max):
        if self._make_unsigned(x_min):
            self.sign_bits = 0
        if self.set_maxval:
            if not isinstance(x_max, torch.Tensor):
                x_max = torch.tensor([float(x_max)], device=self.maxval.device)
                x_min = torch.tensor([float(x_min)], device=self.maxval.device)
            mx = torch.abs(torch.max(torch.abs(x_min), x_max))
            self._assign_maxval(mx.reshape(1) if mx.dim() == 0 else mx)

    def fix_ranges(self):
        """A learned maxval becomes a plain tensor again, same data (the reference calls a parameter_to_fixed
        that it never defines)."""
        if isinstance(self.maxval, nn.Parameter):
            data = self.maxval.detach()
            del self.maxval
            self.maxval = data

    def learn_maxval(self):
        self.learning_maxval = True
        if not isinstance(self.maxval, nn.Parameter):
            self.maxval = nn.Parameter(self.maxval.detach())

    def make_range_trainable(self):
        if self.learning_mantissa_bits:
            raise NotImplementedError("learned mantissa widths are out of scope: an approx layer's error table "
                                      "belongs to one format and the kernels take an integer width")
        if not self.learning_maxval:
            # (the reference is a silent no-op here; training nothing is the failure to avoid)
            raise NotImplementedError("this FPQuantizer was not built with learn_maxval=True: nothing to learn")
        self.learn_maxval()

    def reset(self):
        pass

    def extra_repr(self):
        return f"n_bits={self.n_bits}, mantissa_bits={self._mbits_int}, per_channel={self.per_channel}"
