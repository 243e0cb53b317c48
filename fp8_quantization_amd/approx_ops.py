"""Host side of the approx_v9 hot path: torch custom ops over the gfx950 C-ABI.

Mirrors the reference module approx/approx_matmul_whole_v9.py (revollllt/FP8_quantization
@ 2024-11-08): ``custom_matmul_vectorize`` keeps its signature and argument meaning
(v9:10-18), ``quant_to_fp_any_vectorize_torch`` (v9:333) and ``float_to_fpany_absint_torch``
(v9:233, here taking (E, M, bias) instead of a param dict) are the element codecs,
``get_error_table_NN`` the table selection (v9:555).  All arithmetic runs in
libfp8approx.so; these wrappers only marshal pointers, biases and flags.

Bias typing follows the reference: Python ints select the int-bias semantics, int tensors the
tensor-bias semantics (quirk F5 -- param_prepare's integer powers flush min_norm to 0), which
is what approx_multiply passes for single-column products (approx_calculation.py:800-809).
"""
import ctypes
import os
from typing import Optional

import torch
from torch import nn

from . import _lib
from .error_tables import get_error_table_NN  # noqa: F401  (re-exported, v9:555)

__all__ = ["custom_matmul_vectorize", "approx_matmul", "approx_bmm", "approx_matmul_block", "approx_terms", "approx_conv2d", "qamaa_matmul", "qamaa_conv2d",
           "quant_to_fp_any_vectorize_torch", "float_to_fpany_absint_torch", "get_error_table_NN",
           "make_flags", "make_flags_v5", "fp8_fake_quantize", "bn_act_epilogue", "dense_format", "dense_matmul",
           "dense_conv2d", "grouped_conv2d", "dense_conv2d_fused", "approx_matmul_check", "approx_conv2d_check", "approx_bmm_check",
           "CheckStats", "format_self_check", "SELF_CHECK_LABELS", "fp8_mse_losses", "bn_train", "grad_bmm", "grad_split_auto",
           "ste_linear", "ste_bmm", "ste_conv2d", "fp8_fake_quantize_train", "fp8_fake_quantize_backward"]


def make_flags(with_approx=True, with_s2nn2s_opt=False, quant_btw_mult_accu=True, golden_clip_OF=False,
               tensor_bias=False):
    return ((_lib.APPROX if with_approx else 0) | (_lib.S2N if with_s2nn2s_opt else 0) |
            (_lib.QBMA if quant_btw_mult_accu else 0) | (_lib.GCLIP if golden_clip_OF else 0) |
            (_lib.TB if tensor_bias else 0))


def make_flags_v5(sim_hw_add_OFUF=False, with_OF_opt=False, with_UF_opt=False):
    """Flags of the v5 integer-adder model (approx_matmul_whole_v5.py:155-183)."""
    return (_lib.V5 | (_lib.OFUF if sim_hw_add_OFUF else 0) | (_lib.OF_OPT if with_OF_opt else 0) |
            (_lib.UF_OPT if with_UF_opt else 0))


def _uses_table(flags):
    return bool(flags & (_lib.APPROX | _lib.V5))


_BIAS_CACHE = {}

# bench.py sets this to a list to time every approx launch with HIP events on the current
# stream: entries (start_event, end_event, approx_MACs).  None = no instrumentation.
_PROFILE = None


def _prof_start():
    if _PROFILE is None:
        return None
    ev = torch.cuda.Event(enable_timing=True)
    ev.record()
    return ev


def _prof_end(start, macs, nbytes=0):
    """nbytes: the launch's algorithmic HBM bytes (operands read once, output written once), for
    the memory-bound dense exact product; 0 for the approx ops (priced by MACs)."""
    if start is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        _PROFILE.append((start, ev, int(macs), int(nbytes)))


def _bias_dev(b, device, n=None):
    """Device int32 bias vector from an int or a (float/int) tensor; no host sync for tensors."""
    if isinstance(b, torch.Tensor):
        i32 = getattr(b, "_fp8a_i32", None)  # set by fp8_fake_quantize: no conversion launch
        if i32 is not None and i32.device == device:
            return i32
        t = b.detach().reshape(-1)
        if t.device != device:
            t = t.to(device)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)  # float biases are torch.round() outputs: exact
        return t.contiguous()
    key = (device, int(b))
    t = _BIAS_CACHE.get(key)
    if t is None:
        t = torch.tensor([int(b)], dtype=torch.int32, device=device)
        _BIAS_CACHE[key] = t
    return t


def _table_host(error_table_NN, mant_width, with_approx):
    n = 2 ** mant_width
    if error_table_NN is None or not with_approx:
        return torch.zeros((n, n), dtype=torch.int32)
    t = error_table_NN.detach()
    if t.device.type != "cpu" or t.dtype != torch.int32 or not t.is_contiguous():
        t = t.to(device="cpu", dtype=torch.int32).contiguous()  # host table: packed into kernargs
    if t.shape != (n, n):
        raise AssertionError(f"error table must be {n}x{n}, got {tuple(t.shape)}")
    return t


def _workspace(device, nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _as_f32(x):
    if x.dtype != torch.float32:
        x = x.float()
    return x


# ----------------------------------------------------------------------------------- matmul
@torch.library.custom_op("fp8approx::matmul", mutates_args=())
def _matmul_op(A: torch.Tensor, B: torch.Tensor, bA: torch.Tensor, bB: torch.Tensor, bR: torch.Tensor,
               table: torch.Tensor, E: int, M: int, flags: int) -> torch.Tensor:
    L = _lib.load()
    dev = A.device
    if not A.is_contiguous() and A.stride(1) != 1:
        A = A.contiguous()
    Mr, K = A.shape
    N = B.shape[1]
    C = torch.empty((Mr, N), dtype=torch.float32, device=dev)
    ws = _workspace(dev, L.fp8a_matmul_workspace_size_mnk(Mr, N, K))
    bBs = 0 if bB.numel() == 1 else 1
    rc = L.fp8a_matmul(_lib.dev_ptr(A), A.stride(0), _lib.dev_ptr(B), B.stride(0), B.stride(1),
                       _lib.dev_ptr(C), N, Mr, N, K, E, M, _lib.dev_ptr(bA), _lib.dev_ptr(bB), bBs,
                       _lib.dev_ptr(bR), _lib.host_ptr(table), flags, _lib.dev_ptr(ws), ws.numel(),
                       _lib.stream_ptr(dev))
    _lib.check(rc, "fp8a_matmul")
    return C


@_matmul_op.register_fake
def _(A, B, bA, bB, bR, table, E, M, flags):
    return A.new_empty((A.shape[0], B.shape[1]), dtype=torch.float32)


def approx_matmul(A, B, E, M, bA, bB, bR, table=None, flags=None, **flag_kwargs):
    """C[m, n] = sum_k approx_v9 term(A[m, k], B[k, n]) on the GPU.

    A [M, K] and B [K, N] float32 device tensors (any strides with a unit stride dimension;
    weight.t() views are consumed in place).  bB: int, 1-element or per-column [N] tensor.
    """
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise AssertionError(f"approx_matmul: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")  # v9:20
    if flags is None:
        flags = make_flags(**flag_kwargs)
    A, B = _as_f32(A), _as_f32(B)
    if B.stride(0) != 1 and B.stride(1) != 1:
        B = B.contiguous()
    dev = A.device
    tab = _table_host(table, M, _uses_table(flags))
    bB_ = _bias_dev(bB, dev)
    if bB_.numel() not in (1, B.shape[1]):
        raise AssertionError(f"approx_matmul: {bB_.numel()} column biases for {B.shape[1]} columns")
    ev = _prof_start()
    C = _matmul_op(A, B, _bias_dev(bA, dev), bB_, _bias_dev(bR, dev), tab, int(E), int(M), int(flags))
    _prof_end(ev, A.shape[0] * A.shape[1] * B.shape[1])
    return C


# ----------------------------------------------------------------------------------- batched matmul
def _bmm_view(t, what):
    """(nb0, nb1, s0, s1) of a [b, r, c] / [b0, b1, r, c] view: the two-stride batch form."""
    if t.dim() == 3:
        return 1, t.shape[0], 0, t.stride(0)
    if t.dim() == 4:
        return t.shape[0], t.shape[1], t.stride(0), t.stride(1)
    raise AssertionError(f"approx_bmm: {what} needs one or two leading batch dims, got {tuple(t.shape)}")


def _bmm_geometry(A, B):
    """fp8a_bmm's and fp8a_bmm_check's (nb0, nb1, M, N, K, lda, sa0, sa1, sbk, sbn, sb0, sb1)."""
    nb0, nb1, sa0, sa1 = _bmm_view(A, "A")
    _, _, sb0, sb1 = _bmm_view(B, "B")
    return (nb0, nb1, A.shape[-2], B.shape[-1], A.shape[-1], A.stride(-2), sa0, sa1, B.stride(-2), B.stride(-1),
            sb0, sb1)


def _bmm_operands(who, A, B, M, bA, bB, bR, table, flags):
    """approx_bmm's and approx_bmm_check's operands: float32, A with a unit k stride, the host table and the device
    biases.  Returns (A, B, bA, bB, bR, table)."""
    A, B = _as_f32(A), _as_f32(B)
    if A.stride(-1) != 1 and A.shape[-1] > 1:
        A = A.contiguous()
    dev = A.device
    tab = _table_host(table, M, _uses_table(flags))
    bB_ = _bias_dev(bB, dev)
    if bB_.numel() not in (1, B.shape[-1]):
        raise AssertionError(f"{who}: {bB_.numel()} column biases for {B.shape[-1]} columns")
    return A, B, _bias_dev(bA, dev), bB_, _bias_dev(bR, dev), tab


@torch.library.custom_op("fp8approx::bmm", mutates_args=("out",))
def _bmm_op(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, bA: torch.Tensor, bB: torch.Tensor,
            bR: torch.Tensor, table: torch.Tensor, E: int, M: int, flags: int) -> None:
    L = _lib.load()
    _, _, sc0, sc1 = _bmm_view(out, "out")
    bBs = 0 if bB.numel() == 1 else 1
    rc = L.fp8a_bmm(_lib.dev_ptr(A), _lib.dev_ptr(B), _lib.dev_ptr(out), *_bmm_geometry(A, B), out.stride(-2), sc0, sc1,
                    E, M, _lib.dev_ptr(bA), _lib.dev_ptr(bB), bBs, _lib.dev_ptr(bR), _lib.host_ptr(table), flags,
                    _lib.stream_ptr(A.device))
    _lib.check(rc, "fp8a_bmm")


@_bmm_op.register_fake
def _(A, B, out, bA, bB, bR, table, E, M, flags):
    return None


def approx_bmm(A, B, E, M, bA, bB, bR, table=None, flags=None, out=None, **flag_kwargs):
    """C[..., m, n] = sum_k approx_v9 term(A[..., m, k], B[..., k, n]) on the GPU, one launch for all batch items.

    A [..., M, K] and B [..., K, N] float32 device tensors with one or two equal leading batch dims.  Views are
    consumed in place -- head views cut from [B, S, H*d] buffers, a transposed B -- as long as A's k stride
    is 1 (else a contiguous copy is taken).  bA, bR: int or 1-element tensor; bB: int, 1-element or per-column
    [N] tensor.  out: None, or a float32 view of C's shape with unit n stride that does not overlap A or B
    (attention writes its context straight into [B, S, H, d]).  Returns C (out when given).
    """
    if A.dim() not in (3, 4) or A.dim() != B.dim() or A.shape[:-2] != B.shape[:-2] or A.shape[-1] != B.shape[-2]:
        raise AssertionError(f"approx_bmm: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")  # v9:20
    if flags is None:
        flags = make_flags(**flag_kwargs)
    shape = tuple(A.shape[:-1]) + (B.shape[-1],)
    dev = A.device
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != dev or \
            (out.stride(-1) != 1 and shape[-1] > 1):
        raise AssertionError(f"approx_bmm: out must be a float32 {shape} view with unit n stride on {dev}")
    A, B, bA_, bB_, bR_, tab = _bmm_operands("approx_bmm", A, B, M, bA, bB, bR, table, flags)
    ev = _prof_start()
    _bmm_op(A, B, out, bA_, bB_, bR_, tab, int(E), int(M), int(flags))
    _prof_end(ev, A.numel() * B.shape[-1])
    return out


@torch.library.custom_op("fp8approx::matmul_block", mutates_args=())
def _matmul_block_op(A: torch.Tensor, B: torch.Tensor, bA: Optional[torch.Tensor], bB: torch.Tensor,
                     bR: torch.Tensor, table: torch.Tensor, E: int, M: int, flags: int, bn: Optional[torch.Tensor],
                     in_maxval: Optional[torch.Tensor], in_nbits: int, in_mbits: int, in_sign_bits: int,
                     res: Optional[torch.Tensor], post_act: int, post_lo: float, post_hi: float,
                     out_maxval: Optional[torch.Tensor], out_nbits: int, out_mbits: int, out_sign_bits: int
                     ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8a_matmul_block: C = fq_out(clamp(bn(fq_in(A) @ B) + res)); returns C and the input /
    output quantizers' float and int32 biases (1-element tensors, unset when unused)."""
    L = _lib.load()
    dev = A.device
    A = A.contiguous()
    Mr, K = A.shape
    N = B.shape[1]
    C = torch.empty((Mr, N), dtype=torch.float32, device=dev)
    ib, iib = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    ob, oib = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    if res is not None:
        res = res.contiguous()
        if res.shape != C.shape or res.dtype != torch.float32 or res.device != dev:
            raise AssertionError(f"approx_matmul_block: residual must be float32 {tuple(C.shape)} on {dev}")
    if bn is not None and (bn.shape != (N, 2) or bn.dtype != torch.float32 or not bn.is_contiguous()):
        raise AssertionError(f"approx_matmul_block: epilogue parameters must be contiguous float32 [{N}, 2]")
    ws = _workspace(dev, L.fp8a_matmul_block_workspace_size(Mr, N, K))
    opt = lambda t: _lib.dev_ptr(t) if t is not None else None  # noqa: E731
    rc = L.fp8a_matmul_block(_lib.dev_ptr(A), K, _lib.dev_ptr(B), B.stride(0), B.stride(1), _lib.dev_ptr(C), N, Mr,
                             N, K, E, M, opt(bA), _lib.dev_ptr(bB), 0 if bB.numel() == 1 else 1, _lib.dev_ptr(bR),
                             _lib.host_ptr(table), flags, opt(bn), 0, 0.0, 0.0, opt(in_maxval), int(in_nbits),
                             int(in_mbits), int(in_sign_bits), _lib.dev_ptr(ib), _lib.dev_ptr(iib), opt(res),
                             int(post_act), float(post_lo), float(post_hi), opt(out_maxval), int(out_nbits),
                             int(out_mbits), int(out_sign_bits), _lib.dev_ptr(ob), _lib.dev_ptr(oib), _lib.dev_ptr(ws),
                             ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "fp8a_matmul_block")
    return C, ib, iib, ob, oib


@_matmul_block_op.register_fake
def _(A, B, bA, bB, bR, table, E, M, flags, bn, in_maxval, in_nbits, in_mbits, in_sign_bits, res, post_act, post_lo,
      post_hi, out_maxval, out_nbits, out_mbits, out_sign_bits):
    one = A.new_empty((1,))
    onei = A.new_empty((1,), dtype=torch.int32)
    return A.new_empty((A.shape[0], B.shape[1])), one, onei, one.clone(), onei.clone()


def bias_epilogue(bias, device):
    """The store epilogue {1, bias} per column for a linear's bias: x * 1 + bias is exactly the
    reference's ``out += bias``."""
    with torch.no_grad():
        b = _as_f32(bias.detach()).reshape(-1).to(device)
        return torch.stack((torch.ones_like(b), b), dim=1).contiguous()


def approx_matmul_block(A, B, E, M, bA, bB, bR, table=None, flags=None, bias=None, qin=None, post=None,
                        bias_epi=None):
    """approx_matmul with the linear layer's neighbours fused into the same launch:
    C = fq_out(clamp(fq_in(A) @ B + bias + residual)).

    bias: the linear's bias [N] or None (applied as the store's x * 1 + bias, i.e. exactly the
    reference's ``out += bias``); bias_epi: the same as a prebuilt ``bias_epilogue`` tensor.  qin / post: as approx_conv2d (per-tensor quantizer tuples; A is
    then UNQUANTIZED and bA unused).  Returns ``(C, input quantizer bias or None, output quantizer
    bias or None)``."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise AssertionError(f"approx_matmul: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")  # v9:20
    A, B = _as_f32(A), _as_f32(B)
    if B.stride(0) != 1 and B.stride(1) != 1:
        B = B.contiguous()
    dev = A.device
    tab = _table_host(table, M, _uses_table(flags))
    bB_ = _bias_dev(bB, dev)
    if bB_.numel() not in (1, B.shape[1]):
        raise AssertionError(f"approx_matmul: {bB_.numel()} column biases for {B.shape[1]} columns")
    bn = bias_epi if bias_epi is not None else (bias_epilogue(bias, dev) if bias is not None else None)
    iq = _quantizer_args(qin) if qin is not None else (None, 0, 0, 0)
    res, pact, plo, phi, oq = post if post is not None else (None, 0, 0.0, 0.0, None)
    oq = _quantizer_args(oq) if oq is not None else (None, 0, 0, 0)
    ev = _prof_start()
    C, ib, iib, ob, oib = _matmul_block_op(
        A, B, None if qin is not None else _bias_dev(bA, dev), bB_, _bias_dev(bR, dev), tab, int(E), int(M),
        int(flags), bn, iq[0].to(dev) if iq[0] is not None else None, iq[1], iq[2], iq[3],
        _as_f32(res) if res is not None else None, int(pact), float(plo), float(phi),
        oq[0].to(dev) if oq[0] is not None else None, oq[1], oq[2], oq[3])
    _prof_end(ev, A.shape[0] * A.shape[1] * B.shape[1])
    ib._fp8a_i32 = iib
    ob._fp8a_i32 = oib
    return C, (ib if qin is not None else None), (ob if oq[0] is not None else None)


def approx_terms(A, B, E, M, bA, bB, bR, table=None, flags=None, **flag_kwargs):
    """Per-product terms T[m, k, n] (the values the reference sums at v9:113); parity tool."""
    if A.shape[1] != B.shape[0]:
        raise AssertionError("approx_terms: inner dimensions differ")
    if flags is None:
        flags = make_flags(**flag_kwargs)
    L = _lib.load()
    A, B = _as_f32(A), _as_f32(B)
    dev = A.device
    Mr, K = A.shape
    N = B.shape[1]
    T = torch.empty((Mr, K, N), dtype=torch.float32, device=dev)
    bA_, bB_, bR_ = _bias_dev(bA, dev), _bias_dev(bB, dev), _bias_dev(bR, dev)
    tab = _table_host(table, M, _uses_table(flags))
    rc = L.fp8a_terms(_lib.dev_ptr(A), A.stride(0), _lib.dev_ptr(B), B.stride(0), B.stride(1), _lib.dev_ptr(T),
                      Mr, N, K, int(E), int(M), _lib.dev_ptr(bA_), _lib.dev_ptr(bB_), 0 if bB_.numel() == 1 else 1,
                      _lib.dev_ptr(bR_), _lib.host_ptr(tab), int(flags), _lib.stream_ptr(dev))
    _lib.check(rc, "fp8a_terms")
    return T


# ----------------------------------------------------------------------------------- self-check
class _CheckStatsStruct(ctypes.Structure):
    """fp8a_check_stats (include/fp8approx.h): 96 bytes, natural alignment."""
    _fields_ = [("n_out", ctypes.c_uint64), ("sum_err", ctypes.c_double), ("sum_err2", ctypes.c_double),
                ("sum_gold2", ctypes.c_double), ("a_norm", ctypes.c_uint64), ("a_total", ctypes.c_uint64),
                ("b_norm", ctypes.c_uint64), ("b_total", ctypes.c_uint64), ("r_norm", ctypes.c_uint64),
                ("r_total", ctypes.c_uint64), ("max_err", ctypes.c_float), ("prod_max_abs", ctypes.c_float),
                ("prod_max_rel", ctypes.c_float), ("has_prod", ctypes.c_uint32)]


CHECK_STATS_BYTES = ctypes.sizeof(_CheckStatsStruct)


class CheckStats:
    """The raw fields of fp8a_check_stats plus the figures the reference prints from them
    (approx_matmul_whole_v9.py:124-157).  ``raw`` keeps the struct's bytes, ``S`` the device tensor
    of sum_k |v_k| (the scale of the project's 1e-5 S bar) in the output's shape, when the op
    returned one."""
    FIELDS = tuple(n for n, _ in _CheckStatsStruct._fields_)

    def __init__(self, S=None, raw=None, **fields):
        for n in self.FIELDS:
            setattr(self, n, fields.pop(n, 0))
        if fields:
            raise TypeError(f"unknown CheckStats fields: {sorted(fields)}")
        self.S = S
        self.raw = raw

    @classmethod
    def from_bytes(cls, buf, S=None):
        buf = bytes(buf)
        st = _CheckStatsStruct.from_buffer_copy(buf)
        return cls(S=S, raw=buf, **{n: getattr(st, n) for n in cls.FIELDS})

    @property
    def max(self):
        return self.max_err

    @property
    def mean(self):
        return self.sum_err / self.n_out if self.n_out else 0.0

    @property
    def rmse(self):
        return (self.sum_err2 / self.n_out) ** 0.5 if self.n_out else 0.0

    @property
    def sqnr_db(self):
        """10 log10(sum G^2 / sum e^2): inf when the approx sum equals the golden one everywhere."""
        import math
        if self.sum_err2 == 0.0:
            return math.inf
        return 10.0 * math.log10(self.sum_gold2 / self.sum_err2) if self.sum_gold2 > 0.0 else -math.inf

    @staticmethod
    def _pct(num, den):
        return 100.0 * num / den if den else None

    @property
    def a_norm_pct(self):
        return self._pct(self.a_norm, self.a_total)

    @property
    def b_norm_pct(self):
        return self._pct(self.b_norm, self.b_total)

    @property
    def r_norm_pct(self):
        """None with with_s2nn2s_opt: the reference has no R_3d mask there (v9:122)."""
        return self._pct(self.r_norm, self.r_total)

    def as_dict(self):
        d = {n: getattr(self, n) for n in self.FIELDS}
        d.update(mean=self.mean, rmse=self.rmse, sqnr_db=self.sqnr_db, a_norm_pct=self.a_norm_pct,
                 b_norm_pct=self.b_norm_pct, r_norm_pct=self.r_norm_pct)
        return d

    def __repr__(self):
        return "CheckStats(" + ", ".join(f"{k}={v}" for k, v in self.as_dict().items()) + ")"


# the labels of the reference's self-check block, in its order (v9:147-157)
SELF_CHECK_LABELS = ("====== Self-Checking Mode ======", "With Approximation    =", "With S2N & N2S Opt    =",
                     "Quant btw Mult & Accu =", "Normal Values in A_2d :", "Normal Values in B_2d :",
                     "Normal Values in R_3d :", "MatMul Max  Error     :", "MatMul Mean Error     :",
                     "MatMul RMSE           :")


def format_self_check(stats, flags):
    """The reference's self-check block (v9:147-157) from a CheckStats: same labels, same order;
    the R_3d line only without with_s2nn2s_opt."""
    L = SELF_CHECK_LABELS
    s2n = bool(flags & _lib.S2N)
    lines = ["", L[0], f"{L[1]} {bool(flags & _lib.APPROX)}", f"{L[2]} {s2n}", f"{L[3]} {bool(flags & _lib.QBMA)}",
             f"{L[4]} {stats.a_norm}/{stats.a_total} = {stats.a_norm_pct:.1f}%",
             f"{L[5]} {stats.b_norm}/{stats.b_total} = {stats.b_norm_pct:.1f}%"]
    if not s2n:
        lines.append(f"{L[6]} {stats.r_norm}/{stats.r_total} = {stats.r_norm_pct:.1f}%")
    lines += [f"{L[7]} {stats.max_err}", f"{L[8]} {stats.mean}", f"{L[9]} {stats.rmse}"]
    return "\n".join(lines)


def _aligned_workspace(device, nbytes):
    """A 256-byte aligned uint8 view of at least nbytes."""
    buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % 256
    return buf[off:off + int(nbytes)]


def _check_prod(prod, like):
    if prod is None:
        return None
    prod = _as_f32(prod).contiguous()
    if prod.shape != like.shape or prod.device != like.device:
        raise AssertionError(f"self-check: prod must be {tuple(like.shape)} on {like.device}")
    return prod


def _run_check(entry, call, shape, dev, nbytes, prod):
    """The approx_*_check functions' tail: C, G, the stats struct and an aligned workspace of nbytes; the C-ABI call
    ``call(C's pointer, G, Cprod, stats, workspace, workspace_bytes, stream) -> rc``; S as a view of the workspace's
    head in C's shape; one synchronising read-back of the struct.  Returns ``(C, G, CheckStats)``."""
    C = torch.empty(shape, dtype=torch.float32, device=dev)
    G = torch.empty_like(C)
    prod = _check_prod(prod, C)
    stats = torch.empty(CHECK_STATS_BYTES, dtype=torch.uint8, device=dev)
    ws = _aligned_workspace(dev, nbytes)
    rc = call(_lib.dev_ptr(C), _lib.dev_ptr(G), _lib.dev_ptr(prod), _lib.dev_ptr(stats), _lib.dev_ptr(ws), ws.numel(),
              _lib.stream_ptr(dev))
    _lib.check(rc, entry)
    S = ws[:C.numel() * 4].view(torch.float32).view(C.shape)
    return C, G, CheckStats.from_bytes(stats.cpu().numpy().tobytes(), S=S)


def approx_matmul_check(A, B, E, M, bA, bB, bR, table=None, flags=None, prod=None, **flag_kwargs):
    """The fused self-check of one product (fp8a_matmul_check): returns ``(C, G, CheckStats)`` with
    C the approx sum, G the golden sum (v9:30-36, 145) and the error / normal-value statistics of
    the reference's self_check_mode, reduced on the GPU -- no [M, K, N] tensor.  prod: a production
    result (approx_matmul's) to compare C against (prod_max_abs / prod_max_rel).  Operands and
    biases as approx_matmul.  Reads the struct back with one synchronising copy."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise AssertionError(f"approx_matmul_check: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")  # v9:20
    if flags is None:
        flags = make_flags(**flag_kwargs)
    L = _lib.load()
    A, B = _as_f32(A), _as_f32(B)
    if A.stride(1) != 1:
        A = A.contiguous()
    if B.stride(0) != 1 and B.stride(1) != 1:
        B = B.contiguous()
    dev = A.device
    Mr, K = A.shape
    N = B.shape[1]
    tab = _table_host(table, M, _uses_table(flags))
    bA_, bB_, bR_ = _bias_dev(bA, dev), _bias_dev(bB, dev), _bias_dev(bR, dev)
    if bB_.numel() not in (1, N):
        raise AssertionError(f"approx_matmul_check: {bB_.numel()} column biases for {N} columns")

    def call(C, *tail):
        return L.fp8a_matmul_check(_lib.dev_ptr(A), A.stride(0), _lib.dev_ptr(B), B.stride(0), B.stride(1), C, N, Mr, N,
                                   K, int(E), int(M), _lib.dev_ptr(bA_), _lib.dev_ptr(bB_),
                                   0 if bB_.numel() == 1 else 1, _lib.dev_ptr(bR_), _lib.host_ptr(tab), int(flags), *tail)
    return _run_check("fp8a_matmul_check", call, (Mr, N), dev, L.fp8a_check_workspace_size(Mr, N, K), prod)


def approx_conv2d_check(x, w, E, M, bA, bW, bR, table=None, flags=None, stride=(1, 1), padding=(0, 0),
                        dilation=(1, 1), groups=1, prod=None, **flag_kwargs):
    """The fused self-check of one convolution (fp8a_conv2d_check): ``(y, G, CheckStats)`` in NCHW,
    the statistics over all groups; single-output-channel groups take the tensor-bias semantics as
    approx_conv2d.  prod: approx_conv2d's result (before any conv bias) to compare y against."""
    if flags is None:
        flags = make_flags(**flag_kwargs)
    flags &= ~_lib.TB
    L = _lib.load()
    x, w = _as_f32(x).contiguous(), _as_f32(w).contiguous()
    dev = x.device
    tab = _table_host(table, M, _uses_table(flags))
    bW_ = _bias_dev(bW, dev)
    if bW_.numel() == 1:
        bW_ = bW_.expand(w.shape[0]).contiguous()
    if bW_.numel() != w.shape[0]:
        raise AssertionError(f"approx_conv2d_check: {bW_.numel()} weight biases for {w.shape[0]} output channels")
    bA_, bR_ = _bias_dev(bA, dev), _bias_dev(bR, dev)
    Bn, Cin, H, W = x.shape
    Cout, cig, kh, kw = w.shape
    if groups <= 0 or Cin % groups or Cout % groups or cig != Cin // groups:
        raise AssertionError(f"approx_conv2d_check: weight {tuple(w.shape)} does not fit {Cin} channels in {groups} groups")
    stride, padding, dilation = [int(v) for v in stride], [int(v) for v in padding], [int(v) for v in dilation]
    geo = (*_conv_geometry(x, w, stride, padding, dilation), int(groups))
    nbytes = L.fp8a_conv2d_check_workspace_size(*geo)
    if nbytes == 0:
        raise AssertionError("approx_conv2d_check: empty or inconsistent convolution geometry")

    def call(y, *tail):
        return L.fp8a_conv2d_check(_lib.dev_ptr(x), _lib.dev_ptr(w), y, *geo, int(E), int(M), _lib.dev_ptr(bA_),
                                   _lib.dev_ptr(bW_), _lib.dev_ptr(bR_), _lib.host_ptr(tab), int(flags), *tail)
    return _run_check("fp8a_conv2d_check", call, _conv_out_shape(x, w, stride, padding, dilation), dev, nbytes, prod)


def approx_bmm_check(A, B, E, M, bA, bB, bR, table=None, flags=None, prod=None, **flag_kwargs):
    """The fused self-check of one batched product (fp8a_bmm_check): ``(C, G, CheckStats)`` with C, G and
    ``CheckStats.S`` dense in the product's shape [..., M, N], the statistics over all batch items (every
    item's A and B counted once).  Operands and biases as approx_bmm: one or two equal leading batch dims,
    views consumed in place as long as A's k stride is 1.  prod: approx_bmm's result (any float32 tensor of
    C's shape; made contiguous) to compare C against.  Reads the struct back with one synchronising copy."""
    if A.dim() not in (3, 4) or A.dim() != B.dim() or A.shape[:-2] != B.shape[:-2] or A.shape[-1] != B.shape[-2]:
        raise AssertionError(f"approx_bmm_check: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")  # v9:20
    if flags is None:
        flags = make_flags(**flag_kwargs)
    L = _lib.load()
    A, B, bA_, bB_, bR_, tab = _bmm_operands("approx_bmm_check", A, B, M, bA, bB, bR, table, flags)
    geo = _bmm_geometry(A, B)  # (nb0, nb1, M, N, K, the strides)

    def call(C, *tail):
        return L.fp8a_bmm_check(_lib.dev_ptr(A), _lib.dev_ptr(B), C, *geo, int(E), int(M), _lib.dev_ptr(bA_),
                                _lib.dev_ptr(bB_), 0 if bB_.numel() == 1 else 1, _lib.dev_ptr(bR_), _lib.host_ptr(tab),
                                int(flags), *tail)
    return _run_check("fp8a_bmm_check", call, tuple(A.shape[:-1]) + (geo[3],), A.device,
                      L.fp8a_bmm_check_workspace_size(*geo[:5]), prod)


def custom_matmul_vectorize(A, B, expo_width, mant_width, custom_bias_A, custom_bias_B, custom_bias_R,
                            error_table_NN, with_approx=True, with_s2nn2s_opt=False, sim_hw_add_OFUF=False,
                            with_OF_opt=False, with_UF_opt=False, golden_clip_OF=False, quant_btw_mult_accu=True,
                            debug_mode=False, self_check_mode=False):
    """Drop-in for approx_matmul_whole_v9.custom_matmul_vectorize (v9:10-169).

    sim_hw_add_OFUF / with_OF_opt / with_UF_opt are accepted and ignored, as in v9.
    """
    assert A.shape[1] == B.shape[0]
    tb = [isinstance(b, torch.Tensor) for b in (custom_bias_A, custom_bias_B, custom_bias_R)]
    if any(tb) and not all(tb):
        raise NotImplementedError("mixed int / tensor biases: pass all three the same way")
    flags = make_flags(with_approx, with_s2nn2s_opt, quant_btw_mult_accu, golden_clip_OF, tensor_bias=all(tb))
    out = approx_matmul(A, B, expo_width, mant_width, custom_bias_A, custom_bias_B, custom_bias_R,
                        error_table_NN, flags=flags)
    if self_check_mode:  # v9:119-157 on the fused check kernel: no [M, K, N] tensor
        _, _, stats = approx_matmul_check(A, B, expo_width, mant_width, custom_bias_A, custom_bias_B, custom_bias_R,
                                          error_table_NN, flags=flags, prod=out)
        print(format_self_check(stats, flags))
    return out


# ----------------------------------------------------------------------------------- codecs
def _codec_bias(custom_bias, device):
    if custom_bias is None:
        raise NotImplementedError("pass the bias explicitly")
    return _bias_dev(custom_bias, device), isinstance(custom_bias, torch.Tensor)


def quant_to_fp_any_vectorize_torch(arr, expo_width, mant_width, custom_bias=None, clip_OF=True):
    """Q_R (v9:333-362) on the GPU.  custom_bias None means the IEEE-style default 2^(E-1)-1."""
    if custom_bias is None:
        custom_bias = 2 ** (expo_width - 1) - 1
    L = _lib.load()
    x = _as_f32(arr).contiguous()
    b, tb = _codec_bias(custom_bias, x.device)
    out = torch.empty_like(x)
    rc = L.fp8a_quant(_lib.dev_ptr(x), x.numel(), int(expo_width), int(mant_width), _lib.dev_ptr(b),
                      make_flags(False, False, False, clip_OF, tb), _lib.dev_ptr(out), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_quant")
    return out


def float_to_fpany_absint_torch(values, expo_width, mant_width, custom_bias, clip_OF=False):
    """DEC (v9:233-291): returns (expo, mant) int32 tensors shaped like values."""
    L = _lib.load()
    x = _as_f32(values).contiguous()
    b, tb = _codec_bias(custom_bias, x.device)
    e = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    m = torch.empty_like(e)
    rc = L.fp8a_decompose(_lib.dev_ptr(x), 1, x.numel(), x.numel(), int(expo_width), int(mant_width),
                          _lib.dev_ptr(b), 0, make_flags(False, False, False, clip_OF, tb), _lib.dev_ptr(e),
                          _lib.dev_ptr(m), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_decompose")
    return e, m


# ----------------------------------------------------------------------------------- conv
def _conv_geometry(x, w, stride, padding, dilation):
    """(Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw): the C-ABI's geometry arguments."""
    Bn, Cin, H, W = x.shape
    Cout, _, kh, kw = w.shape
    return (Bn, Cin, H, W, Cout, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1])


def _conv_out_shape(x, w, stride, padding, dilation):
    Bn, _, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw = _conv_geometry(x, w, stride, padding, dilation)
    return (Bn, Cout, (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1)


def _conv_lead_args(x, w, y, geo, groups, E, M, bA, bW, bR, table, flags):
    """The leading arguments of fp8a_conv2d and its bn_act / block / chain forms."""
    return (_lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y), *geo, groups, E, M, _lib.dev_ptr(bA), _lib.dev_ptr(bW),
            _lib.dev_ptr(bR), _lib.host_ptr(table), flags)


@torch.library.custom_op("fp8approx::conv2d", mutates_args=())
def _conv2d_op(x: torch.Tensor, w: torch.Tensor, bA: torch.Tensor, bW: torch.Tensor, bR: torch.Tensor,
               table: torch.Tensor, E: int, M: int, flags: int, stride: list[int], padding: list[int],
               dilation: list[int], groups: int, bn: Optional[torch.Tensor] = None, act: int = 0,
               act_lo: float = 0.0, act_hi: float = 0.0) -> torch.Tensor:
    L = _lib.load()
    x = x.contiguous()
    w = w.contiguous()
    geo = _conv_geometry(x, w, stride, padding, dilation)
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, L.fp8a_conv2d_workspace_size(*geo, groups))
    lead = _conv_lead_args(x, w, y, geo, groups, E, M, bA, bW, bR, table, flags)
    tail = (_lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
    if bn is None:
        _lib.check(L.fp8a_conv2d(*lead, *tail), "fp8a_conv2d")
        return y
    Cout = w.shape[0]
    if bn.shape != (Cout, 2) or bn.dtype != torch.float32 or not bn.is_contiguous() or bn.device != x.device:
        raise AssertionError(f"approx_conv2d: epilogue parameters must be contiguous float32 [{Cout}, 2] "
                             f"on {x.device}, got {tuple(bn.shape)} {bn.dtype} on {bn.device}")
    rc = L.fp8a_conv2d_bn_act(*lead, _lib.dev_ptr(bn), int(act), float(act_lo), float(act_hi), *tail)
    _lib.check(rc, "fp8a_conv2d_bn_act")
    return y


def _conv2d_fake(x, w, bA, bW, bR, table, E, M, flags, stride, padding, dilation, *rest, **kw):
    return x.new_empty(_conv_out_shape(x, w, stride, padding, dilation))


_conv2d_op.register_fake(_conv2d_fake)


def _block_call(entry, x, w, bA, bW, bR, table, E, M, flags, stride, padding, dilation, groups, in_q, res, post,
                out_q, bn, act, chain=None):
    """fp8a_conv2d_block, or fp8a_conv2d_chain with chain = (in_image, out_image, next_ph, next_pw, next_maxval,
    next_nbits, next_mbits, next_sign_bits, next_bR, next_Mw, next_form).  in_q / out_q: (maxval, n_bits,
    mantissa bits, sign bits); post: (clamp, lo, hi); act: (act, lo, hi)."""
    L = _lib.load()
    x = x.contiguous()
    w = w.contiguous()
    dev = x.device
    geo = _conv_geometry(x, w, stride, padding, dilation)
    Bn, Cin, H, W, Cout = geo[:5]
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=dev)
    # the input / output quantizers' float and int32 biases
    ib, iib, ob, oib = (torch.empty(1, dtype=t, device=dev) for t in (torch.float32, torch.int32) * 2)
    if res is not None:
        res = res.contiguous()
        if res.shape != y.shape or res.dtype != torch.float32 or res.device != dev:
            raise AssertionError(f"approx_conv2d: residual must be float32 {tuple(y.shape)} on {dev}")
    if bn is not None and (bn.shape != (Cout, 2) or bn.dtype != torch.float32 or not bn.is_contiguous()):
        raise AssertionError(f"approx_conv2d: epilogue parameters must be contiguous float32 [{Cout}, 2]")
    extra = ()
    if chain is not None:
        in_image, out_image, next_ph, next_pw, next_maxval, *next_q, next_bR, next_Mw, next_form = chain
        # (a single-output-channel-group consumer reads table-form words: an image without border)
        in_pad = tuple(padding) if groups == 1 else (0, 0)
        # (form 1, the table form, has no border; forms 0 and 2 -- matrix-core and v5 words -- carry the
        # consumer's padding, as fp8a_conv2d_chain sizes them)
        out_pad = (0, 0) if next_form == 1 else (next_ph, next_pw)
        for img, shp in ((in_image, (Bn, Cin, H, W) + in_pad), (out_image, tuple(y.shape) + out_pad)):
            if img is not None and img.numel() < L.fp8a_word_image_bytes(*shp):
                raise AssertionError("approx_conv2d: word image smaller than fp8a_word_image_bytes")
        extra = (_lib.dev_ptr(in_image), _lib.dev_ptr(out_image), int(next_ph), int(next_pw), _lib.dev_ptr(next_maxval),
                 *map(int, next_q), _lib.dev_ptr(next_bR), int(next_Mw), int(next_form))
    ws = _workspace(dev, L.fp8a_conv2d_block_workspace_size(*geo, groups))
    rc = getattr(L, entry)(*_conv_lead_args(x, w, y, geo, groups, E, M, bA, bW, bR, table, flags), _lib.dev_ptr(bn),
                           int(act[0]), float(act[1]), float(act[2]), _lib.dev_ptr(in_q[0]), *map(int, in_q[1:]),
                           _lib.dev_ptr(ib), _lib.dev_ptr(iib), _lib.dev_ptr(res), int(post[0]), float(post[1]),
                           float(post[2]), _lib.dev_ptr(out_q[0]), *map(int, out_q[1:]), _lib.dev_ptr(ob),
                           _lib.dev_ptr(oib), *extra, _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, entry)
    return y, ib, iib, ob, oib


def _block_fake(x, w, *args, **kw):
    one = x.new_empty((1,))
    onei = x.new_empty((1,), dtype=torch.int32)
    return _conv2d_fake(x, w, *args, **kw), one, onei, one.clone(), onei.clone()


@torch.library.custom_op("fp8approx::conv2d_block", mutates_args=())
def _conv2d_block_op(x: torch.Tensor, w: torch.Tensor, bA: Optional[torch.Tensor], bW: torch.Tensor,
                     bR: torch.Tensor, table: torch.Tensor, E: int, M: int, flags: int, stride: list[int],
                     padding: list[int], dilation: list[int], groups: int, in_maxval: Optional[torch.Tensor],
                     in_nbits: int, in_mbits: int, in_sign_bits: int, res: Optional[torch.Tensor], post_act: int,
                     post_lo: float, post_hi: float, out_maxval: Optional[torch.Tensor], out_nbits: int,
                     out_mbits: int, out_sign_bits: int, bn: Optional[torch.Tensor] = None, act: int = 0,
                     act_lo: float = 0.0, act_hi: float = 0.0
                     ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8a_conv2d_block: y = fq_out(clamp(bn_act(conv(fq_in(x))) + res)); returns y and the input /
    output quantizers' float and int32 biases (1-element tensors, unset when unused)."""
    return _block_call("fp8a_conv2d_block", x, w, bA, bW, bR, table, E, M, flags, stride, padding, dilation, groups,
                       (in_maxval, in_nbits, in_mbits, in_sign_bits), res, (post_act, post_lo, post_hi),
                       (out_maxval, out_nbits, out_mbits, out_sign_bits), bn, (act, act_lo, act_hi))


_conv2d_block_op.register_fake(_block_fake)


# in_image is mutated too: an image that arrived invalid is re-decoded in place by the consumer's
# gated pre-pass (xm_decode_a / tbx_decode_a write its words from x)
@torch.library.custom_op("fp8approx::conv2d_chain", mutates_args=("in_image", "out_image"))
def _conv2d_chain_op(x: torch.Tensor, w: torch.Tensor, bA: Optional[torch.Tensor], bW: torch.Tensor,
                     bR: torch.Tensor, table: torch.Tensor, E: int, M: int, flags: int, stride: list[int],
                     padding: list[int], dilation: list[int], groups: int, in_maxval: Optional[torch.Tensor],
                     in_nbits: int, in_mbits: int, in_sign_bits: int, res: Optional[torch.Tensor], post_act: int,
                     post_lo: float, post_hi: float, out_maxval: Optional[torch.Tensor], out_nbits: int,
                     out_mbits: int, out_sign_bits: int, in_image: Optional[torch.Tensor],
                     out_image: Optional[torch.Tensor], next_ph: int, next_pw: int,
                     next_maxval: Optional[torch.Tensor], next_nbits: int, next_mbits: int, next_sign_bits: int,
                     next_bR: Optional[torch.Tensor], next_Mw: int, bn: Optional[torch.Tensor] = None, act: int = 0,
                     act_lo: float = 0.0, act_hi: float = 0.0, next_form: int = 0
                     ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp8a_conv2d_chain: fp8a_conv2d_block that reads its input's word image (in_image) and / or
    emits the next convolution's (out_image); same results and return values as conv2d_block."""
    return _block_call("fp8a_conv2d_chain", x, w, bA, bW, bR, table, E, M, flags, stride, padding, dilation, groups,
                       (in_maxval, in_nbits, in_mbits, in_sign_bits), res, (post_act, post_lo, post_hi),
                       (out_maxval, out_nbits, out_mbits, out_sign_bits), bn, (act, act_lo, act_hi),
                       (in_image, out_image, next_ph, next_pw, next_maxval, next_nbits, next_mbits, next_sign_bits,
                        next_bR, next_Mw, next_form))


_conv2d_chain_op.register_fake(_block_fake)


def word_image_bytes(Bn, C, H, W, ph, pw):
    """fp8a_word_image_bytes: bytes of a convolution input's word image (0: bad arguments)."""
    return int(_lib.load().fp8a_word_image_bytes(int(Bn), int(C), int(H), int(W), int(ph), int(pw)))


def new_word_image(Bn, C, H, W, ph, pw, device):
    """A freshly initialised word image (fp8a_word_image_init) for a convolution input of shape
    [Bn, C, H, W] and padding (ph, pw): a 256-byte aligned uint8 device tensor."""
    n = word_image_bytes(Bn, C, H, W, ph, pw)
    if n == 0:
        raise AssertionError("new_word_image: bad shape")
    buf = torch.empty(n + 256, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % 256
    img = buf[off:off + n]
    rc = _lib.load().fp8a_word_image_init(_lib.dev_ptr(img), int(Bn), int(C), int(H), int(W), int(ph), int(pw),
                                          _lib.stream_ptr(torch.device(device)))
    _lib.check(rc, "fp8a_word_image_init")
    return img


def conv2d_wants_image(Cout, kernel, padding, groups, E, M, table, flags, stride=(1, 1), dilation=(1, 1)):
    """fp8a_conv2d_wants_image: the input word image a convolution would read -- 0 none, 1 the
    matrix-core form (image of its padding), 2 the tensor-bias table form (image without border)."""
    tab = _table_host(table, M, _uses_table(flags))
    return int(_lib.load().fp8a_conv2d_wants_image(int(Cout), int(kernel[0]), int(kernel[1]), int(padding[0]),
                                                   int(padding[1]), int(groups), int(E), int(M),
                                                   _lib.host_ptr(tab), int(flags) & ~_lib.TB, int(stride[0]),
                                                   int(stride[1]), int(dilation[0]), int(dilation[1])))


def _quantizer_args(q):
    """(maxval [1] device tensor, n_bits, mantissa bits, sign bits) of a per-tensor quantizer tuple."""
    mx, nb, mb, sb = q
    mx = _as_f32(mx).reshape(-1).contiguous()
    if mx.numel() != 1:
        raise AssertionError("approx_conv2d: fused quantizers must be per tensor")
    return mx, int(nb), int(mb), int(sb)


def approx_conv2d(x, w, E, M, bA, bW, bR, table=None, flags=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1),
                  groups=1, epilogue=None, qin=None, post=None, chain=None, **flag_kwargs):
    """approx_v9 convolution, NCHW in / NCHW out (pre-BN), K ordered (c, ky, kx) like the
    reference im2col (approx_calculation.py:724-747); single-output-channel groups get the
    tensor-bias semantics (approx_calculation.py:800-809).  bW: per output channel.

    epilogue: optional ``(scale_shift [Cout, 2] float32 device tensor, act, lo, hi)`` fusing
    the layer's eval-mode BatchNorm (y * scale + shift) and a clamp activation into the
    kernel's store (fp8a_conv2d_bn_act, include/fp8approx.h); see ``bn_act_epilogue``.

    qin: optional ``(maxval [1] device tensor, n_bits, mantissa_bits, sign_bits)`` of the layer's
    per-tensor input activation quantizer: x is then UNQUANTIZED, the op applies
    quantize_to_fp8_ste_MM itself (fp8a_conv2d_qin: inside the E4M3 operand pre-decode where that
    path runs); bA is unused.

    post: optional ``(residual tensor or None, clamp (0/1), lo, hi, output quantizer tuple or
    None)``: a residual block's tail in the store, y = fq_out(clamp(y + residual))
    (fp8a_conv2d_block).

    chain: optional ``(in_image or None, out or None)`` -- the word-image hand-off
    (fp8a_conv2d_chain): in_image is x's word image emitted by the previous convolution (needs
    qin); out = ``(image, next padding (ph, pw), next input quantizer tuple, next result bias
    [1] int32 device tensor, next mantissa width)`` emits the next convolution's.  Bit-identical
    results; x / y are still read / written as fp32.

    With qin, post or chain the result is ``(y, input quantizer bias or None, output quantizer bias
    or None)`` -- the float biases the quantizers would have set as their custom_bias."""
    if flags is None:
        flags = make_flags(**flag_kwargs)
    flags &= ~_lib.TB
    dev = x.device
    tab = _table_host(table, M, _uses_table(flags))
    bW_ = _bias_dev(bW, dev)
    if bW_.numel() == 1:
        bW_ = bW_.expand(w.shape[0]).contiguous()
    if bW_.numel() != w.shape[0]:
        raise AssertionError(f"approx_conv2d: {bW_.numel()} weight biases for {w.shape[0]} output channels")
    ev = _prof_start()
    macs = w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3]  # per output pixel
    lead = (_as_f32(x), _as_f32(w), None if qin is not None else _bias_dev(bA, dev), bW_, _bias_dev(bR, dev), tab,
            int(E), int(M), int(flags), [int(s) for s in stride], [int(p) for p in padding],
            [int(d) for d in dilation], int(groups))
    if qin is None and post is None and chain is None:
        y = _conv2d_op(*lead, *(epilogue or ()))
        _prof_end(ev, y.shape[0] * y.shape[2] * y.shape[3] * macs)
        return y

    def quantizer(q):  # (maxval on the device, n_bits, mantissa bits, sign bits), or none
        if q is None:
            return (None, 0, 0, 0)
        mx, *bits = _quantizer_args(q)
        return (mx.to(dev), *bits)

    res, pact, plo, phi, oq = post if post is not None else (None, 0, 0.0, 0.0, None)
    block = (*lead, *quantizer(qin), res, int(pact), float(plo), float(phi), *quantizer(oq))
    if chain is None:
        y, ib, iib, ob, oib = _conv2d_block_op(*block, *(epilogue or ()))
    else:
        in_img, out = chain
        if in_img is not None and qin is None:
            raise AssertionError("approx_conv2d: an input word image needs the fused input quantizer")
        if out is not None:
            oimg, (nph, npw), nq, nbR, nM = out[:5]
            nform = out[5] if len(out) > 5 else 0
            nbR = _bias_dev(nbR, dev)
        else:
            oimg, nph, npw, nq, nbR, nM, nform = None, 0, 0, None, None, 0, 0
        y, ib, iib, ob, oib = _conv2d_chain_op(*block, in_img, oimg, int(nph), int(npw), *quantizer(nq), nbR, int(nM),
                                               *(epilogue or ()), next_form=int(nform))
    ib._fp8a_i32 = iib
    ob._fp8a_i32 = oib
    _prof_end(ev, y.shape[0] * y.shape[2] * y.shape[3] * macs)
    return y, (ib if qin is not None else None), (ob if oq is not None else None)


def bn_act_epilogue(running_mean, running_var, gamma, beta, eps, activation=None):
    """Epilogue parameters for approx_conv2d: eval-mode F.batch_norm as one scale/shift per
    channel (scale = gamma / sqrt(var + eps), shift = beta - mean * scale, the transform ATen's
    eval batch norm applies) and ReLU / ReLU6 / Hardtanh as a clamp.  Returns None when the
    activation is not a clamp (the caller then runs it unfused)."""
    clamp = _clamp_of(activation)
    if clamp is None:
        return None
    act, lo, hi = clamp
    with torch.no_grad():
        invstd = 1.0 / torch.sqrt(running_var.float() + eps)
        scale = invstd * gamma.float() if gamma is not None else invstd
        shift = -running_mean.float() * scale
        if beta is not None:
            shift = shift + beta.float()
        return torch.stack((scale, shift), dim=1).contiguous(), act, lo, hi


def _clamp_of(activation):
    """bn_act_epilogue's activation -> (act, lo, hi) mapping; None when the activation is not a clamp."""
    if activation is None:
        return 0, 0.0, 0.0
    if type(activation) is nn.ReLU:
        return 1, 0.0, float("inf")
    if type(activation) is nn.ReLU6:
        return 1, 0.0, 6.0
    if type(activation) is nn.Hardtanh:
        return 1, float(activation.min_val), float(activation.max_val)
    return None


def bn_train(x, gamma, beta, running_mean, running_var, momentum, eps, activation=None, out_quantizer=None,
             out=None, stats_only=False):
    """Training-mode batch norm over dim 1 of x ([N, C, ...] or [B, F]) on the deterministic kernels of
    csrc/bn_train.h (fp8a_bn_train): batch statistics from shifted double sums in a fixed order, the
    running buffers updated IN PLACE (None: not updated), then y = clamp(x * scale + shift) and the
    optional per-tensor output quantizer ``(maxval, n_bits, mantissa_bits, sign_bits)``, bit for bit
    fp8_fake_quantize on the unquantized result.

    activation: None / ReLU / ReLU6 / Hardtanh as in bn_act_epilogue; any other activation returns
    None (the caller runs batch norm without it and the activation afterwards).  out: the output
    tensor (may be x: in place); stats_only: no output is written and y is None.

    Returns (y, save_mean, save_var [biased], scale_shift [C, 2], q_bias or None)."""
    L = _lib.load()
    clamp = _clamp_of(activation)
    if clamp is None:
        return None
    act, lo, hi = clamp
    if not x.is_cuda:
        raise RuntimeError("fp8approx kernels need HIP device tensors (no CPU fallback)")
    if x.dim() < 2:
        raise ValueError(f"bn_train: expected at least 2 dims, got {x.dim()}")
    if x.dtype != torch.float32 or not x.is_contiguous():
        if out is x:
            raise AssertionError("bn_train: in place needs a contiguous float32 tensor")
        x = _as_f32(x).contiguous()
    dev = x.device
    N, C = x.shape[0], x.shape[1]
    inner = x.numel() // max(N * C, 1)
    if N == 0 or C == 0 or inner == 0:
        raise AssertionError("bn_train: empty input")
    if N * inner == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")

    def par(t, what):
        if t is None:
            return None
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != C or t.device != dev:
            raise AssertionError(f"bn_train: {what} must be a contiguous float32 [{C}] tensor on {dev}")
        return t.detach()
    gamma, beta = par(gamma, "gamma"), par(beta, "beta")
    running_mean, running_var = par(running_mean, "running_mean"), par(running_var, "running_var")
    if stats_only:
        y = None
    elif out is None:
        y = torch.empty_like(x)
    else:
        if out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
            raise AssertionError("bn_train: out must match x (contiguous float32)")
        y = out
    save_mean = torch.empty(C, dtype=torch.float32, device=dev)
    save_var = torch.empty(C, dtype=torch.float32, device=dev)
    ss = torch.empty((C, 2), dtype=torch.float32, device=dev)
    mx, nb, mb, sb = (None, 0, 0, 0)
    qb = qib = None
    if out_quantizer is not None:
        if y is None:
            raise AssertionError("bn_train: an output quantizer needs an output")
        mx, nb, mb, sb = _quantizer_args(out_quantizer)
        if mx.device != dev:
            mx = mx.to(dev)
        qb = torch.empty(1, dtype=torch.float32, device=dev)
        qib = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = int(L.fp8a_bn_train_workspace_size(N, C, inner))
    ws = _workspace(dev, nbytes)
    rc = L.fp8a_bn_train(_lib.dev_ptr(x), _lib.dev_ptr(y), N, C, inner, _lib.dev_ptr(gamma), _lib.dev_ptr(beta),
                         float(eps), float(momentum), _lib.dev_ptr(running_mean), _lib.dev_ptr(running_var),
                         _lib.dev_ptr(save_mean), _lib.dev_ptr(save_var), _lib.dev_ptr(ss), act, lo, hi,
                         _lib.dev_ptr(mx), nb, mb, sb, _lib.dev_ptr(qb), _lib.dev_ptr(qib), _lib.dev_ptr(ws), nbytes,
                         _lib.stream_ptr(dev))
    _lib.check(rc, "fp8a_bn_train")
    if running_mean is not None:  # the kernel wrote them: caches keyed on _version (the eval epilogue) see it
        torch.autograd.graph.increment_version(running_mean)
    if running_var is not None:
        torch.autograd.graph.increment_version(running_var)
    if qb is not None:
        qb._fp8a_i32 = qib
    return y, save_mean, save_var, ss, qb


# ----------------------------------------------------------------------------------- FP8 fake quant
def fp8_fake_quantize(x, maxval, n_bits, mantissa_bits, sign_bits=1, per_row=False):
    """quantize_to_fp8_ste_MM forward (fp8_quantizer.py:97-173): returns (values, float bias).

    The bias has the reference's shape: [1] per tensor, [C, 1, ..., 1] per channel."""
    L = _lib.load()
    x = _as_f32(x).contiguous()
    mx = _as_f32(maxval).reshape(-1).contiguous()
    if mx.device != x.device:
        mx = mx.to(x.device)
    rows = mx.numel() if per_row else 1
    out = torch.empty_like(x)
    bias = torch.empty(rows, dtype=torch.float32, device=x.device)
    ibias = torch.empty(rows, dtype=torch.int32, device=x.device)
    rc = L.fp8a_fp8_quantize(_lib.dev_ptr(x), rows, x.numel() // rows, _lib.dev_ptr(mx), int(per_row), int(n_bits),
                             int(mantissa_bits), int(sign_bits), _lib.dev_ptr(out), _lib.dev_ptr(bias),
                             _lib.dev_ptr(ibias), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_fp8_quantize")
    if per_row and rows > 1:
        bias = bias.view([-1] + [1] * (x.dim() - 1))
    # the same bias as int32, written by the same kernel: the approx ops take it as is (_bias_dev)
    bias._fp8a_i32 = ibias
    return out, bias


def fp8_fake_quantize_train(x, maxval, n_bits, mantissa_bits, sign_bits=1, per_row=False):
    """fp8_fake_quantize for a forward that autograd records (fp8a_fq_train_forward, csrc/fq_train.h): returns
    (values, float bias, code).  Values and bias are fp8_fake_quantize's bit for bit; code is one uint8 per
    element, x's shape, carrying what fp8_fake_quantize_backward needs of x and maxval."""
    L = _lib.load()
    x = _as_f32(x).contiguous()
    with torch.no_grad():  # (maxval may be a Parameter)
        mx = _as_f32(maxval).reshape(-1).contiguous()
        if mx.device != x.device:
            mx = mx.to(x.device)
    rows = mx.numel() if per_row else 1
    out = torch.empty_like(x)
    code = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    bias = torch.empty(rows, dtype=torch.float32, device=x.device)
    ibias = torch.empty(rows, dtype=torch.int32, device=x.device)
    rc = L.fp8a_fq_train_forward(_lib.dev_ptr(x), rows, x.numel() // rows, _lib.dev_ptr(mx), int(n_bits),
                                 int(mantissa_bits), int(sign_bits), _lib.dev_ptr(out), _lib.dev_ptr(code),
                                 _lib.dev_ptr(bias), _lib.dev_ptr(ibias), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_fq_train_forward")
    if per_row and rows > 1:
        bias = bias.view([-1] + [1] * (x.dim() - 1))
    bias._fp8a_i32 = ibias
    return out, bias, code


def fp8_fake_quantize_backward(g, code, rows, sign_bits=1):
    """The quantizer's backward in one pass over g and fp8_fake_quantize_train's code
    (fp8a_fq_train_backward): returns (grad_x, grad_maxval) -- grad_x = g wx in g's shape, grad_maxval float32
    [rows], the row's sum of g wm accumulated in double in a fixed order (two calls: identical bytes)."""
    L = _lib.load()
    g = _as_f32(g).contiguous()
    if tuple(code.shape) != tuple(g.shape) or code.dtype != torch.uint8 or code.device != g.device:
        raise AssertionError(f"fp8_fake_quantize_backward: code must be a uint8 {tuple(g.shape)} tensor on {g.device}")
    code = code.contiguous()
    rows = int(rows)
    inner = g.numel() // max(rows, 1)
    gx = torch.empty_like(g)
    gmax = torch.empty(max(rows, 0), dtype=torch.float32, device=g.device)
    nbytes = int(L.fp8a_fq_train_workspace_size(rows, inner))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=g.device)
    rc = L.fp8a_fq_train_backward(_lib.dev_ptr(g), _lib.dev_ptr(code), rows, inner, int(sign_bits), _lib.dev_ptr(gx),
                                  _lib.dev_ptr(gmax), _lib.dev_ptr(ws), nbytes, _lib.stream_ptr(g.device))
    _lib.check(rc, "fp8a_fq_train_backward")
    return gx, gmax


def fp8_mse_losses(x, grid, mbit_list, n_bits, sign_bits, per_channel):
    """The FP8 MSE range search's losses in one pass over x (fp8a_fp8_mse_search, csrc/fq_mse.h):

        sse[m][i][r] = sum over row r of (x - fp8_fake_quantize(x, grid[i][r], mbit_list[m]))^2

    x viewed as [rows][inner], rows = x.shape[0] if per_channel else 1; grid float32 [n_cand][rows].
    Returns a float64 [n_mbits][n_cand][rows] device tensor (a candidate with maxval 0: NaN)."""
    L = _lib.load()
    if not x.is_cuda:
        raise RuntimeError("fp8approx kernels need HIP device tensors (no CPU fallback)")
    x = _as_f32(x).contiguous()
    rows = x.shape[0] if per_channel else 1
    inner = x.numel() // max(rows, 1)
    grid = _as_f32(grid).to(x.device).reshape(-1, rows).contiguous()
    n_cand = grid.shape[0]
    mb = (ctypes.c_int32 * len(mbit_list))(*[int(m) for m in mbit_list])
    sse = torch.empty((len(mbit_list), n_cand, rows), dtype=torch.float64, device=x.device)
    nbytes = int(L.fp8a_fp8_mse_workspace_size(rows, inner, n_cand, len(mbit_list)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    rc = L.fp8a_fp8_mse_search(_lib.dev_ptr(x), rows, inner, _lib.dev_ptr(grid), n_cand,
                               ctypes.cast(mb, ctypes.c_void_p), len(mbit_list), int(n_bits), int(sign_bits),
                               _lib.dev_ptr(sse), _lib.dev_ptr(ws), nbytes, _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_fp8_mse_search")
    return sse


# ----------------------------------------------------------------------------------- qamaa
def _res_quant_params(res_quantizer):
    """(maxval device tensor, n_bits, mantissa bits, sign bits) of a res QuantizationManager /
    FPQuantizer, as approx_multiply reads them (approx_calculation.py:790-794)."""
    q = getattr(res_quantizer, "quantizer", res_quantizer)
    mb = q.mantissa_bits
    mb = int(torch.clamp(torch.round(torch.as_tensor(mb, dtype=torch.float32)), 1, q.n_bits - q.sign_bits).item()) \
        if isinstance(mb, torch.Tensor) else int(mb)
    return q.maxval.detach(), int(q.n_bits), mb, int(q.sign_bits)  # (a learned maxval: outside autograd)


def qamaa_matmul(A, B, maxval, n_bits, mantissa_bits, sign_bits=1):
    """quantize_after_mult_and_add: fq(sum_k fq(A[m,k] * B[k,n])) on the GPU."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise AssertionError(f"qamaa_matmul: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")
    L = _lib.load()
    A, B = _as_f32(A), _as_f32(B)
    if A.stride(1) != 1:
        A = A.contiguous()
    if B.stride(0) != 1 and B.stride(1) != 1:
        B = B.contiguous()
    mx = _as_f32(maxval).reshape(-1).to(A.device).contiguous()
    C = torch.empty((A.shape[0], B.shape[1]), dtype=torch.float32, device=A.device)
    ev = _prof_start()
    rc = L.fp8a_matmul_qamaa(_lib.dev_ptr(A), A.stride(0), _lib.dev_ptr(B), B.stride(0), B.stride(1),
                             _lib.dev_ptr(C), A.shape[0], B.shape[1], A.shape[1], _lib.dev_ptr(mx), int(n_bits),
                             int(mantissa_bits), int(sign_bits), _lib.stream_ptr(A.device))
    _lib.check(rc, "fp8a_matmul_qamaa")
    _prof_end(ev, A.shape[0] * A.shape[1] * B.shape[1])
    return C


def qamaa_conv2d(x, w, maxval, n_bits, mantissa_bits, sign_bits=1, stride=(1, 1), padding=(0, 0),
                 dilation=(1, 1), groups=1):
    """Convolution form of qamaa (groups with > 1 output channel)."""
    L = _lib.load()
    x = _as_f32(x).contiguous()
    w = _as_f32(w).contiguous()
    mx = _as_f32(maxval).reshape(-1).to(x.device).contiguous()
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=x.device)
    rc = L.fp8a_conv2d_qamaa(_lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y),
                             *_conv_geometry(x, w, stride, padding, dilation), groups, _lib.dev_ptr(mx),
                             int(n_bits), int(mantissa_bits), int(sign_bits), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_conv2d_qamaa")
    return y


# ------------------------------------------------------------------- the exact product (dense)
def dense_format(mant_width):
    """fp8a_dense operand format for values on a grid with ``mant_width`` mantissa bits.  Default
    bf16 (every FP8 / E3M4 / E2M5 grid value is exact in bf16 at any exponent; measured exact
    accumulation); FP8A_DENSE_FMT=fp8 selects the block-scaled OCP fp8 form -- e4m3
    for 3 mantissa bits, e5m2 for fewer, None (the fp32 contraction) for wider mantissas."""
    if os.environ.get("FP8A_DENSE_FMT", "bf16") != "fp8":
        return _lib.DENSE_BF16 if 0 < mant_width <= 7 else None
    if mant_width == 3:
        return _lib.DENSE_E4M3
    if 0 < mant_width <= 2:
        return _lib.DENSE_E5M2
    return None


@torch.library.custom_op("fp8approx::dense_matmul", mutates_args=())
def _dense_matmul_op(A: torch.Tensor, B: torch.Tensor, fmt: int) -> torch.Tensor:
    L = _lib.load()
    dev = A.device
    Mr, K = A.shape
    N = B.shape[1]
    C = torch.empty((Mr, N), dtype=torch.float32, device=dev)
    ws = _workspace(dev, L.fp8a_dense_matmul_workspace_size(Mr, N, K))
    rc = L.fp8a_dense_matmul(_lib.dev_ptr(A), A.stride(0), A.stride(1), _lib.dev_ptr(B), B.stride(0), B.stride(1),
                             _lib.dev_ptr(C), N, Mr, N, K, int(fmt), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "fp8a_dense_matmul")
    return C


@_dense_matmul_op.register_fake
def _(A, B, fmt):
    return A.new_empty((A.shape[0], B.shape[1]), dtype=torch.float32)


def dense_matmul(A, B, fmt):
    """A [M, K] @ B [K, N] (fp32 values on an FP8 grid, any strides) on the matrix core: the
    reference's exact branch ``x @ y`` (approx_calculation.py:797, 811), equal to the fp32 product
    up to summation order (off-grid values: their units in fp32).  fmt: dense_format() -- the bf16
    form (dn_gemm_bf16, v_mfma_f32_16x16x32_bf16) by default, the block-scaled fp8 form
    (v_mfma_scale_f32_16x16x128_f8f6f4) with FP8A_DENSE_FMT=fp8."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0]:
        raise AssertionError(f"dense_matmul: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")
    A, B = _as_f32(A), _as_f32(B)
    ev = _prof_start()
    C = _dense_matmul_op(A, B, int(fmt))
    _prof_end(ev, A.shape[0] * A.shape[1] * B.shape[1], 4 * (A.numel() + B.numel() + C.numel()))
    return C


@torch.library.custom_op("fp8approx::dense_conv2d", mutates_args=())
def _dense_conv2d_op(x: torch.Tensor, w: torch.Tensor, fmt: int, stride: list[int], padding: list[int],
                     dilation: list[int]) -> torch.Tensor:
    L = _lib.load()
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=x.device)
    geo = _conv_geometry(x, w, stride, padding, dilation)
    ws = _workspace(x.device, L.fp8a_dense_conv2d_workspace_size(*geo))
    rc = L.fp8a_dense_conv2d(_lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y), *geo, int(fmt), _lib.dev_ptr(ws),
                             ws.numel(), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_dense_conv2d")
    return y


@_dense_conv2d_op.register_fake
def _(x, w, fmt, stride, padding, dilation):
    return x.new_empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32)


def dense_conv2d(x, w, fmt, stride=(1, 1), padding=(0, 0), dilation=(1, 1)):
    """Exact-product convolution (groups = 1) on the matrix core (the bf16 form by default, the
    block-scaled fp8 form with FP8A_DENSE_FMT=fp8; see dense_matmul): the reference's im2col +
    ``x @ y`` (approx_calculation.py:811) without the im2col image."""
    if x.dim() != 4 or w.dim() != 4 or x.shape[1] != w.shape[1]:
        raise AssertionError(f"dense_conv2d: shape mismatch {tuple(x.shape)} * {tuple(w.shape)}")
    x = _as_f32(x).contiguous()
    w = _as_f32(w).contiguous()
    ev = _prof_start()
    y = _dense_conv2d_op(x, w, int(fmt), [int(v) for v in stride], [int(v) for v in padding],
                         [int(v) for v in dilation])
    _prof_end(ev, y.shape[0] * y.shape[2] * y.shape[3] * w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3],
              4 * (x.numel() + w.numel() + y.numel()))
    return y


@torch.library.custom_op("fp8approx::grouped_conv2d", mutates_args=())
def _grouped_conv2d_op(x: torch.Tensor, w: torch.Tensor, groups: int, stride: list[int], padding: list[int],
                       dilation: list[int]) -> torch.Tensor:
    L = _lib.load()
    geo = _conv_geometry(x, w, stride, padding, dilation)
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=x.device)
    rc = L.fp8a_grouped_conv2d(_lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y), *geo[:5], int(groups), *geo[5:],
                               _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_grouped_conv2d")
    return y


@_grouped_conv2d_op.register_fake
def _(x, w, groups, stride, padding, dilation):
    return x.new_empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32)


def grouped_conv2d(x, w, groups, stride=(1, 1), padding=(0, 0), dilation=(1, 1)):
    """Exact-product grouped / depthwise convolution on the HIP kernel fp8a_grouped_conv2d: the
    reference's per-group im2col + ``x @ w^T`` (QCustomConv2dTorch, approx_calculation.py:686-711;
    the exact branch's ``x @ y[:, i]``, :797) -- fp32 FMAs in im2col k order, any fp32 input."""
    if x.dim() != 4 or w.dim() != 4 or x.shape[1] != w.shape[1] * groups or w.shape[0] % groups:
        raise AssertionError(f"grouped_conv2d: shape mismatch {tuple(x.shape)} * {tuple(w.shape)} / {groups}")
    x = _as_f32(x).contiguous()
    w = _as_f32(w).contiguous()
    ev = _prof_start()
    y = _grouped_conv2d_op(x, w, int(groups), [int(v) for v in stride], [int(v) for v in padding],
                           [int(v) for v in dilation])
    _prof_end(ev, y.numel() * w.shape[1] * w.shape[2] * w.shape[3], 4 * (x.numel() + w.numel() + y.numel()))
    return y


def dense_conv2d_fused(x, w, groups=1, stride=(1, 1), padding=(0, 0), dilation=(1, 1), fmt=None, qin=None, rq=None,
                       bn=None, oq=None, wq=None):
    """A config-1 layer in one launch family (fp8a_dense_conv2d_fused): y = oq(clamp(bn(rq(conv(qin(x), wq(w)))))).
    qin / rq / oq: (maxval, n_bits, mantissa bits, sign bits) of a per-tensor FP8 quantizer or None;
    wq: the same for the weight quantizer, per tensor or per output channel (maxval [Cout]); bn:
    (scale_shift [C][2], act, lo, hi) from bn_act_epilogue or None.  Returns (y, biases): each
    given quantizer's float bias tensor (its custom_bias: [1], or [Cout, 1, 1, 1] for a per-channel
    wq, as fp8_fake_quantize returns it), keyed "qin" / "rq" / "oq" / "wq"."""
    if x.dim() != 4 or w.dim() != 4 or x.shape[1] != w.shape[1] * groups or w.shape[0] % groups:
        raise AssertionError(f"dense_conv2d_fused: shape mismatch {tuple(x.shape)} * {tuple(w.shape)} / {groups}")
    L = _lib.load()
    x = _as_f32(x).contiguous()
    w = _as_f32(w).contiguous()
    geo = _conv_geometry(x, w, stride, padding, dilation)
    Cout, kh, kw = geo[4:7]
    y = torch.empty(_conv_out_shape(x, w, stride, padding, dilation), dtype=torch.float32, device=x.device)
    keep, biases, qargs = [], {}, []
    for name, q in (("wq", wq), ("qin", qin), ("rq", rq), ("oq", oq)):
        if q is None:
            qargs += [None, 0, 0, 0, None, None] if name != "wq" else [None, 0, 0, 0, 0, None, None]
            continue
        mx = _as_f32(q[0]).reshape(-1).to(x.device).contiguous()
        rows = mx.numel()
        if name == "wq" and rows not in (1, Cout):
            raise AssertionError(f"dense_conv2d_fused: weight quantizer with {rows} maxvals for {Cout} channels")
        if name != "wq" and rows != 1:
            raise AssertionError(f"dense_conv2d_fused: {name} must be a per-tensor quantizer")
        b = torch.empty(rows, dtype=torch.float32, device=x.device)
        ib = torch.empty(rows, dtype=torch.int32, device=x.device)
        keep.append(mx)
        head = [_lib.dev_ptr(mx)] + ([int(rows > 1)] if name == "wq" else [])
        qargs += head + [int(q[1]), int(q[2]), int(q[3]), _lib.dev_ptr(b), _lib.dev_ptr(ib)]
        if rows > 1:
            b = b.view(-1, 1, 1, 1)
        b._fp8a_i32 = ib
        biases[name] = b
    ep, act, lo, hi = (None, 0, 0.0, 0.0) if bn is None else bn
    if ep is not None:
        ep = _as_f32(ep).to(x.device).contiguous()
    ws = _workspace(x.device, L.fp8a_dense_conv2d_workspace_size(*geo) if groups == 1 else 16)
    fmt = dense_format(3) if fmt is None else fmt
    ev = _prof_start()
    rc = L.fp8a_dense_conv2d_fused(_lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y), *geo, int(groups), int(fmt),
                                   *qargs[:19], _lib.dev_ptr(ep) if ep is not None else None, int(act), float(lo),
                                   float(hi), *qargs[19:], _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_dense_conv2d_fused")
    _prof_end(ev, y.numel() * w.shape[1] * kh * kw, 4 * (x.numel() + w.numel() + y.numel()))
    return y, biases


# ----------------------------------------------------------------------------------- max pool
@torch.library.custom_op("fp8approx::max_pool2d", mutates_args=())
def _max_pool2d_op(x: torch.Tensor, kernel: list[int], stride: list[int], padding: list[int]) -> torch.Tensor:
    L = _lib.load()
    x = x.contiguous()
    Bn, C, H, W = x.shape
    Ho = (H + 2 * padding[0] - kernel[0]) // stride[0] + 1
    Wo = (W + 2 * padding[1] - kernel[1]) // stride[1] + 1
    y = torch.empty((Bn, C, Ho, Wo), dtype=x.dtype, device=x.device)
    rc = L.fp8a_max_pool2d(_lib.dev_ptr(x), _lib.dev_ptr(y), Bn, C, H, W, kernel[0], kernel[1], stride[0], stride[1],
                           padding[0], padding[1], _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_max_pool2d")
    return y


@_max_pool2d_op.register_fake
def _(x, kernel, stride, padding):
    Bn, C, H, W = x.shape
    return x.new_empty((Bn, C, (H + 2 * padding[0] - kernel[0]) // stride[0] + 1,
                        (W + 2 * padding[1] - kernel[1]) // stride[1] + 1))


class MaxPool2d(nn.Module):
    """nn.MaxPool2d (dilation 1, floor mode) on the HIP kernel fp8a_max_pool2d; same values
    (max is exact, NaN propagates).  ``from_module`` keeps other configurations on torch."""

    def __init__(self, kernel_size, stride, padding):
        super().__init__()
        pair = lambda v: [int(v), int(v)] if isinstance(v, int) else [int(t) for t in v]  # noqa: E731
        self.kernel_size, self.stride, self.padding = pair(kernel_size), pair(stride), pair(padding)

    @staticmethod
    def from_module(m):
        if (type(m) is nn.MaxPool2d and m.dilation in (1, (1, 1)) and not m.ceil_mode and not m.return_indices
                and m.stride is not None):
            mp = MaxPool2d(m.kernel_size, m.stride, m.padding)
            if all(2 * p <= k for p, k in zip(mp.padding, mp.kernel_size)):
                return mp
        return m

    def forward(self, x):
        # (an input that autograd records -- a layer under ste_backward -- pools on torch: the kernel has no backward)
        if x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda or (x.requires_grad and torch.is_grad_enabled()):
            return nn.functional.max_pool2d(x, self.kernel_size, self.stride, self.padding)
        return _max_pool2d_op(x, self.kernel_size, self.stride, self.padding)

    def extra_repr(self):
        return f"kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding} (HIP)"


# ----------------------------------------------------------------------------------- avg pool
@torch.library.custom_op("fp8approx::avg_pool2d_plane", mutates_args=())
def _avg_pool2d_plane_op(x: torch.Tensor, kernel: list[int], stride: list[int]) -> torch.Tensor:
    L = _lib.load()
    x = x.contiguous()
    Bn, C, H, W = x.shape
    y = torch.empty((Bn, C, 1, 1), dtype=x.dtype, device=x.device)
    rc = L.fp8a_avg_pool2d_plane(_lib.dev_ptr(x), _lib.dev_ptr(y), Bn, C, H, W, kernel[0], kernel[1], stride[0],
                                 stride[1], _lib.stream_ptr(x.device))
    _lib.check(rc, "fp8a_avg_pool2d_plane")
    return y


@_avg_pool2d_plane_op.register_fake
def _(x, kernel, stride):
    return x.new_empty((x.shape[0], x.shape[1], 1, 1))


class AvgPool2d(nn.AvgPool2d):
    """nn.AvgPool2d (padding 0, floor mode, no divisor override) whose output is one value per
    plane -- the MobileNetV2 head's AvgPool2d(input_size // 32) -- on the HIP kernel
    fp8a_avg_pool2d_plane: the window summed in row-major order in fp32 and divided by kh kw, as
    ATen's avg_pool2d does (the same bits).  Other inputs / geometries run torch's pooling; still an
    nn.AvgPool2d, so quantize_sequential wraps it like the original (model_wrap.py)."""

    def __init__(self, kernel_size, stride=None):
        super().__init__(kernel_size, stride)

    def forward(self, x):
        pair = lambda v: [int(v), int(v)] if isinstance(v, int) else [int(t) for t in v]  # noqa: E731
        k, s = pair(self.kernel_size), pair(self.stride)
        if (x.dtype == torch.float32 and x.dim() == 4 and x.is_cuda and k[0] <= x.shape[2] < k[0] + s[0]
                and not (x.requires_grad and torch.is_grad_enabled())  # (recorded by autograd: torch's pooling)
                and k[1] <= x.shape[3] < k[1] + s[1] and x.shape[2] * x.shape[3] <= 4096):
            return _avg_pool2d_plane_op(x, k, s)
        return super().forward(x)


# ----------------------------------------------------------------------------------- STE backward
# finetune.py sets this to a dict to time the backward's parts with HIP events on the current stream:
# name ("grad_gemm", "im2col", "fold") -> [(start_event, end_event), ...].  None = no instrumentation.
_STE_PROFILE = None


class _ste_timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.start = None
        if _STE_PROFILE is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record()

    def __exit__(self, *exc):
        if self.start is not None and _STE_PROFILE is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            _STE_PROFILE.setdefault(self.name, []).append((self.start, end))
        return False


def _grad_batch(t, nd, what):
    """(n0, n1, s0, s1) of the leading batch dims of a view with nd trailing matrix dims."""
    b = t.dim() - nd
    if b == 0:
        return 1, 1, 0, 0
    if b == 1:
        return 1, t.shape[0], 0, t.stride(0)
    if b == 2:
        return t.shape[0], t.shape[1], t.stride(0), t.stride(1)
    raise AssertionError(f"grad_bmm: {what} has more than two leading batch dims: {tuple(t.shape)}")


# grad_split_auto's rule: split until the product pass has GRAD_SPLIT_BLOCKS_PER_CU workgroups
# per compute unit, never below GRAD_SPLIT_MIN_STAGES 32-k stages per part, never above GRAD_SPLIT_MAX_BYTES of
# workspace.  From profiles/grad_split/sweep.jsonl and sweep_fine.jsonl (tools/grad_bench.py --split-k
# 1,2,4,...,64,auto and 1,48,56,64,128,256,512,auto on one MI355X, 256 CUs; ms at split 1 -> the best fixed split):
#   ResNet-18 layer2.conv2 dW    36 tiles, 1568 stages   3.485 -> 0.361 at 64 (48 .. 64 level; 16: 0.393, 128: 0.384)
#   ResNet-18 conv1 dW            3 tiles, 25088 stages  60.97 -> 0.397 at 256 (64: 0.976, 128: 0.519, 512: 0.478)
#   ResNet-18 layer4.1.conv2 dW 576 tiles, 98 stages     0.367 -> 0.303 at 4 (8, 16 within 2 %; 32: 0.344)
#   ViT fc1 dW                  576 tiles, 394 stages    1.034 -> 0.586 at 16 (8: 0.587, 4: 0.618, 32: 0.619)
#   the six data-gradient and attention products (2364 .. 14976 workgroups unsplit): no split gains more than 3 %
#   (fc1 dX at 2), attention loses 1.5x .. 2.9x.
# The guide's 1/2 - 1 workgroups per CU is too low for this kernel (several of its workgroups fit a CU): the dW
# shapes keep gaining up to 7 - 18 per CU.  8 per CU (2048) is the largest power of two below the smallest product
# that must stay unsplit (fc1 dX, 2364); the minimum of 8 stages keeps a part's walk longer than its prologue and, by
# itself, leaves attention's K = 197 and 64 alone; the rule's workspace is its target times 16 KB, 32 MiB, so the
# byte cap binds only where a caller's own split_k meets it.  What auto then does (spread.jsonl; run-to-run spread
# 0.2 - 0.7 %): layer2.conv2 57 parts, 0.367 (1.5 % above the best fixed); layer4.1.conv2 4, 0.306 (the best); fc1 dW
# 4, 0.623 (6 % above: 8 would need a target above fc1 dX's blocks); conv1 683, 0.499 (26 % above 256 parts: with 3
# tiles the reduce pass is 48 workgroups walking 683 partials each -- a cap on the parts, or a wider reduce, is what
# that shape still needs); 1 on the other six.
GRAD_SPLIT_BLOCKS_PER_CU = 8
GRAD_SPLIT_MIN_STAGES = 8
GRAD_SPLIT_MAX_BYTES = 64 << 20


def check_split_k(split_k, what="split_k"):
    """split_k as grad_bmm takes it: an int >= 1 or "auto"; anything else is a ValueError naming `what`."""
    if split_k == "auto" or (isinstance(split_k, int) and not isinstance(split_k, bool) and split_k >= 1):
        return split_k
    raise ValueError(f"{what} must be an int >= 1 or \"auto\", got {split_k!r}")


def _split_kw(split_k):
    """grad_bmm's keywords for a backward's split_k: none at 1.  Not the same as passing split_k=1: the default
    backward then calls grad_bmm(A, B, out=, k2=) as it always has, so a stand-in for grad_bmm with those two
    keywords (tests/test_gpu_ste.py replaces it with a float64 twin) keeps working."""
    return {} if split_k == 1 else {"split_k": split_k}


def grad_split_auto(nb, M, N, K, device):
    """The number of splits along K that grad_bmm(..., split_k="auto") asks for on a product of nb items of
    [M x K] @ [K x N]: 1 when its nb * tiles workgroups already reach GRAD_SPLIT_BLOCKS_PER_CU per compute unit of
    `device`; else as many as reach it, with at least GRAD_SPLIT_MIN_STAGES stages per part and at most
    GRAD_SPLIT_MAX_BYTES of workspace."""
    blocks = nb * (-(-M // 64)) * (-(-N // 64))
    target = GRAD_SPLIT_BLOCKS_PER_CU * torch.cuda.get_device_properties(device).multi_processor_count
    if blocks <= 0 or blocks >= target:
        return 1
    nst = -(-K // 32)
    s = min(-(-target // blocks), nst // GRAD_SPLIT_MIN_STAGES, GRAD_SPLIT_MAX_BYTES // (blocks * 64 * 64 * 4))
    return max(1, s)


def _grad_launch(A, B, C, nb, M, N, K0, K1, oa, ob, oc, sa, sb, sc, split_k=1):
    """One fp8a_grad_bmm launch (split_k != 1: one fp8a_grad_bmm_split, with its workspace from the caching
    allocator on the current stream); oa / ob / oc: element offsets of the first batch item, sa / sb / sc the
    operands' (batch, ...) element strides."""
    L = _lib.load()
    ptr = lambda t, o: ctypes.c_void_p(t.data_ptr() + 4 * o)  # noqa: E731
    if split_k == "auto":
        split_k = grad_split_auto(nb, M, N, K0 * K1, A.device)
    if split_k == 1:
        with _ste_timed("grad_gemm"):
            rc = L.fp8a_grad_bmm(ptr(A, oa), ptr(B, ob), ptr(C, oc), nb, M, N, K0, K1, *sa, *sb, *sc,
                                 _lib.stream_ptr(A.device))
        _lib.check(rc, "fp8a_grad_bmm")
        return
    _, nbytes = _lib.grad_split_plan(nb, M, N, K0, K1, split_k)
    # (a K too short to split plans one part and no workspace: the entry then takes none and launches unsplit)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=A.device) if nbytes else None
    with _ste_timed("grad_gemm"):
        rc = L.fp8a_grad_bmm_split(ptr(A, oa), ptr(B, ob), ptr(C, oc), nb, M, N, K0, K1, *sa, *sb, *sc, split_k,
                                   _lib.dev_ptr(ws) if nbytes else None, nbytes, _lib.stream_ptr(A.device))
    _lib.check(rc, "fp8a_grad_bmm_split")


def grad_bmm(A, B, out=None, k2=False, split_k=1):
    """The gradient GEMM (fp8a_grad_bmm, csrc/gemm_grad.h): C[..., m, n] = sum_k A[..., m, k] B[..., k, n] as an
    exact fp32 product on the bf16 matrix core -- A any float32 (a gradient), B a bf16-exact operand (a saved
    FP8-quantized forward operand; anything else is still summed correctly, on the kernel's fp32 path).

    A [..., M, K] and B [..., K, N] float32 device views with the same zero, one or two leading batch dims, or
    with k2 the two-level reduction A [..., M, K0, K1], B [..., K0, K1, N] (a convolution's weight gradient
    reduces over (image, pixel) this way).  Views are read in place whatever their strides (expand() gives a
    broadcast operand its zero stride); out: None, or the float32 view of [..., M, N] that receives C (any
    positive strides: a transposed view is written through its strides), not overlapping A or B.  Two batch
    dims that do not collapse into one stride in every operand run one launch per index of the shorter one.

    split_k: 1 (one launch, no split), an int >= 2 or "auto" (grad_split_auto): the reduction split into that many
    parts along K (fewer when K has fewer 32-k stages), each summed by its own workgroups into a workspace and
    the parts added in index order by a second launch (fp8a_grad_bmm_split) -- deterministic, and exact wherever
    the unsplit product is; every launch of the call gets the same split_k."""
    check_split_k(split_k)
    nk = 2 if k2 else 1
    if A.dim() < 1 + nk or B.dim() != A.dim() or A.shape[:-1 - nk] != B.shape[:-1 - nk] or \
            A.shape[-nk:] != B.shape[-1 - nk:-1]:
        raise AssertionError(f"grad_bmm: shape mismatch {tuple(A.shape)} @ {tuple(B.shape)}")
    A, B = _as_f32(A), _as_f32(B)
    if not A.is_cuda or B.device != A.device:
        raise RuntimeError("fp8approx kernels need HIP device tensors (no CPU fallback)")
    batch = tuple(A.shape[:-1 - nk])
    M, N = A.shape[-1 - nk], B.shape[-1]
    K0, K1 = (A.shape[-2], A.shape[-1]) if k2 else (1, A.shape[-1])
    shape = batch + (M, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=A.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != A.device:
        raise AssertionError(f"grad_bmm: out must be a float32 {shape} view on {A.device}")
    n0, n1, a0, a1 = _grad_batch(A, 1 + nk, "A")
    _, _, b0, b1 = _grad_batch(B, 1 + nk, "B")
    _, _, c0, c1 = _grad_batch(out, 2, "out")
    sa = (A.stride(-1 - nk), A.stride(-2) if k2 else 0, A.stride(-1))
    sb = (B.stride(-3) if k2 else 0, B.stride(-2), B.stride(-1))
    sc = (out.stride(-2), out.stride(-1))
    if n0 == 1 or n1 == 1 or all(s0 == n1 * s1 for s0, s1 in ((a0, a1), (b0, b1), (c0, c1))):
        # one batch stride per operand
        one = lambda s0, s1: s0 if n1 == 1 else s1  # noqa: E731
        _grad_launch(A, B, out, n0 * n1, M, N, K0, K1, 0, 0, 0, (one(a0, a1), *sa), (one(b0, b1), *sb),
                     (one(c0, c1), *sc), split_k)
    elif n0 <= n1:
        for i in range(n0):
            _grad_launch(A, B, out, n1, M, N, K0, K1, i * a0, i * b0, i * c0, (a1, *sa), (b1, *sb), (c1, *sc),
                         split_k)
    else:
        for i in range(n1):
            _grad_launch(A, B, out, n0, M, N, K0, K1, i * a1, i * b1, i * c1, (a0, *sa), (b0, *sb), (c0, *sc),
                         split_k)
    return out


class _LinearSTE(torch.autograd.Function):
    """y = launch(xq, wq) (the approx product of xq [R, K] and wq [N, K], unchanged); backward the
    straight-through estimator: the exact product's gradients dX = dY Wq, dW = dY^T Xq."""

    @staticmethod
    def forward(ctx, xq, wq, launch, split_k):
        ctx.save_for_backward(xq, wq)
        ctx.split_k = split_k
        return launch(xq, wq)

    @staticmethod
    def backward(ctx, dy):
        xq, wq = ctx.saved_tensors
        dx = grad_bmm(dy, wq, **_split_kw(ctx.split_k)) if ctx.needs_input_grad[0] else None
        dw = grad_bmm(dy.t(), xq, **_split_kw(ctx.split_k)) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None


class _BmmSTE(torch.autograd.Function):
    """c = launch(aq, bq) (the batched approx product, unchanged); backward dA = dC Bq^T and dB = Aq^T dC, the
    latter as dB^T = dC^T Aq written through dB's transposed strides, so the gradient is the A operand of
    both products."""

    @staticmethod
    def forward(ctx, aq, bq, launch, split_k):
        ctx.save_for_backward(aq, bq)
        ctx.split_k = split_k
        return launch(aq, bq)

    @staticmethod
    def backward(ctx, dc):
        aq, bq = ctx.saved_tensors
        da = db = None
        if ctx.needs_input_grad[0]:
            da = grad_bmm(dc, bq.transpose(-1, -2), **_split_kw(ctx.split_k))
        if ctx.needs_input_grad[1]:
            db = torch.empty(bq.shape, dtype=torch.float32, device=bq.device)
            grad_bmm(dc.transpose(-1, -2), aq, out=db.transpose(-1, -2), **_split_kw(ctx.split_k))
        return da, db, None, None


class _Conv2dSTE(torch.autograd.Function):
    """y = launch(xq, wq) (the approx convolution, unchanged); backward the exact convolution's gradients on
    the gradient GEMM.  The saved input goes through fp8a_im2col once ([Bn L, Cin kh kw], L = Ho Wo);
    dW[g] = sum over (image, pixel) of dY[:, g] cols[:, g] is one launch with the groups as the batch index and
    the two-level K = (image, pixel); dXcol[b, g] = Wq[g]^T dY[b, g] is written straight into F.fold's
    [Bn, Cin kh kw, L] layout (one launch for groups = 1; grouped: one per image or per group, whichever is
    fewer) and F.fold scatters it back.  Transient memory: the im2col image and dXcol, each kh kw times the
    input (9x for a 3 x 3 convolution).  Single-output-channel groups get the same exact gradient: the
    tensor-bias semantics (F5) are a quirk of the forward product only."""

    @staticmethod
    def forward(ctx, xq, wq, launch, stride, padding, dilation, groups, split_k):
        ctx.save_for_backward(xq, wq)
        ctx.split_k = split_k
        ctx.geo = (tuple(stride), tuple(padding), tuple(dilation), int(groups))
        return launch(xq, wq)

    @staticmethod
    def backward(ctx, dy):
        xq, wq = ctx.saved_tensors
        stride, padding, dilation, G = ctx.geo
        Bn, Cin, H, W = xq.shape
        Cout, Cg, kh, kw = wq.shape
        dy = _as_f32(dy).contiguous()
        Ln = dy.shape[2] * dy.shape[3]
        Og, Kg = Cout // G, Cg * kh * kw
        dyg = dy.view(Bn, G, Og, Ln)
        dx = dw = None
        if ctx.needs_input_grad[1]:
            L = _lib.load()
            x = xq.contiguous()
            cols = torch.empty((Bn, Ln, G, Kg), dtype=torch.float32, device=x.device)
            with _ste_timed("im2col"):
                rc = L.fp8a_im2col(_lib.dev_ptr(x), _lib.dev_ptr(cols), Bn, Cin, H, W, kh, kw, stride[0], stride[1],
                                   padding[0], padding[1], dilation[0], dilation[1], _lib.stream_ptr(x.device))
            _lib.check(rc, "fp8a_im2col")
            dw = torch.empty((G, Og, Kg), dtype=torch.float32, device=x.device)
            # A [G, Og, Bn, L] (the gradient), B [G, Bn, L, Kg] (the im2col image)
            grad_bmm(dyg.permute(1, 2, 0, 3), cols.permute(2, 0, 1, 3), out=dw, k2=True, **_split_kw(ctx.split_k))
            del cols
            dw = dw.view(wq.shape)
        if ctx.needs_input_grad[0]:
            w = wq.contiguous().view(G, Og, Kg)
            dxcol = torch.empty((Bn, G, Kg, Ln), dtype=torch.float32, device=dy.device)
            # C^T [Bn, G, L, Kg] = A [Bn, G, L, Og] (the gradient, pixels as rows) @ B [G, Og, Kg]
            grad_bmm(dyg.transpose(-1, -2), w.unsqueeze(0).expand(Bn, G, Og, Kg), out=dxcol.transpose(-1, -2),
                     **_split_kw(ctx.split_k))
            with _ste_timed("fold"):
                dx = torch.nn.functional.fold(dxcol.view(Bn, G * Kg, Ln), (H, W), (kh, kw), dilation, padding, stride)
        return dx, dw, None, None, None, None, None, None


def ste_linear(xq, wq, launch, split_k=1):
    """launch(xq, wq) -> [R, N] with the straight-through backward (xq [R, K], wq [N, K] quantized operands);
    split_k: grad_bmm's, for every product of the backward (ste_bmm and ste_conv2d alike)."""
    return _LinearSTE.apply(xq, wq, launch, check_split_k(split_k))


def ste_bmm(aq, bq, launch, split_k=1):
    """launch(aq, bq) -> [..., M, N] with the straight-through backward (quantized batched operands)."""
    return _BmmSTE.apply(aq, bq, launch, check_split_k(split_k))


def ste_conv2d(xq, wq, launch, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1, split_k=1):
    """launch(xq, wq) -> NCHW y with the straight-through backward (quantized NCHW input and weights)."""
    return _Conv2dSTE.apply(xq, wq, launch, stride, padding, dilation, groups, check_split_k(split_k))
