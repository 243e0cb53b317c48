"""The gradient GEMM (fp8a_grad_bmm, csrc/gemm_grad.h) without a GPU: the exports, the argument checks -- every
one answered before the library touches a device -- and the three-piece bf16 split restated in numpy.

The split: p0 = trunc16(x), p1 = trunc16(x - p0), p2 = trunc16(x - p0 - p1), trunc16 keeping the top 16 bits
of the fp32 pattern, and -- as the kernel does not rely on bf16 subnormals -- a piece whose exponent field is
zero counted as lost (flushed to zero).  It is exact (p0 + p1 + p2 == x, summed in float64) for every finite
fp32 value of exponent field >= 24 (its last bit is then worth 2^-126 or more), which is the kernel's own test
(gr_split); below that a piece can be subnormal, so the value is flagged and its tile recomputed in fp32."""
import ctypes

import numpy as np

from fp8_quantization_amd import _lib

PTR = ctypes.c_void_p(4096)  # a non-null pointer value the host side never dereferences
# nb, M, N, K0, K1, then A's, B's and C's strides (dense [nb, M, K0, K1] @ [nb, K0, K1, N])
GOOD = dict(nb=2, M=3, N=5, K0=2, K1=7, sa_i=42, sa_m=14, sa_k0=7, sa_k1=1, sb_i=70, sb_k0=35, sb_k1=5, sb_n=1,
            sc_i=15, sc_m=5, sc_n=1)
ORDER = tuple(GOOD)


def call(A=PTR, B=ctypes.c_void_p(8192), C=ctypes.c_void_p(16384), **kw):
    d = dict(GOOD, **kw)
    L = _lib.load()
    rc = L.fp8a_grad_bmm(A, B, C, *[d[k] for k in ORDER], None)
    return rc, L.fp8a_last_error().decode()


def test_exports():
    L = _lib.load()
    assert "fp8a_grad_bmm" in _lib.SYMBOLS and "fp8a_grad_stats" in _lib.SYMBOLS
    assert callable(L.fp8a_grad_bmm) and callable(L.fp8a_grad_stats)
    from fp8_quantization_amd import approx_ops
    for name in ("grad_bmm", "ste_linear", "ste_conv2d", "ste_bmm"):
        assert name in approx_ops.__all__ and callable(getattr(approx_ops, name))
    import fp8_quantization_amd as fa
    assert fa.grad_bmm is approx_ops.grad_bmm
    assert callable(_lib.grad_stats)


def test_every_einval_returns_before_a_hip_call():
    """(Where there is no HIP device, a call that got as far as HIP would not return FP8A_EINVAL.)"""
    for ext in ("nb", "M", "N", "K0", "K1"):
        assert call(**{ext: -1}) == (_lib.EINVAL, "fp8a_grad_bmm: negative extent")
    for st in ORDER[5:]:
        assert call(**{st: -1}) == (_lib.EINVAL, "fp8a_grad_bmm: negative stride")
    assert call(K0=1 << 20, K1=1 << 11) == (_lib.EINVAL, "fp8a_grad_bmm: K0 * K1 exceeds 2^31 - 1")
    assert call(C=None) == (_lib.EINVAL, "fp8a_grad_bmm: null pointer")
    assert call(A=None) == (_lib.EINVAL, "fp8a_grad_bmm: null pointer")
    assert call(B=None) == (_lib.EINVAL, "fp8a_grad_bmm: null pointer")
    for st in ("sc_i", "sc_m", "sc_n"):
        assert call(**{st: 0}) == (_lib.EINVAL, "fp8a_grad_bmm: a zero stride of C over an extent above 1")
    assert call(C=PTR) == (_lib.EINVAL, "fp8a_grad_bmm: C overlaps an operand")  # the same base as A
    assert call(C=ctypes.c_void_p(8192)) == (_lib.EINVAL, "fp8a_grad_bmm: C overlaps an operand")  # as B
    # two dense spans that meet: C starts inside A's 84 floats
    assert call(C=ctypes.c_void_p(4096 + 4 * 80)) == (_lib.EINVAL, "fp8a_grad_bmm: C overlaps an operand")
    assert call(M=1 << 38, N=64, sc_m=64) == (_lib.EINVAL, "fp8a_grad_bmm: more than 2^31 - 1 tiles")
    rc = _lib.load().fp8a_grad_stats(None, 0)
    assert (rc, _lib.load().fp8a_last_error().decode()) == (_lib.EINVAL, "null pointer")


def test_empty_extents_return_ok_without_a_device():
    for ext in ("nb", "M", "N"):
        assert call(A=None, B=None, C=None, **{ext: 0})[0] == _lib.OK


# ---------------------------------------------------------------------------------- the split in numpy
def trunc16(x):
    """The bf16 truncation of fp32 values, a piece with a zero exponent field flushed to zero."""
    u = np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    u = np.where((u & np.uint32(0x7F800000)) == 0, np.uint32(0), u)
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    p0 = trunc16(x)
    r1 = x - p0          # exact in fp32
    p1 = trunc16(r1)
    r2 = r1 - p1         # exact in fp32
    return p0, p1, trunc16(r2)


def kernel_accepts(x):
    """gr_split's test: zero, or finite with exponent field >= 24."""
    u = np.asarray(x, np.float32).view(np.uint32)
    e = (u >> np.uint32(23)) & np.uint32(0xFF)
    return ((u & np.uint32(0x7FFFFFFF)) == 0) | ((e >= 24) & (e != 0xFF))


def test_split_is_exact_on_random_bit_patterns():
    rng = np.random.default_rng(20261020)
    n = 100_000
    expo = rng.integers(-100, 101, n).astype(np.uint32) + np.uint32(127)
    u = (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)) | (expo << np.uint32(23)) | \
        rng.integers(0, 1 << 23, n).astype(np.uint32)
    x = u.view(np.float32)
    p = split3(x)
    for q in p:  # every piece is a bf16: the low 16 bits of its pattern are zero
        assert not (q.view(np.uint32) & np.uint32(0xFFFF)).any()
    assert np.array_equal(sum(q.astype(np.float64) for q in p), x.astype(np.float64))
    assert kernel_accepts(x).all()
    # each piece times a bf16-exact operand is exact in fp32: at most 16 significant bits
    b = trunc16(rng.standard_normal(n).astype(np.float32))
    for q in p:
        prod = q.astype(np.float64) * b.astype(np.float64)
        assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)


def test_split_is_inexact_hence_flagged_below_the_window():
    x = np.array([2.0 ** -130], np.float32)
    assert x[0] != 0.0
    assert sum(q.astype(np.float64) for q in split3(x))[0] != float(x[0])
    assert not kernel_accepts(x)[0]
    # the kernel's window is the restated split's: every accepted value of the low binades splits exactly, the
    # first rejected binade (field 23) holds values that do not
    lo = (np.uint32(24) << np.uint32(23)) | np.arange(0, 1 << 23, 4099, dtype=np.uint32)
    v = lo.view(np.float32)
    assert kernel_accepts(v).all()
    assert np.array_equal(sum(q.astype(np.float64) for q in split3(v)), v.astype(np.float64))
    w = ((np.uint32(23) << np.uint32(23)) | np.uint32(1)).view(np.float32).reshape(1)  # 2^-104 (1 + 2^-23)
    assert not kernel_accepts(w)[0]
    assert sum(q.astype(np.float64) for q in split3(w))[0] != float(w[0])
    for bad in (np.inf, -np.inf, np.nan):
        assert not kernel_accepts(np.array([bad], np.float32))[0]
    assert kernel_accepts(np.array([0.0, -0.0], np.float32)).all()


# ---------------------------------------------------------------------------------- the switch, host side
def test_switch_is_opt_in_and_rejects_v5_and_qamaa():
    import pytest
    import torch
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch, QCustomMatMul
    from fp8_quantization_amd.resnet_workload import approx_qparams
    assert "ste_backward" not in approx_qparams()["custom_approx_params"]
    assert approx_qparams(ste_backward=True)["custom_approx_params"]["ste_backward"] is True
    qamaa = dict(approx_flag=True, quantize_after_mult_and_add=True, res_quantizer_flag=True,
                 original_quantize_res=False)
    x = torch.zeros(2, 4)
    for kw in (dict(approx_version=5, expo_width=5, mant_width=2), dict(run_method=qamaa)):
        m = QCustomLinearTorch(in_features=4, out_features=3, **approx_qparams(ste_backward=True, **kw))
        with pytest.raises(NotImplementedError, match="ste_backward"):
            m(x)  # (raised before any quantizer or product runs)
        with torch.no_grad(), pytest.raises(NotImplementedError, match="ste_backward"):
            m(x)
    # the layer hands its switch to the quantizers it owns, and takes it back when the key goes
    m = QCustomMatMul(**approx_qparams(ste_backward=True))
    assert m.a_quantizer.quantizer.ste_backward is False
    assert m._ste_on() is True
    assert all(q.quantizer.ste_backward for q in (m.a_quantizer, m.b_quantizer, m.res_quantizer))
    with torch.no_grad():
        assert m._ste_on() is False and m.a_quantizer.quantizer.ste_backward is True
    del m.custom_approx_params["ste_backward"]
    assert m._ste_on() is False and m.a_quantizer.quantizer.ste_backward is False
    with pytest.raises(NotImplementedError):
        m.a_quantizer.quantizer.make_range_trainable()
