"""The implicit-GEMM convolution backward without a GPU: the three exports, every argument check
-- answered on fake pointers before the library touches a device --, the workspace plan against §3ah's restated
here, and the conv_backward key through approx_qparams and the operator classes."""
import ctypes

import pytest

from fp8_quantization_amd import _lib

DY, OP, OUT = (ctypes.c_void_p(a << 32) for a in (1, 2, 3))   # far apart, never dereferenced
WS = ctypes.c_void_p(1 << 40)
BASE = dict(Bn=3, Cin=8, H=13, W=11, Cout=12, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, groups=1)
WIDE = dict(BASE, Bn=2, Cin=72, H=5, W=4, Cout=70)
EINVAL = _lib.EINVAL


def dgrad(dy=DY, w=OP, dx=OUT, **kw):
    L = _lib.load()
    return L.fp8a_grad_conv2d_dgrad(dy, w, dx, *dict(BASE, **kw).values(), None), L.fp8a_last_error().decode()


def wgrad(dy=DY, x=OP, dwgt=OUT, splits=3, ws=WS, ws_bytes=1 << 30, **kw):
    L = _lib.load()
    return (L.fp8a_grad_conv2d_wgrad(dy, x, dwgt, *dict(BASE, **kw).values(), splits, ws, ws_bytes, None),
            L.fp8a_last_error().decode())


def size(geo, splits):
    L = _lib.load()
    S, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.fp8a_grad_conv2d_wgrad_workspace_size(*geo.values(), splits, ctypes.byref(S), ctypes.byref(n))
    return rc, int(S.value), int(n.value)


def test_exports():
    from fp8_quantization_amd import approx_ops
    L = _lib.load()
    for name in ("fp8a_grad_conv2d_dgrad", "fp8a_grad_conv2d_wgrad_workspace_size", "fp8a_grad_conv2d_wgrad"):
        assert name in _lib.SYMBOLS and callable(getattr(L, name))
    for name in ("grad_conv2d_input", "grad_conv2d_weight"):
        assert name in approx_ops.__all__ and callable(getattr(approx_ops, name))


@pytest.mark.parametrize("call, who", [(dgrad, "fp8a_grad_conv2d_dgrad: "), (wgrad, "fp8a_grad_conv2d_wgrad: ")])
def test_geometry_checks_return_before_a_hip_call(call, who):
    """(Where there is no HIP device, a call that got as far as HIP would not return FP8A_EINVAL.)"""
    for null in call.__code__.co_varnames[:3]:
        assert call(**{null: None}) == (EINVAL, who + "null pointer")
    for k in BASE:
        if k not in ("ph", "pw"):
            assert call(**{k: 0}) == (EINVAL, who + "non-positive size"), k
    assert call(ph=-1) == (EINVAL, who + "negative padding")
    for kw in (dict(groups=3), dict(groups=4, Cout=10), dict(groups=8)):
        assert call(**kw) == (EINVAL, who + "groups does not divide both channel counts")
    assert call(kh=16) == (EINVAL, who + "empty output")              # 13 + 2 < 16
    assert call(kw=7, dw=2, pw=0) == (EINVAL, who + "empty output")   # 11 < 13
    wide = who + "index range beyond the 32-bit in-tile arithmetic"
    assert call(Bn=1 << 21) == (EINVAL, wide)                         # 2^21 x 8 x 143 elements of x
    assert call(H=1 << 16, W=1 << 15) == (EINVAL, wide)
    assert call(Cin=1 << 17, Cout=1 << 14, kh=1, kw=1, ph=0, pw=0) == (EINVAL, wide)   # 2^31 weights
    assert call(sh=1 << 16) == (EINVAL, wide)
    overlap = who + ("dx" if call is dgrad else "dw") + " overlaps an operand"
    assert call(**{call.__code__.co_varnames[2]: DY}) == (EINVAL, overlap)
    assert call(**{call.__code__.co_varnames[2]: ctypes.c_void_p((2 << 32) + 64)}) == (EINVAL, overlap)


def test_dgrad_block_count_is_checked():
    # 2^30 residue classes of one row tile each, times 2^12 images
    assert dgrad(Bn=1 << 12, Cin=1, Cout=1, H=1, W=1 << 18, kh=1, kw=1, ph=0, pw=0, sh=1 << 15, sw=1 << 15) == \
        (EINVAL, "fp8a_grad_conv2d_dgrad: more than 2^31 - 1 blocks")


def test_workspace_checks_return_before_a_hip_call():
    who = "fp8a_grad_conv2d_wgrad: "
    for s in (0, -2):
        assert wgrad(splits=s) == (EINVAL, who + "splits below 1")
    need = 3 * 1 * 2 * 4096 * 4    # K = 429: 14 stages in 3 parts; [12 x 72]: two tiles
    assert wgrad(ws=None) == (EINVAL, who + "null workspace")
    assert wgrad(ws_bytes=need - 1) == (EINVAL, who + f"workspace of {need - 1} bytes, {need} needed")
    assert wgrad(ws=ctypes.c_void_p((1 << 40) + 8)) == (EINVAL, who + "workspace not 16-byte aligned")
    for p in (DY, OP, OUT, ctypes.c_void_p((1 << 32) - 16)):
        assert wgrad(ws=p) == (EINVAL, who + "the workspace overlaps dy, x or dw")
    sz = "fp8a_grad_conv2d_wgrad_workspace_size: "
    L = _lib.load()
    assert L.fp8a_grad_conv2d_wgrad_workspace_size(*BASE.values(), 2, None, None) == EINVAL
    assert L.fp8a_last_error().decode() == sz + "null pointer"
    assert size(BASE, 0)[0] == EINVAL and L.fp8a_last_error().decode() == sz + "splits below 1"
    assert size(dict(BASE, groups=3), 2)[0] == EINVAL


def plan(geo, splits):
    """§3ah's plan on K = Bn Ho Wo, and the workspace of S parts of G x tiles dense 64 x 64 fp32 tiles."""
    ho = (geo["H"] + 2 * geo["ph"] - geo["dh"] * (geo["kh"] - 1) - 1) // geo["sh"] + 1
    wo = (geo["W"] + 2 * geo["pw"] - geo["dw"] * (geo["kw"] - 1) - 1) // geo["sw"] + 1
    nst = -(-geo["Bn"] * ho * wo // 32)
    per = -(-nst // splits)
    S = -(-nst // per)
    G = geo["groups"]
    tiles = -(-(geo["Cout"] // G) // 64) * -(-(geo["Cin"] // G * geo["kh"] * geo["kw"]) // 64)
    return S, S * G * tiles * 4096 * 4 if S > 1 else 0


@pytest.mark.parametrize("geo", [BASE, WIDE, dict(BASE, groups=4, sh=2, sw=2), dict(BASE, Bn=1, H=4, W=4, sh=2, sw=2)],
                         ids=["base", "wide", "grouped-s2", "K=4"])
def test_workspace_size_equals_the_plan(geo):
    for splits in (1, 3, 64):
        S, nbytes = plan(geo, splits)
        assert size(geo, splits) == (_lib.OK, S, nbytes), splits
        assert _lib.grad_conv_wgrad_plan(tuple(geo.values()), splits) == (S, nbytes)
    assert plan(BASE, 3) == (3, 98304) and plan(WIDE, 64) == (2, 2 * 2 * 11 * 16384)
    assert plan(dict(BASE, Bn=1, H=4, W=4, sh=2, sw=2), 64) == (1, 0)      # one stage: too short to split


def test_the_conv_backward_key():
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    from fp8_quantization_amd.approx_ops import ste_conv2d
    from fp8_quantization_amd.resnet_workload import approx_qparams
    assert "conv_backward" not in approx_qparams(ste_backward=True)["custom_approx_params"]
    assert "conv_backward" not in approx_qparams(ste_backward=True, conv_backward="im2col")["custom_approx_params"]
    qp = approx_qparams(ste_backward=True, conv_backward="implicit")
    assert qp["custom_approx_params"]["conv_backward"] == "implicit"
    QCustomBNConv2dTorch(in_channels=4, out_channels=8, kernel_size=3, bias=False, **qp)
    for bad in ("direct", "auto", 1, None):
        qp["custom_approx_params"]["conv_backward"] = bad
        with pytest.raises(ValueError, match="conv_backward"):
            QCustomBNConv2dTorch(in_channels=4, out_channels=8, kernel_size=3, bias=False, **qp)
        with pytest.raises(ValueError, match="backward"):
            ste_conv2d(None, None, None, backward=bad)
