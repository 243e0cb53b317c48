"""The depthwise convolution backward without a GPU: exports, argument checks, plan, the key."""
import ctypes

import pytest

from fp8_quantization_amd import _lib

DY, OP, OUT = (ctypes.c_void_p(a << 32) for a in (1, 2, 3))   # far apart, never dereferenced
WS = ctypes.c_void_p(1 << 40)
BASE = dict(Bn=3, C=5, H=13, W=11, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
EINVAL = _lib.EINVAL


def dgrad(dy=DY, w=OP, dx=OUT, **kw):
    L = _lib.load()
    return L.fp8a_grad_dwconv2d_dgrad(dy, w, dx, *dict(BASE, **kw).values(), None), L.fp8a_last_error().decode()


def wgrad(dy=DY, x=OP, dwgt=OUT, splits=3, ws=WS, ws_bytes=1 << 30, **kw):
    L = _lib.load()
    return (L.fp8a_grad_dwconv2d_wgrad(dy, x, dwgt, *dict(BASE, **kw).values(), splits, ws, ws_bytes, None),
            L.fp8a_last_error().decode())


def size(geo, splits):
    L = _lib.load()
    S, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.fp8a_grad_dwconv2d_wgrad_workspace_size(*geo.values(), splits, ctypes.byref(S), ctypes.byref(n))
    return rc, int(S.value), int(n.value)


def test_exports():
    from fp8_quantization_amd import approx_ops
    L = _lib.load()
    for name in ("fp8a_grad_dwconv2d_dgrad", "fp8a_grad_dwconv2d_wgrad_workspace_size", "fp8a_grad_dwconv2d_wgrad"):
        assert name in _lib.SYMBOLS and callable(getattr(L, name))
    for name in ("grad_dwconv2d_input", "grad_dwconv2d_weight"):
        assert name in approx_ops.__all__ and callable(getattr(approx_ops, name))
    assert approx_ops.CONV_BACKWARDS == ("im2col", "implicit", "depthwise")


@pytest.mark.parametrize("call, who", [(dgrad, "fp8a_grad_dwconv2d_dgrad: "), (wgrad, "fp8a_grad_dwconv2d_wgrad: ")])
def test_geometry_checks_return_before_a_hip_call(call, who):
    for null in call.__code__.co_varnames[:3]:
        assert call(**{null: None}) == (EINVAL, who + "null pointer")
    for k in BASE:
        if k not in ("ph", "pw"):
            assert call(**{k: 0}) == (EINVAL, who + "non-positive size"), k
    assert call(ph=-1) == (EINVAL, who + "negative padding")
    assert call(kh=7, ph=0, H=6) == (EINVAL, who + "empty output")
    assert call(kw=3, dw=6, pw=0) == (EINVAL, who + "empty output")    # 11 < 13
    big = who + "a kernel beyond the runtime-geometry instance (kh, kw <= 7, (k - 1) d <= 32)"
    assert call(kh=8, ph=4) == (EINVAL, big)
    assert call(kw=2, dw=33, pw=20) == (EINVAL, big)
    wide = who + "index range beyond the 32-bit in-tile arithmetic"
    assert call(Bn=1 << 22) == (EINVAL, wide)                          # 2^22 x 5 x 143 elements of x
    assert call(H=1 << 16, W=1 << 15) == (EINVAL, wide)
    assert call(sh=1 << 16) == (EINVAL, wide)
    assert call(C=1 << 28, H=1, W=1, kh=1, kw=1, ph=1, pw=1) == (EINVAL, wide)   # dy: 2^28 x 3 x 9
    overlap = who + ("dx" if call is dgrad else "dw") + " overlaps an operand"
    assert call(**{call.__code__.co_varnames[2]: DY}) == (EINVAL, overlap)
    assert call(**{call.__code__.co_varnames[2]: ctypes.c_void_p((2 << 32) + 64)}) == (EINVAL, overlap)


def test_workspace_checks_return_before_a_hip_call():
    who = "fp8a_grad_dwconv2d_wgrad: "
    for s in (0, -2):
        assert wgrad(splits=s) == (EINVAL, who + "splits below 1")
    need = 3 * 5 * 9 * 4    # 39 rows in 3 parts of 13; 5 channels of 9 sums
    assert wgrad(ws=None) == (EINVAL, who + "null workspace")
    assert wgrad(ws_bytes=need - 1) == (EINVAL, who + f"workspace of {need - 1} bytes, {need} needed")
    assert wgrad(ws=ctypes.c_void_p((1 << 40) + 8)) == (EINVAL, who + "workspace not 16-byte aligned")
    for p in (DY, OP, OUT, ctypes.c_void_p((1 << 32) - 16)):
        assert wgrad(ws=p) == (EINVAL, who + "the workspace overlaps dy, x or dw")
    sz = "fp8a_grad_dwconv2d_wgrad_workspace_size: "
    L = _lib.load()
    assert (L.fp8a_grad_dwconv2d_wgrad_workspace_size(*BASE.values(), 2, None, None), L.fp8a_last_error().decode()) == \
        (EINVAL, sz + "null pointer")
    assert size(BASE, 0)[0] == EINVAL and L.fp8a_last_error().decode() == sz + "splits below 1"
    assert size(dict(BASE, kh=8, ph=4), 2)[0] == EINVAL


def plan(geo, splits):
    """The split by output rows: R = Bn Ho, per = ceil(R / splits), S = ceil(R / per); S C kh kw floats when S > 1."""
    ho = (geo["H"] + 2 * geo["ph"] - geo["dh"] * (geo["kh"] - 1) - 1) // geo["sh"] + 1
    R = geo["Bn"] * ho
    per = -(-R // splits)
    S = -(-R // per)
    return S, S * geo["C"] * geo["kh"] * geo["kw"] * 4 if S > 1 else 0


@pytest.mark.parametrize("geo", [BASE, dict(BASE, H=37, W=70, kh=5, kw=5, ph=2, pw=2), dict(BASE, sh=2, sw=2),
                                 dict(BASE, Bn=1, C=9, H=7, W=7)], ids=["base", "5x5", "s2", "R=7"])
def test_workspace_size_equals_the_plan(geo):
    for splits in (1, 3, 64):
        S, nbytes = plan(geo, splits)
        assert size(geo, splits) == (_lib.OK, S, nbytes), splits
        assert _lib.grad_dwconv_wgrad_plan(tuple(geo.values()), splits) == (S, nbytes)
    assert plan(BASE, 3) == (3, 540) and plan(BASE, 64) == (39, 39 * 180)
    assert plan(dict(BASE, H=37, W=70, kh=5, kw=5, ph=2, pw=2), 64) == (56, 56 * 500)   # 111 rows, 2 per part: 56 parts
    assert plan(dict(BASE, Bn=1, C=9, H=7, W=7), 64) == (7, 7 * 324)                    # R = 7 < splits: a row each


def test_the_conv_backward_key_takes_depthwise():
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    from fp8_quantization_amd.resnet_workload import approx_qparams
    qp = approx_qparams(ste_backward=True, conv_backward="depthwise")
    assert qp["custom_approx_params"]["conv_backward"] == "depthwise"
    QCustomBNConv2dTorch(in_channels=8, out_channels=8, kernel_size=3, groups=8, bias=False, **qp)
    QCustomBNConv2dTorch(in_channels=4, out_channels=8, kernel_size=3, bias=False, **qp)


def test_a_weight_that_is_not_depthwise_is_refused():
    from fp8_quantization_amd.approx_ops import _dwconv_geo
    assert _dwconv_geo((3, 5, 13, 11), (5, 1, 3, 3), 2, 1, 1, "t") == ((3, 5, 13, 11, 3, 3, 2, 2, 1, 1, 1, 1), (3, 5, 7, 6))
    for wshape in ((5, 2, 3, 3), (10, 1, 3, 3), (4, 1, 3, 3)):
        with pytest.raises(AssertionError):
            _dwconv_geo((3, 5, 13, 11), wshape, 1, 1, 1, "t")
