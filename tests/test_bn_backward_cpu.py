"""The batch-norm backward's host side (fp8a_bn_train_backward, csrc/bn_bwd.h) without a device: the exported
symbols, the workspace query against bn_parts() restated, every argument refusal on fake pointers (each returns
before any launch, so no device is touched), and the operators' bn_backward key."""
import ctypes

import pytest

from fp8_quantization_amd import _lib

FAKE = ctypes.c_void_p(4096)          # non-null, 16-byte aligned, never dereferenced


def parts(N, C, inner):
    """bn_parts (csrc/bn_train.h), restated."""
    lin = inner < 16
    tile, groups = (256, (C + 63) // 64) if lin else (4096, C)
    return max(1, min((N * inner + tile - 1) // tile, (2048 + groups - 1) // groups))


def test_symbols_are_exported():
    assert {"fp8a_bn_train_backward", "fp8a_bn_train_backward_workspace_size"} <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert L.fp8a_bn_train_backward and L.fp8a_bn_train_backward_workspace_size


@pytest.mark.parametrize("shape", [(3, 5, 49), (64, 16, 64), (1, 2, 4097), (2, 4, 4225), (5, 2, 4096), (33, 70, 1),
                                   (2, 3, 1), (64, 96, 12544), (4096, 4096, 1)])
def test_workspace_size_is_bn_parts_restated(shape):
    N, C, inner = shape
    got = _lib.load().fp8a_bn_train_backward_workspace_size(N, C, inner)
    assert got == C * (parts(N, C, inner) * 16 + 16)     # (G, H) double pairs per part + one coefficient record


def call(N=2, C=3, inner=49, x=FAKE, dy=FAKE, dx=FAKE, mean=FAKE, var=FAKE, ss=FAKE, act=0, ws=FAKE, ws_bytes=1 << 20):
    return _lib.load().fp8a_bn_train_backward(x, dy, dx, N, C, inner, None, mean, var, 1e-5, ss, act, 0.0, 6.0, None, None,
                                              ws, ws_bytes, None)


@pytest.mark.parametrize("kw, code", [
    (dict(N=0), _lib.EINVAL), (dict(C=0), _lib.EINVAL), (dict(inner=0), _lib.EINVAL), (dict(N=-1), _lib.EINVAL),
    (dict(inner=2 ** 31 - 4096), _lib.EINVAL),                       # the inner limit
    (dict(N=1, inner=1), _lib.EFORMAT),                              # n == 1: torch's ValueError
    (dict(act=2), _lib.EINVAL),
    (dict(ws_bytes=3 * (16 + 16) - 1), _lib.EINVAL),                 # one byte short
    (dict(x=None), _lib.EINVAL), (dict(dy=None), _lib.EINVAL), (dict(dx=None), _lib.EINVAL),
    (dict(mean=None), _lib.EINVAL), (dict(var=None), _lib.EINVAL), (dict(ss=None), _lib.EINVAL),
    (dict(ws=None), _lib.EINVAL), (dict(ws=ctypes.c_void_p(4104)), _lib.EINVAL),
    (dict(ss=ctypes.c_void_p(4100)), _lib.EINVAL)], ids=str)
def test_refusals_come_before_any_launch(kw, code):
    assert call(**kw) == code
    assert _lib.load().fp8a_last_error()
    for bad in ((0, 3, 49), (2, 0, 49), (2, 3, 0), (2, 3, 2 ** 31)):
        assert _lib.load().fp8a_bn_train_backward_workspace_size(*bad) == 0


def test_the_bn_backward_key():
    from fp8_quantization_amd.resnet_workload import _conv, approx_qparams
    assert "bn_backward" not in approx_qparams(ste_backward=True)["custom_approx_params"]
    assert "bn_backward" not in approx_qparams(ste_backward=True, bn_backward="torch")["custom_approx_params"]
    qp = approx_qparams(ste_backward=True, bn_backward="fused")
    assert qp["custom_approx_params"]["bn_backward"] == "fused"
    _conv(qp, 4, 8, 3, 1, 1, True)
    for bad in ("miopen", 1, None):
        qp["custom_approx_params"]["bn_backward"] = bad
        with pytest.raises(ValueError, match="bn_backward"):
            _conv(qp, 4, 8, 3, 1, 1, True)
