"""The layer norm block's host side (fp8a_layer_norm / _backward) without a device: the exported symbols, every refusal
on fake pointers (each returns before any launch), the layer_norm key's validation, and QuantLayerNorm's bytes with the
key absent, "torch" or "fused" on CPU tensors (no fused route there)."""
import ctypes

import pytest
import torch

from fp8_quantization_amd import _lib

FAKE = ctypes.c_void_p(4096)          # non-null, 16-byte aligned, never dereferenced
NAMES = {"fp8a_layer_norm", "fp8a_layer_norm_backward_workspace_size", "fp8a_layer_norm_backward"}


def test_symbols_and_names_are_exported():
    from fp8_quantization_amd import approx_ops
    assert NAMES <= set(_lib.SYMBOLS) and all(getattr(_lib.load(), name) for name in NAMES)
    for name in ("layer_norm", "layer_norm_backward", "layer_norm_ste", "LAYER_NORMS", "check_layer_norm"):
        assert name in approx_ops.__all__ and hasattr(approx_ops, name)
    assert _lib.load().fp8a_layer_norm_backward_workspace_size(19, 768) == 3 * 768 * 16   # runs of 8 rows
    assert _lib.load().fp8a_layer_norm_backward_workspace_size(8197, 12) == 513 * 12 * 16  # runs of 16


def call(backward, rows=8, n=768, x=FAKE, g=FAKE, gamma=FAKE, stat=FAKE, out=FAKE, mx=FAKE, n_bits=8, M=3, S=1, ws=FAKE,
         nbytes=1 << 20):
    L = _lib.load()
    if backward:
        return L.fp8a_layer_norm_backward(x, g, rows, n, gamma, stat, stat, mx, n_bits, M, S, out, FAKE, FAKE, ws, nbytes,
                                          None)
    return L.fp8a_layer_norm(x, rows, n, gamma, FAKE, 1e-5, mx, n_bits, M, S, out, stat, stat, None, None, None)


BAD = [dict(x=None), dict(out=None), dict(gamma=None), dict(stat=None), dict(rows=-1), dict(rows=2 ** 31), dict(n=0),
       dict(n=4097), dict(M=0), dict(M=8), dict(M=7, S=1), dict(S=2)]
BAD_BWD = [dict(g=None), dict(ws=None), dict(ws=ctypes.c_void_p(4104)), dict(nbytes=768 * 16 - 1)]


@pytest.mark.parametrize("backward, kw", [(False, kw) for kw in BAD] + [(True, kw) for kw in BAD + BAD_BWD], ids=str)
def test_refusals_come_before_any_launch(backward, kw):
    assert call(backward, **kw) == _lib.EINVAL
    assert _lib.load().fp8a_last_error()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_no_rows_is_success_and_a_format_is_read_only_with_a_maxval(backward):
    assert call(backward, rows=0) == _lib.OK
    assert call(backward, rows=0, mx=None, M=0) == _lib.OK


def test_the_layer_norm_key_and_cpu_tensors_keep_the_torch_lines():
    from fp8_quantization_amd.model_wrap import QuantLayerNorm
    from fp8_quantization_amd.resnet_workload import approx_qparams
    assert "layer_norm" not in approx_qparams(layer_norm="torch")["custom_approx_params"]
    assert approx_qparams(layer_norm="fused")["custom_approx_params"]["layer_norm"] == "fused"
    for bad in ("apex", 1, None):
        with pytest.raises(ValueError, match="layer_norm.*" + repr(bad)):
            QuantLayerNorm(8, **approx_qparams(layer_norm=bad))
    x = torch.randn(3, 5, 8, generator=torch.Generator().manual_seed(0))
    outs = []
    for key in (None, "torch", "fused"):
        torch.manual_seed(1)
        ln = QuantLayerNorm(8, eps=1e-12, **approx_qparams(**({} if key is None else {"layer_norm": key})))
        with torch.no_grad():
            ln.weight.normal_()
            ln.bias.normal_()
        ln.fix_ranges()  # (the quantizers stay off: no device here; the fused plan holds, the tensor is on the CPU)
        assert ln._fused_plan() == (key == "fused", None)
        outs.append(ln(x))
        assert torch.equal(ln.run_forward(x, ln.weight, ln.bias), torch.nn.functional.layer_norm(x, (8,), ln.weight, ln.bias, 1e-12))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
