"""The attention softmax block's host side (fp8a_attn_softmax / _backward) without a device: the exported symbols, every
refusal on fake pointers (each returns before any launch), and the attention_softmax key: its validation, and the
attention module's bytes with the key absent, "torch" or "fused" on CPU tensors (no fused route there)."""
import ctypes

import pytest
import torch

from fp8_quantization_amd import _lib

FAKE = ctypes.c_void_p(4096)          # non-null, 16-byte aligned, never dereferenced


def test_symbols_are_exported():
    assert {"fp8a_attn_softmax", "fp8a_attn_softmax_backward"} <= set(_lib.SYMBOLS)
    assert _lib.load().fp8a_attn_softmax and _lib.load().fp8a_attn_softmax_backward


def call(backward, rows=8, n=197, s=FAKE, g=FAKE, out=FAKE, mx=FAKE, n_bits=8, M=3, S=1):
    L = _lib.load()
    if backward:
        return L.fp8a_attn_softmax_backward(s, g, rows, n, 0.125, mx, n_bits, M, S, out, None)
    return L.fp8a_attn_softmax(s, rows, n, 0.125, mx, n_bits, M, S, out, None, None, None)


BAD = [dict(s=None), dict(out=None), dict(rows=-1), dict(rows=2 ** 31), dict(n=0), dict(n=4097), dict(n=-3), dict(M=0),
       dict(M=8), dict(M=7, S=1), dict(S=2)]


@pytest.mark.parametrize("backward, kw", [(False, kw) for kw in BAD] + [(True, kw) for kw in BAD + [dict(g=None)]], ids=str)
def test_refusals_come_before_any_launch(backward, kw):
    assert call(backward, **kw) == _lib.EINVAL
    assert _lib.load().fp8a_last_error()


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_no_rows_is_success_and_a_format_is_read_only_with_a_maxval(backward):
    assert call(backward, rows=0) == _lib.OK
    assert call(backward, rows=0, mx=None, M=0) == _lib.OK


def test_the_attention_softmax_key():
    from fp8_quantization_amd import vit_workload as vw
    from fp8_quantization_amd.resnet_workload import approx_qparams
    from tests.test_vit_attention_cpu import TINY
    assert "attention_softmax" not in approx_qparams(attention_softmax="torch")["custom_approx_params"]
    assert approx_qparams(attention_softmax="fused")["custom_approx_params"]["attention_softmax"] == "fused"
    for bad in ("flash", 1, None):
        with pytest.raises(ValueError, match="attention_softmax.*" + repr(bad)):
            vw.vit_b16_approx(seed=0, approx_attention=True, attention_softmax=bad, **TINY)


def test_the_module_is_the_parents_with_the_key_absent_and_on_cpu_tensors(monkeypatch):
    """The calibrated tiny ViT of tests/test_vit_attention_cpu.py against the parent's lines by hand."""
    from fp8_quantization_amd.quantization import fp8_quantizer as fq
    from tests.test_vit_attention_cpu import _calibrated_tiny
    monkeypatch.setattr(fq, "fp8_fake_quantize", fq.fp8_fake_quantize)  # (_calibrated_tiny replaces it)
    m, x = _calibrated_tiny(0)
    att = m.vit.encoder.layer[0].attention.attention
    assert "attention_softmax" not in att.custom_approx_params
    seen = {}
    hook = att.register_forward_hook(lambda mod, i, o: seen.update(x=i[0]))
    with torch.no_grad():
        m(x)
    hook.remove()
    for mgr in m.modules():  # (the managers alone, as that file does: the products stay the exact ones)
        if hasattr(mgr, "fix_ranges") and hasattr(mgr, "quantizer"):
            mgr.fix_ranges()
    H, d = att.num_attention_heads, att.attention_head_size
    xin = seen["x"]

    def heads(t):
        return t.view(t.shape[:-1] + (H, d)).permute(0, 2, 1, 3)
    with torch.no_grad():
        got = att(xin)
        qk, pv = att.qk_matmul, att.pv_matmul
        q, k, v = heads(att.query(xin)), heads(att.key(xin)), heads(att.value(xin))
        s = qk.res_quantizer(torch.matmul(qk.a_quantizer(q), qk.b_quantizer(k.transpose(-1, -2))))
        c = pv.res_quantizer(torch.matmul(pv.a_quantizer(torch.softmax(s * d ** -0.5, -1)), pv.b_quantizer(v)))
        want = att.quantize_activations(c.permute(0, 2, 1, 3).reshape(xin.shape[0], xin.shape[1], H * d))
        assert torch.equal(got, want)
        for value in ("torch", "fused"):
            monkeypatch.setitem(att.custom_approx_params, "attention_softmax", value)
            assert torch.equal(att(xin), want)
