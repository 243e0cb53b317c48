"""``approx_attention`` on the quantized ViT without a GPU: the option's module tree and state dict, its
errors, the calibration-state forward (the exact product on the quantized operands, with the FP8 fake
quantizer as the CPU oracle's restatement) and the rank-0 quantizer broadcast of the six new quantizers."""
import os
import socket

import numpy as np
import pytest
import torch

from fp8_quantization_amd import vit_workload as vw
from fp8_quantization_amd.approx_calculation import QCustomMatMul

TINY = dict(image_size=32, patch_size=8, hidden=32, layers=2, heads=2, mlp=64, num_labels=10)


def _classes(m):
    return [(n, type(x).__name__) for n, x in m.named_modules()]


def test_option_off_changes_nothing():
    base = vw.vit_b16_approx(seed=0, **TINY)
    off = vw.vit_b16_approx(seed=0, approx_attention=False, **TINY)
    assert list(base.state_dict()) == list(off.state_dict())
    assert _classes(base) == _classes(off)
    assert not any(isinstance(m, QCustomMatMul) for m in off.modules())


def test_option_on_adds_the_two_operators_under_every_attention():
    base = vw.vit_b16_approx(seed=0, **TINY)
    on = vw.vit_b16_approx(seed=0, approx_attention=True, **TINY)
    new = set(on.state_dict()) - set(base.state_dict())
    assert set(base.state_dict()) <= set(on.state_dict())
    for i in range(TINY["layers"]):
        att = on.vit.encoder.layer[i].attention.attention
        for name in ("qk_matmul", "pv_matmul"):
            op = getattr(att, name)
            assert isinstance(op, QCustomMatMul)
            assert [n for n, _ in op.named_children()] == ["a_quantizer", "b_quantizer", "res_quantizer"]
            assert f"vit.encoder.layer.{i}.attention.attention.{name}._quant_a" in new
    assert all(".qk_matmul." in k or ".pv_matmul." in k for k in new)
    macs = vw.vit_approx_macs_per_image(**{k: v for k, v in TINY.items() if k != "heads"})
    assert vw.vit_approx_macs_per_image(approx_attention=True, **{k: v for k, v in TINY.items() if k != "heads"}) == \
        macs + TINY["layers"] * 2 * 17 * 17 * TINY["hidden"]
    assert vw.vit_approx_macs_per_image(approx_attention=True) - vw.vit_approx_macs_per_image() == \
        12 * 2 * 197 * 197 * 768


def test_option_errors():
    no_approx = dict(approx_flag=False, quantize_after_mult_and_add=False, res_quantizer_flag=True,
                     original_quantize_res=True)
    with pytest.raises(ValueError):
        vw.vit_b16_approx(seed=0, approx_attention=True, run_method=no_approx, **TINY)
    vw.vit_b16_approx(seed=0, approx_attention=False, run_method=no_approx, **TINY)  # off: as before
    qamaa = dict(approx_flag=True, quantize_after_mult_and_add=True, res_quantizer_flag=True,
                 original_quantize_res=False)
    with pytest.raises(NotImplementedError, match="QCustomMatMul"):
        vw.vit_b16_approx(seed=0, approx_attention=True, run_method=qamaa, **TINY)
    with pytest.raises(NotImplementedError, match="QCustomMatMul"):
        vw.vit_b16_approx(seed=0, approx_attention=True, approx_version=5, **TINY)
    from fp8_quantization_amd import imagenet
    args = imagenet.parse(["--synthetic", "4", "--arch", "resnet18", "--approx-attention"])
    with pytest.raises(ValueError):
        imagenet.build_model(args.arch, None, imagenet.approx_cfg(args), 32)
    assert "approx_attention" not in imagenet.approx_cfg(imagenet.parse(["--synthetic", "4", "--arch", "vit_b16"]))


def test_res_flag_error_is_kept():
    from fp8_quantization_amd.resnet_workload import approx_qparams
    qp = approx_qparams(run_method=dict(approx_flag=True, quantize_after_mult_and_add=False, res_quantizer_flag=False,
                                        original_quantize_res=False))
    op = QCustomMatMul(**qp)
    with pytest.raises(ValueError, match="res_quantizer_flag"):
        op(torch.zeros(1, 2, 3), torch.zeros(1, 3, 2))


# ---------------------------------------------------------------------------------- calibration forward
def _install_fake_quant():
    """The FP8 fake quantizer as the CPU oracle's restatement (tests/test_distributed_cpu.py's stand-in)."""
    from fp8_quantization_amd.quantization import fp8_quantizer as fq
    from oracle import oracle

    def fake_quant(x, maxval, n_bits, M, sign_bits=1, per_row=False):
        assert sign_bits == 1
        mx = torch.as_tensor(maxval, dtype=torch.float32).reshape(-1).cpu().numpy()
        out, bias = oracle.fp8_fake_quant(x.detach().cpu().numpy(), mx, n_bits - 1 - M, M, per_row and mx.size > 1)
        b = torch.from_numpy(np.ascontiguousarray(bias))
        if per_row and mx.size > 1:
            b = b.view([-1] + [1] * (x.dim() - 1))
        return torch.from_numpy(out).to(x.device), b

    fq.fp8_fake_quantize = fake_quant


def _calibrated_tiny(seed):
    """The tiny model with approx_attention, every approx product switched off (no GPU here), after one
    calibration forward on CPU; returns (model, input)."""
    from fp8_quantization_amd.quantization.base_quantized_classes import QuantizedModule
    _install_fake_quant()
    m = vw.vit_b16_approx(seed=seed, approx_attention=True, **TINY).eval()
    for mod in m.modules():
        if isinstance(mod, QuantizedModule):
            mod.approx_flag = False
    m.quantized()
    m.estimate_ranges()
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(seed + 1))
    return m, x


def test_calibration_forward_is_the_exact_product(monkeypatch):
    from fp8_quantization_amd.quantization import fp8_quantizer as fq
    monkeypatch.setattr(fq, "fp8_fake_quantize", fq.fp8_fake_quantize)  # restored after the test
    m, x = _calibrated_tiny(0)
    att = m.vit.encoder.layer[0].attention.attention
    seen = {}
    hooks = [att.register_forward_hook(lambda mod, i, o: seen.update(x=i[0], ctx=o))]
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    for op in (att.qk_matmul, att.pv_matmul):
        for q in (op.a_quantizer, op.b_quantizer, op.res_quantizer):
            b = q.get_fp_bias()
            assert b is not None and b.numel() == 1 and float(b) == round(float(b))
    # the same attention by hand: the quantizers without range update on the calibrated ranges
    H, d = att.num_attention_heads, att.attention_head_size
    with torch.no_grad():
        xin = seen["x"]

        def heads(t):
            return t.view(t.shape[:-1] + (H, d)).permute(0, 2, 1, 3)
        for mgr in m.modules():
            if hasattr(mgr, "fix_ranges") and hasattr(mgr, "quantizer"):
                mgr.fix_ranges()
        q, k, v = heads(att.query(xin)), heads(att.key(xin)), heads(att.value(xin))
        qk, pv = att.qk_matmul, att.pv_matmul
        s = qk.res_quantizer.quantizer(torch.matmul(qk.a_quantizer.quantizer(q), qk.b_quantizer.quantizer(k.transpose(-1, -2))))
        p = torch.softmax(s * d ** -0.5, -1)
        c = pv.res_quantizer.quantizer(torch.matmul(pv.a_quantizer.quantizer(p), pv.b_quantizer.quantizer(v)))
        want = att.quantize_activations(c.permute(0, 2, 1, 3).reshape(xin.shape[0], xin.shape[1], H * d))
    assert torch.equal(seen["ctx"], want)
    # ... and with the quantizers off it is softmax(q k^T / sqrt(d)) v itself
    m.full_precision()
    with torch.no_grad():
        got = att(xin)
        q, k, v = heads(att.query(xin)), heads(att.key(xin)), heads(att.value(xin))
        ref = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * d ** -0.5, -1), v)
    assert torch.allclose(got, ref.permute(0, 2, 1, 3).reshape(got.shape), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------- gloo broadcast
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bias_list(m):
    out = []
    for lay in m.vit.encoder.layer:
        att = lay.attention.attention
        for op in (att.qk_matmul, att.pv_matmul):
            for q in (op.a_quantizer, op.b_quantizer, op.res_quantizer):
                b = q.get_fp_bias()
                out.append(None if b is None else float(b.reshape(-1)[0]))
                out.append(float(q.quantizer.maxval.reshape(-1)[0]))
    return out


def _bcast_worker(rank, ws, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from fp8_quantization_amd.distributed import broadcast_quant_state
        if rank == 0:
            m, x = _calibrated_tiny(0)
            with torch.no_grad():
                m(x)
        else:  # never calibrated: no bias anywhere
            m = vw.vit_b16_approx(seed=7, approx_attention=True, **TINY).eval()
        before = _bias_list(m)
        broadcast_quant_state(m, src=0)
        q.put((rank, before, _bias_list(m)))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_broadcast_carries_the_six_quantizers_per_layer():
    import torch.multiprocessing as mp
    ws, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bcast_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in range(ws)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, b0, a0), (_, b1, a1) = res
    assert len(a0) == TINY["layers"] * 2 * 3 * 2 and None not in a0
    assert all(v is None for v in b1[0::2])  # rank 1 had no bias before
    assert a1 == a0 == b0
