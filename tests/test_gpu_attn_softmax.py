"""The attention softmax block on the GPU (csrc/attn_softmax.h; approx_ops.attention_softmax*; the attention module's
attention_softmax key) against float64 torch on the CPU.  Every bar comes from that reference and from torch's own
fp32 CPU result on the same input, never from the kernel (DESIGN.md §3ak's convention); the quantized forward is
bracketed by the monotone quantizer on p_ref -+ bar, with at most 2 % of the elements where the two ends differ.
scale = 0.125 is a power of two, so scale * s is the same number in fp32 and float64."""
import numpy as np
import pytest
import torch

from tests import store_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.125
SHAPES = [(7, 1),       # a degenerate row: p = 1, ds = 0
          (7, 5),       # a partly filled lane set
          (6, 64),      # V = 1 full; the last workgroup has 2 live rows
          (5, 65),      # one element past the lane stride (V = 2); 1 live row
          (9, 197),     # the workload's length (V = 4); 1 live row
          (5, 1024),    # the widest wave form (V = 16)
          (3, 1025),    # the first workgroup form
          (3, 4096)]    # the largest
QUANTS = {"none": None, "s8m3": (1.0, 8, 3, 1), "u8m3": (0.25, 8, 3, 0)}  # (maxval, n_bits, M, sign_bits)
CASES = [(s, q) for s in SHAPES for q in QUANTS]
IDS = [f"{s[0]}x{s[1]}-{q}" for s, q in CASES]


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")


_REF = {}


def ref(shape, qname):
    """s ~ 8 N(0, 1), row 0 all equal, row 1 (not under the unsigned quantizer) with two entries of 1e4: exp overflows
    unless the maximum is subtracted; g ~ N(0, 1); the float64 and torch-fp32 CPU results and their bars, computed once."""
    if (shape, qname) in _REF:
        return _REF[shape, qname]
    rows, n = shape
    gen = torch.Generator().manual_seed(1000 * n + rows)
    s = torch.randn(shape, generator=gen) * 8
    s[0] = 3.25
    if qname != "u8m3":  # (there the quantizer resolves 2^-36: a row of n - 2 exact zeros would make the bracket
        s[1, :2] = 1e4   # [fake_quant(-bar) = 0, fake_quant(+bar) > 0] two-valued for a third of a 3-row tensor)
    g = torch.randn(shape, generator=gen)
    q = QUANTS[qname]
    lo, hi = (None, None) if q is None else (-q[0] if q[3] else 0.0, q[0])

    def both(dtype):
        x = s.to(dtype).requires_grad_(True)
        p = torch.softmax(x * SCALE, -1)
        (p if q is None else p.clamp(lo, hi)).backward(g.to(dtype))
        return p.detach(), x.grad
    p64, d64 = both(torch.float64)
    p32, d32 = both(torch.float32)
    bar = max(4 * float((p32.double() - p64).abs().max()), 2.0 ** -24)
    ulp = 2.0 ** (np.floor(np.log2(float(d64.abs().max()))) - 23) if float(d64.abs().max()) > 0 else 0.0
    dbar = max(4 * float((d32.double() - d64).abs().max()), ulp)
    _REF[shape, qname] = dict(s=s, g=g, q=q, p=p64, ds=d64, bar=bar, dbar=dbar)
    return _REF[shape, qname]


def quantizer(r):
    return None if r["q"] is None else (torch.tensor([r["q"][0]], device=DEV),) + r["q"][1:]


@pytest.mark.parametrize("shape, qname", CASES, ids=IDS)
def test_forward(shape, qname):
    from fp8_quantization_amd.approx_ops import attention_softmax
    r = ref(shape, qname)
    out = torch.full(shape, float("nan"), device=DEV)
    y, bias = attention_softmax(r["s"].to(DEV), SCALE, quantizer(r), out=out)
    y = y.cpu().double()
    if r["q"] is None:
        err = float((y - r["p"]).abs().max())
        print(f"forward {shape}: max |y - p_ref| = {err:.3g}, bar = {r['bar']:.3g}")
        assert bias is None and err <= r["bar"]
        assert float((y.sum(-1) - 1).abs().max()) <= shape[1] * 2.0 ** -23
        return
    lo, _ = sr.fake_quant((r["p"] - r["bar"]).numpy(), *r["q"])
    hi, _ = sr.fake_quant((r["p"] + r["bar"]).numpy(), *r["q"])
    share = float((lo != hi).mean())
    print(f"forward {shape} {qname}: {share:.4%} of the elements have two admissible values")
    assert share <= 0.02                                   # (the reference alone: the check stays sharp)
    assert bool(((lo <= y.numpy()) & (y.numpy() <= hi)).all())
    want = sr.fq_bias(*r["q"])
    assert float(bias) == want and int(bias._fp8a_i32) == int(want)


@pytest.mark.parametrize("shape, qname", CASES, ids=IDS)
def test_backward_alias_and_determinism(shape, qname):
    from fp8_quantization_amd.approx_ops import attention_softmax, attention_softmax_backward
    r = ref(shape, qname)
    s, q = r["s"].to(DEV), quantizer(r)
    if r["q"] is not None and shape[1] > 1:  # the clamp mask is unambiguous (n = 1: ds = 0 whatever the weight)
        assert float((r["p"] - r["q"][0]).abs().min()) > r["bar"]
    outs = [attention_softmax_backward(s, r["g"].to(DEV), SCALE, q, out=torch.full(shape, float("nan"), device=DEV))
            for _ in range(2)]
    g = r["g"].to(DEV)
    outs.append(attention_softmax_backward(s, g, SCALE, q, out=g))  # in place
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))
    ds = outs[0].cpu().double()
    err = float((ds - r["ds"]).abs().max())
    print(f"backward {shape} {qname}: max |ds - ref| = {err:.3g}, bar = {r['dbar']:.3g}")
    assert err <= r["dbar"]
    if shape[1] == 1:
        assert not bool(ds.any())
    ys = [attention_softmax(s, SCALE, q, out=torch.full(shape, float("nan"), device=DEV))[0] for _ in range(2)]
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))


# ------------------------------------------------------------------------------------------ the operator
def _attention(key, ste=False):
    from fp8_quantization_amd.resnet_workload import approx_qparams
    from fp8_quantization_amd.vit_workload import QuantizedViTSelfAttention, ViTSelfAttention
    torch.manual_seed(5)
    qp = approx_qparams(ste_backward=ste, **({} if key is None else {"attention_softmax": key}))
    att = QuantizedViTSelfAttention(ViTSelfAttention(32, 2, 0.0), **qp)
    att.enable_approx_attention(**qp)
    for lin in (att.query, att.key, att.value):
        lin.flatten_leading_dims = True  # (as the ViT builder sets it: token rows [B, S, D])
    att = att.to(DEV).eval()
    for m in att.modules():  # (the model wrapper's quantized(): every quantized module under it)
        if hasattr(m, "quantized"):
            m.quantized()
    att.estimate_ranges()
    x = torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        att(x)
    att.fix_ranges()
    return att, x


def test_operator_takes_the_fused_route_and_the_torch_key_changes_nothing():
    from fp8_quantization_amd.approx_ops import attention_softmax, attention_softmax_backward
    att, x = _attention("fused", ste=True)
    seen = {}

    def on_scores(mod, i, o):
        seen["scores"] = o
        o.register_hook(lambda gr: seen.update(ds=gr))

    def on_operand(mod, i, o):
        seen["operand"] = i[0]
        i[0].register_hook(lambda gr: seen.update(g=gr))
    hooks = [att.qk_matmul.register_forward_hook(on_scores), att.pv_matmul.register_forward_hook(on_operand)]
    out = att(x)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    (out * w).sum().backward()
    for h in hooks:
        h.remove()
    fq = att.pv_matmul.a_quantizer.quantizer
    q = (fq.maxval, fq.n_bits, fq._mbits_int, fq.sign_bits)
    scale = att.attention_head_size ** -0.5
    y, bias = attention_softmax(seen["scores"].detach(), scale, q)
    assert torch.equal(seen["operand"].view(torch.int32), y.view(torch.int32))
    assert torch.equal(fq.custom_bias, bias)
    ds = attention_softmax_backward(seen["scores"].detach(), seen["g"], scale, q)
    assert torch.equal(seen["ds"].view(torch.int32), ds.view(torch.int32))
    with torch.no_grad():  # the key at "torch": the bytes of the module without the key
        (a, xa), (b, xb) = _attention("torch"), _attention(None)
        assert torch.equal(a(xa).view(torch.int32), b(xb).view(torch.int32))
