"""The straight-through backward (custom_approx_params["ste_backward"]) on the GPU.

Operators against a float64 twin on the CPU -- F.linear / F.conv2d / torch.matmul on the same quantized
operands: each gradient within 1e-5 * S of the twin's, S the same gradient product evaluated on |gradient| and
|operand| (the project's sum bar; the gradient GEMM's products are exact, only its summation order differs),
and no tile recomputed (the saved operands are on their FP8 grids).

Models (a ResNet basic block with a strided downsample branch, the tiny ViT of the attention tests with
approx attention): every parameter gradient against the twin MODEL -- the same model and the same recorded
forward, with every gradient GEMM replaced by the float64 product on the CPU (rounded to fp32 once).  The bar
per tensor: max |g - g_twin| <= 1e-5 * max S, S the same backward with every gradient GEMM evaluated on
|A| and |B| -- what the sums of all GEMMs on the way to that tensor are bounded by, the elementwise steps between
them (masks, the BN affine, ReLU gates, softmax and layer-norm Jacobians in fp32 torch) being the same code
in both runs.  fp32 rounds at 2^-24 = 6e-8 per operation, so 1e-5 leaves a factor of 170 for the depth.

The quantizer's own gradient is compared bit for bit with the reference's autograd (tests/golden/ste_quant.npz,
gen_golden_ste.py), a tie on the clamp bound passes half, the switch absent leaves outputs outside autograd,
and with the switch the forward's bytes are those of today's unfused forward.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(image_size=32, patch_size=8, hidden=32, layers=2, heads=2, mlp=64, num_labels=10)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _qp(**kw):
    from fp8_quantization_amd.resnet_workload import approx_qparams
    return approx_qparams(ste_backward=True, **kw)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _calibrate(m, *xs):
    from fp8_quantization_amd.quantization.base_quantized_classes import QuantizedModule
    for sub in m.modules():  # (a model's quantized(): every quantized layer's switches)
        if isinstance(sub, QuantizedModule):
            sub.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(*xs)
    m.fix_ranges()
    return m


def _assert_bar(got, ref, S, what):
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / S.clamp_min(1e-300)).max())
    print(f"{what}: max err / S = {worst:.3e}")
    assert bool((err <= 1e-5 * S).all()), f"{what}: outside 1e-5 S (worst {worst:.3e})"


def _twin_grads(prod, xq, wq, dy):
    """Gradients of the bilinear prod(x, w) in float64 on the CPU at upstream dy, and their S."""
    x, w, g = (t.detach().double().cpu() for t in (xq, wq, dy))
    out = []
    for a, b, u in ((x, w, g), (x.abs(), w.abs(), g.abs())):
        a, b = a.clone().requires_grad_(), b.clone().requires_grad_()
        out.append(torch.autograd.grad(prod(a, b), (a, b), u))
    return out  # [(dx, dw), (Sx, Sw)]


def _grad_stats(reset=False):
    from fp8_quantization_amd import _lib
    return _lib.grad_stats(reset)


def _operator_case(m, x, prod):
    """Calibrate m on x, then its product (run_forward) on the quantized operands as autograd leaves."""
    m = _calibrate(m.to(DEV).eval(), x)
    with torch.no_grad():
        xq = m.activation_quantizer(x)
        wq, bias = m.get_params()
    xq, wq = xq.detach().requires_grad_(), wq.detach().requires_grad_()
    _grad_stats(reset=True)
    y = m.run_forward(xq, wq, bias)
    assert y.requires_grad
    dy = _rand(y.shape, 7).to(DEV)
    y.backward(dy)
    st = _grad_stats(reset=True)
    assert st["launches"] >= 2 and st["recomputed"] == 0, st
    (dx, dw), (Sx, Sw) = _twin_grads(prod, xq, wq, dy)
    _assert_bar(xq.grad, dx, Sx, "dX")
    _assert_bar(wq.grad, dw, Sw, "dW")
    return st


# ------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("shape", [(5, 19), (2, 5, 19)], ids=["2d", "vit3d"])
def test_linear(shape):
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    m = QCustomLinearTorch(in_features=19, out_features=7, bias=True, **_qp())
    m.flatten_leading_dims = len(shape) == 3
    torch.nn.init.normal_(m.weight, generator=torch.Generator().manual_seed(1))
    _operator_case(m, _rand(shape, 2).to(DEV), lambda a, b: F.linear(a, b))


CONVS = {"g1": dict(cin=4, cout=6, k=3, stride=2, pad=1, groups=1),
         "g2": dict(cin=4, cout=6, k=3, stride=2, pad=1, groups=2),
         "depthwise": dict(cin=4, cout=4, k=3, stride=2, pad=1, groups=4),
         "1x1": dict(cin=4, cout=6, k=1, stride=1, pad=0, groups=1)}


@pytest.mark.parametrize("name", list(CONVS))
def test_conv(name):
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    c = CONVS[name]
    m = QCustomBNConv2dTorch(in_channels=c["cin"], out_channels=c["cout"], kernel_size=c["k"], stride=c["stride"],
                             padding=c["pad"], groups=c["groups"], bias=False, activation=None, **_qp())
    torch.nn.init.normal_(m.weight, generator=torch.Generator().manual_seed(3))
    st = _operator_case(m, _rand((2, c["cin"], 7, 7), 4).to(DEV),
                        lambda a, b: F.conv2d(a, b, None, c["stride"], c["pad"], 1, c["groups"]))
    # dW is one launch (groups as the batch index); dXcol one for groups = 1, else one per image or group
    assert st["launches"] == 1 + (1 if c["groups"] == 1 else min(2, c["groups"])), st


def test_bmm_on_head_views_with_a_transposed_k():
    """[2, 3, 5, 8] @ [2, 3, 8, 6]: both operands head views of [b, S, H d] buffers, read in place by the
    forward and by both gradient products of this operator (quantizers off: the buffers hold values on the
    default grid, bias 2^(E - 1))."""
    from fp8_quantization_amd.approx_calculation import QCustomMatMul
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    b, H, S, T, d = 2, 3, 5, 6, 8
    op = QCustomMatMul(**_qp()).to(DEV).eval()
    op.fix_ranges()
    mx = torch.tensor([240.0], device=DEV)  # bias 8 = 2^(E - 1)
    qbuf = fp8_fake_quantize(_rand((b, S, H * d), 5).to(DEV), mx, 8, 3)[0].requires_grad_()
    kbuf = fp8_fake_quantize(_rand((b, T, H * d), 6).to(DEV), mx, 8, 3)[0].requires_grad_()

    def heads(t):
        return t.view(t.shape[:-1] + (H, d)).permute(0, 2, 1, 3)
    _grad_stats(reset=True)
    c = op(heads(qbuf), heads(kbuf).transpose(-1, -2))
    assert c.shape == (b, H, S, T) and c.requires_grad
    dc = _rand(c.shape, 8).to(DEV)
    c.backward(dc)
    st = _grad_stats(reset=True)
    assert st["launches"] == 2 * b and st["recomputed"] == 0, st  # (the head views' two batch strides do not collapse)
    (dq, dk), (Sq, Sk) = _twin_grads(lambda x, y: torch.matmul(heads(x), heads(y).transpose(-1, -2)), qbuf, kbuf, dc)
    _assert_bar(qbuf.grad, dq, Sq, "dQ")
    _assert_bar(kbuf.grad, dk, Sk, "dK")


# ------------------------------------------------------------------------------------------ quantizer
def _golden_cases():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ste_quant.npz"))
    return z, sorted({k.split("/")[0] for k in z.files})


def test_quantizer_gradient_is_the_references_bit_for_bit():
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    z, names = _golden_cases()
    assert len(names) == 12 and sum(z[n + "/x"].size for n in names) == 4032
    for n in names:
        n_bits, mbits, sign_bits, per_channel = (int(v) for v in z[n + "/meta"])
        q = FPQuantizer(n_bits=n_bits, per_channel=bool(per_channel), mantissa_bits=mbits, set_maxval=True)
        q.maxval = torch.from_numpy(z[n + "/maxval"]).to(DEV)
        q.sign_bits = sign_bits
        q.ste_backward = True
        x = torch.from_numpy(z[n + "/x"]).to(DEV).requires_grad_()
        y = q(x)
        assert y.requires_grad
        y.sum().backward()
        assert np.array_equal(x.grad.cpu().numpy().view(np.int32), z[n + "/grad"].view(np.int32)), n
        # an upstream gradient goes through unchanged where the mask passes
        x.grad = None
        g = _rand(x.shape, 9).to(DEV)
        q(x).backward(g)
        assert torch.equal(x.grad, g * torch.from_numpy(z[n + "/grad"]).to(DEV)), n


def test_quantizer_tie_passes_half_and_off_means_off():
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    q = FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True)
    q.maxval = torch.tensor([2.0], device=DEV)
    x = torch.tensor([2.0, -2.0, 1.5, 3.0, -7.0, 0.0], device=DEV, requires_grad=True)
    assert not q(x).requires_grad  # the switch absent: the kernel's output, outside autograd
    q.ste_backward = True
    q(x).sum().backward()
    assert x.grad.tolist() == [0.5, 0.5, 1.0, 0.0, 0.0, 1.0]  # (ATen's max / min split a tie)
    with pytest.raises(NotImplementedError):
        q.make_range_trainable()


def test_switch_absent_outputs_do_not_require_grad():
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch, QCustomLinearTorch, QCustomMatMul
    from fp8_quantization_amd.resnet_workload import approx_qparams
    qp = approx_qparams()
    assert "ste_backward" not in qp["custom_approx_params"]
    # (no bias: a trainable bias is added by torch, `out += bias`, and that sum is recorded today as well)
    lin = _calibrate(QCustomLinearTorch(in_features=19, out_features=7, bias=False, **qp).to(DEV).eval(),
                     _rand((5, 19), 2).to(DEV))
    conv = _calibrate(QCustomBNConv2dTorch(in_channels=4, out_channels=6, kernel_size=3, padding=1, bias=False,
                                           activation=torch.nn.ReLU(), **approx_qparams()).to(DEV).eval(),
                      _rand((2, 4, 7, 7), 4).to(DEV))
    mm = _calibrate(QCustomMatMul(**approx_qparams()).to(DEV).eval(), _rand((2, 5, 8), 5).to(DEV),
                    _rand((2, 8, 6), 6).to(DEV))
    assert lin.weight.requires_grad and conv.weight.requires_grad and torch.is_grad_enabled()
    assert not lin(_rand((5, 19), 2).to(DEV).requires_grad_()).requires_grad
    assert not conv(_rand((2, 4, 7, 7), 4).to(DEV).requires_grad_()).requires_grad
    assert not mm(_rand((2, 5, 8), 5).to(DEV).requires_grad_(), _rand((2, 8, 6), 6).to(DEV)).requires_grad


# ------------------------------------------------------------------------------------------ models
def _twin_grad_bmm(use_abs):
    def f(A, B, out=None, k2=False):
        a, b = A.detach().double().cpu(), B.detach().double().cpu()
        if use_abs:
            a, b = a.abs(), b.abs()
        c = torch.einsum("...mkl,...kln->...mn", a, b) if k2 else a @ b
        c = c.float().to(A.device)
        if out is None:
            return c
        out.copy_(c)
        return out
    return f


def _param_grads(model, loss_fn, monkeypatch, mode):
    from fp8_quantization_amd import approx_ops
    with monkeypatch.context() as mp:
        if mode != "kernel":
            mp.setattr(approx_ops, "grad_bmm", _twin_grad_bmm(mode == "abs"))
        model.zero_grad(set_to_none=True)
        out = model_out = loss_fn()
        model_out.backward(_rand(out.shape, 11).to(DEV))
    return out.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _model_case(model, loss_fn, monkeypatch, frozen=()):
    _grad_stats(reset=True)
    out, g = _param_grads(model, loss_fn, monkeypatch, "kernel")
    st = _grad_stats(reset=True)
    assert st["launches"] > 0 and st["recomputed"] == 0, st
    out_t, gt = _param_grads(model, loss_fn, monkeypatch, "twin")
    _, gs = _param_grads(model, loss_fn, monkeypatch, "abs")
    assert torch.equal(out.view(torch.int32), out_t.view(torch.int32))  # the same recorded forward
    names = [n for n, _ in model.named_parameters()]
    assert sorted(set(names) - set(g)) == sorted(frozen), sorted(set(names) - set(g))
    assert set(g) == set(gt) == set(gs)
    for n in g:
        err = float((g[n].double() - gt[n].double()).abs().max())
        S = float(gs[n].double().abs().max())
        print(f"{n}: max err {err:.3e}, max S {S:.3e}, ratio {err / max(S, 1e-300):.3e}")
        assert err <= 1e-5 * S, f"{n}: max |g - g_twin| = {err:.3e} > 1e-5 * {S:.3e}"
        assert float(gt[n].abs().max()) > 0.0, f"{n}: the twin's gradient is all zero"
    return out


def _resnet_block(qp):
    from fp8_quantization_amd.resnet_workload import BasicBlock, QuantizedBlock
    torch.manual_seed(12)
    down = torch.nn.Sequential(torch.nn.Conv2d(4, 6, 1, 2, bias=False), torch.nn.BatchNorm2d(6))
    fp = BasicBlock(4, 6, 2, down)
    for bn in (fp.bn1, fp.bn2, down[1]):  # non-trivial eval statistics and affine
        bn.running_mean.normal_(0.0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.data.uniform_(0.5, 1.5)
        bn.bias.data.normal_(0.0, 0.2)
    return QuantizedBlock(fp, **qp).to(DEV).eval()


def _unfused(monkeypatch):
    """Today's unfused forward: every fused store and hand-off off."""
    from fp8_quantization_amd import chain, model_wrap
    from fp8_quantization_amd.approx_calculation import ApproxLinearMixin
    from fp8_quantization_amd.quantization.hijacker import QuantizationHijacker
    from fp8_quantization_amd.quantization.quantized_folded_bn import BNFusedHijacker
    monkeypatch.setattr(QuantizationHijacker, "fuse_input_quant", False)
    monkeypatch.setattr(BNFusedHijacker, "fuse_bn_act", False)
    monkeypatch.setattr(ApproxLinearMixin, "fuse_linear_block", False)
    monkeypatch.setattr(model_wrap, "FUSE_BLOCK", False)
    monkeypatch.setattr(chain, "CHAIN", False)


def test_resnet_block_parameter_gradients_and_forward_bytes(monkeypatch):
    from fp8_quantization_amd.resnet_workload import approx_qparams
    x = _rand((2, 4, 7, 7), 13).to(DEV)
    m = _calibrate(_resnet_block(_qp()), x)
    out = _model_case(m, lambda: m(x), monkeypatch)
    assert out.requires_grad is False and m(x).requires_grad
    # the switch set: the bytes of today's unfused forward (the same model without the switch)
    ref = _calibrate(_resnet_block(approx_qparams()), x)
    with monkeypatch.context() as mp, torch.no_grad():
        _unfused(mp)
        want = ref(x)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    with torch.no_grad():  # ... and without autograd the switch changes nothing: the fused forward, as ever
        assert torch.equal(m(x).view(torch.int32), ref(x).view(torch.int32))


def test_tiny_vit_parameter_gradients_and_forward_bytes(monkeypatch):
    from fp8_quantization_amd.vit_workload import vit_b16_approx
    xcal, x = _rand((4, 3, 32, 32), 14).to(DEV), _rand((3, 3, 32, 32), 15).to(DEV)
    m = _calibrate(vit_b16_approx(seed=43, approx_attention=True, ste_backward=True, **TINY).to(DEV).eval(), xcal)
    # (the patch projection is the exact convolution, QCustomConv2dTorch: not an approx operator, so its weight
    # has no backward; its bias is added by torch)
    frozen = [n for n, _ in m.named_parameters() if n.endswith("patch_embeddings.projection.weight")]
    assert len(frozen) == 1
    out = _model_case(m, lambda: m(x), monkeypatch, frozen=frozen)
    ref = _calibrate(vit_b16_approx(seed=43, approx_attention=True, **TINY).to(DEV).eval(), xcal)
    with monkeypatch.context() as mp, torch.no_grad():
        _unfused(mp)
        want = ref(x)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))

