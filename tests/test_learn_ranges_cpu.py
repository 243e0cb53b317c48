"""Learned FP8 ranges without a device: the quantizer's / managers' / model's state machine on host tensors,
the fixture's self-check (tests/golden/learn_maxval.npz against the numpy closed form, learn_ranges_ref.py) and
the argument validation of the three fp8a_fq_train_* entry points (every check runs before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

from fp8_quantization_amd import _lib

from . import learn_ranges_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learn_maxval.npz")


def _quantizer(**kw):
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    return FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True, **kw)


def _manager(**kw):
    from fp8_quantization_amd.quantization import FPQuantizer, QuantizationManager
    return QuantizationManager(qmethod=FPQuantizer, qparams=dict(n_bits=8, mantissa_bits=3, set_maxval=True, **kw))


# ------------------------------------------------------------------------------------------ state machine
def test_learn_ranges_makes_maxval_a_parameter_and_fix_ranges_restores_it():
    from fp8_quantization_amd.quantization.quantization_manager import Qstates
    mgr = _manager(learn_maxval=True)
    mgr.set_quant_range(-1.5, 2.5)
    q = mgr.quantizer
    assert not isinstance(q.maxval, nn.Parameter) and list(mgr.parameters()) == [] and q.maxval.tolist() == [2.5]
    mgr.learn_ranges()
    assert mgr.state == Qstates.learn_ranges and q.state == Qstates.learn_ranges
    p = q.maxval
    assert isinstance(p, nn.Parameter) and p.requires_grad and p.tolist() == [2.5]
    assert [id(t) for t in mgr.parameters()] == [id(p)] and "quantizer.maxval" in mgr.state_dict()
    mgr.learn_ranges()  # twice: nothing changes
    assert q.maxval is p and len(list(mgr.parameters())) == 1
    with torch.no_grad():
        p.mul_(2.0)
    mgr.fix_ranges()
    assert mgr.state == Qstates.fix_ranges
    assert not isinstance(q.maxval, nn.Parameter) and not q.maxval.requires_grad and q.maxval.tolist() == [5.0]
    assert list(mgr.parameters()) == [] and "quantizer.maxval" not in mgr.state_dict()
    mgr.learn_ranges()  # ... and back
    assert isinstance(q.maxval, nn.Parameter) and q.maxval.tolist() == [5.0]


def test_unsupported_requests_raise():
    with pytest.raises(NotImplementedError, match="mantissa"):
        _quantizer(learn_mantissa_bits=True).make_range_trainable()
    with pytest.raises(NotImplementedError, match="mantissa"):
        _quantizer(learn_maxval=True, learn_mantissa_bits=True).make_range_trainable()
    q = _quantizer()
    with pytest.raises(NotImplementedError):  # neither flag: not the reference's silent no-op
        q.make_range_trainable()
    assert not isinstance(q.maxval, nn.Parameter)
    with pytest.raises(NotImplementedError):
        _manager().learn_ranges()


def test_range_updates_keep_a_parameters_identity():
    q = _quantizer(learn_maxval=True)
    q.make_range_trainable()
    p = q.maxval
    q.set_quant_range(-0.5, 3.0)
    assert q.maxval is p and p.tolist() == [3.0] and p.requires_grad and p.grad_fn is None
    q.set_quant_range(torch.tensor([-1.0, -4.0]), torch.tensor([2.0, 3.0]))  # another shape: still the Parameter
    assert q.maxval is p and p.tolist() == [2.0, 4.0] and p.is_leaf
    # (forward's device move takes the same route; test_gpu_learn_ranges.py runs it on a host-built quantizer)
    plain = _quantizer()
    plain.set_quant_range(-0.5, 3.0)  # a plain tensor is replaced, as ever
    assert not isinstance(plain.maxval, nn.Parameter) and plain.maxval.tolist() == [3.0]


def test_learned_range_with_the_switch_off_raises_before_any_kernel():
    q = _quantizer(learn_maxval=True)
    q.make_range_trainable()
    with pytest.raises(RuntimeError, match="ste_backward"):
        q(torch.zeros(4))


class _Uninitialized(nn.Module):
    """A quantizer that reports itself uninitialized (the reference's integer quantizers before calibration)."""
    is_initialized = False
    state = None

    def __init__(self, per_channel=False, **kw):
        super().__init__()

    def make_range_trainable(self):
        raise AssertionError("learn_ranges reached an uninitialized quantizer")


def test_layer_and_model_learn_ranges_skip_uninitialized_quantizers():
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    from fp8_quantization_amd.model_wrap import QuantizedModel
    from fp8_quantization_amd.quantization import QuantizationManager
    from fp8_quantization_amd.quantization.quantization_manager import Qstates
    from fp8_quantization_amd.resnet_workload import approx_qparams

    class Tiny(QuantizedModel):
        def __init__(self):
            super().__init__((1, 19))
            self.fc = QCustomLinearTorch(in_features=19, out_features=7, **approx_qparams(learn_maxval=True))
            self.extra = QuantizationManager(qmethod=_Uninitialized)

    for target in (lambda m: m.fc, lambda m: m):
        m = Tiny()
        target(m).learn_ranges()
        mgrs = (m.fc.activation_quantizer, m.fc.weight_quantizer, m.fc.res_quantizer)
        assert all(g.state == Qstates.learn_ranges and isinstance(g.quantizer.maxval, nn.Parameter) for g in mgrs)
        assert m.extra.state == Qstates.estimate_ranges
        assert sum(n.endswith("quantizer.maxval") for n, _ in m.named_parameters()) == 3
        target(m).fix_ranges()
        assert not any(n.endswith("maxval") for n, _ in m.named_parameters())
        assert all(g.state == Qstates.fix_ranges for g in mgrs)
    with pytest.raises(AssertionError, match="uninitialized"):
        m.extra.learn_ranges()  # the manager itself does not skip (quantization_manager.py:100-102)


def test_approx_qparams_learn_maxval_reaches_every_quantizer_of_a_small_resnet():
    from fp8_quantization_amd.distributed import quantizers
    from fp8_quantization_amd.resnet_workload import BasicBlock, QuantizedResNet, ResNet, approx_qparams
    assert approx_qparams()["fp8_kwargs"]["learn_maxval"] is False
    torch.manual_seed(0)
    m = QuantizedResNet(ResNet(BasicBlock, [1, 1, 1, 1], num_classes=10), input_size=(1, 3, 32, 32),
                        **approx_qparams(learn_maxval=True, ste_backward=True))
    qs = quantizers(m)
    assert len(qs) > 20 and all(q.learning_maxval for q in qs)
    before = len(list(m.parameters()))
    m.learn_ranges()
    assert all(isinstance(q.maxval, nn.Parameter) for q in qs)
    assert len(list(m.parameters())) == before + len({id(q) for q in qs})
    m.fix_ranges()
    assert len(list(m.parameters())) == before
    plain = QuantizedResNet(ResNet(BasicBlock, [1, 1, 1, 1], num_classes=10), input_size=(1, 3, 32, 32),
                            **approx_qparams())
    with pytest.raises(NotImplementedError):
        plain.learn_ranges()


def test_finetune_flags():
    from fp8_quantization_amd import finetune
    a = finetune.parse(["--synthetic", "8"])
    assert a.learn_ranges is False and a.range_lr is None and "learn_maxval" not in finetune.approx_cfg(a)
    a = finetune.parse(["--synthetic", "8", "--learn-ranges", "--range-lr", "1e-5"])
    assert a.learn_ranges and a.range_lr == 1e-5 and finetune.approx_cfg(a)["learn_maxval"] is True


# ------------------------------------------------------------------------------------------ fixture
def test_fixture_budget_and_closed_form():
    z = np.load(GOLDEN)
    names = sorted({k.split("/")[0] for k in z.files})
    assert len(names) == 12 and all(z[n + "/x"].shape == (5, 333) for n in names)
    ties = 0
    for n in names:
        n_bits, mbits, sign_bits, per_channel = (int(v) for v in z[n + "/meta"])
        x, g, maxval = z[n + "/x"], z[n + "/g"], z[n + "/maxval"]
        assert maxval.shape == ((5,) if per_channel else (1,))
        assert np.array_equal(g, np.round(g * 512) / 512) and np.abs(g * 512).max() <= 127
        gx, gm, budget = lr.closed_form(x, maxval, g, sign_bits, per_channel)
        assert (budget <= lr.BUDGET).all(), (n, budget / lr.U)
        wx, wm = lr.weights(x, maxval, sign_bits, per_channel)
        assert 0.1 < (wx == 0).mean() < 0.3 and (np.abs(wm) == 0.5).mean() > 0.01, n
        ties += int((np.abs(wm) == 0.5).sum())
        if sign_bits == 0:
            assert (x == 0).mean() > 0.01 and not (wm < 0).any()
        assert np.array_equal(lr.bits(z[n + "/grad_x"]), lr.bits(gx)), n
        assert np.array_equal(z[n + "/grad_maxval"].view(np.int32), gm.astype(np.float32).view(np.int32)), n
        assert (gm.astype(np.float32).astype(np.float64) == gm).all()  # the sums are exact in fp32
    assert ties > 400


# ------------------------------------------------------------------------------------------ C ABI
FAKE = ctypes.c_void_p(4096)  # never dereferenced: every call below fails a check before any HIP call


def _fwd(L, x=FAKE, rows=1, inner=100, maxval=FAKE, n_bits=8, mbits=3, sign_bits=1, y=FAKE, code=FAKE):
    return L.fp8a_fq_train_forward(x, rows, inner, maxval, n_bits, mbits, sign_bits, y, code, None, None, None)


def _bwd(L, g=FAKE, code=FAKE, rows=1, inner=100, sign_bits=1, gx=FAKE, gmax=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = L.fp8a_fq_train_workspace_size(rows, inner)
    return L.fp8a_fq_train_backward(g, code, rows, inner, sign_bits, gx, gmax, ws, ws_bytes, None)


def test_workspace_query_is_host_only_and_follows_the_split_rule():
    L = _lib.load()
    f = L.fp8a_fq_train_workspace_size
    T = 4096
    assert f(1, T) == 8 and f(1, T + 1) == 16 and f(1, 3 * T + 37) == 32     # a part per tile
    assert f(960, 9) == 960 * 8 and f(961, 64) == 961 * 8                     # short rows: one thread each
    assert f(512, 4608) == 512 * 2 * 8                                        # two tiles, two parts
    assert f(1, 1 << 33) == 2048 * 8 and f(4096, 1 << 20) == 4096 * 8         # the target caps the parts
    assert f(1, 0) == 8
    for bad in ((0, 10), (-1, 10), (1, -1), ((1 << 24) + 1, 10)):
        assert f(*bad) == 0, bad
    old = _lib.set_option("fqt_target_wgs", 2)
    try:
        assert old == 2048 and f(1, 7 * T + 5) == 16 and f(3, 7 * T + 5) == 3 * 8
        assert _lib.set_option("fqt_target_wgs", 0) == 2 and _lib.set_option("fqt_target_wgs", old) == 1
    finally:
        _lib.set_option("fqt_target_wgs", 2048)


@pytest.mark.parametrize("call,kw,rc,msg", [
    (_fwd, dict(x=None), _lib.EINVAL, "null"), (_fwd, dict(maxval=None), _lib.EINVAL, "null"),
    (_fwd, dict(y=None), _lib.EINVAL, "null"), (_fwd, dict(code=None), _lib.EINVAL, "null"),
    (_fwd, dict(rows=0), _lib.EINVAL, "rows"), (_fwd, dict(rows=-3), _lib.EINVAL, "rows"),
    (_fwd, dict(inner=-1), _lib.EINVAL, "inner"),
    (_fwd, dict(mbits=0), _lib.EFORMAT, "format"), (_fwd, dict(mbits=7), _lib.EFORMAT, "format"),
    (_fwd, dict(mbits=7, sign_bits=0, n_bits=7), _lib.EFORMAT, "format"), (_fwd, dict(sign_bits=2), _lib.EFORMAT, "format"),
    (_bwd, dict(g=None), _lib.EINVAL, "null"), (_bwd, dict(code=None), _lib.EINVAL, "null"),
    (_bwd, dict(gx=None), _lib.EINVAL, "null"), (_bwd, dict(gmax=None), _lib.EINVAL, "null"),
    (_bwd, dict(ws=None), _lib.EINVAL, "null"),
    (_bwd, dict(rows=0), _lib.EINVAL, "rows"), (_bwd, dict(inner=-1), _lib.EINVAL, "inner"),
    (_bwd, dict(sign_bits=-1), _lib.EFORMAT, "format"),
    (_bwd, dict(inner=3 * 4096, ws_bytes=16), _lib.EINVAL, "workspace"), (_bwd, dict(ws_bytes=0), _lib.EINVAL, "workspace"),
    (_bwd, dict(ws=ctypes.c_void_p(4100)), _lib.EINVAL, "misaligned"),
])
def test_entry_points_reject_bad_arguments_before_any_hip_call(call, kw, rc, msg):
    L = _lib.load()
    assert call(L, **kw) == rc
    assert msg in L.fp8a_last_error().decode()
    exc = {_lib.EINVAL: AssertionError, _lib.EFORMAT: ValueError}[rc]
    with pytest.raises(exc, match=msg):
        _lib.check(rc, "fp8a_fq_train")
