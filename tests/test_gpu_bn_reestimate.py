"""BN statistics re-estimation on the GPU: the training-mode forward of BNFusedHijacker on the
bn_train kernels (fuse_bn_train), bn_reestimate.reestimate_bn_stats, the eval forward afterwards, the
driver flag, and the reference fixture tests/golden/bn_reestimate.npz.

Bars (u = 2^-24; see tests/test_gpu_bn_train.py for the kernel's own): against float64 two-pass
statistics of the recorded pre-BN tensor, n values per channel, K the channel's first value,
D = max |x - K|, A = max |x|, Dm = max |x - mean|:
  fused     |mean - mean64| <= u |mean64| + n 2^-52 D;  the unbiased variance in the buffer within
            u v + 4 n 2^-52 D^2 n / (n - 1) of v = var64 n / (n - 1)  (csrc/bn_train.h);
  unfused   (MIOpen / the reference's torch, fp32 sums in an unknown order: the any-order bounds of
            tests/test_bn_reestimate_cpu.py)  n u A  and  ((n + 4) u Dm^2 + 2 Dm n u A) n / (n - 1).
Outputs: y = x * scale + shift; two evaluations from statistics (mean_a, var_a), (mean_b, var_b) differ
by at most |x| |scale_a - scale_b| + |shift_a - shift_b| (evaluated in float64 from the two runs' own
buffers) plus the roundings of each evaluation: one for the fused multiply-add, and for the unfused
(x - mean) * invstd * gamma + beta four, each at most u (|x scale| + |shift|) -- so
  |y_a - y_b| <= propagated + (1 + R) u (|x scale| + |shift|),  R = 4 for an unfused side, 1 for a fused.
"""
import copy
import json

import numpy as np
import pytest
import torch
from torch import nn

from tests import golden_io as gio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


def stats64(pre):
    """float64 (mean, biased var, n, D, A, Dm) per channel of a pre-BN tensor (CPU)."""
    x = pre.detach().cpu().double().transpose(0, 1).reshape(pre.shape[1], -1)
    n = x.shape[1]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, var, n, (x - x[:, :1]).abs().amax(1), x.abs().amax(1), (x - mean[:, None]).abs().amax(1)


def fused_bars(pre):
    mean, var, n, D, A, Dm = stats64(pre)
    unb = var * n / (n - 1)
    return U * mean.abs() + n * 2.0 ** -52 * D, U * unb + 4 * n * 2.0 ** -52 * D * D * n / (n - 1)


def unfused_bars(pre):
    mean, var, n, D, A, Dm = stats64(pre)
    return n * U * A + 1e-45, ((n + 4) * U * Dm ** 2 + 2 * Dm * n * U * A) * n / (n - 1) + 1e-45


def record_pre(mod, store):
    """Record (a clone of) every product mod.run_forward returns: the pre-BN tensor."""
    f = type(mod).run_forward

    def run_forward(x, weight, bias, offsets=None, **kw):
        y = f(mod, x, weight, bias, offsets=offsets, **kw)
        store.append((y[0] if isinstance(y, tuple) else y).detach().clone())
        return y
    mod.run_forward = run_forward


def out_bar(pre, m_a, v_a, m_b, v_b, gamma, beta, eps, n, R):
    """The output bar of the module doc from the two runs' buffers (unbiased variances in)."""
    view = [1, -1] + [1] * (pre.dim() - 2)
    x = pre.detach().cpu().double()
    g, b = gamma.detach().cpu().double(), beta.detach().cpu().double()
    sc = [g / torch.sqrt(v.cpu().double() * (n - 1) / n + eps) for v in (v_a, v_b)]
    sh = [b - m.cpu().double() * s for m, s in zip((m_a, m_b), sc)]
    mag = x.abs() * sc[0].abs().view(view) + sh[0].abs().view(view)
    return x.abs() * (sc[0] - sc[1]).abs().view(view) + (sh[0] - sh[1]).abs().view(view) + (1 + R) * U * mag


LAYERS = {"conv": dict(cin=16, cout=48, groups=1, act=nn.ReLU6(), quantize_input=True),
          "depthwise": dict(cin=32, cout=32, groups=32, act=nn.ReLU6(), quantize_input=True),
          "own_output_quantizer": dict(cin=16, cout=40, groups=1, act=nn.ReLU(), quantize_input=False),
          # not a clamp: batch norm alone on the kernels, the activation after them, unfused
          "non_clamp": dict(cin=16, cout=24, groups=1, act=nn.SiLU(), quantize_input=True)}


@pytest.mark.parametrize("kind", list(LAYERS))
def test_operator_training_forward_fused_vs_unfused(kind):
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    from fp8_quantization_amd.resnet_workload import approx_qparams
    c = LAYERS[kind]
    qp = approx_qparams()
    qp["quantize_input"] = c["quantize_input"]
    torch.manual_seed(3)
    m = QCustomBNConv2dTorch(in_channels=c["cin"], out_channels=c["cout"], kernel_size=3, padding=1, groups=c["groups"],
                             bias=False, activation=c["act"], **qp)
    with torch.no_grad():
        m.gamma.normal_(1, 0.2)
        m.beta.normal_(0, 0.2)
    m = m.to(DEV).eval()
    m.quantized()
    m.estimate_ranges()
    x = torch.randn(4, c["cin"], 11, 11, device=DEV)
    with torch.no_grad():
        m(x)
    m.fix_ranges()
    runs = {}
    for fuse in (True, False):
        mod = copy.deepcopy(m)
        mod.training, mod.momentum, mod.fuse_bn_train = True, 1.0, fuse
        pre, qin = [], []
        record_pre(mod, pre)
        if not c["quantize_input"]:  # the unquantized output, as the layer's own quantizer receives it
            mod.activation_quantizer.register_forward_pre_hook(lambda _m, inp: qin.append(inp[0].detach().clone()))
        with torch.no_grad():
            y = mod(x)
        assert len(pre) == 1
        runs[fuse] = dict(mod=mod, pre=pre[0], y=y, qin=qin)
        assert mod._fused_epilogue() is None and not mod.block_epilogue_ok()  # the eval stores decline
    on, off = runs[True], runs[False]
    assert torch.equal(bits(on["pre"]), bits(off["pre"]))
    assert on["qin"] == []  # fused: the quantizer ran inside the apply kernel ...
    if not c["quantize_input"]:
        assert len(off["qin"]) == 1
        assert torch.equal(on["mod"].activation_quantizer.quantizer.custom_bias.reshape(-1),
                           off["mod"].activation_quantizer.quantizer.custom_bias.reshape(-1))  # ... and left its bias
    mean, var, n, *_ = stats64(on["pre"])
    unb = var * n / (n - 1)
    for r, bars, tag in ((on, fused_bars(on["pre"]), "fused"), (off, unfused_bars(off["pre"]), "unfused")):
        em = (r["mod"].running_mean.cpu().double() - mean).abs()
        ev = (r["mod"].running_var.cpu().double() - unb).abs()
        print(kind, tag, "mean err / bar", (em / bars[0]).max().item(), "var err / bar", (ev / bars[1]).max().item())
        assert (em <= bars[0]).all() and (ev <= bars[1]).all(), tag
    mo, mf = on["mod"], off["mod"]
    if kind == "non_clamp":  # exactly the activation module on the kernels' plain batch norm
        from fp8_quantization_amd.approx_ops import bn_train
        plain = bn_train(on["pre"].clone(), mo.gamma, mo.beta, None, None, 1.0, mo.epsilon)[0]
        assert torch.equal(bits(on["y"]), bits(c["act"](plain)))
        return
    bar = out_bar(on["pre"], mo.running_mean, mo.running_var, mf.running_mean, mf.running_var, mo.gamma, mo.beta,
                  mo.epsilon, n, R=4)
    if c["quantize_input"]:
        err = (on["y"].cpu().double() - off["y"].cpu().double()).abs()
        print(kind, "output err / bar", (err / bar).max().item())
        assert (err <= bar).all()
    else:
        # the quantizer is monotone: the fused output lies between the quantized ends of the bar
        # around the unfused run's unquantized value
        q = off["mod"].activation_quantizer.quantizer
        v = off["qin"][0]
        b32 = (bar * (1 + 2.0 ** -20)).float().to(DEV)
        fq = lambda t: fp8_fake_quantize(t, q.maxval, q.n_bits, q._mbits_int, q.sign_bits)[0]  # noqa: E731
        assert (fq(v - b32) <= on["y"]).all() and (on["y"] <= fq(v + b32)).all()
        print(kind, "quantized outputs that differ:", (on["y"] != off["y"]).float().mean().item())


# ------------------------------------------------------------------------------------ model level
def _mbv2():
    from fp8_quantization_amd.mobilenet_workload import mobilenet_v2_approx
    torch.manual_seed(11)
    return mobilenet_v2_approx(input_size=64, width_mult=0.5, n_class=100, bn_stats_batches=1), (3, 64, 64)


def _resnet18():
    from fp8_quantization_amd.quantization.quantized_folded_bn import BNFusedHijacker
    from fp8_quantization_amd.resnet_workload import resnet18_approx
    torch.manual_seed(12)
    m = resnet18_approx()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, BNFusedHijacker):
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.5, 2.0)
    return m, (3, 32, 32)


_MODELS = {}


def calibrated(arch):
    """(calibrated E4M3 model on the GPU, batches) -- built once; the tests work on deep copies."""
    if arch not in _MODELS:
        m, shape = {"mobilenet_v2": _mbv2, "resnet18": _resnet18}[arch]()
        m = m.to(DEV).eval()
        g = torch.Generator().manual_seed(5)
        xs = [torch.randn((4,) + shape, generator=g).to(DEV) for _ in range(3)]
        m.quantized()
        m.estimate_ranges()
        with torch.no_grad():
            m(xs[0])
        m.fix_ranges()
        _MODELS[arch] = (m, xs)
    return _MODELS[arch]


def bn_layers(model):
    from fp8_quantization_amd.bn_reestimate import bn_fused_layers
    return bn_fused_layers(model)


@pytest.mark.parametrize("arch", ["mobilenet_v2", "resnet18"])
def test_model_reestimate_is_reproducible_and_eval_picks_it_up(arch):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
    base, xs = calibrated(arch)
    with torch.no_grad():
        logits0 = base(xs[2]).clone()  # (also fills every layer's _bn_act_cache with the OLD statistics)
    runs = []
    for _ in range(2):
        m = copy.deepcopy(base)
        layers = bn_layers(m)
        moms = [l.momentum for _, l in layers]
        pres = []
        with torch.no_grad():
            m(xs[2])  # this copy's own _bn_act_cache entries: the re-estimation must invalidate them
        if not runs:
            record_pre(layers[0][1], pres)
        assert reestimate_bn_stats(m, [(x, 0) for x in xs[:2]], num_batches=2) == 2
        assert [l.momentum for _, l in layers] == moms
        assert all(not mod.training for mod in m.modules())
        runs.append((m, pres))
    a, b = runs[0][0], runs[1][0]
    for (name, la), (_, lb) in zip(bn_layers(a), bn_layers(b)):
        assert torch.equal(bits(la.running_mean), bits(lb.running_mean)), name
        assert torch.equal(bits(la.running_var), bits(lb.running_var)), name
        assert torch.isfinite(la.running_var).all()
    # layer 0: the mean of the two batches' statistics, against float64 of the recorded pre-BN tensors
    pres = runs[0][1]
    assert len(pres) == 2
    l0 = bn_layers(a)[0][1]
    s = [stats64(p) for p in pres]
    n = s[0][2]
    want_m = (s[0][0] + s[1][0]) / 2
    want_v = (s[0][1] + s[1][1]) / 2 * n / (n - 1)
    bm = sum(fused_bars(p)[0] for p in pres) / 2 + 2 * U * want_m.abs()   # + the fp32 sum and division
    bv = sum(fused_bars(p)[1] for p in pres) / 2 + 2 * U * want_v
    assert ((l0.running_mean.cpu().double() - want_m).abs() <= bm).all()
    assert ((l0.running_var.cpu().double() - want_v).abs() <= bv).all()
    # the eval forward afterwards == a fresh copy whose buffers were set by hand (the fused eval store,
    # block tail and chain are back on, and the cached scale / shift follow the new statistics)
    fresh = copy.deepcopy(base)
    for _, l in bn_layers(fresh):
        l.__dict__.pop("_bn_act_cache", None)
    with torch.no_grad():
        for (_, lf), (_, la) in zip(bn_layers(fresh), bn_layers(a)):
            lf.running_mean.copy_(la.running_mean)
            lf.running_var.copy_(la.running_var)
        _lib.path_stats(reset=True)
        la_ = a(xs[2])
        pa = _lib.path_stats(reset=True)
        lf_ = fresh(xs[2])
        pf = _lib.path_stats(reset=True)
    assert torch.equal(bits(la_), bits(lf_))
    assert pa == pf
    assert all(l._fused_epilogue() is not None for _, l in bn_layers(a) if getattr(l, "supports_bn_act_epilogue", False))
    assert not torch.equal(bits(la_), bits(logits0))  # the statistics did change the forward


def test_driver_flag(capsys):
    from fp8_quantization_amd import imagenet
    base = ["--synthetic", "8", "--batch-size", "4", "--image-size", "64", "--arch", "mobilenet_v2", "--num-workers", "0"]

    def run(extra):
        torch.manual_seed(21)  # the synthetic-weights model's initialisation
        imagenet.main(base + extra)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])
    on = run(["--reestimate-bn-stats", "--bn-batches", "2"])
    assert on["reestimate_bn_stats"] is True and on["bn_batches"] == 2 and on["images"] == 8
    on2 = run(["--reestimate-bn-stats", "--bn-batches", "2"])
    plain, no = run([]), run(["--no-reestimate-bn-stats"])
    assert plain["reestimate_bn_stats"] is False and plain["bn_batches"] is None
    for k in ("top_1_accuracy", "top_5_accuracy", "loss", "images"):
        assert plain[k] == no[k], k          # default off: the run is what it always was
        assert on[k] == on2[k], k            # two re-estimated runs: identical statistics, identical result
    # (a random-weights network scores at chance either way: the loss itself says nothing here)
    assert np.isfinite(on["loss"]) and np.isfinite(plain["loss"])


# ------------------------------------------------------------------------------------ the fixture
def _g8_model():
    from fp8_quantization_amd.mobilenet_workload import mobilenet_v2_approx
    case = gio.meta()["g8"][0]
    assert case["name"] == "mbv2_e4m3"
    g = gio.load("g8_mbv2.npz")
    m = mobilenet_v2_approx(input_size=case["input_size"], width_mult=case["width_mult"], n_class=case["n_class"],
                            expo_width=case["E"], mant_width=case["M"], withComp=case["with_comp"],
                            run_method=case.get("run_method"))
    state = {k: torch.from_numpy(g[f"mbv2_e4m3__state__{k}"]) for k in case["state_keys"]}
    missing, unexpected = torch.nn.Module.load_state_dict(m, state, strict=False)
    assert not unexpected and not missing
    m = m.to(DEV).eval()
    m.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(torch.from_numpy(g["mbv2_e4m3__x_cal"]).to(DEV))
    m.fix_ranges()
    return m


def test_fixture_teacher_forced():
    """bn_train on the reference's recorded pre-BN tensors reproduces its recorded per-batch statistics
    within (our derived bar + the reference's own recorded distance from float64), and its recorded
    layer outputs within the output bar on top of that."""
    from fp8_quantization_amd.approx_ops import bn_train
    from tests.test_bn_reestimate_cpu import ref_distance
    g = gio.load("bn_reestimate.npz")
    model = _g8_model()
    mods = dict(model.named_modules())
    for name in (str(s) for s in g["teacher"]):
        mod = mods[name]
        assert mod.quantize_input  # (no output quantizer of its own in this network)
        for b in (0, 1):
            pre = torch.from_numpy(g[f"pre{b}/{name}"])
            rm, rv = torch.zeros_like(mod.running_mean), torch.ones_like(mod.running_var)
            y = bn_train(pre.to(DEV), mod.gamma, mod.beta, rm, rv, 1.0, mod.epsilon,
                         activation=mod.activation_function)[0]
            dm, dv, n = ref_distance(g, name, b)
            bm, bv = fused_bars(pre)
            rmean, rvar = torch.from_numpy(g[f"stat_mean{b}/{name}"]), torch.from_numpy(g[f"stat_var{b}/{name}"])
            em = (rm.cpu().double() - rmean.double()).abs()
            ev = (rv.cpu().double() - rvar.double()).abs()
            assert (em <= bm + torch.from_numpy(dm)).all(), (name, b)
            assert (ev <= bv + torch.from_numpy(dv) * n / (n - 1) + U * rvar.double()).all(), (name, b)
            bar = out_bar(pre, rm, rv, rmean, rvar, mod.gamma, mod.beta, mod.epsilon, n, R=4)
            err = (y.cpu().double() - torch.from_numpy(g[f"out{b}/{name}"]).double()).abs()
            print(name, b, "output err / bar", (err / bar).max().item())
            assert (err <= bar).all(), (name, b)


# measured on an MI355X (the BN re-estimation section): the largest normalised distance of
# our re-estimated statistics from the reference's over the 52 layers; the bar is 4x that (a different
# kernel choice for a product moves its sum within 1e-5 sum |v| and can flip a quantizer step).
# Measured: every mean bit-equal to the reference's (0.0), variances within 2.08e-7.  A measured 0 gives
# no bar, so each figure is floored at 2^-23, one fp32 ulp of a statistic of the size it is divided by.
E2E_MEASURED = (0.0, 2.08e-7)
E2E_FLOOR = 2.0 ** -23


def test_fixture_end_to_end_distance():
    """Not teacher-forced: our re-estimation of the whole network against the reference's final
    statistics, max |d mean| / sqrt(var_ref + eps) and max |d var| / (var_ref + eps) per layer."""
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
    g = gio.load("bn_reestimate.npz")
    model = _g8_model()
    mods = dict(model.named_modules())
    names = [str(s) for s in g["layers"]]
    for name in names:  # the fixture's initial statistics are the ones g8's state holds
        assert np.array_equal(mods[name].running_mean.cpu().numpy(), g[f"init_mean/{name}"])
    reestimate_bn_stats(model, [(torch.from_numpy(g[k]), 0) for k in ("x0", "x1")], num_batches=2)
    worst_m = worst_v = 0.0
    for name in names:
        mod = mods[name]
        vr = torch.from_numpy(g[f"final_var/{name}"]).double() + mod.epsilon
        dm = ((mod.running_mean.cpu().double() - torch.from_numpy(g[f"final_mean/{name}"]).double()).abs() / vr.sqrt()).max().item()
        dv = ((mod.running_var.cpu().double() - torch.from_numpy(g[f"final_var/{name}"]).double()).abs() / vr).max().item()
        print(f"{name:28s} dmean {dm:.3e} dvar {dv:.3e}")
        worst_m, worst_v = max(worst_m, dm), max(worst_v, dv)
    print("worst", worst_m, worst_v)
    assert worst_m <= 4 * max(E2E_MEASURED[0], E2E_FLOOR) and worst_v <= 4 * max(E2E_MEASURED[1], E2E_FLOOR)
