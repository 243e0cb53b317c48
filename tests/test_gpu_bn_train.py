"""Training-mode batch norm on the GPU (fp8a_bn_train, csrc/bn_train.h; approx_ops.bn_train).

The reference values are float64 two-pass statistics computed by torch on the CPU from the same x.
With u = 2^-24, n values per channel, K_c the channel's first value and D = max |x - K_c|:

  S1  the kernel's double sums are additions of n terms in a fixed tree, so (csrc/bn_train.h)
          |mean^ - mean64| <= dm = n 2^-52 D,     |var^ - var64| <= dv = 4 n 2^-52 D^2
      before the one fp32 rounding:  |save_mean - mean64| <= u |mean64| + dm,
                                     |save_var  - var64 | <= u var64 + dv.
  S2  scale = gamma / sqrt(var + eps) and shift = beta - mean * scale are computed in double from
      (mean^, var^) and rounded once.  Propagation (scale is decreasing and convex in var, so the
      derivative at the smaller variance bounds the difference):
          ds  = |gamma| dv / (2 (max(var64 - dv, 0) + eps)^1.5)
          dsh = |mean64| ds + |scale64| dm + dm ds + 2^-52 (|beta| + |mean64 scale64|)
      (the last term: the double product and subtraction, which matter only where beta cancels
      mean * scale), and the check is 2 fp32 ulps of the float64 value + ds (dsh).
  S3  running buffers: momentum 1 -> running_mean bit-equal to save_mean, running_var within 1 ulp of
      fp32(var64 n / (n - 1)); momentum m -> within 1 ulp of the float64 formula + m dm
      (m dv n / (n - 1)); null pointers leave the buffers untouched.
  A1  apply, from the kernel's RETURNED fp32 scale / shift: one fused multiply-add, so
          |y - t| <= u |t| (1 + 2^-20) + 2^-150,   t = x * scale + shift in float64
      (the double product is exact, the double sum adds 2^-53; 2^-150: a subnormal result); the
      clamp then holds exactly.
  A2  with an output quantizer y is bit-identical to fp8_fake_quantize of the unquantized bn_train
      output, and q_bias equals that call's bias.
  D   two calls return identical bytes in every output; in place equals out of place; statistics only
      leaves the same statistics; one capture + 2 replays under torch.cuda.graph equal eager.
Nothing here is measured: a failure means the kernel or the derivation is wrong.
"""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
EPS = float(np.float32(1e-5))  # (the C-ABI takes eps as fp32: the reference uses the same value)
SHAPES = [(3, 5, 7, 7),       # ragged inner = 49, no float4
          (2, 4, 65, 65),     # inner = 4225: an image's run crosses a 4096-value tile
          (5, 2, 64, 64),     # several parts per channel
          (1, 3, 4, 4),       # one image
          (2, 3, 1, 1),       # n = 2
          (33, 70),           # linear, inner = 1: the lanes-along-channels mapping
          (64, 16, 12, 12)]   # float4 path
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


_CASES = {}


def case(shape):
    """x (normal draws; one channel constant, one 4096 + 2^-8 U(-1, 1), one all zeros), gamma, beta and
    the float64 reference, computed once per shape and never modified."""
    if shape in _CASES:
        return _CASES[shape]
    g = torch.Generator().manual_seed(1234 + sum(shape) * 7 + len(shape))
    x = torch.randn(shape, generator=g) * 1.7 + 0.3
    C = shape[1]
    x[:, 0] = -2.625                                                     # var = 0
    x[:, 1] = 4096.0 + 2.0 ** -8 * (torch.rand(x[:, 1].shape, generator=g) * 2 - 1)   # cancellation
    if C > 2:
        x[:, 2] = 0.0
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    x64 = x.double().transpose(0, 1).reshape(C, -1)
    n = x64.shape[1]
    mean = x64.mean(dim=1)
    var = ((x64 - mean[:, None]) ** 2).mean(dim=1)
    D = (x64 - x64[:, :1]).abs().amax(dim=1)
    dm = n * 2.0 ** -52 * D
    dv = 4 * n * 2.0 ** -52 * D * D
    scale = gamma.double() / torch.sqrt(var + EPS)
    shift = beta.double() - mean * scale
    ds = gamma.double().abs() * dv / (2 * ((var - dv).clamp(min=0) + EPS) ** 1.5)
    dsh = mean.abs() * ds + scale.abs() * dm + dm * ds + 2.0 ** -52 * (beta.double().abs() + (mean * scale).abs())
    c = dict(x=x, gamma=gamma, beta=beta, n=n, C=C, mean=mean, var=var, dm=dm, dv=dv, scale=scale, shift=shift,
             ds=ds, dsh=dsh)
    _CASES[shape] = c
    return c


def ulp32(v64):
    """The fp32 spacing at |v| (float64 tensor in, float64 tensor out)."""
    return torch.from_numpy(np.spacing(np.abs(v64.numpy()).astype(np.float32)).astype(np.float64))


def run(shape, momentum=1.0, rm=None, rv=None, **kw):
    from fp8_quantization_amd.approx_ops import bn_train
    c = case(shape)
    x = c["x"].to(DEV)
    return bn_train(x, c["gamma"].to(DEV), c["beta"].to(DEV), rm, rv, momentum, EPS, **kw), x


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_against_float64(shape):
    c = case(shape)
    (y, sm, sv, ss, qb), _ = run(shape)
    sm, sv, ss = sm.cpu().double(), sv.cpu().double(), ss.cpu().double()
    em, ev = (sm - c["mean"]).abs(), (sv - c["var"]).abs()
    bm, bv = U * c["mean"].abs() + c["dm"], U * c["var"] + c["dv"]
    print("mean err / bar", (em / bm.clamp(min=1e-300)).max().item(), "var err / bar",
          (ev / bv.clamp(min=1e-300)).max().item())
    assert (em <= bm).all(), (em, bm)
    assert (ev <= bv).all(), (ev, bv)
    assert qb is None and y.shape == c["x"].shape
    es, eh = (ss[:, 0] - c["scale"]).abs(), (ss[:, 1] - c["shift"]).abs()
    bs, bh = 2 * ulp32(c["scale"]) + c["ds"], 2 * ulp32(c["shift"]) + c["dsh"]
    print("scale err / bar", (es / bs).max().item(), "shift err / bar", (eh / bh).max().item())
    assert (es <= bs).all(), (es, bs)
    assert (eh <= bh).all(), (eh, bh)
    # the constant channel: var = 0 exactly, scale = gamma / sqrt(eps)
    assert sv[0] == 0.0 and sm[0] == -2.625
    assert abs(ss[0, 0] - c["gamma"][0].double() / np.sqrt(EPS)) <= 2 * ulp32(c["scale"][:1])[0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_running_buffers(shape):
    c = case(shape)
    n, C = c["n"], c["C"]
    unb = c["var"] * n / (n - 1)
    # momentum 1: exactly the fp32-rounded batch values
    rm = torch.full((C,), 3.0, device=DEV)
    rv = torch.full((C,), 7.0, device=DEV)
    v0 = rm._version
    (_, sm, sv, _, _), _ = run(shape, 1.0, rm, rv, stats_only=True)
    assert torch.equal(bits(rm), bits(sm))
    assert rm._version > v0 and rv._version > v0
    want = unb.float().double()
    assert ((rv.cpu().double() - want).abs() <= ulp32(want)).all()
    # momentum 0.1 (the kernel receives it as fp32), random initial buffers
    g = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    m = float(np.float32(0.1))
    run(shape, 0.1, rm, rv, stats_only=True)
    wm = (1 - m) * rm0.double() + m * c["mean"]
    wv = (1 - m) * rv0.double() + m * unb
    assert ((rm.cpu().double() - wm).abs() <= ulp32(wm) + m * c["dm"]).all()
    assert ((rv.cpu().double() - wv).abs() <= ulp32(wv) + m * c["dv"] * n / (n - 1)).all()
    # null running pointers: nothing else is touched (the earlier buffers keep their bytes)
    keep_m, keep_v = rm.clone(), rv.clone()
    run(shape, 0.1, None, None, stats_only=True)
    assert torch.equal(bits(rm), bits(keep_m)) and torch.equal(bits(rv), bits(keep_v))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_and_quantizer(shape):
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    c = case(shape)
    (y, _, _, ss, _), x = run(shape)
    ss64 = ss.cpu().double()
    view = [1, -1] + [1] * (len(shape) - 2)
    t = c["x"].double() * ss64[:, 0].view(view) + ss64[:, 1].view(view)
    err = (y.cpu().double() - t).abs()
    bar = U * t.abs() * (1 + 2.0 ** -20) + 2.0 ** -150
    print("apply err / bar", (err / bar).max().item())
    assert (err <= bar).all()
    # the clamp holds exactly
    (yc, _, _, ss2, _), _ = run(shape, activation=nn.ReLU6())
    assert torch.equal(bits(ss2), bits(ss))
    assert torch.equal(bits(yc), bits(torch.clamp(y, 0.0, 6.0)))
    (yh, _, _, _, _), _ = run(shape, activation=nn.Hardtanh(-0.5, 1.25))
    assert torch.equal(bits(yh), bits(torch.clamp(y, -0.5, 1.25)))
    # a non-clamp activation is the caller's business
    assert run(shape, activation=nn.SiLU())[0] is None
    # the output quantizer: the separate pass's bytes
    mx = torch.tensor([2.5], device=DEV)
    for act, base in ((None, y), (nn.ReLU6(), yc)):
        for mb in (3, 2):
            (yq, _, _, _, qb), _ = run(shape, activation=act, out_quantizer=(mx, 8, mb, 1))
            want, wb = fp8_fake_quantize(base, mx, 8, mb, sign_bits=1)
            assert torch.equal(bits(yq), bits(want))
            assert torch.equal(bits(qb), bits(wb)) and torch.equal(qb._fp8a_i32, wb._fp8a_i32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_determinism_and_variants(shape):
    C = case(shape)["C"]
    mx = torch.tensor([3.0], device=DEV)
    kw = dict(activation=nn.ReLU(), out_quantizer=(mx, 8, 3, 1))
    outs = []
    for _ in range(2):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        (r, _) = run(shape, 0.1, rm, rv, **kw)
        outs.append(list(r) + [rm, rv])
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    # in place
    from fp8_quantization_amd.approx_ops import bn_train
    c = case(shape)
    x = c["x"].to(DEV)
    r = bn_train(x, c["gamma"].to(DEV), c["beta"].to(DEV), None, None, 0.1, EPS, out=x, **kw)
    assert r[0].data_ptr() == x.data_ptr()
    for a, b in zip(r, outs[0][:5]):
        assert torch.equal(bits(a), bits(b))
    # statistics only
    (r, _) = run(shape, 0.1, None, None, stats_only=True)
    assert r[0] is None and r[4] is None
    for a, b in zip(r[1:4], outs[0][1:4]):
        assert torch.equal(bits(a), bits(b))


def test_one_value_per_channel_raises():
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import bn_train
    x = torch.randn(1, 3, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn_train(x, None, None, None, None, 0.1, EPS)
    # ... and the C-ABI itself: the code _lib.check maps to ValueError; empty extents to AssertionError
    L = _lib.load()
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    o = torch.empty(8, device=DEV)
    p = _lib.dev_ptr
    call = lambda N, C, inner: L.fp8a_bn_train(p(x), None, N, C, inner, None, None, EPS, 0.1, None, None, p(o), p(o),  # noqa: E731
                                               p(o), 0, 0.0, 0.0, None, 0, 0, 0, None, None, p(ws), 64, None)
    with pytest.raises(ValueError):
        _lib.check(call(1, 3, 1), "fp8a_bn_train")
    for N, C in ((0, 3), (1, 0)):
        with pytest.raises(AssertionError):
            _lib.check(call(N, C, 1), "fp8a_bn_train")


def test_graph_capture_replays_bitwise():
    from fp8_quantization_amd.approx_ops import bn_train
    shape = SHAPES[0]
    c = case(shape)
    x, gamma, beta = c["x"].to(DEV), c["gamma"].to(DEV), c["beta"].to(DEV)
    mx = torch.tensor([3.0], device=DEV)
    rm, rv = torch.zeros(c["C"], device=DEV), torch.ones(c["C"], device=DEV)

    def fn():
        return bn_train(x, gamma, beta, rm, rv, 1.0, EPS, activation=nn.ReLU6(), out_quantizer=(mx, 8, 3, 1))
    eager = [t.clone() for t in fn()] + [rm.clone(), rv.clone()]
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(gs):
        fn()
    torch.cuda.current_stream().wait_stream(gs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=gs, capture_error_mode="thread_local"):
        out = fn()
    for i in range(2):
        for o in out:  # scribble over the captured outputs: the replay must rewrite them
            o.fill_(float("nan"))
        rm.fill_(0.5)  # (finite: momentum 1 multiplies the old value by 0)
        rv.fill_(0.5)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(list(out) + [rm, rv], eager):
            assert torch.equal(bits(a), bits(b)), f"replay {i} differs from the eager call"
