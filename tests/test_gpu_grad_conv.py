"""The implicit-GEMM convolution backward (fp8a_grad_conv2d_dgrad / _wgrad, csrc/gemm_grad_conv.h)
on the GPU against F.conv2d's float64 backward on the CPU:

  1. grad_conv2d_input / grad_conv2d_weight bit for bit on exact-sum inputs (x, w multiples of 1/4, |i| <= 3; dy
     multiples of 2^-20, |i| <= 127, with one three-piece element per plane; u = 2^-22, budget 2^22 u asserted),
     every element written, one launch per call, nothing recomputed, two calls the same bytes;
  2. lost elements (inf in dy, 1 + 2^-12 in x or w): recomputed tiles, untouched outputs bit-equal to the clean run;
  3. ste_conv2d(backward="implicit") and the layers' conv_backward key;
  4. the backward's transient memory on both paths.

The wide case (72 -> 70 channels) takes w in {-1, 0, 1} / 4: with |i| <= 3 its data gradient sums 70 planted
elements of 65793 u times |w| up to 3 per input pixel, 2^23.7 u; with |i| <= 1 the bound is 70 x 65793 + 630 x 127 <
2^22.2 u at every |w| = 1 and the budget assertion holds on the drawn weights (a third of them 0).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_sums as xs
from tests import grad_exact as gx
from tests.test_gpu_grad_split import _assert_bar, _layer_grads, _make_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -22
BASE = (3, 8, 13, 11)
KERNELS = {"3x3": ((3, 3), (1, 1), (1, 1)), "1x1": ((1, 1), (0, 0), (1, 1)), "3x2d": ((3, 2), (1, 0), (1, 2))}
# (x shape, Cout, kernel, stride, groups, |i| of w)
CASES = {f"{k}-s{s[0]}{s[1]}-g{g}": (BASE, 12, k, s, g, 3)
         for k in KERNELS for s in ((1, 1), (2, 2), (2, 1)) for g in (1, 2, 4)}
CASES["wide"] = ((2, 72, 5, 4), 70, "3x3", (1, 1), 1, 1)
CASES["depthwise"] = (BASE, 8, "3x3", (2, 2), 8, 3)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _stats():
    from fp8_quantization_amd import _lib
    return _lib.grad_stats(reset=True)


def _backward64(x, w, dy, geo, use_abs=False):
    """conv_backward64's recipe at any geometry: (dx, dw) of F.conv2d in float64 on the CPU."""
    x, w, dy = (t.double().abs() if use_abs else t.double() for t in (x, w, dy))
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    with np.errstate(invalid="ignore"):
        return torch.autograd.grad(F.conv2d(x, w, None, *geo), (x, w), dy)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dict(x, w, dy, geo, dx, dw): CPU float32 operands, (stride, padding, dilation, groups) and the float64
    gradients; the exact-sum budget is asserted here, once per case."""
    xshape, cout, kname, stride, groups, wmax = CASES[cid]
    k, pad, dil = KERNELS[kname]
    geo = (stride, pad, dil, groups)
    rng = np.random.default_rng([29] + [ord(c) for c in cid])
    x = torch.from_numpy((rng.integers(-3, 4, size=xshape) / 4.0).astype(np.float32))
    w = torch.from_numpy((rng.integers(-wmax, wmax + 1, size=(cout, xshape[1] // groups) + k) / 4.0).astype(np.float32))
    ho, wo = F.conv2d(x, w, None, *geo).shape[2:]
    dy = rng.integers(-127, 128, size=(xshape[0], cout, ho, wo)).astype(np.float64)
    # one element per plane with three nonzero bf16 pieces, at an interior pixel
    dy[:, :, ho // 2, wo // 2] = (2 ** 16 + 2 ** 8 + 1) * rng.choice([-1.0, 1.0], size=dy.shape[:2])
    dy = torch.from_numpy((dy * 2.0 ** -20).astype(np.float32))
    for s in _backward64(x, w, dy, geo, use_abs=True):
        assert gx.budget_of(s.numpy(), U) <= 22, (cid, gx.budget_of(s.numpy(), U))
    dx, dw = _backward64(x, w, dy, geo)
    return dict(x=x, w=w, dy=dy, geo=geo, dx=dx, dw=dw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dgrad(p, dy=None, w=None):
    """(dX on the CPU, stats) of one grad_conv2d_input call into a NaN-filled out."""
    from fp8_quantization_amd.approx_ops import grad_conv2d_input
    out = torch.full(tuple(p["x"].shape), float("nan"), device=DEV)
    _stats()
    res = grad_conv2d_input((p["dy"] if dy is None else dy).to(DEV), (p["w"] if w is None else w).to(DEV),
                            p["x"].shape, *p["geo"], out=out)
    assert res is out
    return out.cpu(), _stats()


def _wgrad(p, split_k, dy=None, x=None):
    from fp8_quantization_amd.approx_ops import grad_conv2d_weight
    out = torch.full(tuple(p["w"].shape), float("nan"), device=DEV)
    _stats()
    res = grad_conv2d_weight((p["dy"] if dy is None else dy).to(DEV), (p["x"] if x is None else x).to(DEV),
                             p["w"].shape, *p["geo"], split_k=split_k, out=out)
    assert res is out
    return out.cpu(), _stats()


# ------------------------------------------------------------------------------------------ 1. the two functions
@pytest.mark.parametrize("cid", list(CASES))
def test_gradients_equal_the_float64_backward_bit_for_bit(cid):
    p = problem(cid)
    want = p["dx"].numpy().astype(np.float32)
    got, st = _dgrad(p)
    assert st["launches"] == 1 and st["recomputed"] == 0, st
    xs.assert_same(got.numpy(), want, f"{cid} dX")
    assert not np.signbit(got.numpy()[want == 0]).any(), f"{cid}: a zero of dX is not +0"
    again, _ = _dgrad(p)
    assert torch.equal(_bits(again), _bits(got)), f"{cid}: dX differs between two calls"
    want = p["dw"].numpy().astype(np.float32)
    for split_k in (1, 3, "auto"):
        got, st = _wgrad(p, split_k)
        assert st["launches"] == 1 and st["recomputed"] == 0, (split_k, st)
        xs.assert_same(got.numpy(), want, f"{cid} dW, split_k = {split_k}")
        again, _ = _wgrad(p, split_k)
        assert torch.equal(_bits(again), _bits(got)), f"{cid}: dW differs between two calls at split_k = {split_k}"


# ------------------------------------------------------------------------------------------ 2. lost elements
def _assert_planted(got, clean, ref, ref_clean, bound, what):
    """Outputs whose float64 reference the plant leaves alone: the clean run's bits; the others: the project's bar
    |got - ref| <= 1e-5 sum |a b|, NaN equal to NaN and inf to inf of the same sign."""
    got, clean, ref, ref_clean, bound = (np.asarray(t) for t in (got, clean, ref, ref_clean, bound))
    same = (ref == ref_clean)
    assert (~same).any(), f"{what}: the plant reaches no output"
    assert (got.view(np.uint32)[same] == clean.view(np.uint32)[same]).all(), f"{what}: an untouched output changed"
    fin = np.isfinite(ref)
    assert ((got == ref) | (np.isnan(got) & np.isnan(ref)))[~fin].all(), f"{what}: a non-finite output differs"
    with np.errstate(invalid="ignore"):
        assert (np.abs(got - ref)[fin] <= 1e-5 * bound[fin]).all(), f"{what}: outside 1e-5 sum |a b|"


@pytest.mark.parametrize("plant", ["dy=+inf", "x=1+2^-12", "w=1+2^-12"])
def test_lost_elements_recompute_their_tiles(plant):
    p = problem("3x3-s11-g1")
    ops = {k: p[k].clone() for k in ("x", "w", "dy")}
    name, value = plant.split("=")
    # (an interior pixel of plane (1, 5): no window of it meets the padding)
    ops[name][(1, 5, 6, 5) if name != "w" else (5, 3, 1, 1)] = float("inf") if name == "dy" else 1 + 2.0 ** -12
    dx, dw = (t.numpy() for t in _backward64(ops["x"], ops["w"], ops["dy"], p["geo"]))
    bx, bw = (t.numpy() for t in _backward64(ops["x"], ops["w"], ops["dy"], p["geo"], use_abs=True))
    if name != "x":
        got, st = _dgrad(p, dy=ops["dy"], w=ops["w"])
        assert st["launches"] == 1 and st["recomputed"] >= 1, st
        _assert_planted(got.numpy(), _dgrad(p)[0].numpy(), dx, p["dx"].numpy(), bx, f"dX, {plant}")
    if name != "w":
        for split_k in (1, 3):
            got, st = _wgrad(p, split_k, dy=ops["dy"], x=ops["x"])
            assert st["launches"] == 1 and st["recomputed"] >= 1, st
            _assert_planted(got.numpy(), _wgrad(p, split_k)[0].numpy(), dw, p["dw"].numpy(), bw,
                            f"dW, {plant}, split_k = {split_k}")


# ------------------------------------------------------------------------------------------ 3. operators
@pytest.mark.parametrize("stride", gx.CONV_STRIDES, ids=lambda s: f"s{s[0]}{s[1]}")
@pytest.mark.parametrize("groups", gx.CONV_GROUPS)
def test_ste_conv2d_implicit_backward_exact(groups, stride):
    from fp8_quantization_amd.approx_ops import ste_conv2d
    x, w, dy = gx.conv_problem(groups, stride)
    pad, dil = gx.CONV["padding"], gx.CONV["dilation"]
    xq, wq = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    _stats()
    y = ste_conv2d(xq, wq, lambda a, b: F.conv2d(a, b, None, stride, pad, dil, groups), stride, pad, dil, groups,
                   backward="implicit")
    y.backward(dy.to(DEV))
    st = _stats()
    assert st["launches"] == 2 and st["recomputed"] == 0, st
    dx, dw = gx.conv_backward64(x, w, dy, groups, stride)
    xs.assert_same(xq.grad.cpu().numpy(), dx.numpy().astype(np.float32), f"dX, G = {groups}, stride {stride}")
    xs.assert_same(wq.grad.cpu().numpy(), dw.numpy().astype(np.float32), f"dW, G = {groups}, stride {stride}")
    with pytest.raises(ValueError, match="backward"):
        ste_conv2d(xq, wq, F.conv2d, backward="direct")


def test_the_layer_key_reaches_the_implicit_backward():
    x = torch.randn((2, 4, 6, 6), generator=torch.Generator().manual_seed(3)).to(DEV)
    dx0, dw0, st0, ops = _layer_grads(_make_conv, x)
    dx1, dw1, st1, _ = _layer_grads(_make_conv, x, conv_backward="im2col")
    assert st1 == st0 and torch.equal(_bits(dx1), _bits(dx0)) and torch.equal(_bits(dw1), _bits(dw0))
    dx2, dw2, st2, ops2 = _layer_grads(_make_conv, x, conv_backward="implicit")
    # one class, one row tile and one column tile per image; dW [40 x 72] @ [72 x 36]: one tile
    assert st2 == dict(launches=2, tiles=2 + 1, recomputed=0), st2
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(ops2, ops))
    _assert_bar(lambda a, b: F.conv2d(a, b, None, 1, 1), ops, dx2, dw2, "conv, conv_backward = implicit")
    with pytest.raises(ValueError, match="conv_backward"):
        _layer_grads(_make_conv, x, conv_backward="direct")


# ------------------------------------------------------------------------------------------ 4. the transient
@pytest.mark.parametrize("path", ["implicit", "im2col"])
def test_backward_transient_memory(path):
    """Sizes, not timings: the implicit path allocates dX, dW, at most a contiguous copy of dy and the planned
    workspace; the default path at least its im2col image, kh kw times the input."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import grad_split_auto, ste_conv2d
    g = torch.Generator().manual_seed(11)
    xq = torch.randn((8, 32, 28, 28), generator=g).to(DEV).requires_grad_()
    wq = torch.randn((32, 32, 3, 3), generator=g).to(DEV).requires_grad_()
    y = ste_conv2d(xq, wq, lambda a, b: F.conv2d(a, b, None, 1, 1), (1, 1), (1, 1), (1, 1), 1, split_k="auto",
                   backward=path)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    nbytes = lambda t: t.numel() * t.element_size()  # noqa: E731
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    torch.autograd.grad(y, (xq, wq), dy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"{path}: peak above the pre-backward level {peak} bytes")
    if path == "implicit":
        geo = (8, 32, 28, 28, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1)
        _, ws = _lib.grad_conv_wgrad_plan(geo, grad_split_auto(1, 32, 32 * 9, 8 * 28 * 28, xq.device))
        assert peak <= nbytes(xq) + nbytes(wq) + nbytes(dy) + ws, (peak, ws)
    else:
        assert peak >= 9 * nbytes(xq), peak
