"""Learned FP8 ranges on the GPU: the quantizer's training kernels (fp8a_fq_train_forward /
fp8a_fq_train_backward), the autograd Function on them, and the route up through a layer, a model and the
fine-tune driver.

Fixture (tests/golden/learn_maxval.npz, gen_golden_learn.py): forward bytes are fp8_fake_quantize's; grad_maxval
is the reference autograd's bit for bit; grad_x is the reference's bit for bit up to the sign of a zero -- the
backward multiplies (a negative g outside the clamp gives -0.0, as the quantizer's backward always did and as
the kernel's contract says) where ATen's max / min backward writes +0.0 (learn_ranges_ref.bits clears it).

Kernel shapes: expected values from the numpy closed form (learn_ranges_ref.py).  An exact-sum g (integers in
[-127, 127] times 2^-9, sum |g wm| <= 2^22 2^-10 per row: every summation order gives the same bits) is
compared bit for bit; a random normal g within 2^-23 sum |g wm| of the float64 sum of the fp32 terms -- the
bound of the double accumulation and the one fp32 rounding, (2^-24 + n 2^-53) sum |g wm| for n < 2^28.

Layer / model: the input and the weight range of every approx layer (and a block's output range) receive a
gradient, checked against the closed form on the (x, g) pair that hooks capture at the quantizer.  A layer's
result quantizer gets none: in the fixed-range approx forward it never runs (hijacker.py:88-102, here as in the
reference) -- it only lends the product its bias -- so its maxval is a Parameter without a gradient.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from . import learn_ranges_ref as lr
from .test_gpu_ste import _calibrate, _qp, _rand, _resnet_block, _unfused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 4096  # the kernels' tile (csrc/fq_train.h FQT_TILE)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learn_maxval.npz")


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _i32(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _pair(x, maxval, g, mbits, sign_bits, per_row):
    """(y, bias, code, grad_x, grad_maxval) of the training pair on device copies of numpy inputs."""
    from fp8_quantization_amd import approx_ops
    xd, md, gd = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (x, maxval, g))
    y, bias, code = approx_ops.fp8_fake_quantize_train(xd, md, 8, mbits, sign_bits, per_row)
    rows = md.numel() if per_row else 1
    gx, gm = approx_ops.fp8_fake_quantize_backward(gd, code, rows, sign_bits)
    return xd, md, gd, y, bias, code, gx, gm


def _assert_forward_is_fake_quantize(xd, md, mbits, sign_bits, per_row, y, bias):
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    want, wb = fp8_fake_quantize(xd, md, 8, mbits, sign_bits, per_row)
    assert np.array_equal(_i32(y), _i32(want))
    assert bias.shape == wb.shape and np.array_equal(_i32(bias), _i32(wb))
    assert torch.equal(bias._fp8a_i32, wb._fp8a_i32)


def _assert_sum(gm, gm64, budget, exact, what):
    got = gm.detach().cpu().numpy()
    if exact:
        assert (budget <= lr.BUDGET).all()
        assert np.array_equal(got.view(np.int32), gm64.astype(np.float32).view(np.int32)), what
    else:
        err = np.abs(got.astype(np.float64) - gm64)
        worst = float((err / np.maximum(budget, 1e-300)).max())
        print(f"{what}: max |grad_maxval - exact| / sum|g wm| = {worst:.3e} (bound {lr.BOUND:.3e})")
        assert (err <= lr.BOUND * budget).all(), what


# ------------------------------------------------------------------------------------------ fixture
def _golden():
    z = np.load(GOLDEN)
    return z, sorted({k.split("/")[0] for k in z.files})


def test_fixture_forward_bytes_and_reference_gradients_bit_for_bit():
    z, names = _golden()
    assert len(names) == 12
    for n in names:
        _, mbits, sign_bits, per_channel = (int(v) for v in z[n + "/meta"])
        out = [_pair(z[n + "/x"], z[n + "/maxval"], z[n + "/g"], mbits, sign_bits, bool(per_channel)) for _ in range(2)]
        xd, md, gd, y, bias, code, gx, gm = out[0]
        _assert_forward_is_fake_quantize(xd, md, mbits, sign_bits, bool(per_channel), y, bias)
        assert code.dtype == torch.uint8 and code.shape == xd.shape
        assert np.array_equal(lr.bits(gx.cpu().numpy()), lr.bits(z[n + "/grad_x"])), n
        assert gm.shape == z[n + "/grad_maxval"].shape
        assert np.array_equal(_i32(gm), z[n + "/grad_maxval"].view(np.int32)), n
        for a, b in zip(out[0][3:], out[1][3:]):  # two calls: identical bytes
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), n


def test_fixture_through_the_quantizer_with_a_learned_maxval():
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    z, names = _golden()
    for n in names:
        n_bits, mbits, sign_bits, per_channel = (int(v) for v in z[n + "/meta"])
        q = FPQuantizer(n_bits=n_bits, per_channel=bool(per_channel), mantissa_bits=mbits, set_maxval=True,
                        learn_maxval=True)
        q.maxval = torch.from_numpy(z[n + "/maxval"]).to(DEV)
        q.sign_bits = sign_bits
        q.ste_backward = True
        q.make_range_trainable()
        x = torch.from_numpy(z[n + "/x"]).to(DEV).requires_grad_()
        q(x).backward(torch.from_numpy(z[n + "/g"]).to(DEV))
        assert np.array_equal(lr.bits(x.grad.cpu().numpy()), lr.bits(z[n + "/grad_x"])), n
        assert q.maxval.grad.shape == q.maxval.shape
        assert np.array_equal(_i32(q.maxval.grad), z[n + "/grad_maxval"].view(np.int32)), n


# ------------------------------------------------------------------------------------------ kernel shapes
def _inputs(rows, inner, sign_bits, seed, per_row, maxval=None, amp=127):
    """x with about a fifth outside the clamp and ties on both bounds, maxval per row (drawn unless given), and
    the two gradients: exact-sum and normal."""
    rng = np.random.default_rng(seed)
    if maxval is None:
        maxval = np.float32(0.5) + rng.integers(1, 12, size=rows if per_row else 1).astype(np.float32) * np.float32(0.25)
    mx = maxval.reshape(-1, 1) if per_row else maxval[0]
    x = (rng.standard_normal((rows, inner)).astype(np.float32) * mx / np.float32(1.28)).astype(np.float32)
    if sign_bits == 0:
        x[rng.random((rows, inner)) < 0.05] = 0.0
    tie = rng.random((rows, inner)) < 0.05
    side = np.where(rng.random((rows, inner)) < 0.5, np.float32(-1.0), np.float32(1.0))
    x = np.where(tie, side * mx, x).astype(np.float32)
    return x, maxval, lr.exact_sum_g(rng, (rows, inner), amp), rng.standard_normal((rows, inner)).astype(np.float32)


def _shape_case(rows, inner, per_row, sign_bits=1, mbits=3, seed=0, amp=127):
    x, maxval, g_exact, g_rand = _inputs(rows, inner, sign_bits, seed, per_row, amp=amp)
    for g, exact in ((g_exact, True), (g_rand, False)):
        want_gx, gm64, budget = lr.closed_form(x, maxval, g, sign_bits, per_row)
        xd, md, gd, y, bias, code, gx, gm = _pair(x, maxval, g, mbits, sign_bits, per_row)
        _assert_forward_is_fake_quantize(xd, md, mbits, sign_bits, per_row, y, bias)
        assert np.array_equal(_i32(gx), want_gx.view(np.int32))  # (the closed form multiplies too: zero signs included)
        assert gm.shape == (rows if per_row else 1,)
        _assert_sum(gm, gm64, budget, exact, f"{rows} x {inner} {'exact-sum' if exact else 'normal'} g")
        again = _pair(x, maxval, g, mbits, sign_bits, per_row)
        assert torch.equal(gm.view(torch.int32), again[7].view(torch.int32)) and torch.equal(code, again[5])


@pytest.mark.parametrize("inner", [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 37])
def test_per_tensor_shapes(inner):
    _shape_case(1, inner, False, sign_bits=1, seed=inner)
    _shape_case(1, inner, False, sign_bits=0, mbits=2, seed=inner + 1)


@pytest.mark.parametrize("inner", [1, 9, 27, 65, T + 1])
@pytest.mark.parametrize("rows", [1, 5, 64, 961])
def test_per_channel_shapes(rows, inner):
    _shape_case(rows, inner, True, sign_bits=1, seed=rows * 10007 + inner)


@pytest.mark.parametrize("rows,inner,per_row", [(1, 16 * T, False), (1, 16 * T + 1, False), (3, 70 * T + 1, True)])
def test_rows_split_over_many_workgroups(rows, inner, per_row):
    """16 parts per row: the last split that one thread per row sums; 17 and 71: a wave per row (71: some lanes
    sum two parts)."""
    from fp8_quantization_amd import _lib
    assert _lib.load().fp8a_fq_train_workspace_size(rows, inner) == rows * ((inner + T - 1) // T) * 8
    _shape_case(rows, inner, per_row, seed=inner, amp=7)


def test_a_workgroup_walks_several_tiles_with_a_ragged_last_one():
    from fp8_quantization_amd import _lib
    L = _lib.load()
    old = _lib.set_option("fqt_target_wgs", 1)
    try:
        assert L.fp8a_fq_train_workspace_size(1, 3 * T + 37) == 8       # one workgroup: four tiles
        _shape_case(1, 3 * T + 37, False, seed=11)
        assert L.fp8a_fq_train_workspace_size(3, 4 * T + 36) == 3 * 8   # one per row: five tiles each
        _shape_case(3, 4 * T + 36, True, seed=12)                       # (inner % 4 == 0: the 16-byte form)
        _lib.set_option("fqt_target_wgs", 6)
        assert L.fp8a_fq_train_workspace_size(3, 4 * T + 37) == 3 * 2 * 8  # two per row: tiles [0, 2), [2, 5)
        _shape_case(3, 4 * T + 37, True, seed=13)
    finally:
        _lib.set_option("fqt_target_wgs", old)


@pytest.mark.parametrize("offset", [3, 4], ids=["unaligned", "aligned"])
def test_views_into_nan_buffers_and_untouched_frames(offset):
    """The C ABI on interior pointers: x and g sit inside NaN-filled buffers, every output inside a sentinel
    buffer whose frame stays untouched.  offset 3: no pointer is 16-byte aligned (the single-value form);
    offset 4: all are (the 16-byte form on the full tile, single values on the ragged one)."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    rows, inner, pad = 3, T + 8, 64
    n = rows * inner
    x, maxval, g, _ = _inputs(rows, inner, 1, 21, True)
    want_gx, gm64, budget = lr.closed_form(x, maxval, g, 1, True)

    def framed(dtype, fill, payload=None, count=n):
        buf = torch.full((count + 2 * pad,), fill, dtype=dtype, device=DEV)
        if payload is not None:
            buf[offset:offset + count] = torch.from_numpy(payload.reshape(-1)).to(DEV)
        return buf

    def ptr(buf):
        return ctypes.c_void_p(buf.data_ptr() + offset * buf.element_size())

    xb, gb = framed(torch.float32, float("nan"), x), framed(torch.float32, float("nan"), g)
    yb, gxb = framed(torch.float32, 12345.0), framed(torch.float32, 12345.0)
    cb = framed(torch.uint8, 0xAB)
    bb, ib = framed(torch.float32, 12345.0, count=rows), framed(torch.int32, 777, count=rows)
    gmb = framed(torch.float32, 12345.0, count=rows)
    md = torch.from_numpy(maxval).to(DEV)
    ws = torch.empty(int(L.fp8a_fq_train_workspace_size(rows, inner)), dtype=torch.uint8, device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))
    _lib.check(L.fp8a_fq_train_forward(ptr(xb), rows, inner, _lib.dev_ptr(md), 8, 3, 1, ptr(yb), ptr(cb), ptr(bb),
                                       ptr(ib), s), "fp8a_fq_train_forward")
    _lib.check(L.fp8a_fq_train_backward(ptr(gb), ptr(cb), rows, inner, 1, ptr(gxb), ptr(gmb), _lib.dev_ptr(ws),
                                        ws.numel(), s), "fp8a_fq_train_backward")
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    want, wb = fp8_fake_quantize(torch.from_numpy(x).to(DEV), md, 8, 3, 1, True)
    assert np.array_equal(_i32(yb[offset:offset + n]), _i32(want.reshape(-1)))
    assert np.array_equal(_i32(bb[offset:offset + rows]), _i32(wb.reshape(-1)))
    assert torch.equal(ib[offset:offset + rows], wb._fp8a_i32)
    assert np.array_equal(_i32(gxb[offset:offset + n]), want_gx.reshape(-1).view(np.int32))
    _assert_sum(gmb[offset:offset + rows], gm64, budget, True, "framed")
    for buf, fill, count in ((yb, 12345.0, n), (gxb, 12345.0, n), (cb, 0xAB, n), (bb, 12345.0, rows), (ib, 777, rows),
                             (gmb, 12345.0, rows)):
        assert bool((buf[:offset] == fill).all()) and bool((buf[offset + count:] == fill).all())
    assert bool(torch.isnan(xb[:offset]).all()) and bool(torch.isnan(gb[offset + n:]).all())


@pytest.mark.parametrize("shape,per_row", [((1, 3 * T + 5), False), ((7, 9), True), ((4, T + 3), True)])
def test_all_inside_gives_plus_zero_and_all_above_gives_the_sum_of_g(shape, per_row):
    rows = shape[0] if per_row else 1
    rng = np.random.default_rng(5)
    maxval = np.full(rows, 2.0, np.float32)
    g = lr.exact_sum_g(rng, shape)
    inside = rng.uniform(-1.9, 1.9, size=shape).astype(np.float32)
    *_, gx, gm = _pair(inside, maxval, g, 3, 1, per_row)
    assert np.array_equal(_i32(gm), np.zeros(rows, np.int32))  # +0.0, not -0.0
    assert np.array_equal(_i32(gx), g.view(np.int32))
    above = rng.uniform(2.5, 9.0, size=shape).astype(np.float32)
    *_, gx, gm = _pair(above, maxval, g, 3, 1, per_row)
    want = g.astype(np.float64).reshape(rows, -1).sum(axis=1).astype(np.float32)
    assert np.array_equal(_i32(gm), want.view(np.int32))
    assert np.array_equal(_i32(gx), (g * np.float32(0.0)).view(np.int32))
    *_, gx, gm = _pair(-above, maxval, g, 3, 1, per_row)  # all below a signed quantizer's lower bound
    assert np.array_equal(_i32(gm), (-want + np.float32(0.0)).view(np.int32))  # (a zero sum is +0.0)
    *_, gx, gm = _pair(-above, maxval, g, 3, 0, per_row)  # unsigned: the constant 0 takes the gradient
    assert np.array_equal(_i32(gm), np.zeros(rows, np.int32))


def test_zero_signs_infinities_and_nans():
    """grad_x and the terms of grad_maxval are multiplications: -3 * 0 = -0.0 and inf * 0 = NaN."""
    mx = np.array([2.0], np.float32)
    x = np.array([[3.0, 3.0, -3.0, 1.0, np.nan, 3.0, 0.5]], np.float32)
    g = np.array([[-3.0, 3.0, -2.0, -1.0, 7.0, 0.0, 1.0]], np.float32)
    *_, gx, gm = _pair(x, mx, g, 3, 1, False)
    got = gx.cpu().numpy()[0]
    assert got.tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 1.0]  # a NaN in x: wx = wm = 0
    assert np.signbit(got).tolist() == [True, False, True, True, False, False, False]
    assert gm.tolist() == [-3.0 + 3.0 + 2.0]
    # an infinite g beyond the bound: grad_x = inf * 0, grad_maxval = inf * 1 + 1 * 0
    *_, gx, gm = _pair(np.array([[5.0, 1.0]], np.float32), mx, np.array([[np.inf, 1.0]], np.float32), 3, 1, False)
    assert np.isnan(gx.cpu().numpy()[0, 0]) and gm.tolist() == [np.inf]
    # ... and inside the clamp: grad_x = inf, its term of grad_maxval inf * 0
    *_, gx, gm = _pair(np.array([[1.0, 5.0]], np.float32), mx, np.array([[np.inf, 1.0]], np.float32), 3, 1, False)
    assert gx.tolist() == [[np.inf, 0.0]] and bool(torch.isnan(gm).all())


def test_empty_rows_are_a_successful_no_op_with_a_zero_gradient():
    from fp8_quantization_amd import approx_ops
    x = torch.empty((4, 0), device=DEV)
    y, bias, code = approx_ops.fp8_fake_quantize_train(x, torch.full((4,), 2.0, device=DEV), 8, 3, 1, True)
    assert y.shape == (4, 0) and code.shape == (4, 0)
    gx, gm = approx_ops.fp8_fake_quantize_backward(x, code, 4, 1)
    assert gx.shape == (4, 0) and np.array_equal(_i32(gm), np.zeros(4, np.int32))


def test_one_row_past_two_to_the_31_elements():
    """64-bit element offsets: one per-tensor row of 2^31 + 4 T + 5 values; the head, a slice across 2^31 and the
    ragged tail against the closed form, grad_maxval the exact sum of the (few) non-zero terms."""
    from fp8_quantization_amd import approx_ops
    n, k = 2 ** 31 + 4 * T + 5, 3000
    rng = np.random.default_rng(31)
    spans = [(0, k), (2 ** 31 - k, 2 ** 31 + k), (n - k, n)]
    mx = np.array([2.0], np.float32)
    x = torch.full((n,), 0.5, device=DEV)
    g = torch.zeros((n,), device=DEV)
    parts = []
    for a, b in spans:
        xs, _, gs, _ = _inputs(1, b - a, 1, a % 1000, False, maxval=mx)
        x[a:b] = torch.from_numpy(xs[0]).to(DEV)
        g[a:b] = torch.from_numpy(gs[0]).to(DEV)
        parts.append((xs, gs))
    y, bias, code = approx_ops.fp8_fake_quantize_train(x, torch.from_numpy(mx).to(DEV), 8, 3, 1, False)
    assert float(y[2 ** 30]) == 0.5 and float(y[2 ** 31 + 2 * k]) == 0.5 and int(code[2 ** 31 + 2 * k]) == 2
    for (a, b), (xs, _) in zip(spans, parts):
        want, _ = approx_ops.fp8_fake_quantize(torch.from_numpy(xs).to(DEV), torch.from_numpy(mx).to(DEV), 8, 3, 1)
        assert np.array_equal(_i32(y[a:b]), _i32(want.reshape(-1))), (a, b)
    del x, y
    gx, gm = approx_ops.fp8_fake_quantize_backward(g, code, 1, 1)
    total, budget = 0.0, 0.0
    for (a, b), (xs, gs) in zip(spans, parts):
        want_gx, gm64, bud = lr.closed_form(xs, mx, gs, 1, False)
        assert np.array_equal(_i32(gx[a:b]), want_gx.reshape(-1).view(np.int32)), (a, b)
        total, budget = total + float(gm64[0]), budget + float(bud[0])
    assert budget <= lr.BUDGET and budget > 0
    assert np.array_equal(_i32(gm), np.array([total], np.float32).view(np.int32))
    assert float(gx[2 ** 31 + 2 * k]) == 0.0


# ------------------------------------------------------------------------------------------ quantizer
def _learned_quantizer(maxval=2.0, **kw):
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    q = FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True, learn_maxval=True, **kw)
    q.maxval = torch.tensor([maxval])  # on the host: the first forward moves it
    q.ste_backward = True
    q.make_range_trainable()
    return q


def test_tie_vector_with_a_learnable_maxval():
    q = _learned_quantizer()
    p = q.maxval
    x = torch.tensor([2.0, -2.0, 1.5, 3.0, -7.0, 0.0], device=DEV, requires_grad=True)
    q(x).sum().backward()
    assert q.maxval is p and p.device.type == "cuda" and isinstance(p, torch.nn.Parameter)  # moved in place
    assert x.grad.tolist() == [0.5, 0.5, 1.0, 0.0, 0.0, 1.0]
    assert p.grad.tolist() == [0.5 - 0.5 + 1.0 - 1.0] and p.grad.shape == p.shape
    p.grad = None
    q(torch.tensor([2.0, 1.5, 3.0, 0.0, -1.0], device=DEV, requires_grad=True)).sum().backward()  # one-sided
    assert p.grad.tolist() == [1.5]
    q.sign_bits = 0  # unsigned: the lower bound is the constant 0
    p.grad = None
    q(torch.tensor([2.0, -2.0, 1.5, 3.0, -7.0, 0.0], device=DEV, requires_grad=True)).sum().backward()
    assert p.grad.tolist() == [1.5]


def test_first_layer_input_without_grad_still_trains_the_range():
    q = _learned_quantizer()
    x = torch.tensor([2.0, -2.5, 1.5, 3.0], device=DEV)
    y = q(x)
    assert y.requires_grad and not x.requires_grad
    y.backward(torch.tensor([1.0, 2.0, 4.0, 8.0], device=DEV))
    assert q.maxval.grad.tolist() == [0.5 - 2.0 + 8.0]


def test_learned_with_the_switch_off_raises_and_no_grad_bytes_are_the_fixed_quantizers():
    from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
    q = _learned_quantizer(maxval=1.75)
    x = _rand((3, 50), 3).to(DEV)
    q.ste_backward = False
    with pytest.raises(RuntimeError, match="ste_backward"):
        q(x)
    fixed = FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True)
    fixed.maxval = torch.tensor([1.75], device=DEV)
    want = fixed(x)
    for switch in (False, True):
        q.ste_backward = switch
        with torch.no_grad():
            got = q(x)
        assert not got.requires_grad and np.array_equal(_i32(got), _i32(want))
        assert np.array_equal(_i32(q.custom_bias), _i32(fixed.custom_bias))
    q.ste_backward = True
    assert np.array_equal(_i32(q(x)), _i32(want))  # the recorded forward: the same bytes
    q.fix_ranges()
    assert not isinstance(q.maxval, torch.nn.Parameter) and q.maxval.tolist() == [1.75] and not q(x).requires_grad


# ------------------------------------------------------------------------------------------ layer, model
class _Capture:
    """Forward hooks on every FPQuantizer of a module: the input of its last recorded forward and the gradient
    that arrives at its output."""

    def __init__(self, module):
        from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
        self.seen, self.handles = {}, []
        for name, q in module.named_modules():
            if isinstance(q, FPQuantizer):
                self.handles.append(q.register_forward_hook(self._hook(name, q)))

    def _hook(self, name, q):
        def fn(mod, inp, out):
            if out.requires_grad:
                rec = self.seen[name] = dict(q=q, x=inp[0].detach().clone(), g=None)
                out.register_hook(lambda g: rec.__setitem__("g", g.detach().clone()))
        return fn

    def close(self):
        for h in self.handles:
            h.remove()


def _assert_range_gradients(cap, expect):
    """Every captured quantizer's maxval gradient against the closed form on its (x, g); returns name -> grad."""
    assert sorted(cap.seen) == sorted(expect), sorted(cap.seen)
    out = {}
    for name, rec in cap.seen.items():
        q, p = rec["q"], rec["q"].maxval
        assert rec["g"] is not None and p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert p.grad.shape == p.shape
        per_row = p.numel() != 1
        x = rec["x"].cpu().numpy()
        x = x.reshape(p.numel(), -1) if per_row else x.reshape(1, -1)
        g = rec["g"].cpu().numpy().reshape(x.shape)
        _, gm64, budget = lr.closed_form(x, p.detach().cpu().numpy().reshape(-1), g, q.sign_bits, per_row)
        _assert_sum(p.grad.reshape(-1), gm64, budget, False, name)
        out[name] = p.grad.detach().clone()
    return out


def _layers():
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch, QCustomLinearTorch
    qp = _qp(learn_maxval=True)
    conv = QCustomBNConv2dTorch(in_channels=4, out_channels=6, kernel_size=3, stride=2, padding=1, bias=False,
                                activation=None, **qp)
    torch.nn.init.normal_(conv.weight, generator=torch.Generator().manual_seed(3))
    lin = QCustomLinearTorch(in_features=19, out_features=7, bias=True, **_qp(learn_maxval=True))
    torch.nn.init.normal_(lin.weight, generator=torch.Generator().manual_seed(1))
    return {"conv": (conv, _rand((2, 4, 7, 7), 4).to(DEV)), "linear": (lin, _rand((5, 19), 2).to(DEV))}


@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_layer_ranges_receive_gradients_and_a_moved_range_is_honoured(kind, monkeypatch):
    from fp8_quantization_amd.quantization.quantization_manager import Qstates
    m, x = _layers()[kind]
    m = _calibrate(m.to(DEV).eval(), x)
    x = x * 1.5  # (beyond the calibrated input range: the upper and lower bounds clamp)
    m.learn_ranges()
    mgrs = (m.activation_quantizer, m.weight_quantizer, m.res_quantizer)
    assert all(g.state == Qstates.learn_ranges and isinstance(g.quantizer.maxval, torch.nn.Parameter) for g in mgrs)
    cap = _Capture(m)
    y = m(x)
    assert y.requires_grad
    y.backward(_rand(y.shape, 7).to(DEV))
    cap.close()
    grads = _assert_range_gradients(cap, ["activation_quantizer.quantizer", "weight_quantizer.quantizer"])
    assert all(float(g.abs().max()) > 0 for g in grads.values())
    assert m.weight_quantizer.quantizer.maxval.numel() == y.shape[1]  # (per output channel)
    assert m.res_quantizer.quantizer.maxval.grad is None  # never runs in the fixed-range approx forward (module doc)

    # a range that moved is honoured by the product: the bytes of a fresh layer with that maxval fixed
    q = m.activation_quantizer.quantizer
    before = q.custom_bias.clone()
    with torch.no_grad():
        q.maxval.mul_(2.0)
    got = m(x)
    assert not torch.equal(q.custom_bias, before)
    fresh, x0 = _layers()[kind]
    with torch.no_grad():  # (a linear's bias is drawn from the global generator)
        for name, p in fresh.named_parameters():
            p.copy_(m.get_parameter(name))
    fresh = _calibrate(fresh.to(DEV).eval(), x0)
    fresh.activation_quantizer.quantizer.maxval = q.maxval.detach().clone()
    with torch.no_grad():
        want = fresh(x)
    assert np.array_equal(_i32(got), _i32(want))

    # fixed again: plain tensors, and the fused eval forward's bytes are the unfused one's
    m.fix_ranges()
    assert all(g.state == Qstates.fix_ranges and not isinstance(g.quantizer.maxval, torch.nn.Parameter) for g in mgrs)
    with torch.no_grad():
        fused = m(x)
        with monkeypatch.context() as mp:
            _unfused(mp)
            unfused = m(x)
    assert np.array_equal(_i32(fused), _i32(unfused)) and np.array_equal(_i32(fused), _i32(want))


def test_resnet_block_range_gradients_and_two_sgd_steps():
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.distributed import quantizers
    xcal = _rand((2, 4, 7, 7), 13).to(DEV)
    m = _calibrate(_resnet_block(_qp(learn_maxval=True)), xcal)
    x = xcal * 1.5
    m.learn_ranges()
    qs = quantizers(m)
    assert len(qs) == 10 and all(isinstance(q.maxval, torch.nn.Parameter) for q in qs)  # 3 convs x 3, the block's own
    cal = [q.maxval.detach().clone() for q in qs]
    cap = _Capture(m)
    _lib.grad_stats(reset=True)
    dy = _rand((2, 6, 4, 4), 11).to(DEV)
    m(x).backward(dy)
    cap.close()
    ran = [n for n, q in m.named_modules() if q in qs and not n.endswith("res_quantizer.quantizer")]
    assert len(ran) == 7
    _assert_range_gradients(cap, ran)
    moved = [q.maxval.grad is not None and bool((q.maxval.grad != 0).any()) for q in qs]
    assert sum(moved) >= 5, moved
    first = [None if q.maxval.grad is None else q.maxval.grad.clone() for q in qs]
    opt = torch.optim.SGD([q.maxval for q in qs], lr=1e-3)
    opt.step()
    opt.zero_grad(set_to_none=True)
    m(x).backward(dy)  # operands re-quantized on the moved grids
    opt.step()
    assert _lib.grad_stats(reset=True)["recomputed"] == 0
    for q, c, g0 in zip(qs, cal, first):
        now = q.maxval.detach()
        assert bool(torch.isfinite(now).all()) and bool((now > 0).all())
        if g0 is None:
            assert torch.equal(now, c)
        else:
            assert bool((now != c)[g0 != 0].all()) and isinstance(q.maxval, torch.nn.Parameter)


def test_finetune_driver_learns_ranges_and_ends_fixed(tmp_path, monkeypatch):
    from fp8_quantization_amd import finetune
    from fp8_quantization_amd.distributed import quantizers
    from fp8_quantization_amd.quantization.quantization_manager import QuantizationManager, Qstates
    built = []
    build = finetune.build_model
    monkeypatch.setattr(finetune, "build_model", lambda *a, **k: built.append(build(*a, **k)) or built[-1])
    out = tmp_path / "records.json"
    rc = finetune.main(["--synthetic", "8", "--arch", "resnet18", "--image-size", "64", "--batch-size", "4",
                        "--steps", "2", "--learn-ranges", "--output", str(out)])
    assert rc == 0
    recs = json.loads(out.read_text())
    assert len(recs) == 2
    qs = quantizers(built[0])
    for r in recs:
        assert r["learned_ranges"] == len(qs) > 60 and r["bad_ranges"] == 0 and r["recomputed_tiles"] == 0
        assert r["quantizer_ms"] > 0 and np.isfinite(r["max_range_change"]) and r["max_range_change"] >= 0
        assert np.isfinite(r["loss"])
    assert recs[-1]["max_range_change"] > 0
    assert not any(isinstance(q.maxval, torch.nn.Parameter) or q.maxval.requires_grad for q in qs)
    assert all(g.state == Qstates.fix_ranges for g in built[0].modules() if isinstance(g, QuantizationManager))
