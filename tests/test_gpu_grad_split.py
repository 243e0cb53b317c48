"""The gradient GEMM's split along K (fp8a_grad_bmm_split: gemm_grad_split_kernel + grad_reduce_kernel,
csrc/gemm_grad.h) on the device.  Plan, model, cases and mutants: tests/grad_split.py; the
conditions on the inputs and what each mutant changes: tests/test_grad_split_cpu.py.

Comparisons 1 - 7 have no tolerance: exact_sums.assert_same (equal bits, zeros by value) against float64 numpy /
torch on the CPU, or equal bytes between two device results.  Every launch runs between two
_lib.grad_stats(reset=True).

  1. both families on 2 x 2, 3 x 1 and 1 x 3 tile grids, K of five and three stages (one ragged, one across k0
     rows), split_k 2 .. 5, A and C with unit stride on either index: bits; 1 launch, tiles S, 0 recomputed;
  2. operands inside NaN-filled buffers with a k0 step that does not collapse, C and the workspace each the
     interior of a sentinel buffer (the raw entry point): bits, both frames untouched, no NaN in a sum;
  3. the plan's edges: more splits than stages, split_k = 1 through the new entry, K = 0;
  4. the slice identity on operands where the order of the adds matters: the split result is P_0 + P_1 + ... of
     the unsplit kernel's results on the parts' K-slices, added in fp32 in index order; two calls, equal bytes;
  5. a lost element recomputes the (tile, part) blocks that stage it, and only those change;
  6. ste_conv2d / ste_linear / ste_bmm with split_k = 3 and "auto" against float64 autograd;
  7. the operators' grad_split_k key;
  8. grad_split_auto's rule;
  9. general operands against the float64 product under the project's bar 1e-5 sum |a b|.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_sums as xs
from tests import grad_exact as gx
from tests import grad_split as gs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT_BITS = gx.SENTINEL.view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _stats():
    from fp8_quantization_amd import _lib
    return _lib.grad_stats(reset=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _lay_a(A, layout):
    """A [nb, M, K0, K1] on the device with unit stride on k1 or on m."""
    if layout == "k1":
        return _dev(A)
    return _dev(A.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)


def _lay_b(B, layout):
    """B [nb, K0, K1, N] with unit stride on k1 (with A's "k1") or on n."""
    if layout == "m":
        return _dev(B)
    return _dev(B.transpose(0, 3, 1, 2)).permute(0, 2, 3, 1)


def _out(nb, M, N, layout):
    if layout == "n":
        return torch.full((nb, M, N), float(gx.SENTINEL), device=DEV)
    return torch.full((nb, N, M), float(gx.SENTINEL), device=DEV).transpose(1, 2)


def _launch(a, b, out, split_k):
    """One grad_bmm launch on device views a [nb, M, K0, K1], b [nb, K0, K1, N] (single-level when K0 = 1)."""
    from fp8_quantization_amd.approx_ops import grad_bmm
    _stats()
    if a.shape[2] == 1:
        res = grad_bmm(a[:, :, 0], b[:, 0], out=out, split_k=split_k)
    else:
        res = grad_bmm(a, b, out=out, k2=True, split_k=split_k)
    assert out is None or res is out
    return res, _stats()


def _expect_stats(st, nb, M, N, K, split_k, recomputed=0):
    S = gs.plan(K, split_k)[1]
    assert st == dict(launches=1, tiles=gx.num_tiles(nb, M, N) * S, recomputed=recomputed), (st, S)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ 1. exact sums
@pytest.mark.parametrize("a_layout,c_layout", [("k1", "n"), ("m", "m"), ("k1", "m"), ("m", "n")])
@pytest.mark.parametrize("cid", list(gs.CASES))
def test_exact_sums_for_every_split(cid, a_layout, c_layout):
    p = gs.problem(cid)
    nb, M, K0, K1 = p["A"].shape
    N = p["B"].shape[-1]
    a, b = _lay_a(p["A"], a_layout), _lay_b(p["B"], a_layout)
    assert (a.stride(3) if a_layout == "k1" else a.stride(1)) == 1
    for split_k in gs.SPLITS:
        out = _out(nb, M, N, c_layout)
        assert (out.stride(2) if c_layout == "n" else out.stride(1)) == 1
        _, st = _launch(a, b, out, split_k)
        _expect_stats(st, nb, M, N, K0 * K1, split_k)
        xs.assert_same(out.cpu().numpy(), p["want"], f"{cid} split_k {split_k}, A unit {a_layout}, C unit {c_layout}",
                       p["T"])


# ------------------------------------------------------------------------------------------ 2. padded views
def _raw_split(a, b, c, split_k, ws_ptr, ws_bytes):
    """fp8a_grad_bmm_split on device views a [nb, M, K0, K1], b [nb, K0, K1, N], c [nb, M, N]."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    nb, M, K0, K1 = a.shape
    rc = L.fp8a_grad_bmm_split(_lib.dev_ptr(a), _lib.dev_ptr(b), _lib.dev_ptr(c), nb, M, b.shape[-1], K0, K1,
                               *a.stride(), *b.stride(), *c.stride(), split_k, ws_ptr, ws_bytes,
                               _lib.stream_ptr(a.device))
    _lib.check(rc, "fp8a_grad_bmm_split")


WS_FRAME = 64   # floats of sentinel before and after the workspace (256 bytes: the interior stays 16-byte aligned)


@pytest.mark.parametrize("split_k", [2, 5])
@pytest.mark.parametrize("layout", ["k1", "m"])
@pytest.mark.parametrize("k0,k1", gs.PAD_K)
def test_non_collapsing_views_with_poisoned_surroundings(k0, k1, layout, split_k):
    from fp8_quantization_amd import _lib
    p = gs.problem(f"W-{k0}x{k1}-70x67")
    nb, M = p["A"].shape[:2]
    N = p["B"].shape[-1]
    ba, bb = gx.padded(p["A"], p["B"], layout)
    a, b = gx.a_view(_dev(ba), layout, M, k1), gx.b_view(_dev(bb), layout, k1, N)
    assert a.stride(2) != k1 * a.stride(3) and b.stride(1) != k1 * b.stride(2)
    cb = _dev(gx.c_buffer(nb, M, N, layout))
    S, nbytes = _lib.grad_split_plan(nb, M, N, k0, k1, split_k)
    assert (S, nbytes) == (gs.plan(k0 * k1, split_k)[1], gs.workspace_bytes(nb, M, N, k0 * k1, split_k)) and S > 1
    wsb = torch.full((nbytes // 4 + 2 * WS_FRAME,), float(gx.SENTINEL), device=DEV)
    ws_ptr = ctypes.c_void_p(wsb.data_ptr() + 4 * WS_FRAME)
    assert ws_ptr.value % 16 == 0
    _stats()
    _raw_split(a, b, gx.c_view(cb, layout), split_k, ws_ptr, nbytes)
    _expect_stats(_stats(), nb, M, N, k0 * k1, split_k)
    host = cb.cpu().numpy()
    xs.assert_same(np.ascontiguousarray(gx.c_view(host, layout)), p["want"],
                   f"padded {k0} x {k1}, unit {layout}, split_k {split_k}", p["T"])
    gx.c_view(host, layout)[...] = gx.SENTINEL
    assert (host.view(np.uint32) == SENT_BITS).all(), "C's sentinel frame was written"
    ws = wsb.cpu().numpy()
    frame = np.concatenate([ws[:WS_FRAME], ws[-WS_FRAME:]])
    assert (frame.view(np.uint32) == SENT_BITS).all(), "the workspace's sentinel frame was written"
    inner = ws[WS_FRAME:-WS_FRAME]
    assert np.isfinite(inner).all(), "a NaN of the padding reached a partial sum"
    assert not (inner.view(np.uint32) == SENT_BITS).any(), "a workspace element was left unwritten"


# ------------------------------------------------------------------------------------------ 3. the plan's edges
@pytest.mark.parametrize("K,split_k,S", [(5, 4, 1), (33, 7, 2), (96, 64, 3)])
def test_more_splits_than_stages(K, split_k, S):
    from fp8_quantization_amd import _lib
    assert gs.plan(K, split_k)[1] == S == _lib.grad_split_plan(2, 70, 67, 1, K, split_k)[0]
    A, B = gx.family("G", 2, 70, 1, K, 67)
    T = gx.terms(A, B)
    assert xs.within_budget(T, axis=2)
    out = _out(2, 70, 67, "n")
    _, st = _launch(_dev(A), _dev(B), out, split_k)
    _expect_stats(st, 2, 70, 67, K, split_k)
    xs.assert_same(out.cpu().numpy(), xs.expected(T, axis=2), f"K = {K}, split_k {split_k}", T)


def test_one_split_through_the_new_entry_is_the_unsplit_launch():
    from fp8_quantization_amd.approx_ops import grad_bmm
    A, B = gs.slice_operands(2, 80)
    a, b = _dev(A), _dev(B)
    _stats()
    want = grad_bmm(a, b, k2=True)
    assert _stats() == dict(launches=1, tiles=gx.num_tiles(3, 70, 67), recomputed=0)
    got = torch.full_like(want, float("nan"))
    _raw_split(a, b, got, 1, None, 0)                                   # (S = 1: no workspace is asked for)
    assert _stats() == dict(launches=1, tiles=gx.num_tiles(3, 70, 67), recomputed=0)
    assert torch.equal(_bits(got), _bits(want))
    again = grad_bmm(a, b, k2=True, split_k=1)
    assert torch.equal(_bits(again), _bits(want))


def test_an_empty_reduction_gives_zeros():
    from fp8_quantization_amd.approx_ops import grad_bmm
    a, b = torch.randn((2, 5, 0), device=DEV), torch.randn((2, 0, 7), device=DEV)
    out = torch.full((2, 5, 7), 3.0, device=DEV)
    _stats()
    assert torch.equal(grad_bmm(a, b, out=out, split_k=3).cpu(), torch.zeros(2, 5, 7))
    assert _stats() == dict(launches=1, tiles=2, recomputed=0)
    assert grad_bmm(torch.randn((0, 5, 40), device=DEV), torch.randn((0, 40, 7), device=DEV), split_k=2).shape == (0, 5, 7)


# ------------------------------------------------------------------------------------------ 4. the slice identity
def _slice_identity(a, b, split_k):
    """P_0 + P_1 + ... on the device: the unsplit grad_bmm on each part's K-slice of the contiguous a [nb, M, K0, K1],
    b [nb, K0, K1, N], added in fp32 in index order.  Returns (sum, blocks the slices recomputed per part)."""
    from fp8_quantization_amd.approx_ops import grad_bmm
    nb, M, K0, K1 = a.shape
    af, bf = a.reshape(nb, M, K0 * K1), b.reshape(nb, K0 * K1, -1)
    acc, rec = None, []
    for (kb, ke) in gs.ranges(K0 * K1, split_k):
        _stats()
        P = grad_bmm(af[:, :, kb:ke], bf[:, kb:ke])
        rec.append(_stats()["recomputed"])
        acc = P if acc is None else acc + P
    return acc, rec


@pytest.mark.parametrize("K0,K1", [(1, 160), (2, 80)])
def test_split_equals_the_index_order_sum_of_the_slices(K0, K1):
    A, B = gs.slice_operands(K0, K1)
    a, b = _dev(A), _dev(B)
    unsplit, _ = _launch(a, b, None, 1)
    for split_k in (2, 3, 5):
        want, rec = _slice_identity(a, b, split_k)
        assert rec == [0] * len(rec)
        got, st = _launch(a, b, None, split_k)
        _expect_stats(st, 3, 70, 67, 160, split_k)
        assert torch.equal(_bits(got), _bits(want)), \
            f"split_k {split_k}: {int((_bits(got) != _bits(want)).sum())} outputs are not the index-order sum of the slices"
        again, _ = _launch(a, b, None, split_k)
        assert torch.equal(_bits(again), _bits(got)), "two split calls give different bytes"
        # (the data tells orders apart: the same parts added to one long fp32 chain round differently)
        assert int((_bits(got) != _bits(unsplit)).sum()) > 100


# ------------------------------------------------------------------------------------------ 5. lost elements
LOST_K = (5, 32)          # five stages; split_k = 2: part 0 = stages 0 .. 2 (k < 96), part 1 = stages 3, 4
LOST = [("A", "+inf", 100, 1), ("B", "1+2^-12", 5, 0)]   # (operand, what, its flat k, the part that stages it)


@pytest.mark.parametrize("M,N", gx.TWO_LEVEL)
@pytest.mark.parametrize("operand,what,k,part", LOST, ids=[f"{o}{w}" for o, w, _, _ in LOST])
def test_a_lost_element_recomputes_the_blocks_that_stage_it(operand, what, k, part, M, N):
    nb, (K0, K1), split_k = gx.NB, LOST_K, 2
    assert gs.ranges(K0 * K1, split_k)[part][0] <= k < gs.ranges(K0 * K1, split_k)[part][1]
    A, B = gx.sparse(np.float32(1 + 2.0 ** -20), 0.5, nb, M, K0, K1, N)
    clean, st = _launch(_dev(A), _dev(B), None, split_k)
    _expect_stats(st, nb, M, N, K0 * K1, split_k)
    xs.assert_same(clean.cpu().numpy(), gx.product64(A, B), "the clean sparse case")
    num_mt, num_nt = -(-M // 64), -(-N // 64)
    if operand == "A":                                   # the only nonzero of a row of the last row tile
        m = (num_mt - 1) * 64 + (M - (num_mt - 1) * 64) // 2
        A[1, m] = 0.0
        A[1, m, k // K1, k % K1] = np.float32(np.inf)
        tiles = [(1, m // 64, nt) for nt in range(num_nt)]
    else:                                                # a column of the last column tile
        n = (num_nt - 1) * 64 + (N - (num_nt - 1) * 64) // 2
        B[1, k // K1, k % K1, n] = gx.B_REJECTED[what]
        tiles = [(1, mt, n // 64) for mt in range(num_mt)]
    assert len(tiles) in (1, 3)
    a, b = _dev(A), _dev(B)
    got, st = _launch(a, b, None, split_k)
    _expect_stats(st, nb, M, N, K0 * K1, split_k, recomputed=len(tiles))   # the (tile, part) blocks, one part each
    want, rec = _slice_identity(a, b, split_k)
    assert rec[part] == len(tiles) and sum(rec) == len(tiles)
    got, want, clean = got.cpu().numpy(), want.cpu().numpy(), clean.cpu().numpy()
    keep = np.ones(got.shape, bool)
    for (i, mt, nt) in tiles:
        keep[i, 64 * mt:64 * mt + 64, 64 * nt:64 * nt + 64] = False
    assert np.array_equal(got.view(np.uint32)[keep], clean.view(np.uint32)[keep]), \
        "a tile that staged no lost element differs from the clean run"
    assert not np.array_equal(got.view(np.uint32), clean.view(np.uint32))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), "non-finite outputs differ from the slices' sum"
    assert np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]), \
        "the touched tiles are not the index-order sum of the slices"
    ref = gx.product64(A, B)
    assert np.array_equal(got, ref, equal_nan=True)
    if operand == "A":
        assert not np.isfinite(got[1, m]).any()


# ------------------------------------------------------------------------------------------ 6. operators
SPLIT_KS = [3, "auto"]


@pytest.mark.parametrize("split_k", SPLIT_KS)
@pytest.mark.parametrize("stride", gx.CONV_STRIDES, ids=lambda s: f"s{s[0]}{s[1]}")
@pytest.mark.parametrize("groups", gx.CONV_GROUPS)
def test_ste_conv2d_backward_exact(groups, stride, split_k):
    from fp8_quantization_amd.approx_ops import ste_conv2d
    x, w, dy = gx.conv_problem(groups, stride)
    pad, dil = gx.CONV["padding"], gx.CONV["dilation"]
    xq, wq = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    _stats()
    y = ste_conv2d(xq, wq, lambda a, b: F.conv2d(a, b, None, stride, pad, dil, groups), stride, pad, dil, groups,
                   split_k=split_k)
    y.backward(dy.to(DEV))
    st = _stats()
    assert st["launches"] == 1 + (1 if groups == 1 else min(x.shape[0], groups)) and st["recomputed"] == 0, st
    if split_k == 3:
        # dW: groups items of one tile, K = 3 images x 117 (s11) or 63 (s21) pixels: 11 or 6 stages, three parts;
        # dXcol: (image, group) items of [L x Kg] (2 or 1 tiles), K = the group's output channels: one stage, one part
        Bn, L = x.shape[0], dy.shape[2] * dy.shape[3]
        assert gs.plan(Bn * L, 3)[1] == 3 and gs.plan(w.shape[0] // groups, 3)[1] == 1
        assert st["tiles"] == groups * 3 + Bn * groups * -(-L // 64), st
    dx, dw = gx.conv_backward64(x, w, dy, groups, stride)
    xs.assert_same(xq.grad.cpu().numpy(), dx.numpy().astype(np.float32), f"dX, G = {groups}, stride {stride}")
    xs.assert_same(wq.grad.cpu().numpy(), dw.numpy().astype(np.float32), f"dW, G = {groups}, stride {stride}")


@pytest.mark.parametrize("split_k", SPLIT_KS)
def test_ste_linear_backward_exact(split_k):
    from fp8_quantization_amd.approx_ops import ste_linear
    xq, wq, dy = gx.linear_problem()
    xd, wd = _dev(xq).requires_grad_(), _dev(wq).requires_grad_()
    _stats()
    y = ste_linear(xd, wd, F.linear, split_k=split_k)
    y.backward(_dev(dy))
    st = _stats()
    assert st["launches"] == 2 and st["recomputed"] == 0, st
    if split_k == 3:   # dX [70 x 130]: K = 67, three stages, 2 x 3 tiles; dW [67 x 130]: K = 70, the same
        assert st["tiles"] == 2 * 6 * 3, st
    d = dy.astype(np.float64)
    xs.assert_same(xd.grad.cpu().numpy(), (d @ wq.astype(np.float64)).astype(np.float32), "linear dX")
    xs.assert_same(wd.grad.cpu().numpy(), (d.T @ xq.astype(np.float64)).astype(np.float32), "linear dW")


@pytest.mark.parametrize("split_k", SPLIT_KS)
def test_ste_bmm_backward_exact_on_head_views(split_k):
    from fp8_quantization_amd.approx_ops import ste_bmm
    q, k, dc = gx.bmm_problem()
    qd, kd = _dev(q).requires_grad_(), _dev(k).requires_grad_()
    _stats()
    c = ste_bmm(gx.heads(qd), gx.heads(kd).transpose(-1, -2), torch.matmul, split_k=split_k)
    c.backward(_dev(dc))
    st = _stats()
    assert st["launches"] == 2 * gx.BMM["b"] and st["recomputed"] == 0, st
    if split_k == 3:   # per launch 3 heads of [70 x 70] @ [70 x 8]: 2 tiles, K = 70: three stages
        assert st["tiles"] == st["launches"] * 3 * 2 * 3, st
    q64, k64 = (torch.from_numpy(t).double().requires_grad_() for t in (q, k))
    dq, dk = torch.autograd.grad(torch.matmul(gx.heads(q64), gx.heads(k64).transpose(-1, -2)), (q64, k64),
                                 torch.from_numpy(dc).double())
    xs.assert_same(qd.grad.cpu().numpy(), dq.numpy().astype(np.float32), "bmm dQ")
    xs.assert_same(kd.grad.cpu().numpy(), dk.numpy().astype(np.float32), "bmm dK")


# ------------------------------------------------------------------------------------------ 7. the operator switch
def _calibrate(m, x):
    from fp8_quantization_amd.quantization.base_quantized_classes import QuantizedModule
    m = m.to(DEV).eval()
    for sub in m.modules():
        if isinstance(sub, QuantizedModule):
            sub.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(x)
    m.fix_ranges()
    return m


def _layer_grads(make, x, **cfg):
    """(dX, dW, grad_stats, (xq, wq, dy)) of a layer's product on its quantized operands, with `cfg` in
    custom_approx_params."""
    from fp8_quantization_amd.resnet_workload import approx_qparams
    torch.manual_seed(5)
    qp = approx_qparams(ste_backward=True)
    qp["custom_approx_params"].update(cfg)
    m = _calibrate(make(qp), x)
    with torch.no_grad():
        xq = m.activation_quantizer(x)
        wq, bias = m.get_params()
    xq, wq = xq.detach().requires_grad_(), wq.detach().requires_grad_()
    _stats()
    y = m.run_forward(xq, wq, bias)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    y.backward(dy)
    return xq.grad, wq.grad, _stats(), (xq.detach(), wq.detach(), dy)


def _assert_bar(prod, ops, dx, dw, what):
    """The project's bar on both gradients of the bilinear prod(x, w) at upstream dy: |got - ref| <= 1e-5 S, ref and S
    (the same gradients of |x|, |w|, |dy|) from float64 autograd on the CPU."""
    x, w, g = (t.double().cpu() for t in ops)
    ref = S = None
    for a, b, u in ((x, w, g), (x.abs(), w.abs(), g.abs())):
        a, b = a.clone().requires_grad_(), b.clone().requires_grad_()
        ref, S = S, torch.autograd.grad(prod(a, b), (a, b), u)
    for name, got, r, s in zip(("dX", "dW"), (dx, dw), ref, S):
        err = (got.double().cpu() - r).abs()
        print(f"{what} {name}: max |got - ref| / S = {float((err / s.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 1e-5 * s).all()), f"{what} {name}: outside 1e-5 S"


def _make_conv(qp):
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    return QCustomBNConv2dTorch(in_channels=4, out_channels=40, kernel_size=3, padding=1, bias=False, **qp)


def _make_linear(qp):
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    return QCustomLinearTorch(in_features=40, out_features=40, bias=True, **qp)


# unsplit tiles: conv dW [40 x 72] @ [72 x 36] 1, dXcol 2 images of [36 x 40] @ [40 x 36] 2; linear 70 rows: dX
# [70 x 40] @ [40 x 40] 2, dW [40 x 70] @ [70 x 40] 1.  Every K has two or three stages: S = 2 at grad_split_k = 2.
SWITCH = {"conv": (_make_conv, (2, 4, 6, 6), 3, lambda a, b: F.conv2d(a, b, None, 1, 1)),
          "linear": (_make_linear, (70, 40), 3, F.linear)}


@pytest.mark.parametrize("kind", list(SWITCH))
def test_the_operator_key_reaches_the_gradient_gemm(kind):
    make, shape, tiles, prod = SWITCH[kind]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    dx0, dw0, st0, ops = _layer_grads(make, x)
    assert st0 == dict(launches=2, tiles=tiles, recomputed=0), st0
    _assert_bar(prod, ops, dx0, dw0, f"{kind}, key absent")
    dx1, dw1, st1, _ = _layer_grads(make, x, grad_split_k=1)
    assert st1 == st0 and torch.equal(_bits(dx1), _bits(dx0)) and torch.equal(_bits(dw1), _bits(dw0))
    dx2, dw2, st2, ops2 = _layer_grads(make, x, grad_split_k=2)
    assert st2 == dict(launches=2, tiles=2 * tiles, recomputed=0), st2
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(ops2, ops))     # the same product, the same dy
    _assert_bar(prod, ops, dx2, dw2, f"{kind}, grad_split_k = 2")              # (a wrong result through the key)
    _, _, sta, _ = _layer_grads(make, x, grad_split_k="auto")
    assert sta["launches"] == 2 and sta["recomputed"] == 0
    with pytest.raises(ValueError, match="grad_split_k"):
        _layer_grads(make, x, grad_split_k=0)


# ------------------------------------------------------------------------------------------ 8. grad_split_auto
def test_grad_split_auto_rule():
    from fp8_quantization_amd import approx_ops as ao
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    target = ao.GRAD_SPLIT_BLOCKS_PER_CU * cus
    assert ao.grad_split_auto(64 * 12, 197, 197, 64, DEV) == 1            # attention: 16 tiles x 768 items
    assert ao.grad_split_auto(target, 64, 64, 1 << 16, DEV) == 1          # exactly the target block count
    assert ao.grad_split_auto(1, 64, 64, 1 << 16, DEV) > 1
    assert ao.grad_split_auto(1, 64, 64, 31, DEV) == 1 and ao.grad_split_auto(1, 64, 64, 0, DEV) == 1
    for (nb, M, N, K) in [(1, 64, 64, 1 << 16), (1, 128, 1152, 50176), (1, 64, 147, 802816), (1, 512, 4608, 3136),
                          (1, 64, 64, 300), (3, 70, 67, 4096), (1, 3072, 768, 12608), (1, 4096, 4096, 1 << 20)]:
        s = ao.grad_split_auto(nb, M, N, K, DEV)
        nst, blocks = -(-K // 32), nb * -(-M // 64) * -(-N // 64)
        assert 1 <= s <= max(1, nst // ao.GRAD_SPLIT_MIN_STAGES), (nb, M, N, K, s)
        assert s == 1 or gs.workspace_bytes(nb, M, N, K, s) <= ao.GRAD_SPLIT_MAX_BYTES, (nb, M, N, K, s)
        assert s == 1 or blocks < target


# ------------------------------------------------------------------------------------------ 9. general operands
def test_general_operands_meet_the_bar_with_auto():
    from fp8_quantization_amd.approx_ops import grad_bmm, grad_split_auto
    g = torch.Generator().manual_seed(9)
    nb, M, N, K0, K1 = 1, 70, 147, 64, 49
    A = torch.randn((nb, M, K0, K1), generator=g) * torch.exp2(torch.randint(-8, 9, (nb, M, 1, 1), generator=g).float())
    B = (torch.randn((nb, K0, K1, N), generator=g).view(torch.int32) & -65536).view(torch.float32)
    ref = torch.einsum("imkl,ikln->imn", A.double(), B.double())
    S = torch.einsum("imkl,ikln->imn", A.double().abs(), B.double().abs())
    s = grad_split_auto(nb, M, N, K0 * K1, DEV)
    assert s > 1                                          # 6 tiles, 98 stages
    got, st = _launch(A.to(DEV), B.to(DEV), None, "auto")
    _expect_stats(st, nb, M, N, K0 * K1, s)
    ratio = ((got.cpu().double() - ref).abs() / S.clamp_min(1e-300)).max()
    print(f"K = {K0} x {K1}, auto = {s} splits: max |got - ref| / sum |a b| = {float(ratio):.3e}")
    assert bool(((got.cpu().double() - ref).abs() <= 1e-5 * S).all()), f"outside 1e-5 S (worst {float(ratio):.3e})"
