"""The gradient GEMM (gemm_grad_kernel, csrc/gemm_grad.h), fp8a_im2col and the three STE backward Functions on
sums that can be compared bit for bit (data, rule and model: tests/grad_exact.py; the conditions
on the inputs and the mutants each case catches: tests/test_grad_exact_cpu.py).

No comparison here has a tolerance: exact_sums.assert_same (equal bits, zeros by value) against float64 numpy /
torch on the CPU; non-finite outputs by value with NaN equal to NaN.  Every launch goes through approx_ops.grad_bmm
(or the Function under test) between two _lib.grad_stats(reset=True).

  1. both families at the K edges (32, 33, 64, 1, 7, 96, 5; 2 x 37) and on 3 x 1 / 1 x 3 tile grids, A and C each
     with unit stride on either index: bits, 0 tiles recomputed, the tile counter equal to the grid;
  2. operands that are views of NaN-filled buffers with a k0 step that does not collapse (K0 x K1 = 2 x 37,
     15 x 5, 37 x 2, 74 x 1, either unit stride), C the interior of a sentinel buffer: bits, 0 recomputed, the
     frame untouched;
  3. routing (every output one product a 2^j) and every position pair of two stages, 1 +- 2^-21;
  4. the acceptance window at its edge: exponent field 24 accepted; fields 23, 1, 0, NaN, -inf in A and a bf16
     subnormal, +inf, NaN, 1 + 2^-12 in B each recompute exactly the tiles that stage them; both signed zeros none;
  5. products whose piece terms, or the whole product, are fp32 subnormals: the IEEE product, subnormals kept;
  6. fp8a_im2col against F.unfold, the grid-stride loop included;
  7. ste_conv2d (groups 1, 2, 4; a 3 x 2 kernel with dilation, stride 1 and (2, 1)), ste_linear and ste_bmm on
     head views, with torch's own product as the forward launch.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_sums as xs
from tests import grad_exact as gx

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
    v = _dev(A.transpose(0, 2, 3, 1)).permute(0, 3, 1, 2)
    assert v.stride(1) == 1
    return v


def _lay_b(B, layout):
    """B [nb, K0, K1, N] with unit stride on k1 (with A's "k1") or on n."""
    if layout == "m":
        return _dev(B)
    v = _dev(B.transpose(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert v.stride(2) == 1 or v.shape[2] == 1
    return v


def _out(nb, M, N, layout):
    """A sentinel-filled [nb, M, N] view with unit stride on n or on m."""
    if layout == "n":
        return torch.full((nb, M, N), float(gx.SENTINEL), device=DEV)
    v = torch.full((nb, N, M), float(gx.SENTINEL), device=DEV).transpose(1, 2)
    assert v.stride(1) == 1
    return v


def _launch(a, b, out):
    """One grad_bmm launch on device views a [nb, M, K0, K1], b [nb, K0, K1, N]: the single-level form when
    K0 = 1.  Returns grad_stats of the launch."""
    from fp8_quantization_amd.approx_ops import grad_bmm
    _stats()
    if a.shape[2] == 1:
        res = grad_bmm(a[:, :, 0], b[:, 0], out=out)
    else:
        res = grad_bmm(a, b, out=out, k2=True)
    assert res is out
    return _stats()


def _run(A, B, a_layout="k1", c_layout="n", recomputed=0):
    nb, M = A.shape[:2]
    N = B.shape[-1]
    out = _out(nb, M, N, c_layout)
    st = _launch(_lay_a(A, a_layout), _lay_b(B, a_layout), out)
    assert st == dict(launches=1, tiles=gx.num_tiles(nb, M, N), recomputed=recomputed), st
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. exact sums
@pytest.mark.parametrize("cid", list(gx.edge_cases()))
def test_exact_sums_at_the_edges(cid):
    p = gx.problem(cid)
    xs.assert_same(_run(p["A"], p["B"]), p["want"], cid, p["T"])


@pytest.mark.parametrize("c_layout", ["n", "m"])
@pytest.mark.parametrize("a_layout", ["k1", "m"])
@pytest.mark.parametrize("cid", [f"{fam}-2x37-{M}x{N}" for fam in "WG" for (M, N) in gx.TWO_LEVEL])
def test_exact_sums_unit_strides(cid, a_layout, c_layout):
    p = gx.problem(cid)
    xs.assert_same(_run(p["A"], p["B"], a_layout, c_layout), p["want"], f"{cid} A unit {a_layout}, C unit {c_layout}",
                   p["T"])


# ------------------------------------------------------------------------------------------ 2. padded views
@pytest.mark.parametrize("layout", ["k1", "m"])
@pytest.mark.parametrize("k0,k1", gx.PAD_K)
def test_non_collapsing_views_with_poisoned_surroundings(k0, k1, layout):
    p = gx.problem(f"W-pad-{k0}x{k1}")
    nb, M = p["A"].shape[:2]
    N = p["B"].shape[-1]
    ba, bb = gx.padded(p["A"], p["B"], layout)
    a, b = gx.a_view(_dev(ba), layout, M, k1), gx.b_view(_dev(bb), layout, k1, N)
    assert a.stride(2) != k1 * a.stride(3) and b.stride(1) != k1 * b.stride(2)
    assert (a.stride(3) if layout == "k1" else a.stride(1)) == 1
    cb = _dev(gx.c_buffer(nb, M, N, layout))
    st = _launch(a, b, gx.c_view(cb, layout))
    assert st == dict(launches=1, tiles=gx.num_tiles(nb, M, N), recomputed=0), st
    host = cb.cpu().numpy()
    xs.assert_same(np.ascontiguousarray(gx.c_view(host, layout)), p["want"], f"padded {k0} x {k1}, unit {layout}", p["T"])
    gx.c_view(host, layout)[...] = gx.SENTINEL
    assert (host.view(np.uint32) == SENT_BITS).all(), "C's sentinel frame was written"


# ------------------------------------------------------------------------------------------ 3. routing, pairs
def test_routing_every_output_is_one_product():
    p = gx.problem("routing")
    xs.assert_same(_run(p["A"], p["B"]), p["want"], "routing")
    xs.assert_same(_run(p["A"], p["B"], "m", "m"), p["want"], "routing, unit m")


@pytest.mark.parametrize("sign", [1, -1])
def test_wide_range_pairs_exact(sign):
    """1 at k = i and +-2^-21 at k = r for every i != r in 0..63: every position pair of two stages."""
    A, B, want = gx.pairs(sign)
    got = _run(A, B)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{len(bad)} outputs lose the small term, e.g. (i, r, n) = {bad[:6].tolist()}: " \
                         f"got {got[tuple(bad[0])]!r}, expected {want[tuple(bad[0])]!r}"


# ------------------------------------------------------------------------------------------ 4. window edges
def _same_with_nonfinite(got, want, what):
    """Bits where the expected value is finite; +-inf and NaN by value."""
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), f"{what}: non-finite outputs differ"
    xs.assert_same(np.where(fin, got, 0), np.where(fin, want, 0), what)


@pytest.fixture(scope="module")
def window_clean():
    """The clean sparse runs, per (operand, M, N): accepted with 0 tiles recomputed, exact."""
    out = {}

    def get(operand, M, N):
        key = (operand, M, N)
        if key not in out:
            c = gx.window_case(M, N, operand)
            got = _run(c["A"], c["B"])
            xs.assert_same(got, c["want"], f"clean window case {key}")
            out[key] = got
        return out[key]
    return get


@pytest.mark.parametrize("M,N", gx.TWO_LEVEL)
def test_window_field_24_is_accepted(window_clean, M, N):
    assert gx.exponent_field(gx.GOOD_A) == 24
    got = window_clean("A", M, N)                                      # (0 recomputed and exact: asserted inside)
    assert (np.abs(got) == np.float32(2.0 ** -3 * (1 + 2.0 ** -21))).all()


WINDOW = [("A", n, "k1") for n in gx.A_REJECTED] + [("B", n, "k1") for n in gx.B_REJECTED] + \
    [("A", "field23", "m"), ("B", "bf16-subnormal", "m")]


@pytest.mark.parametrize("M,N", gx.TWO_LEVEL)
@pytest.mark.parametrize("operand,name,layout", WINDOW, ids=[f"{o}-{n}-unit-{lay}" for o, n, lay in WINDOW])
def test_window_rejected_elements_recompute_their_tiles(window_clean, operand, name, layout, M, N):
    clean = window_clean(operand, M, N)
    c = gx.window_case(M, N, operand, name)
    num_mt, num_nt = -(-M // 64), -(-N // 64)
    assert len(c["tiles"]) == (num_nt if operand == "A" else num_mt)   # 3 x 1: A 1, B 3; 1 x 3: A 3, B 1
    got = _run(c["A"], c["B"], layout, "n" if layout == "k1" else "m", recomputed=len(c["tiles"]))
    _same_with_nonfinite(got, c["want"], f"{operand} {name}")
    keep = np.ones(got.shape, bool)
    for (i, mt, nt) in c["tiles"]:
        keep[i, 64 * mt:64 * mt + 64, 64 * nt:64 * nt + 64] = False
    assert np.array_equal(got.view(np.uint32)[keep], clean.view(np.uint32)[keep]), "a tile that staged no rejected " \
        "element differs from the clean run"
    assert not np.array_equal(got.view(np.uint32), clean.view(np.uint32))


def test_signed_zeros_force_no_recompute():
    p = gx.problem("W-2x37-130x40")
    A, B = p["A"].copy(), p["B"].copy()
    za, zb = A == 0, B == 0
    assert za.any() and zb.any()
    pos = _run(A, B)
    A[za], B[zb] = -0.0, -0.0
    assert np.signbit(A[za]).all() and np.signbit(B[zb]).all()
    neg = _run(A, B)                                                   # (recomputed == 0 asserted in _run)
    xs.assert_same(neg, p["want"], "-0.0 in A and B", p["T"])
    xs.assert_same(neg, pos, "-0.0 against +0.0")


# ------------------------------------------------------------------------------------------ 5. small products
@pytest.mark.parametrize("name", list(gx.SMALL))
def test_small_products_keep_fp32_subnormals(name):
    """A piece term (or the whole product) below 2^-126 while both operands are inside the accepted window: the
    result is the IEEE fp32 product with subnormals kept, as the kernel's own fp32 recompute gives."""
    c = gx.small_case(name)
    got = _run(c["A"], c["B"])
    vals, counts = np.unique(np.abs(got), return_counts=True)
    print(f"{name}: |a b| = {float(np.abs(c['want']).max()).hex()}; the device gave "
          + ", ".join(f"{float(v).hex()} x {n}" for v, n in zip(vals, counts)))
    xs.assert_same(got, c["want"], name)


# ------------------------------------------------------------------------------------------ 6. fp8a_im2col
def _im2col(x, k, stride, padding, dilation):
    from fp8_quantization_amd import _lib
    L = _lib.load()
    Bn, C, H, W = x.shape
    Ho = (H + 2 * padding[0] - dilation[0] * (k[0] - 1) - 1) // stride[0] + 1
    Wo = (W + 2 * padding[1] - dilation[1] * (k[1] - 1) - 1) // stride[1] + 1
    xd = x.to(DEV)
    out = torch.full((Bn * Ho * Wo, C * k[0] * k[1]), float("nan"), device=DEV)
    rc = L.fp8a_im2col(_lib.dev_ptr(xd), _lib.dev_ptr(out), Bn, C, H, W, k[0], k[1], stride[0], stride[1], padding[0],
                       padding[1], dilation[0], dilation[1], _lib.stream_ptr(xd.device))
    _lib.check(rc, "fp8a_im2col")
    return out.cpu()


IM2COL = {"strided-dilated": ((3, 4, 11, 9), (3, 2), (2, 1), (1, 0), (1, 2)),
          "padding-beyond-the-kernel": ((3, 4, 11, 9), (3, 2), (2, 1), (3, 2), (1, 2)),
          "grid-stride-loop": ((4, 8, 260, 260), (3, 3), (1, 1), (1, 1), (1, 1))}


@pytest.mark.parametrize("name", list(IM2COL))
def test_im2col_equals_unfold(name):
    shape, k, stride, padding, dilation = IM2COL[name]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    want = F.unfold(x, k, dilation=dilation, padding=padding, stride=stride)      # [Bn, C kh kw, L]
    want = want.transpose(1, 2).reshape(-1, want.shape[1]).contiguous()           # [Bn L, (c, ky, kx)]
    if name == "grid-stride-loop":
        assert want.numel() > 65536 * 256
    if name == "padding-beyond-the-kernel":
        assert (want.view(shape[0], -1, want.shape[1])[:, 0] == 0).all()          # a window in the padding alone
    got = _im2col(x, k, stride, padding, dilation)
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------ 7. STE operators
@pytest.mark.parametrize("stride", gx.CONV_STRIDES, ids=lambda s: f"s{s[0]}{s[1]}")
@pytest.mark.parametrize("groups", gx.CONV_GROUPS)
def test_ste_conv2d_backward_exact(groups, stride):
    from fp8_quantization_amd.approx_ops import ste_conv2d
    x, w, dy = gx.conv_problem(groups, stride)
    pad, dil = gx.CONV["padding"], gx.CONV["dilation"]
    xq, wq = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    _stats()
    y = ste_conv2d(xq, wq, lambda a, b: F.conv2d(a, b, None, stride, pad, dil, groups), stride, pad, dil, groups)
    assert y.requires_grad and tuple(y.shape) == tuple(dy.shape)
    y.backward(dy.to(DEV))
    st = _stats()
    assert st["launches"] == 1 + (1 if groups == 1 else min(x.shape[0], groups)) and st["recomputed"] == 0, st
    dx, dw = gx.conv_backward64(x, w, dy, groups, stride)
    xs.assert_same(xq.grad.cpu().numpy(), dx.numpy().astype(np.float32), f"dX, G = {groups}, stride {stride}")
    xs.assert_same(wq.grad.cpu().numpy(), dw.numpy().astype(np.float32), f"dW, G = {groups}, stride {stride}")


def test_ste_linear_backward_exact():
    from fp8_quantization_amd.approx_ops import ste_linear
    xq, wq, dy = gx.linear_problem()
    xd, wd = _dev(xq).requires_grad_(), _dev(wq).requires_grad_()
    _stats()
    y = ste_linear(xd, wd, F.linear)
    y.backward(_dev(dy))
    st = _stats()
    assert st["launches"] == 2 and st["recomputed"] == 0, st
    d = dy.astype(np.float64)
    xs.assert_same(xd.grad.cpu().numpy(), (d @ wq.astype(np.float64)).astype(np.float32), "linear dX")
    xs.assert_same(wd.grad.cpu().numpy(), (d.T @ xq.astype(np.float64)).astype(np.float32), "linear dW")


def test_ste_bmm_backward_exact_on_head_views():
    """[2, 3, 70, 8] @ [2, 3, 8, 70]: both operands head views of [b, S, H d] buffers, the second transposed."""
    from fp8_quantization_amd.approx_ops import ste_bmm
    q, k, dc = gx.bmm_problem()
    qd, kd = _dev(q).requires_grad_(), _dev(k).requires_grad_()
    _stats()
    c = ste_bmm(gx.heads(qd), gx.heads(kd).transpose(-1, -2), torch.matmul)
    assert tuple(c.shape) == dc.shape
    c.backward(_dev(dc))
    st = _stats()
    assert st["launches"] == 2 * gx.BMM["b"] and st["recomputed"] == 0, st
    q64, k64 = (torch.from_numpy(t).double().requires_grad_() for t in (q, k))
    dq, dk = torch.autograd.grad(torch.matmul(gx.heads(q64), gx.heads(k64).transpose(-1, -2)), (q64, k64),
                                 torch.from_numpy(dc).double())
    xs.assert_same(qd.grad.cpu().numpy(), dq.numpy().astype(np.float32), "bmm dQ")
    xs.assert_same(kd.grad.cpu().numpy(), dk.numpy().astype(np.float32), "bmm dK")
