"""fp8a_grad_bmm (gemm_grad_kernel, csrc/gemm_grad.h): the gradient GEMM against float64 torch on the CPU.

Shape nb = 3, M = 70, N = 67, K0 x K1 = 2 x 37: ragged in every extent, two row tiles and two column tiles
per item, three K stages with a ragged tail and a k0 step inside a stage.  A is arbitrary fp32 (normal
values), B bf16-exact (normal values truncated to bf16).

  * bar: |got - ref| <= 1e-5 * S, S the same product of |A| and |B|, ref and S from float64 torch on the CPU
    (the project's sum bar: the products are exact, only the summation order differs);
  * strides: A with unit stride on m and again on k1 (B then with unit stride on n / on k1), C with unit
    stride on m and again on n; the inner K extent also 2 and 1 (several k0 steps inside one thread's eight
    loads); two batch dims that do not collapse (one launch per index of the shorter);
  * two calls give identical bytes, 0 tiles recomputed;
  * one off-grid B element (1 + 2^-12): exactly the tiles that staged it are recomputed, the bar is still
    met, every other tile's bytes equal the clean run;
  * one A element at 2^-130 and one infinity: their tiles are recomputed too.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB, M, N, K0, K1 = 3, 70, 67, 2, 37


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _bf16_exact(t):
    return (t.view(torch.int32) & -65536).view(torch.float32)


def _operands(k0=K0, k1=K1, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((NB, M, k0, k1), generator=g)
    A = A * torch.exp2(torch.randint(-20, 20, (NB, M, 1, 1), generator=g).float())  # rows of very different scale
    B = _bf16_exact(torch.randn((NB, k0, k1, N), generator=g))
    return A, B


def _ref(A, B):
    """(ref, S) in float64 on the CPU."""
    a, b = A.double(), B.double()
    return torch.einsum("imkl,ikln->imn", a, b), torch.einsum("imkl,ikln->imn", a.abs(), b.abs())


@pytest.fixture(scope="module")
def clean():
    A, B = _operands()
    ref, S = _ref(A, B)
    return A, B, ref, S


def _lay_a(A, layout):
    """A on the device as a [nb, M, K0, K1] view with unit stride on k1 or on m."""
    if layout == "k1":
        return A.to(DEV).contiguous()
    v = A.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    assert v.stride(1) == 1
    return v


def _lay_b(B, layout):
    """B as a [nb, K0, K1, N] view with unit stride on n (with A's "m") or on k1."""
    if layout == "m":
        return B.to(DEV).contiguous()
    v = B.permute(0, 3, 1, 2).contiguous().to(DEV).permute(0, 2, 3, 1)
    assert v.stride(2) == 1
    return v


def _out(layout):
    """A sentinel-filled [nb, M, N] view with unit stride on n or on m."""
    if layout == "n":
        return torch.full((NB, M, N), -77.25, device=DEV)
    v = torch.full((NB, N, M), -77.25, device=DEV).transpose(1, 2)
    assert v.stride(1) == 1
    return v


def _run(A, B, a_layout="k1", c_layout="n"):
    from fp8_quantization_amd.approx_ops import grad_bmm
    out = _out(c_layout)
    res = grad_bmm(_lay_a(A, a_layout), _lay_b(B, a_layout), out=out, k2=True)
    assert res is out
    return out.cpu()


def _stats(reset=False):
    from fp8_quantization_amd import _lib
    return _lib.grad_stats(reset)


def _assert_bar(got, ref, S, what=""):
    err = (got.double() - ref).abs()
    bar = 1e-5 * S
    print(f"{what} max err / S = {float((err / S.clamp_min(1e-300)).max()):.3e}")
    bad = err > bar
    assert not bad.any(), f"{what}: {int(bad.sum())} outputs outside 1e-5 S, worst {float((err / S).max()):.3e}"


@pytest.mark.parametrize("c_layout", ["n", "m"])
@pytest.mark.parametrize("a_layout", ["k1", "m"])
def test_bar_determinism_and_no_recompute(clean, a_layout, c_layout):
    A, B, ref, S = clean
    _stats(reset=True)
    got = _run(A, B, a_layout, c_layout)
    again = _run(A, B, a_layout, c_layout)
    st = _stats(reset=True)
    assert st == dict(launches=2, tiles=2 * NB * 2 * 2, recomputed=0), st
    _assert_bar(got, ref, S, f"A unit {a_layout}, C unit {c_layout}")
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("k0,k1", [(37, 2), (74, 1), (1, 74)])
def test_inner_extents(k0, k1):
    from fp8_quantization_amd.approx_ops import grad_bmm
    A, B = _operands(k0, k1, seed=1)
    ref, S = _ref(A, B)
    _stats(reset=True)
    got = grad_bmm(A.to(DEV), B.to(DEV), k2=True).cpu()
    assert _stats(reset=True)["recomputed"] == 0
    _assert_bar(got, ref, S, f"K0 x K1 = {k0} x {k1}")
    if k0 == 1:  # the single-level form is the same launch
        flat = grad_bmm(A.to(DEV)[:, :, 0], B.to(DEV)[:, 0]).cpu()
        assert torch.equal(flat.view(torch.int32), got.view(torch.int32))


def test_two_batch_dims_that_do_not_collapse():
    """Head views of [b, S, H d] buffers: batch strides (S H d, d); the gradient contiguous."""
    from fp8_quantization_amd.approx_ops import grad_bmm
    g = torch.Generator().manual_seed(2)
    b, H, S, d = 2, 3, 5, 8
    dC = torch.randn((b, H, S, S), generator=g)
    Kh = _bf16_exact(torch.randn((b, S, H * d), generator=g))
    ref = torch.einsum("bhst,bthe->bhse", dC.double(), Kh.view(b, S, H, d).double())
    Sa = torch.einsum("bhst,bthe->bhse", dC.double().abs(), Kh.view(b, S, H, d).double().abs())
    kv = Kh.to(DEV).view(b, S, H, d).permute(0, 2, 1, 3)  # [b, H, S, d]
    _stats(reset=True)
    got = grad_bmm(dC.to(DEV), kv).cpu()
    st = _stats(reset=True)
    assert st["launches"] == b and st["recomputed"] == 0, st
    _assert_bar(got, ref, Sa, "head views")


def _tiles_differ(x, y):
    """The (item, row tile, column tile) triples whose bytes differ."""
    d = x.view(torch.int32) != y.view(torch.int32)
    return sorted({(int(i), int(m) // 64, int(n) // 64) for i, m, n in d.nonzero().tolist()})


def test_one_off_grid_b_element(clean):
    A, B, ref, S = clean
    base = _run(A, B)
    B2 = B.clone()
    B2[1, 1, 5, 3] = 1.0 + 2.0 ** -12  # item 1, column tile 0: its two row tiles stage it
    ref2, S2 = _ref(A, B2)
    _stats(reset=True)
    got = _run(A, B2)
    st = _stats(reset=True)
    assert st["recomputed"] == 2, st
    _assert_bar(got, ref2, S2, "off-grid B")
    assert set(_tiles_differ(got, base)) <= {(1, 0, 0), (1, 1, 0)}
    keep = torch.ones((NB, M, N), dtype=torch.bool)
    keep[1, :, :64] = False
    assert torch.equal(got.view(torch.int32)[keep], base.view(torch.int32)[keep])


def test_tiny_and_infinite_a_elements(clean):
    A, B, _, _ = clean
    A2 = A.clone()
    A2[0, 65, 1, 7] = 2.0 ** -130          # item 0, row tile 1: both column tiles
    A2[2, 3, 0, 11] = float("inf")         # item 2, row tile 0: both column tiles
    ref2, S2 = _ref(A2, B)
    _stats(reset=True)
    got = _run(A2, B)
    st = _stats(reset=True)
    assert st["recomputed"] == 4, st
    rows = torch.ones((NB, M), dtype=torch.bool)
    rows[2, 3] = False
    _assert_bar(got[rows], ref2[rows], S2[rows], "tiny / inf A, finite rows")
    # the infinite row: +-inf where one sign of b meets it, NaN where b is zero -- as the fp32 product gives
    assert np.array_equal(got[2, 3].numpy(), ref2[2, 3].float().numpy(), equal_nan=True)
    assert not torch.isfinite(got[2, 3]).any()


def test_empty_extents():
    from fp8_quantization_amd.approx_ops import grad_bmm
    a = torch.randn((2, 5, 0), device=DEV)
    b = torch.randn((2, 0, 7), device=DEV)
    out = torch.full((2, 5, 7), 3.0, device=DEV)
    assert torch.equal(grad_bmm(a, b, out=out).cpu(), torch.zeros(2, 5, 7))  # K = 0: zeros
    assert grad_bmm(torch.randn((0, 5, 4), device=DEV), torch.randn((0, 4, 7), device=DEV)).shape == (0, 5, 7)
    assert grad_bmm(torch.randn((2, 0, 4), device=DEV), torch.randn((2, 4, 7), device=DEV)).shape == (2, 0, 7)
