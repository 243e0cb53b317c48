"""``approx_attention`` on a tiny ViT (32x32 images, 8x8 patches -> 17 tokens, hidden 32, 2 heads of 16,
2 layers, MLP 64, batch 3), E4M3 and E3M4: calibrated, ranges fixed, one forward with QK^T and PV as
batched approx products (QCustomMatMul -> fp8a_bmm).

  * hooks capture both operators' quantized operands, biases and outputs in every layer: each (image, head)
    product within 1e-5 * sum|term| of oracle.matmul at the captured biases; the operands are on their
    grids, so no tile is recomputed;
  * the option is live (logits differ from the option-off model's) and off means off (logits bit-identical
    to a model built without the argument);
  * the validate driver with --approx-attention runs to a JSON that records the option;
  * the forward captured in a graph replays bit-identical to eager.
"""
import json

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import golden_io as gio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(image_size=32, patch_size=8, hidden=32, layers=2, heads=2, mlp=64, num_labels=10)
T, H, D, BATCH = 17, 2, 16, 3


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


def _model(E, M, **kw):
    from fp8_quantization_amd.vit_workload import vit_b16_approx
    return vit_b16_approx(seed=E * 10 + M, expo_width=E, mant_width=M, **kw, **TINY).to(DEV).eval()


def _inputs():
    g = torch.Generator().manual_seed(3)
    return torch.randn((4, 3, 32, 32), generator=g).to(DEV), torch.randn((BATCH, 3, 32, 32), generator=g).to(DEV)


def _calibrate(m, xcal):
    m.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(xcal)
    m.fix_ranges()


def _ib(t):
    return int(t.reshape(-1)[0].item())


@pytest.mark.parametrize("fmt", [(4, 3), (3, 4)], ids=["E4M3", "E3M4"])
def test_attention_products_match_oracle(fmt):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_calculation import QCustomMatMul
    E, M = fmt
    xcal, xev = _inputs()
    on = _model(E, M, approx_attention=True)
    _calibrate(on, xcal)
    ops = [(n, m) for n, m in on.named_modules() if isinstance(m, QCustomMatMul)]
    assert len(ops) == 2 * TINY["layers"]
    seen, hooks = {}, []
    for name, op in ops:
        rec = seen.setdefault(name, {})
        hooks.append(op.a_quantizer.register_forward_hook(lambda m, i, o, rec=rec: rec.update(a=o.cpu())))
        hooks.append(op.b_quantizer.register_forward_hook(lambda m, i, o, rec=rec: rec.update(b=o.cpu())))
        hooks.append(op.register_forward_hook(lambda m, i, o, rec=rec: rec.update(c=o.cpu())))
    _lib.bmm_stats(reset=True)
    with torch.no_grad():
        logits_on = on(xev)
    for h in hooks:
        h.remove()
    st = _lib.bmm_stats(reset=True)
    assert st["launches"] == len(ops) and st["recomputed"] == 0, st
    assert torch.isfinite(logits_on).all()

    for name, op in ops:
        rec = seen[name]
        Eo, Mo, table, flags = op._approx_config()
        assert (Eo, Mo) == (E, M)
        bA, bB, bR = (_ib(q.get_fp_bias()) for q in (op.a_quantizer, op.b_quantizer, op.res_quantizer))
        a, b, c = rec["a"].numpy(), rec["b"].numpy(), rec["c"].numpy()
        kn = (D, T) if name.endswith("qk_matmul") else (T, D)
        assert a.shape == (BATCH, H, T, kn[0]) and b.shape == (BATCH, H) + kn and c.shape == (BATCH, H, T, kn[1])
        tab = np.ascontiguousarray(table.numpy(), np.int32)
        for i in range(BATCH):
            for h in range(H):
                ref, S = orc.matmul(a[i, h], np.ascontiguousarray(b[i, h]), E, M, bA, np.array([bB], np.int32), bR, tab,
                                    int(flags), with_abs=True)
                bad = np.abs(c[i, h].astype(np.float64) - ref) > gio.sum_tolerance(S.astype(np.float64))
                assert not bad.any(), f"{name} item {i, h}: {np.count_nonzero(bad)} outside the bar"

    # the option is live, and off is what the model was without it
    off = _model(E, M, approx_attention=False)
    base = _model(E, M)
    _calibrate(off, xcal)
    _calibrate(base, xcal)
    with torch.no_grad():
        logits_off, logits_base = off(xev), base(xev)
    assert torch.equal(logits_off.view(torch.int32), logits_base.view(torch.int32))
    assert not torch.equal(logits_on, logits_off)


def test_forward_graph_replays_bit_identical():
    xcal, xev = _inputs()
    m = _model(4, 3, approx_attention=True)
    _calibrate(m, xcal)
    with torch.no_grad():
        eager = m(xev).clone()
        gs = torch.cuda.Stream()
        gs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(gs):
            for _ in range(2):
                m(xev)
        torch.cuda.current_stream().wait_stream(gs)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=gs, capture_error_mode="thread_local"):
            out = m(xev)
    for i in range(3):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), f"replay {i} differs from eager"


def test_validate_driver_records_the_option(tmp_path):
    """(No tiny ViT is selectable from the command line: vit_b16 at 32 x 32 pixels, 5 tokens.)"""
    from fp8_quantization_amd import imagenet as inet
    out = tmp_path / "res.json"
    inet.main(["--synthetic", "8", "--arch", "vit_b16", "--image-size", "32", "--batch-size", "4", "--num-workers", "0",
               "--approx-attention", "--output", str(out)])
    res = json.loads(out.read_text())
    assert res["images"] == 8 and res["approx_attention"] is True and res["approx_params"]["approx_attention"] is True
    assert np.isfinite(res["loss"])
