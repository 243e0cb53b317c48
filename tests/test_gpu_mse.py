"""FP8 MSE range estimation on the GPU (fp8a_fp8_mse_search, csrc/fq_mse.h; FP_MSE_Estimator).

T1  the fused kernel's sse against a float64 sum of the literal fp32 terms
    (x - fp8_fake_quantize(x, grid[i]))^2, within B * sse.  B is derived, not tuned: an fp32 partial
    of the kernel covers L = MSE_L terms (csrc/fq_mse.h), all non-negative, so the standard summation
    bound gives a relative error of at most (L - 1) 2^-24 < L 2^-24; every later stage is in double
    (well under 2^12 additions on either side of the comparison: 2^-40 covers both).
T2  the fused estimator against the reference's FP_MSE_Estimator (tests/golden/mse_cases.npz): mses
    after every batch within (B + ref_dev) relative; picked width, maxval bits and final sign_bits
    exact; the zero row gives maxval 0 and NaN losses.
T3  fused and literal estimator paths pick identically; "mse_group" 0 and 1 give byte-identical
    sse; two calls give identical bytes.
T4  operator level: a QCustomBNConv2dTorch calibrated with MSE ranges (weights per channel,
    activations per tensor) gives the same approx forward bit for bit with the input quantizer
    fused and unfused, and its quantizers hold exactly the estimator's picks.
"""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["w8x3x3x3", "act2x5x7x7", "pc4x37", "two_batches", "unsigned", "zero_row"]
SHAPES = [(5, 27), (3, 4099), (1, 1_000_003), (2, 70_001)]
WIDTHS = {"m3": [3], "m1to6": [1, 2, 3, 4, 5, 6]}


def kernel_bound():
    src = open(os.path.join(ROOT, "fp8_quantization_amd", "csrc", "fq_mse.h")).read()
    v = int(re.search(r"constexpr int MSE_V = (\d+);", src).group(1))
    assert re.search(r"constexpr int MSE_L = MSE_V;", src)
    return v * 2.0 ** -24 + 2.0 ** -40


B = kernel_bound()


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "mse_cases.npz"))


_INPUTS = {}


def t1_input(shape):
    """x [rows][inner] with zeros, negatives and values above most candidates, and its grid."""
    if shape not in _INPUTS:
        from fp8_quantization_amd.quantization import mse_search_grid
        rows, inner = shape
        rng = np.random.default_rng(rows * 7919 + inner)
        x = rng.standard_normal(shape).astype(np.float32) * np.linspace(0.4, 3.0, rows, dtype=np.float32)[:, None]
        x[:, ::7] = 0.0
        top = np.abs(x).max(1)
        x[:, 3 % inner] = 0.97 * top          # above most of the 0.1 .. 1.2 max candidates
        x[:, 11 % inner] = -0.93 * top
        xt = torch.from_numpy(x).to(DEV)
        _INPUTS[shape] = (xt, mse_search_grid(xt, rows > 1))
    return _INPUTS[shape]


_LITERAL = {}


def literal_sse(shape, wkey, sign_bits):
    """float64 sums of the literal fp32 terms, [n_mbits][n_cand][rows] (computed once per case)."""
    key = (shape, wkey, sign_bits)
    if key not in _LITERAL:
        from fp8_quantization_amd.approx_ops import fp8_fake_quantize
        x, grid = t1_input(shape)
        rows = shape[0]
        out = torch.empty((len(WIDTHS[wkey]), grid.shape[0], rows), dtype=torch.float64, device=DEV)
        for m, M in enumerate(WIDTHS[wkey]):
            for i in range(grid.shape[0]):
                q, _ = fp8_fake_quantize(x, grid[i], 8, M, sign_bits=sign_bits, per_row=rows > 1)
                out[m, i] = ((x - q) ** 2).double().sum(1)
        _LITERAL[key] = out.cpu().numpy()
    return _LITERAL[key]


def fused_sse(shape, wkey, sign_bits):
    from fp8_quantization_amd.approx_ops import fp8_mse_losses
    x, grid = t1_input(shape)
    return fp8_mse_losses(x, grid, WIDTHS[wkey], 8, sign_bits, shape[0] > 1)


# ------------------------------------------------------------------------------------------ T1
@pytest.mark.parametrize("sign_bits", [1, 0])
@pytest.mark.parametrize("wkey", list(WIDTHS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_literal_terms(shape, wkey, sign_bits):
    want = literal_sse(shape, wkey, sign_bits)
    got = fused_sse(shape, wkey, sign_bits).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.isfinite(want).all() and (want > 0).any()
    err = np.abs(got - want)
    worst = float((err / np.maximum(want, 1e-300)).max())
    print(f"T1 {shape} {wkey} sign_bits={sign_bits}: worst relative error {worst:.3g}, bar {B:.3g}")
    assert (err <= B * want).all(), worst


# ------------------------------------------------------------------------------------------ T2 / T3
def run_estimator(cases, name, fused):
    from fp8_quantization_amd.quantization import FPQuantizer, RangeEstimators
    nb, per_channel, msearch, unsigned = (int(v) for v in cases[f"{name}/meta"][:4])
    q = FPQuantizer(n_bits=8, per_channel=bool(per_channel), mantissa_bits=3, maxval=None, set_maxval=True,
                    mse_include_mantissa_bits=bool(msearch), allow_unsigned=bool(unsigned))
    est = RangeEstimators.MSE.cls(per_channel=bool(per_channel), quantizer=q, fused=fused)
    mses = []
    for b in range(nb):
        lo, hi = est(torch.from_numpy(cases[f"{name}/x{b}"]).to(DEV))
        mses.append(est.mses.cpu().numpy().copy())
    return dict(mses=mses, lo=lo.cpu().numpy(), hi=hi.cpu().numpy(), grid=est.search_grid.cpu().numpy(),
                mbits=q._mbits_int, mbits_tensor=float(q.mantissa_bits), sign_bits=int(q.sign_bits))


_RUNS = {}


def estimator_run(cases, name, fused):
    if (name, fused) not in _RUNS:
        _RUNS[(name, fused)] = run_estimator(cases, name, fused)
    return _RUNS[(name, fused)]


@pytest.mark.parametrize("name", CASES)
def test_fused_estimator_matches_reference(cases, name):
    r = estimator_run(cases, name, True)
    meta = cases[f"{name}/meta"]
    assert r["grid"].tobytes() == cases[f"{name}/search_grid"].tobytes()
    bar = B + float(cases[f"{name}/ref_dev"][0])
    for b, got in enumerate(r["mses"]):
        want = cases[f"{name}/mses{b}"]
        assert got.shape == want.shape
        assert (np.isnan(got) == np.isnan(want)).all()
        ok = ~np.isnan(want)
        rel = np.abs(got[ok].astype(np.float64) - want[ok]) / want[ok]
        print(f"T2 {name} batch {b}: worst relative deviation {float(rel.max()):.3g}, bar {bar:.3g}")
        assert (rel <= bar).all(), float(rel.max())
    assert r["mbits"] == int(meta[4]) and r["mbits_tensor"] == float(meta[4])
    assert r["sign_bits"] == int(meta[5])
    assert r["hi"].astype(np.float32).tobytes() == cases[f"{name}/maxval"].tobytes()
    assert np.array_equal(r["lo"].astype(np.float32), cases[f"{name}/xmin"])
    if name == "zero_row":
        assert r["hi"][1] == 0.0 and np.isnan(r["mses"][-1][:, :, 1]).all()
        assert np.isfinite(r["mses"][-1][:, :, [0, 2]]).all()


@pytest.mark.parametrize("name", CASES)
def test_fused_and_literal_paths_pick_identically(cases, name):
    f, lit = estimator_run(cases, name, True), estimator_run(cases, name, False)
    assert f["mbits"] == lit["mbits"] and f["sign_bits"] == lit["sign_bits"]
    assert f["hi"].tobytes() == lit["hi"].tobytes() and np.array_equal(f["lo"], lit["lo"])
    assert f["grid"].tobytes() == lit["grid"].tobytes()
    # the literal path is the reference's loop over this project's quantizer: it meets the fixture too
    assert lit["mbits"] == int(cases[f"{name}/meta"][4])
    assert lit["hi"].astype(np.float32).tobytes() == cases[f"{name}/maxval"].tobytes()


@pytest.mark.parametrize("sign_bits", [1, 0])
@pytest.mark.parametrize("wkey", list(WIDTHS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grouped_form_and_repeat_are_byte_identical(shape, wkey, sign_bits):
    from fp8_quantization_amd import _lib
    old = _lib.set_option("mse_group", 0)
    try:
        a = fused_sse(shape, wkey, sign_bits).cpu().numpy().tobytes()
        a2 = fused_sse(shape, wkey, sign_bits).cpu().numpy().tobytes()
        _lib.set_option("mse_group", 1)
        g = fused_sse(shape, wkey, sign_bits).cpu().numpy().tobytes()
        g2 = fused_sse(shape, wkey, sign_bits).cpu().numpy().tobytes()
    finally:
        _lib.set_option("mse_group", old)
    assert a == a2 and g == g2
    assert a == g


def test_rejects_cpu_tensors():
    from fp8_quantization_amd.approx_ops import fp8_mse_losses
    with pytest.raises(RuntimeError):
        fp8_mse_losses(torch.randn(4, 8), torch.ones(111, 1), [3], 8, 1, False)


# ------------------------------------------------------------------------------------------ T4
def test_operator_calibrated_with_mse_fused_equals_unfused_input_quantizer():
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    from fp8_quantization_amd.quantization import FP_MSE_Estimator, QuantizationHijacker, mse_select
    from fp8_quantization_amd.resnet_workload import approx_qparams
    qp = approx_qparams(weight_range_method="MSE", act_range_method="MSE")
    assert qp["weight_range_method"] is FP_MSE_Estimator and qp["act_range_method"] is FP_MSE_Estimator
    torch.manual_seed(3)
    m = QCustomBNConv2dTorch(in_channels=8, out_channels=8, kernel_size=3, padding=1, bias=False,
                             activation=torch.nn.ReLU(), **qp)
    with torch.no_grad():
        m.running_mean.normal_(0, 0.3)
        m.running_var.uniform_(0.3, 2.0)
        m.gamma.normal_(1, 0.2)
        m.beta.normal_(0, 0.2)
    m = m.to(DEV).eval()
    m.quantized()
    m.estimate_ranges()
    x = torch.randn(2, 8, 8, 8, device=DEV)
    with torch.no_grad():
        m(x)
    m.fix_ranges()
    # the quantizers hold exactly the estimator's picks
    for mgr, rows in ((m.weight_quantizer, 8), (m.activation_quantizer, 1), (m.res_quantizer, 1)):
        est, q = mgr.range_estimator, mgr.quantizer
        assert isinstance(est, FP_MSE_Estimator) and est.mses.shape == (1, 111, rows)
        mb, mx = mse_select(est.mses, est.search_grid, [3.0])
        assert mb == 3.0 and q._mbits_int == 3
        assert q.maxval.reshape(-1).cpu().numpy().tobytes() == mx.cpu().numpy().tobytes()
        assert torch.equal(est.current_xmax.reshape(-1), q.maxval.reshape(-1))
    # MSE clamps: the weight ranges lie below the channels' largest |w|
    w, _ = m.get_weight_bias()
    assert bool((m.weight_quantizer.quantizer.maxval.reshape(-1) < w.detach().abs().reshape(8, -1).amax(1)).any())
    old = QuantizationHijacker.fuse_input_quant
    try:
        with torch.no_grad():
            QuantizationHijacker.fuse_input_quant = True
            assert m._fused_input_quantizer(m._qa()) is not None
            y1 = m(x).cpu().numpy()
            QuantizationHijacker.fuse_input_quant = False
            assert m._fused_input_quantizer(m._qa()) is None
            y0 = m(x).cpu().numpy()
    finally:
        QuantizationHijacker.fuse_input_quant = old
    assert np.isfinite(y0).all() and y1.tobytes() == y0.tobytes()
