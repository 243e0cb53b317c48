"""The batch statistics (fp8a_bn_train, csrc/bn_train.h) and the MSE candidate search (fp8a_fp8_mse_search,
csrc/fq_mse.h) on shapes that give a workgroup SEVERAL tiles: tests/reduce_plan.py has the cases, and
tests/test_reduce_plan_cpu.py proves without a GPU that each reaches its branch -- the tile loop's later
iterations, the uneven [t0, t1) split, a ragged tile at the end of a several-tile part, wsum accumulating across
tiles, parts == 1, the lin kernel's flat range over more than one tile, bn_apply_kernel's later grid-stride
iterations -- and that a kernel with one index error in it lands 100 bars or more outside.

The bars are the older files', unchanged:
  BN   S1 / S2 / S3 / A1 / A2 / D of tests/test_gpu_bn_train.py (dm, dv, ds, dsh, ulp32 restated in numpy by
       reduce_plan.py, pinned to that file's case() by the CPU file);
  MSE  T1 / T3 of tests/test_gpu_mse.py with its B = kernel_bound(); "mse_group" 0 and 1 and a repeated call give
       identical bytes.
Nothing here is measured: a failure means a kernel or a derivation is wrong.  A HIP error ends the session.
"""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from tests import reduce_plan as rp
from tests.test_gpu_mse import B, WIDTHS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U, EPS = rp.U, rp.EPS
BN_IDS, MSE_IDS = list(rp.BN_CASES), list(rp.MSE_CASES)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _stop_on_device_error(fn):
    """A HIP error (not a wrong value) ends the session: nothing more is started on a device that faulted."""
    @functools.wraps(fn)
    def run(*args, **kw):
        try:
            return fn(*args, **kw)
        except RuntimeError as ex:
            pytest.exit(f"device error in {fn.__name__}: {ex}", returncode=3)
    return run


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ BN
def bn_run(cid, momentum=1.0, rm=None, rv=None, **kw):
    from fp8_quantization_amd.approx_ops import bn_train
    c = rp.bn_case(cid)
    x = torch.from_numpy(c["x"]).to(DEV)
    r = bn_train(x, torch.from_numpy(c["gamma"]).to(DEV), torch.from_numpy(c["beta"]).to(DEV), rm, rv, momentum, EPS,
                 **kw)
    torch.cuda.synchronize()
    return r, x


def f64(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("cid", BN_IDS)
@_stop_on_device_error
def test_bn_statistics_against_float64(cid):
    """S1 / S2."""
    c = rp.bn_case(cid)
    (y, sm, sv, ss, qb), _ = bn_run(cid)
    assert qb is None and tuple(y.shape) == c["shape"]
    sm, sv, ss = f64(sm), f64(sv), f64(ss)
    pairs = rp.bn_errors_over_bars(c, sm, sv, ss[:, 0], ss[:, 1])
    worst = [float((err / np.maximum(bar, 1e-300)).max()) for (err, bar) in pairs]
    print(f"S {cid}: err / bar  mean {worst[0]:.3g}  var {worst[1]:.3g}  scale {worst[2]:.3g}  shift {worst[3]:.3g}")
    for (err, bar), what in zip(pairs, ("save_mean", "save_var", "scale", "shift")):
        assert (err <= bar).all(), (cid, what, int((err > bar).sum()), int(np.argmax(err - bar)))
    # the constant channel: var = 0 exactly, scale = gamma / sqrt(eps); the zero channel
    assert sv[0] == 0.0 and sm[0] == -2.625 and sv[2] == 0.0 and sm[2] == 0.0
    assert abs(ss[0, 0] - float(c["gamma"][0]) / np.sqrt(EPS)) <= 2 * rp.ulp32(c["scale"][:1])[0]


@pytest.mark.parametrize("cid", BN_IDS)
@_stop_on_device_error
def test_bn_running_buffers(cid):
    """S3."""
    c = rp.bn_case(cid)
    n, C = c["n"], c["C"]
    unb = c["var"] * n / (n - 1)
    rm = torch.full((C,), 3.0, device=DEV)
    rv = torch.full((C,), 7.0, device=DEV)
    (_, sm, sv, _, _), _ = bn_run(cid, 1.0, rm, rv, stats_only=True)
    assert same(rm, sm)
    want = unb.astype(np.float32).astype(np.float64)
    assert (np.abs(f64(rv) - want) <= rp.ulp32(want)).all()
    rng = np.random.default_rng(5)
    rm0, rv0 = rng.standard_normal(C, dtype=np.float32), rng.random(C, dtype=np.float32) + np.float32(0.5)
    rm, rv = torch.from_numpy(rm0).to(DEV), torch.from_numpy(rv0).to(DEV)
    m = float(np.float32(0.1))
    bn_run(cid, 0.1, rm, rv, stats_only=True)
    wm = (1 - m) * rm0.astype(np.float64) + m * c["mean"]
    wv = (1 - m) * rv0.astype(np.float64) + m * unb
    assert (np.abs(f64(rm) - wm) <= rp.ulp32(wm) + m * c["dm"]).all()
    assert (np.abs(f64(rv) - wv) <= rp.ulp32(wv) + m * c["dv"] * n / (n - 1)).all()


@pytest.mark.parametrize("cid", BN_IDS)
@_stop_on_device_error
def test_bn_apply_every_element(cid):
    """A1 over every element, from the kernel's returned fp32 scale / shift: the later grid-stride iterations and
    their (idx / inner) % C.  A2 on bn-vec-uneven."""
    from fp8_quantization_amd.approx_ops import bn_train, fp8_fake_quantize
    c = rp.bn_case(cid)
    pl = c["plan"]
    (y, _, _, ss, _), xd = bn_run(cid)
    ss64 = f64(ss)
    x3 = c["x"].reshape(pl["N"], pl["C"], pl["inner"])
    y3 = y.cpu().numpy().reshape(x3.shape)
    worst = 0.0
    for c0 in range(0, pl["C"], rp.CHUNK):
        c1 = min(c0 + rp.CHUNK, pl["C"])
        t = x3[:, c0:c1].astype(np.float64) * ss64[None, c0:c1, 0, None] + ss64[None, c0:c1, 1, None]
        err = np.abs(y3[:, c0:c1] - t)
        bar = U * np.abs(t) * (1 + 2.0 ** -20) + 2.0 ** -150
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (cid, c0, int((err > bar).sum()))
    print(f"A1 {cid}: apply err / bar {worst:.3g} over {y3.size} elements")
    if cid != "bn-vec-uneven":
        return
    (yc, _, _, ss2, _), _ = bn_run(cid, activation=nn.ReLU6())
    assert same(ss2, ss) and same(yc, torch.clamp(y, 0.0, 6.0))
    mx = torch.tensor([2.5], device=DEV)
    kw = dict(activation=nn.ReLU6(), out_quantizer=(mx, 8, 3, 1))
    (yq, _, _, _, qb), _ = bn_run(cid, **kw)
    want, wb = fp8_fake_quantize(yc, mx, 8, 3, sign_bits=1)
    assert same(yq, want) and same(qb, wb) and torch.equal(qb._fp8a_i32, wb._fp8a_i32)
    r = bn_train(xd, torch.from_numpy(c["gamma"]).to(DEV), torch.from_numpy(c["beta"]).to(DEV), None, None, 1.0, EPS,
                 out=xd, **kw)
    assert r[0].data_ptr() == xd.data_ptr() and same(r[0], yq) and same(r[3], ss)


@pytest.mark.parametrize("cid", BN_IDS)
@_stop_on_device_error
def test_bn_two_calls_identical_bytes(cid):
    """D."""
    C = rp.bn_case(cid)["C"]
    mx = torch.tensor([3.0], device=DEV)
    outs = []
    for _ in range(2):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        r, _ = bn_run(cid, 0.1, rm, rv, activation=nn.ReLU(), out_quantizer=(mx, 8, 3, 1))
        outs.append(list(r) + [rm, rv])
    for a, b in zip(*outs):
        assert same(a, b)


# ------------------------------------------------------------------------------------------ MSE
_INPUTS = {}


def mse_input(cid):
    if cid not in _INPUTS:
        from fp8_quantization_amd.quantization import mse_search_grid
        c = rp.mse_case(cid)
        xt = torch.from_numpy(c["x"]).to(DEV)
        _INPUTS[cid] = (xt, mse_search_grid(xt, c["shape"][0] > 1))
    return _INPUTS[cid]


def literal_sse(cid, sign_bits):
    """float64 sums of the literal fp32 terms, [n_mbits][n_cand][rows]."""
    from fp8_quantization_amd.approx_ops import fp8_fake_quantize
    x, grid = mse_input(cid)
    rows = x.shape[0]
    widths = WIDTHS[rp.MSE_CASES[cid]["widths"]]
    out = torch.empty((len(widths), grid.shape[0], rows), dtype=torch.float64, device=DEV)
    for m, M in enumerate(widths):
        for i in range(grid.shape[0]):
            q, _ = fp8_fake_quantize(x, grid[i], 8, M, sign_bits=sign_bits, per_row=rows > 1)
            out[m, i] = ((x - q) ** 2).double().sum(1)
    return out.cpu().numpy()


def fused_sse(cid, sign_bits):
    from fp8_quantization_amd.approx_ops import fp8_mse_losses
    x, grid = mse_input(cid)
    return fp8_mse_losses(x, grid, WIDTHS[rp.MSE_CASES[cid]["widths"]], 8, sign_bits, x.shape[0] > 1).cpu().numpy()


@pytest.mark.parametrize("sign_bits", [1, 0])
@pytest.mark.parametrize("cid", MSE_IDS)
@_stop_on_device_error
def test_mse_kernel_matches_literal_terms(cid, sign_bits):
    """T1; "mse_group" 0 and 1 and two calls of each: identical bytes."""
    from fp8_quantization_amd import _lib
    want = literal_sse(cid, sign_bits)
    old = _lib.set_option("mse_group", 0)
    try:
        a, a2 = fused_sse(cid, sign_bits), fused_sse(cid, sign_bits)
        _lib.set_option("mse_group", 1)
        g, g2 = fused_sse(cid, sign_bits), fused_sse(cid, sign_bits)
    finally:
        _lib.set_option("mse_group", old)
    assert a.shape == want.shape and a.dtype == np.float64
    assert np.isfinite(want).all() and (want > 0).all()
    err = np.abs(a - want)
    worst = float((err / want).max())
    print(f"T1 {cid} sign_bits={sign_bits}: worst relative error {worst:.3g}, bar {B:.3g}")
    assert (err <= B * want).all(), worst
    assert a.tobytes() == a2.tobytes() and g.tobytes() == g2.tobytes()
    assert a.tobytes() == g.tobytes()


@pytest.mark.parametrize("unsigned", [False, True])
@_stop_on_device_error
def test_mse_tensor_estimator_fused_and_literal_pick_identically(unsigned):
    """T3 on mse-tensor (unsigned: |x| with allow_unsigned, so the estimator drops the sign bit)."""
    from fp8_quantization_amd.quantization import FPQuantizer, RangeEstimators
    x, _ = mse_input("mse-tensor")
    x = x.abs() if unsigned else x
    picks = []
    for fused in (True, False):
        q = FPQuantizer(n_bits=8, per_channel=False, mantissa_bits=3, maxval=None, set_maxval=True,
                        mse_include_mantissa_bits=False, allow_unsigned=unsigned)
        est = RangeEstimators.MSE.cls(per_channel=False, quantizer=q, fused=fused)
        lo, hi = est(x)
        picks.append((q._mbits_int, int(q.sign_bits), hi.cpu().numpy().tobytes(), lo.cpu().numpy().tobytes()))
        assert np.isfinite(est.mses.cpu().numpy()).all() and est.mses.shape == (1, 111, 1)
    assert picks[0][1] == (0 if unsigned else 1)
    assert picks[0] == picks[1], (picks[0][:2], picks[1][:2], np.frombuffer(picks[0][2], np.float32),
                                  np.frombuffer(picks[1][2], np.float32))
