"""FP8 MSE range estimation, the host side (no GPU): the selection and grid construction against
the reference's fixture (tests/golden/mse_cases.npz), the C-ABI's argument checks, the Python
surface (RangeEstimators.MSE, FPQuantizer.mantissa_bits, approx_qparams, the imagenet flags) and
the mantissa width's broadcast.
"""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fp8_quantization_amd import _lib

CASES = ["w8x3x3x3", "act2x5x7x7", "pc4x37", "two_batches", "unsigned", "zero_row"]


@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(os.path.join(golden_dir, "mse_cases.npz"))


def test_fixture_has_every_case(cases):
    for name in CASES:
        nb = int(cases[f"{name}/meta"][0])
        assert all(f"{name}/x{b}" in cases and f"{name}/mses{b}" in cases for b in range(nb))
        assert 0 < float(cases[f"{name}/ref_dev"][0]) < 1e-5
    assert int(cases["two_batches/meta"][0]) == 2 and int(cases["unsigned/meta"][0]) == 2
    # the second batch exceeds the grid the first one defined
    assert np.abs(cases["two_batches/x1"]).max() > cases["two_batches/search_grid"].max()
    assert (cases["unsigned/x0"] >= 0).all() and (cases["unsigned/x1"] < 0).any()
    assert int(cases["unsigned/meta"][5]) == 0          # sign_bits stays 0
    assert (cases["zero_row/x0"][1] == 0).all() and cases["zero_row/maxval"][1] == 0.0
    assert np.isnan(cases["zero_row/mses0"][:, :, 1]).all()


@pytest.mark.parametrize("name", CASES)
def test_selection_reproduces_the_reference_pick(cases, name):
    from fp8_quantization_amd.quantization import mse_select
    meta = cases[f"{name}/meta"]
    nb, msearch = int(meta[0]), int(meta[2])
    mbit_list = [float(m) for m in range(1, 7)] if msearch else [3.0]
    mses = torch.from_numpy(cases[f"{name}/mses{nb - 1}"])
    grid = torch.from_numpy(cases[f"{name}/search_grid"])
    assert mses.shape == (len(mbit_list),) + tuple(grid.shape)
    mbits, maxval = mse_select(mses, grid, mbit_list)
    assert mbits == float(meta[4])
    assert maxval.numpy().tobytes() == cases[f"{name}/maxval"].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_grid_matches_the_reference_bit_for_bit(cases, name):
    from fp8_quantization_amd.quantization import mse_search_grid
    per_channel = bool(cases[f"{name}/meta"][1])
    grid = mse_search_grid(torch.from_numpy(cases[f"{name}/x0"]), per_channel)
    assert grid.dtype == torch.float32 and grid.shape[0] == 111
    assert grid.numpy().tobytes() == cases[f"{name}/search_grid"].tobytes()


def test_workspace_query_is_host_only_and_rejects_bad_arguments():
    L = _lib.load()
    f = L.fp8a_fp8_mse_workspace_size
    a = f(1, 1_000_003, 111, 6)
    assert a > 0 and f(1, 1_000_003, 111, 1) < a
    assert f(8, 27, 111, 1) == 8 * 111 * (16 + 8)          # one part per row: candidates + doubles
    assert f(512, 4608, 111, 6) > f(512, 4096, 111, 6)     # a second tile: a second part per row
    for bad in ((0, 10, 111, 1), (1, 0, 111, 1), (-1, 10, 111, 1), (1, 10, 0, 1), (1, 10, 111, 0),
                (1, 10, 111, 8), (1, 10, 200, 6)):
        assert f(*bad) == 0, bad


def _search(L, rows=1, inner=100, n_cand=111, mbits=(3,), n_mbits=None, n_bits=8, sign_bits=1, ws_bytes=None,
            null_mbits=False):
    arr = (ctypes.c_int32 * max(len(mbits), 1))(*mbits)
    n_mbits = len(mbits) if n_mbits is None else n_mbits
    if ws_bytes is None:
        ws_bytes = L.fp8a_fp8_mse_workspace_size(rows, inner, n_cand, n_mbits)
    # every device pointer NULL: a call that passed the checks could only fail, never launch
    return L.fp8a_fp8_mse_search(None, rows, inner, None, n_cand, None if null_mbits else ctypes.cast(arr, ctypes.c_void_p),
                                 n_mbits, n_bits, sign_bits, None, None, ws_bytes, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(rows=0), "shape"), (dict(inner=0), "shape"), (dict(n_cand=0), "shape"), (dict(n_cand=400, mbits=(1, 2, 3)), "shape"),
    (dict(mbits=(1, 2, 3, 4, 5, 6, 7, 7), sign_bits=0), "shape"), (dict(mbits=(), n_mbits=0), "shape"),
    (dict(mbits=(0,)), "width"), (dict(mbits=(3, 8)), "width"), (dict(mbits=(8,), sign_bits=0, ws_bytes=1 << 20), None),
    (dict(mbits=(8,), sign_bits=1), "width"), (dict(sign_bits=2), "format"), (dict(null_mbits=True), "null"),
    (dict(ws_bytes=16), "workspace"), (dict(), "null"),
])
def test_search_rejects_bad_arguments_before_any_launch(kw, msg):
    L = _lib.load()
    rc = _search(L, **kw)
    assert rc == _lib.EINVAL
    if msg:
        assert msg in L.fp8a_last_error().decode()
    else:   # width 8 is legal without a sign bit: the call gets as far as the pointer check
        assert "pointer" in L.fp8a_last_error().decode()


def test_mse_constructs_through_the_manager():
    from fp8_quantization_amd.quantization import (FP_MSE_Estimator, FPQuantizer, OptMethod, QuantizationManager,
                                                   RangeEstimators)
    assert RangeEstimators.MSE.cls is FP_MSE_Estimator
    mgr = QuantizationManager(qmethod=FPQuantizer, init=RangeEstimators.MSE.cls, per_channel=True,
                              qparams=dict(n_bits=8, mantissa_bits=3, set_maxval=True),
                              range_estim_params=dict(num_candidates=100, opt_method=OptMethod.grid, range_margin=0.5))
    est = mgr.range_estimator
    assert isinstance(est, FP_MSE_Estimator) and est.per_channel and est.quantizer is mgr.quantizer
    assert est.fused and est.num_candidates == 100 and est.mses is None and est.search_grid is None
    with pytest.raises(AssertionError):
        FP_MSE_Estimator(opt_method=OptMethod.golden_section, quantizer=mgr.quantizer)


def test_mantissa_bits_assignment_changes_the_width_forward_hands_down(monkeypatch):
    from fp8_quantization_amd.quantization import FPQuantizer
    from fp8_quantization_amd.quantization import fp8_quantizer as fq
    seen = []

    def fake(x, maxval, n_bits, M, sign_bits=1, per_row=False):
        seen.append((M, sign_bits))
        return x, torch.zeros(1)

    monkeypatch.setattr(fq, "fp8_fake_quantize", fake)
    q = FPQuantizer(n_bits=8, mantissa_bits=3)
    x = torch.randn(4)
    q(x)
    assert isinstance(q.mantissa_bits, torch.Tensor) and float(q.mantissa_bits) == 3.0 and q._mbits_int == 3
    q.mantissa_bits = torch.tensor(5.0)            # what the estimator stores (a 0-dim tensor)
    q(x)
    q.mantissa_bits = torch.Tensor([2.0])
    q(x)
    q.mantissa_bits = 4
    q(x)
    assert [s[0] for s in seen] == [3, 5, 2, 4] and float(q.mantissa_bits) == 4.0
    q.sign_bits = 0
    q.mantissa_bits = torch.Tensor([9.0])          # clamped to n_bits - sign_bits, as the reference rounds and clamps
    q(x)
    assert seen[-1] == (8, 0)
    assert "mantissa_bits=9" in q.extra_repr()


def test_approx_qparams_defaults_are_unchanged_and_methods_map():
    from fp8_quantization_amd.quantization import FPQuantizer, RangeEstimators
    from fp8_quantization_amd.resnet_workload import approx_qparams
    today = dict(
        method=FPQuantizer, act_method=FPQuantizer, n_bits=8, n_bits_act=8, per_channel_weights=True,
        weight_range_method=RangeEstimators.current_minmax.cls, weight_range_options={},
        act_range_method=RangeEstimators.allminmax.cls, act_range_options={}, quantize_input=True,
        fp8_kwargs=dict(maxval=None, mantissa_bits=3, set_maxval=True, learn_maxval=False,
                        learn_mantissa_bits=False, mse_include_mantissa_bits=False, allow_unsigned=False),
        custom_approx_params=dict(expo_width=4, mant_width=3, dnsmp_factor=3, withComp=False, with_approx=True,
                                  with_s2nn2s_opt=True, sim_hw_add_OFUF=False, with_OF_opt=False, with_UF_opt=False,
                                  golden_clip_OF=False, quant_btw_mult_accu=True, debug_mode=False,
                                  self_check_mode=False),
        run_method=dict(approx_flag=True, quantize_after_mult_and_add=False, res_quantizer_flag=True,
                        original_quantize_res=False))
    assert approx_qparams() == today
    qp = approx_qparams(weight_range_method="MSE", act_range_method="running_minmax",
                        act_range_options=dict(momentum=0.5), mse_include_mantissa_bits=True)
    assert qp["weight_range_method"] is RangeEstimators.MSE.cls
    assert qp["act_range_method"] is RangeEstimators.running_minmax.cls and qp["act_range_options"] == dict(momentum=0.5)
    assert qp["fp8_kwargs"]["mse_include_mantissa_bits"] is True
    rest = {k: v for k, v in qp.items() if k not in ("weight_range_method", "act_range_method", "act_range_options",
                                                     "fp8_kwargs")}
    assert rest == {k: today[k] for k in rest}


def test_imagenet_flags_reach_approx_qparams():
    from fp8_quantization_amd import imagenet
    from fp8_quantization_amd.resnet_workload import approx_qparams
    args = imagenet.parse(["--synthetic", "8"])
    cfg = imagenet.approx_cfg(args)
    assert approx_qparams(**cfg) == approx_qparams()
    args = imagenet.parse(["--synthetic", "8", "--weight-quant-method", "MSE", "--act-quant-method", "MSE",
                           "--fp8-mse-include-mantissa-bits"])
    cfg = imagenet.approx_cfg(args)
    assert approx_qparams(**cfg) == approx_qparams(weight_range_method="MSE", act_range_method="MSE",
                                                   mse_include_mantissa_bits=True)
    with pytest.raises(SystemExit):
        imagenet.parse(["--act-quant-method", "percentile"])


# ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, ws, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from fp8_quantization_amd.distributed import broadcast_quant_state
        from fp8_quantization_amd.quantization.fp8_quantizer import FPQuantizer
        holder = torch.nn.Module()
        holder.a = FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True)
        holder.b = FPQuantizer(n_bits=8, mantissa_bits=3, set_maxval=True)
        if rank == 0:   # calibration (the MSE vote) ran here alone
            holder.a.mantissa_bits = torch.tensor(5.0)
            holder.a.maxval = torch.tensor([0.75])
        broadcast_quant_state(holder, src=0)
        out.put((rank, holder.a._mbits_int, float(holder.a.mantissa_bits), holder.b._mbits_int,
                 float(holder.b.mantissa_bits), float(holder.a.maxval[0])))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_broadcast_carries_the_mantissa_width():
    ws = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, out)) for r in range(ws)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=120) for _ in range(ws))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, a_int, a_t, b_int, b_t, mx in res:
        assert (a_int, a_t, b_int, b_t, mx) == (5, 5.0, 3, 3.0, 0.75), rank
