"""The approximate convolutions on non-square geometry against the oracle, bit for bit.

Every entry point takes kh, kw, sh, sw, ph, pw, dh, dw, H and W as separate numbers; every other GPU test gives the
approximate product the same number twice.  The cases here (tests/exact_sums.py: GEO_CONVS, GEO_TBDW) differ in
every pair, are drawn inside the exact-sum budget (proved per case by tests/test_exact_sums_cpu.py, which also
proves that each case tells an exchanged pair: another output shape, or half of the outputs differ), and are compared
with expected(oracle.terms(unfold rows, weights)) by bits through fp8a_conv2d with a caller-owned workspace:

  * the implicit-GEMM paths: 11 geometries (H != W with W % 4 == 0 and != 0, 1 x 7 / 7 x 1, stride / padding /
    dilation that differ by direction, even kw with groups, padding wider than the kernel's reach and wider than the
    word image's aligned border, strided and padded 1 x 1, K = 64) on gemm_f8mx (E4M3, E5M2), gemm_tt (E2M5), E3M4
    (gemm_tt / gemm_tt16 by K), gemm_fast, gemm_v5mx and gemm_fast<TM_V5>; the 128 x 64 instances of gemm_f8mx
    (xm_ncg = 4, xm_wave_rows 0 / 1) on the widest M; the strided 1 x 1 with the fp32 staging and with the pre-pass.
    The path counter that moved is the one the dispatch rule names, flag word 0, no exact launch, no f32 rerun;
  * groups with one output channel (tensor-bias terms): 11 geometries (ph != pw, border wider than the kernel's
    reach, pw > 4, kh = 1 / 5 / 2 with dilated rows, 3 input channels per group, kw = 2, sh != sw) under the
    option sets of the depthwise 3 x 3 cases: the table forms on E4M3 and E5M2 (tbs 0 / 1 / 2, tbx_rw 1 / 2),
    conv_tb_fast_kernel (E3M4 / E2M5), conv_tb_direct_kernel (s2n off), the v5 forms (v5ds 0 / 1).  Gate word 0 and
    no direct-kernel launch behind a fast form; a v5 geometry without a word form asserts the `exact` counter;
  * the fused entry points on one or two of these geometries each: fp8a_conv2d_bn_act, fp8a_conv2d_qamaa, four
    fp8a_conv2d_chain pairs (producer and consumer both against the oracle); fp8a_conv2d_check's two rectangular
    cases are in tests/test_gpu_check.py::test_conv_check_equals_per_group_matmul_check.

Every case prints its `XS <case> path=... K=... budget=...` line (run with -s: profiles/conv_geometry/).
"""
import collections

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_sums as xs
from tests import pairs_cases as pc
from tests.test_gpu_exact_sums import _check_paths, _counted, _dense_log, _launch_conv, _log, _options, _prefetch
from tests.test_gpu_flag_matrix import _stop_on_device_error
from tests.test_gpu_tbx import _dw_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


def _by_name(cases, geo_of):
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault(geo_of(c)["name"], []).append(c)
    return out


def _nhwc_rows(y):
    return y.transpose(0, 2, 3, 1).reshape(-1, y.shape[1])


# ------------------------------------------------------------------------------------------ implicit GEMM
CONV = _by_name(xs.geo_conv_cases(), lambda c: c["cfg"])


@pytest.mark.parametrize("name", list(CONV), ids=list(CONV))
def test_conv_geometry_bit_exact(name):
    cases = CONV[name]
    probs = _prefetch(cases)
    cfg = cases[0]["cfg"]
    Ho, Wo = xs.conv_out_hw(cfg)
    for c in cases:
        p = probs[c["pkey"]]
        (y, flag), paths, fb, _ = _launch_conv(c, p)
        _log(c, p, paths, flag)
        assert y.shape == (cfg["B"], cfg["cout"], Ho, Wo), y.shape
        got = _nhwc_rows(y)
        for (_, _, T, sl) in p["parts"]:
            xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)
        _check_paths(c, paths, flag, fb, xs.case_K(c))


def test_all_padding_outputs_are_exact_zeros():
    """pad-wide: the padding reaches beyond the kernel, so the outer output rows and columns see padding alone.  The
    v9 families give them as zeros (a product with a zero operand is zero); so does the oracle."""
    cfg = next(g for g in xs.GEO_CONVS if g["name"] == "pad-wide")
    (ph, pw), (kh, kw) = cfg["p"], cfg["k"]
    cases = [c for c in CONV["pad-wide"] if not c["flags"] & pc.V5]
    probs = _prefetch(cases)
    for c in cases:
        p = probs[c["pkey"]]
        (y, _), _, _, _ = _launch_conv(c, p)
        rows, cols = ph - kh + 1, pw - kw + 1             # output rows / columns whose window ends before the plane
        assert rows == 1 and cols == 3
        outer = np.ones(y.shape[2:], bool)
        outer[rows:-rows, cols:-cols] = False
        assert np.all(y[:, :, outer] == 0), f"{c['id']}: an all-padding output is not zero"
        assert np.mean(y[:, :, ~outer] != 0) > 0.9, f"{c['id']}: the inner outputs are mostly zero"


# ------------------------------------------------------------------------------------------ one output channel per group
TBDW = _by_name(xs.geo_tbdw_cases(), lambda c: c["geo"])


@_stop_on_device_error
def _launch_tb(c, p):
    g = c["geo"]
    with _options(c["opts"]):
        return _counted(lambda: _dw_raw(p["x"], p["w"], p["bA"], p["bB"], p["bR"], p["table"], c["flags"], g["s"], g["p"],
                                        fmt=(c["E"], c["M"]), dil=g["d"], groups=g["g"]))


@pytest.mark.parametrize("name", list(TBDW), ids=list(TBDW))
def test_tensor_bias_geometry_bit_exact(name):
    """Each option set against the oracle itself (the library has no counter that names the tensor-bias form, so
    none is compared with another): every channel equals the sum of its tensor-bias terms."""
    cases = TBDW[name]
    probs = _prefetch(cases)
    geo = cases[0]["geo"]
    for c in cases:
        p = probs[c["pkey"]]
        (y, gate), paths, fb, _ = _launch_tb(c, p)
        ran = "+".join(k for k, v in paths.items() if v) or "none"
        _dense_log(c, p, f"{ran},gate={gate},tb_launches={fb['tb_launches']}")
        got = _nhwc_rows(y)
        for (_, _, T, sl) in p["parts"]:
            xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)
        assert gate == 0 and fb["tb_launches"] == 0 and fb["exact_launches"] == 0, f"{c['id']}: gate {gate}, {fb}"
        want = dict.fromkeys(paths, 0)
        if c["fam"] == "v5dw":  # the word forms count as `fast`; a geometry they do not take runs the literal kernel
            want["fast" if xs.v5dw_word_form(geo) else "exact"] = 1
        assert paths == want, f"{c['id']}: counters say {paths}"


# ------------------------------------------------------------------------------------------ fused entry points
def _first(cases, name, E, M):
    return next(c for c in cases[name] if (c["E"], c["M"]) == (E, M) and not c["flags"] & pc.V5)


@pytest.mark.parametrize("act", ["none", "relu6"])
@pytest.mark.parametrize("name", ["dense-geo", "dw-p1x0-s2"])
def test_fused_bn_act_on_geometry(name, act):
    """fp8a_conv2d_bn_act: test_gpu_fused_bn.py's comparison (the fused store against the unfused output pushed
    through y * scale + shift and the clamp, within one fp32 rounding) on a rectangular implicit GEMM and a
    rectangular depthwise layer; the unfused output is the oracle's, by bits."""
    from tests.test_gpu_fused_bn import _check
    conv = name in CONV
    c = _first(CONV if conv else TBDW, name, 4, 3)
    g = c["cfg"] if conv else c["geo"]
    p = xs.problem(c["id"])
    try:
        y0, _ = _check(p["x"], p["w"], c["E"], c["M"], p["bA"], np.asarray(p["bB"], np.int32), p["bR"], p["table"],
                       c["flags"], act, 21, stride=xs.pair(g["s"]), padding=xs.pair(g["p"]), dilation=xs.pair(g["d"]),
                       groups=g["g"])
    except RuntimeError as ex:
        pytest.exit(f"device error in fp8a_conv2d_bn_act: {ex}", returncode=3)
    got = _nhwc_rows(y0)
    for (_, _, T, sl) in p["parts"]:
        xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)


@pytest.mark.parametrize("cid", [c["id"] for c in xs.chain_cases()])
def test_chained_pairs_on_geometry(cid):
    """fp8a_conv2d_chain with a rectangular producer and consumer: (a) 3 x 3 on 9 x 16 into a 1 x 7 matrix-core
    consumer, (b) into a depthwise 3 x 3, padding (0, 1), table-form consumer, (c) a staged depthwise producer into a
    1 x 1 consumer, (d) the v5 word form.  The producer's output is the oracle's with and without the emission, the
    image comes back valid and has the size of the layout comment, the consumer gives the same bits and the same
    input-quantizer bias from the image and from y, and those bits are the oracle's."""
    from fp8_quantization_amd.approx_ops import approx_conv2d, new_word_image, word_image_bytes
    c = next(v for v in xs.chain_cases() if v["id"] == cid)
    p = xs.chain_problem(c)
    pp, pc_, pg, geo, E, M = p["producer"], p["pcase"], p["pgeo"], p["geo"], c["E"], c["M"]
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    tab = torch.from_numpy(np.ascontiguousarray(p["table"], np.int32))
    x, w1, bW1, w2, bW2 = dev(pp["x"]), dev(pp["w"]), dev(pp["bB"], torch.int32), dev(p["w"]), dev(p["bB"], torch.int32)
    bR2 = torch.tensor([p["bR"]], dtype=torch.int32, device=DEV)
    qin2 = (torch.tensor([c["mx"]], device=DEV), 8, M, 1)
    args1 = dict(flags=pc_["flags"], stride=xs.pair(pg["s"]), padding=xs.pair(pg["p"]), dilation=xs.pair(pg["d"]),
                 groups=pg["g"])
    args2 = dict(flags=c["flags"], padding=tuple(c["p"]), groups=c["g"])
    Bn, cmid, (Ho, Wo) = pg["B"], pg["cout"], geo["hw"]
    ipad = (0, 0) if c["form"] == 1 else tuple(c["p"])     # (the table form's image has no border)
    assert word_image_bytes(Bn, cmid, Ho, Wo, *ipad) == xs.word_image_bytes(Bn, cmid, Ho, Wo, *ipad)
    try:
        y = approx_conv2d(x, w1, E, M, pp["bA"], bW1, pp["bR"], tab, **args1)
        z, ib, _ = approx_conv2d(y, w2, E, M, None, bW2, bR2, tab, qin=qin2, **args2)
        img = new_word_image(Bn, cmid, Ho, Wo, *ipad, DEV)
        y2 = approx_conv2d(x, w1, E, M, pp["bA"], bW1, pp["bR"], tab,
                           chain=(None, (img, tuple(c["p"]), qin2, bR2, M, c["form"])), **args1)[0]
        z2, ib2, _ = approx_conv2d(y2, w2, E, M, None, bW2, bR2, tab, qin=qin2, chain=(img, None), **args2)
        torch.cuda.synchronize()
        header = int(img[:4].view(torch.int32).item())
        y, y2, z, z2, ib, ib2 = (t.cpu().numpy() for t in (y, y2, z, z2, ib, ib2))
    except RuntimeError as ex:
        pytest.exit(f"device error in fp8a_conv2d_chain: {ex}", returncode=3)
    print(f"XS {cid} path=chain,header={header} K={p['parts'][0][0].shape[1]} budget=2^{xs.case_budget_log2(p):.2f}")
    xs.assert_same(y, p["y"], f"{cid}: the producer's y")
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), "producer output changed by the emission"
    assert header == 0, "the emitted image was flagged invalid"
    assert np.array_equal(z.view(np.uint32), z2.view(np.uint32)), "consumer output differs with the word image"
    assert np.array_equal(ib, ib2) and int(ib.reshape(-1)[0]) == p["bA"], (ib, ib2, p["bA"])
    got = _nhwc_rows(z)
    for (_, _, T, sl) in p["parts"]:
        xs.assert_same(got[:, sl], xs.expected(T), f"{cid}: the consumer's z", T)


def test_chain_helper_takes_pairs():
    """tests/test_gpu_chain.py::_run_pair with pair-valued hw, k and p: pair (a) on its own data, E4M3 and E5M2."""
    from tests.test_gpu_chain import _bits, _run_pair
    for (E, M) in ((4, 3), (5, 2)):
        z, z2, (ib, ib2), header, _ = _run_pair(E, M, cin=8, cmid=24, cout=20, hw=(9, 16), Bn=2, k1=(3, 3), k2=(1, 7),
                                                p1=(1, 1), p2=(0, 3), epilogue=True, post=False, seed=13)
        assert header == 0, "the emitted image was flagged invalid"
        assert torch.equal(_bits(z), _bits(z2)) and torch.equal(ib, ib2)


def test_qamaa_conv_geometry_bit_exact():
    """fp8a_conv2d_qamaa on k3x2-g2 against oracle.matmul_qamaa on each group's unfolded rows, by bits (the inner
    terms meet the budget, as test_gpu_exact_sums.py::test_qamaa_bit_exact)."""
    from fp8_quantization_amd import approx_ops as ops
    c = xs.QAMAA_CONV
    g, p = c["geo"], xs.problem(c["id"])
    try:
        y = ops.qamaa_conv2d(torch.from_numpy(p["x"]).to(DEV), torch.from_numpy(p["w"]).to(DEV),
                             torch.tensor([c["maxval"]], device=DEV), 8, c["M"], stride=g["s"], padding=g["p"],
                             dilation=g["d"], groups=g["g"]).cpu().numpy()
    except RuntimeError as ex:
        pytest.exit(f"device error in fp8a_conv2d_qamaa: {ex}", returncode=3)
    _dense_log(c, p, "qamaa")
    assert y.shape == (g["B"], g["cout"]) + xs.conv_out_hw(g)
    got = _nhwc_rows(y)
    distinct = 0
    for (A, B, T, sl) in p["parts"]:
        want, pre = orc.matmul_qamaa(A, B, c["maxval"], 8, c["M"])
        xs.assert_same(pre, xs.expected(T), "oracle.matmul_qamaa's sums", T)
        xs.assert_same(got[:, sl], want, c["id"])
        distinct += np.unique(want).size
    assert distinct > 50, "the final quantizer left too few distinct values to tell sums apart"
