"""K > 1 sums of every product path against the oracle, bit for bit (tests/exact_sums.py).

The every-code-pair tests pin each term at K = 1 or next to zeros; everything with K > 1 met the oracle only
within 1e-5 * sum|term|.  The cases here are drawn so that every partial sum of their terms, in any order, is
an exact float32 (max sum|T| <= 2^22 u, proved per case on the CPU by tests/test_exact_sums_cpu.py), so each
launch is compared with expected(oracle.terms) by bits (zeros by value), through the production entry points
with a caller-owned workspace, and the path counter that moved is the one the dispatch rule names:

  * matrix launches (fp8a_matmul; lda > K, B passed as W^T, bB per column) at (1, 64, 1), (65, 17, 63),
    (257, 17, 5), (130, 300, 129): gemm_f8mx (E4M3 nocomp / zero table, E5M2), gemm_tt (E2M5; E3M4 at K < 64),
    gemm_tt16 (E3M4 at K >= 64; the signed table), gemm_fast (one table per packing mode under the 8
    (s2n, qbma, gclip) combinations, once with approx off), gemm_v5mx (E5M2 with the adder wrap) and
    gemm_fast<TM_V5> (the other formats, 3 switch sets); per family one launch with one off-grid A value, whose
    units the exact kernel recomputes, and against its clean twin: the other row tiles keep their bits;
  * split-K: (64, 2304, 64) on gemm_f8mx, gemm_tt and gemm_fast with the split count forced to 2, 3 and 6, the
    in-launch sum (splitk_fixup) off and on where it exists;
  * gemm_f8mx schedules on (130, 300, 129) and on a 3 x 3 convolution, each against the oracle (not against each
    other): xm_ncg 1 / 2 / 4, af32_maxct 0 / 64 (the convolution: a 1 x 1 one, the only kind staged from fp32),
    xm_pipe 0 / 1, xm_wave_rows 0 / 1 with xm_ncg = 4 forced (the 128 x 64 instances), xm_sign_rows 0 / 1 on the
    drawn A and on |A| (the positive-rows build), fp8a_xm_sign_stats asserted per launch;
  * gemm_tt's wave-tile forms (tt_band 0 / 1) on tiles built so that one product of an otherwise all-band
    wave-tile sits at the grid's smallest normal, and one product of an otherwise all-zero tile at half the
    quantum (and one mantissa step above it), at a K position that is not the first of the staged tile;
  * convolutions (fp8a_conv2d): the geometries of test_gpu_f8mx.py's conv test with <= 32 channels, on
    gemm_f8mx, gemm_tt / gemm_tt16 and one gemm_fast flag set, expected value from unfold + oracle.terms;
  * fp8a_bmm: 3 batch items as head views of [B, S, H*d] buffers, output in that layout, one format per
    per-term form, one tile with an off-grid operand; bmm_stats asserted;
  * tensor-bias depthwise 3 x 3 (all nine taps nonzero, strides 1 / 2, planes 7 / 9 / 14, per-channel bW): the E4M3
    table forms (tbs 0 / 1 / 2, tbx_rw 1 / 2), conv_tb_fast_kernel, conv_tb_direct_kernel, the v5 forms (v5ds 0 / 1);
  * the exact product (fp8a_dense_matmul / _conv2d in the bf16, e4m3 and e5m2 forms, an off-grid row through
    dn_fix's fp32 units, dn_direct 0 / 1, fp8a_grouped_conv2d with dw3 0 / 1 / 2) against the float64 product;
  * fp8a_matmul_qamaa against oracle.matmul_qamaa.

Every on-grid launch asserts flag word 0 and no exact-kernel launch.  Every case prints one line `XS <case>
path=<counters that moved> K=<K> budget=2^<log2 max sum|T| / u> old_bar=<median>/<max>u` (run with -s:
profiles/exact_sums/exact_sums.log).
"""
import collections
import contextlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_sums as xs
from tests import pairs_cases as pc
from tests.test_gpu_flag_matrix import _stop_on_device_error
from tests.test_gpu_tt import _conv_raw, _matmul_raw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MATRIX_CORE = ("f8mx", "tt", "tt16", "v5mx")


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


# ------------------------------------------------------------------------------------------ launches
@contextlib.contextmanager
def _options(opts):
    from fp8_quantization_amd import _lib
    old = [(k, _lib.set_option(k, v)) for k, v in (opts or {}).items()]
    try:
        yield
    finally:
        for k, v in reversed(old):
            _lib.set_option(k, v)


def _counted(fn):
    """fn() between resets of the counters: (result, path counters, fallback counters, split-K launches)."""
    from fp8_quantization_amd import _lib
    _lib.path_stats(reset=True)
    _lib.fallback_stats(reset=True)
    _lib.splitk_stats(reset=True)
    out = fn()
    return out, _lib.path_stats(reset=True), _lib.fallback_stats(reset=True), _lib.splitk_stats(reset=True)


@_stop_on_device_error
def _launch_mat(c, p):
    """fp8a_matmul as the linear layer passes it: A inside a wider buffer (lda = K + 7), B = W^T of a row-major
    [N][K] weight (sbk = 1, sbn = K), bB per column."""
    Mr, K, N = p["A"].shape[0], p["A"].shape[1], p["B"].shape[1]
    lda = K + 7
    Afull = np.full((Mr, lda), np.float32(0.3), np.float32)  # (the pad columns are off the grid: never read)
    Afull[:, :K] = p["A"]
    W = np.ascontiguousarray(p["B"].T)
    with _options(c.get("opts")):
        return _counted(lambda: _matmul_raw(Afull, lda, W, 1, K, Mr, N, K, c["E"], c["M"], p["bA"], p["bB"], p["bR"],
                                            p["table"], c["flags"]))


@_stop_on_device_error
def _launch_conv(c, p):
    cfg = c["cfg"]
    with _options(c.get("opts")):
        return _counted(lambda: _conv_raw(p["x"], p["w"], c["E"], c["M"], p["bA"], p["bB"], p["bR"], p["table"],
                                          c["flags"], cfg["s"], cfg["p"], cfg["d"], cfg["g"]))


def _prefetch(cases):
    """The cases' problems (operands + oracle terms), computed side by side, once per problem key."""
    keys = list(collections.OrderedDict((c["pkey"], 0) for c in cases))
    with ThreadPoolExecutor(min(12, len(keys))) as ex:
        return dict(zip(keys, ex.map(xs.problem_of.__wrapped__, keys)))


def _log(c, p, paths, flag):
    med, mx = xs.case_old_bar(p)
    ran = "+".join(k if v == 1 else f"{k}x{v}" for k, v in paths.items() if v) + ("!" if flag else "")
    print(f"XS {c['id']} path={ran} K={xs.case_K(c)} budget=2^{xs.case_budget_log2(p):.2f} old_bar={med:.3g}/{mx:.3g}u")


def _check_paths(c, paths, flag, fb, K):
    want = pc.expected_matmul_path(c["E"], c["M"], xs.case_table(c), c["flags"], K=K)
    others = {k: v for k, v in paths.items() if v and k not in (want, "exact")}
    assert paths[want] >= 1 and not others, f"{c['id']}: expected `{want}`, counters say {paths}"
    if c["kind"] != "conv":
        assert paths[want] == 1, paths
    if c.get("offgrid") and not c["flags"] & pc.V5:
        assert flag != 0 and fb["exact_units"] > 0, f"{c['id']}: the off-grid value raised no flag ({flag}, {fb})"
    else:  # every on-grid launch: the path named above alone produced the result, nothing was recomputed (and the v5
        # model decodes any operand to a code while staging, as the oracle does: it has nothing to fall back from)
        assert flag == 0 and paths["exact"] == 0 and fb["exact_launches"] == 0 and fb["f32_reruns"] == 0, \
            f"{c['id']}: flag {flag}, {paths}, {fb}: `{want}` alone did not produce this result"
    return want


def _run(c, p, log=True):
    from fp8_quantization_amd import _lib
    _lib.xm_sign_stats(reset=True)
    if c["kind"] == "conv":
        (y, flag), paths, fb, nsplit = _launch_conv(c, p)
        got = y.transpose(0, 2, 3, 1).reshape(-1, y.shape[1])
        K = xs.case_K(c)
    else:
        (got, flag), paths, fb, nsplit = _launch_mat(c, p)
        K = c["shape"][1]
    signs = _lib.xm_sign_stats(reset=True)
    if log:
        _log(c, p, paths, flag)
    for (_, _, T, sl) in p["parts"]:
        xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)
    _check_paths(c, paths, flag, fb, K)
    if c in SCHED_ALL:  # one gemm_f8mx launch: the tile-table build the option and A's sign select
        assert signs == xs.expected_sign_build(c), f"{c['id']}: sign build {signs}"
    if c.get("split"):
        assert nsplit == 1, f"{c['id']}: the launch did not run split along K"
    elif c["kind"] == "mat" and K < 1024:
        assert nsplit == 0, f"{c['id']}: an unexpected split launch"
    return got


def _groups(cases, key):
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault(key(c), []).append(c)
    return out


def _run_group(cases):
    probs = _prefetch(cases)
    for c in cases:
        _run(c, probs[c["pkey"]])


# ------------------------------------------------------------------------------------------ matrix launches
MAT = _groups(xs.matmul_cases(), lambda c: f"{c['fam']}-E{c['E']}M{c['M']}-{c['table']}-" +
              "x".join(map(str, c["shape"])) + ("-offgrid" if c.get("offgrid") else ""))


@pytest.mark.parametrize("group", list(MAT), ids=list(MAT))
def test_matmul_sums_bit_exact(group):
    _run_group(MAT[group])


OFFGRID = [c for c in xs.matmul_cases() if c.get("offgrid")]


@pytest.mark.parametrize("cid", [c["id"] for c in OFFGRID])
def test_off_grid_row_leaves_the_other_units_alone(cid):
    """Every family's off-grid launch against its clean twin: outside the 128 rows of the tile that holds the marked
    row every output is the clean launch's, bit for bit (and both are the oracle's).  (These two launches are logged
    by test_matmul_sums_bit_exact.)"""
    c = xs.CASES[cid]
    clean = xs.CASES[c["pkey"][:-len("-offgrid")]]
    probs = _prefetch([c, clean])
    got, ref = _run(c, probs[c["pkey"]], log=False), _run(clean, probs[clean["pkey"]], log=False)
    row = probs[c["pkey"]]["spot"][0]
    keep = np.ones(got.shape[0], bool)
    keep[row // 128 * 128:(row // 128 + 1) * 128] = False
    assert np.array_equal(got[keep].view(np.uint32), ref[keep].view(np.uint32))
    assert not np.array_equal(got[row], ref[row]), "the off-grid value did not change its row"


# ------------------------------------------------------------------------------------------ split-K, schedules
SPLITK = _groups(xs.splitk_cases(), lambda c: c["pkey"])


@pytest.mark.parametrize("group", list(SPLITK), ids=list(SPLITK))
def test_splitk_sums_bit_exact(group):
    _run_group(SPLITK[group])


SCHED_ALL = xs.schedule_cases()
SCHED = _groups(SCHED_ALL, lambda c: c["kind"])


@pytest.mark.parametrize("group", list(SCHED), ids=list(SCHED))
def test_f8mx_schedules_bit_exact(group):
    """Every schedule option value against the oracle itself (their own test files compare them with each other)."""
    _run_group(SCHED[group])


# ------------------------------------------------------------------------------------------ wave-tile forms
BAND = _groups(xs.band_cases(), lambda c: c["pkey"])


@pytest.mark.parametrize("group", list(BAND), ids=list(BAND))
def test_tt_wave_tile_forms_bit_exact(group):
    _run_group(BAND[group])


# ------------------------------------------------------------------------------------------ convolutions
CONV = _groups(xs.conv_cases(), lambda c: "-".join(f"{k}{v}" for k, v in c["cfg"].items()))


@pytest.mark.parametrize("group", list(CONV), ids=list(CONV))
def test_conv_sums_bit_exact(group):
    _run_group(CONV[group])


# ------------------------------------------------------------------------------------------ fp8a_bmm
@pytest.mark.parametrize("cid", [c["id"] for c in xs.bmm_cases()])
def test_bmm_sums_bit_exact(cid):
    """Three batch items (one batch row, three heads) cut from [1, S, H*d] buffers: A [1, M, 3 K] as
    [1, 3, M, K], B [1, K, 3 N] as [1, 3, K, N], the output written into a sentinel-filled [1, M, 3 N]."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_bmm
    c = xs.CASES[cid]
    p = xs.problem(cid)
    Mr, K, N = c["shape"]
    nh = c["items"]
    A = torch.from_numpy(np.ascontiguousarray(p["A"].transpose(1, 0, 2).reshape(1, Mr, nh * K))).to(DEV)
    B = torch.from_numpy(np.ascontiguousarray(p["B"].transpose(1, 0, 2).reshape(1, K, nh * N))).to(DEV)
    buf = torch.full((1, Mr, nh * N), -77.25, device=DEV)
    Av = A.view(1, Mr, nh, K).permute(0, 2, 1, 3)
    Bv = B.view(1, K, nh, N).permute(0, 2, 1, 3)
    out = buf.view(1, Mr, nh, N).permute(0, 2, 1, 3)
    _lib.bmm_stats(reset=True)
    try:
        approx_bmm(Av, Bv, c["E"], c["M"], p["bA"], int(p["bB"][0]), p["bR"], torch.from_numpy(p["table"]),
                   flags=c["flags"], out=out)
        torch.cuda.synchronize()
    except RuntimeError as ex:
        pytest.exit(f"device error in fp8a_bmm: {ex}", returncode=3)
    st = _lib.bmm_stats(reset=True)
    got = out.cpu().numpy()[0]
    med, mx = xs.case_old_bar(p)
    print(f"XS {cid} path=bmm{'!' if st['recomputed'] else ''} K={K} budget=2^{xs.case_budget_log2(p):.2f} "
          f"old_bar={med:.3g}/{mx:.3g}u")
    for (_, _, T, z) in p["parts"]:
        xs.assert_same(got[z], xs.expected(T), f"{cid} item {z}", T)
    tiles = nh * ((Mr + 63) // 64) * ((N + 63) // 64)
    recomputed = (N + 63) // 64 if c["offgrid"] else 0  # the row tile of the off-grid value: one per column tile
    assert st == dict(launches=1, tiles=tiles, recomputed=recomputed), st


# ------------------------------------------------------------------------------------------ exact product
def _dense_fmt(form):
    from fp8_quantization_amd import _lib
    return {"e4m3": _lib.DENSE_E4M3, "e5m2": _lib.DENSE_E5M2, "bf16": _lib.DENSE_BF16}[form]


def _dense_log(c, p, what):
    med, mx = xs.case_old_bar(p)
    print(f"XS {c['id']} path={what} K={xs.case_K(c)} budget=2^{xs.case_budget_log2(p):.2f} "
          f"old_bar={med:.3g}/{mx:.3g}u")


@pytest.mark.parametrize("cid", [c["id"] for c in xs.dense_cases()])
def test_exact_product_bit_exact(cid):
    """fp8a_dense_matmul / fp8a_dense_conv2d on the three operand forms, fp8a_grouped_conv2d's depthwise forms:
    the float64 product cast to float32.  The off-grid row goes through dn_fix's fp32 units (counted)."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd import approx_ops as ops
    c = xs.CASES[cid]
    p = xs.problem(cid)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    _lib.dense_stats(reset=True)
    _lib.path_stats(reset=True)
    try:
        with _options(c.get("opts")):
            if c["kind"] == "dense":
                got = ops.dense_matmul(dev(p["A"]), dev(p["B"].T).t(), _dense_fmt(c["form"])).cpu().numpy()
            elif c["kind"] == "dconv":
                g = c["geo"]
                y = ops.dense_conv2d(dev(p["x"]), dev(p["w"]), _dense_fmt(c["form"]), g["stride"], g["pad"], g["dil"])
                got = y.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, g["cout"])
            else:
                y = ops.grouped_conv2d(dev(p["x"]), dev(p["w"]), xs.DENSE_DW["C"], (c["stride"],) * 2, (1, 1), (1, 1))
                got = y.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, xs.DENSE_DW["C"])
    except RuntimeError as ex:
        pytest.exit(f"device error in the exact product: {ex}", returncode=3)
    st, paths = _lib.dense_stats(reset=True), _lib.path_stats(reset=True)
    ran = "+".join(k for k, v in paths.items() if v)
    _dense_log(c, p, ran + (f",fp32_units={st['fp32_units']}" if st["fp32_units"] else ""))
    for (_, _, T, sl) in p["parts"]:
        xs.assert_same(got[:, sl], xs.expected(T), cid, T)
    assert paths["dense"] == 1 and sum(paths.values()) == 1, f"{cid}: counters say {paths}"
    units = (c["shape"][2] + 127) // 128 * 2 if c.get("offgrid") else 0  # the row's unit: one per 64 padded columns
    assert st["fp32_units"] == units and st["fp32_launches"] == int(units > 0), f"{cid}: {st}"


def test_qamaa_bit_exact():
    """fq(sum_k fq(a b)): the inner terms meet the budget, so the sum is exact in any order and its final
    quantization deterministic: bit-equal to oracle.matmul_qamaa."""
    from fp8_quantization_amd import approx_ops as ops
    c = xs.QAMAA
    p = xs.problem(c["id"])
    A, B, T, _ = p["parts"][0]
    try:
        got, paths, fb, nsplit = _counted(lambda: ops.qamaa_matmul(
            torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), torch.tensor([c["maxval"]], device=DEV), 8,
            c["M"]).cpu().numpy())
    except RuntimeError as ex:
        pytest.exit(f"device error in fp8a_matmul_qamaa: {ex}", returncode=3)
    # run_qamaa launches gemm_fast_kernel<TM_QAMAA> itself, outside run_gemm: no path counter moves, and there is no
    # operand decode, hence nothing to fall back from
    _dense_log(c, p, "+".join(k for k, v in paths.items() if v) or "none")
    assert sum(paths.values()) == 0 and nsplit == 0, f"counters say {paths}, {nsplit} split launches"
    assert fb == dict(exact_launches=0, exact_units=0, f32_reruns=0, tb_launches=0), fb
    want, pre = orc.matmul_qamaa(A, B, c["maxval"], 8, c["M"])
    xs.assert_same(pre, xs.expected(T), "oracle.matmul_qamaa's sums", T)
    xs.assert_same(got, want, c["id"])
    assert np.unique(want).size > 50, "the final quantizer left too few distinct values to tell sums apart"


# ------------------------------------------------------------------------------------------ tensor-bias depthwise
TBDW = _groups(xs.tbdw_cases(), lambda c: c["pkey"])


@pytest.mark.parametrize("group", list(TBDW), ids=list(TBDW))
def test_tensor_bias_depthwise_bit_exact(group):
    """fp8a_conv2d on a 3 x 3 depthwise layer, all nine taps nonzero: the E4M3 table forms (tbs 0 / 1 / 2, tbx_rw
    1 / 2), conv_tb_fast_kernel (E3M4 / E2M5), conv_tb_direct_kernel (s2n off) and the v5 forms (v5ds 0 / 1), each
    channel against the sum of its nine tensor-bias terms.  Gate 0 and no direct-kernel launch: the form itself
    produced the result."""
    from tests.test_gpu_tbx import _dw_raw
    cases = TBDW[group]
    p = xs.problem(cases[0]["id"])
    for c in cases:
        try:
            with _options(c["opts"]):
                (y, gate), paths, fb, _ = _counted(lambda: _dw_raw(
                    p["x"], p["w"], p["bA"], p["bB"], p["bR"], p["table"], c["flags"], c["stride"], 1,
                    fmt=(c["E"], c["M"])))
        except RuntimeError as ex:
            pytest.exit(f"device error in the depthwise launch: {ex}", returncode=3)
        # The tensor-bias kernels move no GEMM path counter (the v5 forms count as `fast`), and the library reports
        # no counter that tells conv_tbx / conv_tbs / conv_tbsg / conv_tb_fast apart: the line prints what was
        # measured -- counters, gate word, direct-kernel launches -- not a form name.
        ran = "+".join(k for k, v in paths.items() if v) or "none"
        _dense_log(c, p, f"{ran},gate={gate},tb_launches={fb['tb_launches']}")
        got = y.transpose(0, 2, 3, 1).reshape(-1, c["C"])
        for (_, _, T, sl) in p["parts"]:
            xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)
        assert gate == 0 and fb["tb_launches"] == 0 and fb["exact_launches"] == 0, f"{c['id']}: gate {gate}, {fb}"
        want = dict.fromkeys(paths, 0)
        if c["fam"] == "v5dw":
            want["fast"] = 1
        assert paths == want, f"{c['id']}: counters say {paths}"
