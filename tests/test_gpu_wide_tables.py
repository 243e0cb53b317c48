"""Every table-reading path on error tables over the full int8 range (tests/wide_tables.py),
bit for bit against the CPU oracle, zeros by value.  The oracle is pinned to the reference on exactly these
cases (tests/test_wide_tables_cpu.py).

  * every code pair as a K = 1 fp8a_matmul launch: every format, table and bias triple under the 8
    (s2n, qbma, gclip) flag words, and with the tensor-bias bit under approx x s2n x qbma; the path counter must
    say what the host's table predicates say (pairs_cases.expected_matmul_path: xm_table_form for E4M3 / E5M2,
    tt_table_form for E3M4 / E2M5, else gemm_fast_kernel);
  * E3M4: gemm_tt_kernel<4> (K < 64, no negative entry) and gemm_tt16_kernel (a negative entry, or K >= 64)
    with the single term in an otherwise zero K; a `hi` table (V >= 4) must move the f32 rerun counter;
  * E2M5: `lowpos` / `zero_v` through gemm_tt_kernel<5> with the band / zero wave-tile forms on and off, bit
    identical, and no table with a negative entry ever on gemm_tt_kernel;
  * the tensor-bias 1 x 1 depthwise layer of test_gpu_flag_matrix.py, the form asserted from the gate word and
    the recomputation counter: conv_tb_fast_kernel itself (every bias >= 2), conv_tb_direct_kernel behind its
    raised gate, conv_tb_direct_kernel alone (s2n off); the three depthwise table forms (option "tbs") on
    `lowpos`, the one wide table they take;
  * K > 1 sums, (130, 300, 129) and the split-K shape (64, 2304, 64), `mixed` / `lowpos` / `hi`: within
    1e-5 sum|v| of the double-accumulated oracle and bit-identical run to run;
  * fp8a_bmm on tables with negative V, the two self-check kernels at K = 1, and QCustomLinearTorch with an
    E3M4 `mixed` table against the direct op call.

Every launch prints one token of a "WT ..." line (run with -s: profiles/wide_tables/wide_tables.log).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import golden_io as gio
from tests import pairs_cases as pc
from tests import wide_tables as wt
from tests.test_gpu_flag_matrix import _dw1x1_raw, _flag_text, _grid, _matmul_raw, _only, _terms_equal

pytestmark = pytest.mark.gpu
FL = pc.flag_word(True, True, True, False)
_LINE = []


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


@pytest.fixture(autouse=True)
def _one_log_line_per_test():
    """`WT <case> <terms in the planted class> <flag bits>:<path counters>:<flag word>:<fallback counters> ...`"""
    del _LINE[:]
    yield
    if _LINE:
        print("WT", *_LINE)


def _log(head, fl, paths, flag, fb):
    if not _LINE:
        _LINE.append(head)
    ran = "+".join(f"{k}x{v}" for k, v in paths.items() if v) or "-"
    fbs = "+".join(f"{k}x{v}" for k, v in fb.items() if v) or "-"
    _LINE.append(f"{fl}:{ran}:{flag}:{fbs}")


def _ids(params):
    return [f"E{p[0]}M{p[1]}-" + "-".join("_".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in p[2:])
            for p in params]


def _assert_flag(path, name, flag, fb):
    """The launch's flag word: grid operands and in-range biases raise nothing on gemm_fast_kernel and
    gemm_tt_kernel (no exact rerun: the form itself produced the bits); gemm_tt16_kernel raises bit 8 (the f16
    image holds a V >= 4) for a `hi` table only, and then the f32 form reruns the launch once.  The matrix-core
    form may hand terms beyond the hardware format's range to the exact kernel: not asserted."""
    if path in ("fast", "tt"):
        assert flag == 0 and fb["exact_launches"] == 0 and fb["f32_reruns"] == 0, (path, flag, fb)
    elif path == "tt16":
        assert flag == (8 if name == "hi" else 0) and fb["f32_reruns"] == (1 if name == "hi" else 0), (flag, fb)
        assert fb["exact_launches"] == 0, fb


def _class(name, E, M):
    return f"class={int(np.count_nonzero(wt.pair_class(name, E, M)))}"


# ------------------------------------------------------------------------------------------ K = 1 terms
V9_PARAMS = [(E, M, name, tr) for (E, M) in wt.FORMATS for name in wt.NAMES for tr in wt.v9_triples(E, M)]
TB_PARAMS = [(E, M, name, tr) for (E, M) in wt.FORMATS for name in wt.NAMES for tr in wt.tb_triples(E, M)]


@pytest.mark.parametrize("E,M,name,biases", V9_PARAMS, ids=_ids(V9_PARAMS))
def test_terms_every_code_pair_all_flags(E, M, name, biases):
    bA, bB, bR = biases
    tab = wt.tables(E, M)[name]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bB)
    A, B = a.reshape(-1, 1), b.reshape(1, -1)
    for fl in pc.v9_flag_words(False):
        C, flag, paths, fb = _matmul_raw(A, B, E, M, bA, bB, bR, tab, fl)
        _log(f"terms E{E}M{M}-{name}-{'_'.join(map(str, biases))} {_class(name, E, M)}", fl, paths, flag, fb)
        ref = orc.terms(A, B, E, M, bA, bB, bR, tab, fl)[:, 0, :]
        _terms_equal(C, ref, a, b, f"E{E}M{M} {name} {biases} [{_flag_text(fl)}]")
        want = pc.expected_matmul_path(E, M, tab, fl, K=1)
        assert _only(paths, want), f"[{_flag_text(fl)}] expected one `{want}` launch, counters say {paths}"
        _assert_flag(want, name, flag, fb)


@pytest.mark.parametrize("E,M,name,biases", TB_PARAMS, ids=_ids(TB_PARAMS))
def test_terms_every_code_pair_tensor_bias(E, M, name, biases):
    bA, bB, bR = biases
    tab = wt.tables(E, M)[name]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bB)
    A, B = a.reshape(-1, 1), b.reshape(1, -1)
    for fl in pc.tb_flag_words(False):
        C, flag, paths, fb = _matmul_raw(A, B, E, M, bA, bB, bR, tab, fl)
        _log(f"tb-terms E{E}M{M}-{name}-{'_'.join(map(str, biases))} {_class(name, E, M)}", fl, paths, flag, fb)
        ref = orc.terms(A, B, E, M, bA, bB, bR, tab, fl)[:, 0, :]
        _terms_equal(C, ref, a, b, f"E{E}M{M} {name} {biases} [{_flag_text(fl)}]")
        assert _only(paths, "exact"), paths


@pytest.mark.parametrize("E,M,name,biases", TB_PARAMS, ids=_ids(TB_PARAMS))
def test_tensor_bias_depthwise_1x1_every_code_pair(E, M, name, biases):
    """test_gpu_flag_matrix.py's layer: every output is one tensor-bias term.  s2n on: conv_tb_fast_kernel with
    the gated conv_tb_direct_kernel behind it; s2n off: conv_tb_direct_kernel alone.  The gate word and the
    recomputation counter say which of the two produced the bits."""
    bA, bW_, bR = biases
    tab = wt.tables(E, M)[name]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bW_)
    C = b.size
    side = int(round(a.size ** 0.5))
    assert side * side == a.size
    x = np.broadcast_to(a.reshape(1, 1, side, side), (1, C, side, side)).copy()
    w = b.reshape(C, 1, 1, 1).copy()
    bW = np.full(C, bW_, np.int32)
    for fl in [f & ~pc.TB for f in pc.tb_flag_words(False)]:
        y, gate, paths, fb = _dw1x1_raw(x, w, E, M, bA, bW, bR, tab, fl)
        _log(f"tb1x1 E{E}M{M}-{name}-{'_'.join(map(str, biases))} {_class(name, E, M)}", fl, paths, gate, fb)
        ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, bA, bW, bR, tab, fl | orc.TB)[:, 0, :]
        _terms_equal(y[0].reshape(C, a.size).T, ref, a, b, f"E{E}M{M} {name} {biases} [{_flag_text(fl | pc.TB)}]")
        # a 1 x 1 kernel never takes the depthwise table form (3-wide rows only).  s2n on: conv_tb_fast_kernel,
        # which produces the bits itself (gate 0, no recomputation) exactly when every bias is >= 2 (F5:
        # min_norm = 0, its premise) -- else it raises the gate and conv_tb_direct_kernel recomputes the launch
        # once.  s2n off: conv_tb_direct_kernel alone, no gate exists.
        raised = bool(fl & pc.S2N) and min(biases) < 2
        assert (gate != 0) == raised and fb["tb_launches"] == (1 if raised else 0), (gate, fb, biases)
        assert fb["exact_launches"] == 0 and fb["f32_reruns"] == 0, fb


def test_every_format_has_triples_the_valu_depthwise_form_answers_itself():
    """Coverage guard: per format at least two tensor-bias triples keep conv_tb_fast_kernel's gate down, so its
    own terms (the F7 sign of a negative V among them) are what the test above compares."""
    for (E, M) in wt.FORMATS:
        assert sum(min(tr) >= 2 for tr in wt.tb_triples(E, M)) >= 2, (E, M)


# (test_gpu_custom_table.py's one-nonzero-tap 3 x 3 layer: `lowpos` is the one wide table of xm_table_form, the
# only kind the depthwise table forms take; option "tbs" picks the form)
@pytest.mark.parametrize("tbs", [0, 1, 2], ids=["conv_tbx", "conv_tbs", "conv_tbsg"])
@pytest.mark.parametrize("fmt,biases", [((4, 3), (12, 12, 8)), ((4, 3), (9, 9, 2)), ((5, 2), (20, 20, 9)),
                                        ((5, 2), (28, 28, 40))], ids=lambda v: "_".join(map(str, v)))
def test_depthwise_table_forms_on_lowpos(fmt, biases, tbs):
    from fp8_quantization_amd import _lib
    from tests.test_gpu_custom_table import _dw_raw
    E, M = fmt
    bA, bW_, bR = biases
    tab = wt.tables(E, M)["lowpos"]
    assert pc.xm_table_form(tab, M)
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bW_)
    C = b.size
    x = np.broadcast_to(a.reshape(1, 1, 16, 16), (1, C, 16, 16)).copy()
    w = np.zeros((C, 1, 3, 3), np.float32)
    w[:, 0, 1, 1] = b
    ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, bA, np.full(C, bW_, np.int32), bR, tab, FL | orc.TB)[:, 0, :]
    old = _lib.set_option("tbs", tbs)
    try:
        _lib.fallback_stats(reset=True)
        y, gate = _dw_raw(x, w, bA, np.full(C, bW_, np.int32), bR, tab, FL, 1, 1, fmt)
        fb = _lib.fallback_stats(reset=True)
    finally:
        _lib.set_option("tbs", old)
    _log(f"dw3x3 E{E}M{M}-lowpos-{'_'.join(map(str, biases))} {_class('lowpos', E, M)}", f"tbs{tbs}", {}, gate, fb)
    assert gate == 0 and fb["tb_launches"] == 0, (gate, fb)  # the table form produced these terms
    _terms_equal(y[0].reshape(C, 256).T, ref, a, b, f"depthwise table form tbs={tbs} E{E}M{M} {biases}")


# ------------------------------------------------------------------------------------------ E3M4: both forms
def _one_term_in_k(E, M, biases, K):
    """A [codes, K], B [K, codes]: the code pair's term at k = 0, every other product zero."""
    a, b = pc.all_codes(E, M, biases[0]), pc.all_codes(E, M, biases[1])
    A = np.zeros((a.size, K), np.float32)
    B = np.zeros((K, b.size), np.float32)
    A[:, 0], B[0, :] = a, b
    return a, b, A, B


@pytest.mark.parametrize("name", wt.NAMES)
@pytest.mark.parametrize("K", [8, 64])
@pytest.mark.parametrize("biases", [(6, 9, 4), (6, 9, 9)], ids=lambda v: "_".join(map(str, v)))
def test_e3m4_both_tile_table_forms(name, K, biases):
    E, M = 3, 4
    tab = wt.tables(E, M)[name]
    a, b, A, B = _one_term_in_k(E, M, biases, K)
    C, flag, paths, fb = _matmul_raw(A, B, E, M, *biases, tab, FL)
    _log(f"e3m4-forms {name}-{'_'.join(map(str, biases))}-K{K} {_class(name, E, M)}", FL, paths, flag, fb)
    ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, *biases, tab, FL)[:, 0, :]
    _terms_equal(C, ref, a, b, f"E3M4 {name} {biases} K={K}")
    want = pc.expected_matmul_path(E, M, tab, FL, K=K)
    assert _only(paths, want), (want, paths)
    assert want == ("fast" if not pc.tt_table_form(tab, M) else "tt16" if tab.min() < 0 or K >= 64 else "tt")
    assert want == "tt16" or name != "hi"  # V >= 4 leaves the f16 window: the f32 form reruns the launch
    _assert_flag(want, name, flag, fb)


# ------------------------------------------------------------------------------------------ E2M5: band / zero
@pytest.mark.parametrize("name", ["lowpos", "zero_v"])
@pytest.mark.parametrize("biases", [(4, 7, 4), (4, 7, 1)], ids=lambda v: "_".join(map(str, v)))
def test_e2m5_band_and_zero_wave_tiles_bit_identical(name, biases):
    """(4, 7, 1): most products lie below the result grid's smallest normal (band) or half its quantum (zero)."""
    from fp8_quantization_amd import _lib
    E, M = 2, 5
    tab = wt.tables(E, M)[name]
    a, b, A, B = _one_term_in_k(E, M, biases, 8)
    ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, *biases, tab, FL)[:, 0, :]
    got = []
    for band in (0, 1):
        old = _lib.set_option("tt_band", band)
        try:
            C, flag, paths, fb = _matmul_raw(A, B, E, M, *biases, tab, FL)
        finally:
            _lib.set_option("tt_band", old)
        _log(f"e2m5-band {name}-{'_'.join(map(str, biases))} {_class(name, E, M)}", f"band{band}", paths, flag, fb)
        assert _only(paths, "tt") and flag == 0, (paths, flag)
        _terms_equal(C, ref, a, b, f"E2M5 {name} {biases} tt_band={band}")
        got.append(C)
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))


@pytest.mark.parametrize("name", [n for n in wt.NAMES if wt.tables(2, 5)[n].min() < 0])
def test_e2m5_signed_table_never_reaches_the_tile_table_kernel(name):
    """gemm_tt_kernel<5>'s band / zero thresholds assume V < 4, which only a table without negative entries
    guarantees: the host must keep every other E2M5 table on gemm_fast_kernel, whatever K."""
    E, M = 2, 5
    tab = wt.tables(E, M)[name]
    for K in (1, 8, 64):
        a, b, A, B = _one_term_in_k(E, M, (4, 7, 4), K)
        C, flag, paths, fb = _matmul_raw(A, B, E, M, 4, 7, 4, tab, FL)
        _log(f"e2m5-signed {name} {_class(name, E, M)}", f"K{K}", paths, flag, fb)
        assert _only(paths, "fast"), paths
        _terms_equal(C, orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, 4, 7, 4, tab, FL)[:, 0, :], a, b,
                     f"E2M5 {name} K={K}")


# ------------------------------------------------------------------------------------------ K > 1 sums
@pytest.mark.parametrize("E,M", wt.FORMATS)
@pytest.mark.parametrize("shape", [(130, 300, 129), (64, 2304, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["mixed", "lowpos", "hi"])
def test_sums_within_bar_and_deterministic(E, M, shape, name):
    """`mixed`: gemm_fast_kernel<TM_LUT>; `lowpos`: the matrix-core and tile-table forms; `hi`: on E3M4
    gemm_tt16_kernel leaves its window through the table and gemm_tt_kernel<4, F7> reruns the launch over a real
    K (the split-K shape included)."""
    Mr, K, N = shape
    rng = np.random.default_rng(Mr * 1000 + K * 10 + N + E)
    h = 1 << (E - 1)
    bA, bR = h + 2, h + 4
    bB = rng.integers(h + 4, h + 7, size=N).astype(np.int32)
    A = _grid(rng, E, M, (Mr, K), bA, 0.4)
    B = _grid(rng, E, M, (K, N), bB[None, :], 0.1)
    tab = wt.tables(E, M)[name]
    Cref, S = orc.matmul(A, B, E, M, bA, bB, bR, tab, FL, with_abs=True)
    C, flag, paths, fb = _matmul_raw(A, B, E, M, bA, bB, bR, tab, FL)
    _log(f"sums E{E}M{M}-{name}-{Mr}x{K}x{N} {_class(name, E, M)}", FL, paths, flag, fb)
    want = pc.expected_matmul_path(E, M, tab, FL, K=K)
    assert _only(paths, want), (want, paths)
    _assert_flag(want, name, flag, fb)
    err = np.abs(C.astype(np.float64) - Cref)
    tol = gio.sum_tolerance(S.astype(np.float64))
    assert np.all(err <= tol), f"{np.count_nonzero(err > tol)} sums outside the bar, worst {np.max(err / np.maximum(tol, 1e-300)):.3g} x"
    C2 = _matmul_raw(A, B, E, M, bA, bB, bR, tab, FL)[0]
    assert np.array_equal(C.view(np.uint32), C2.view(np.uint32)), "not deterministic"


# ------------------------------------------------------------------------------------------ fp8a_bmm
SIGNED = {(4, 3): "mixed", (3, 4): "mixed", (2, 5): "neg_small", (5, 2): "mixed"}  # V < 0 in every one


@pytest.mark.parametrize("E,M", wt.FORMATS)
@pytest.mark.parametrize("name", ["mixed", "neg_small", "neg_big"])
def test_bmm_terms_bit_exact(E, M, name):
    """test_gpu_bmm.py's every-code-pair construction (four sign pairs as four batch items) on tables with
    negative V: gemm_bmm_kernel<.., TM_LUT>'s F7 sign rule under s2n + qbma, and the other flag words."""
    from tests.test_gpu_bmm import _terms_check
    tab = wt.tables(E, M)[name]
    assert wt.numerators(tab, M).min() < 0 and pc.table_mode(tab, M) == "TM_LUT"
    for triple in wt.v9_triples(E, M)[:3]:
        for fl in (FL, pc.flag_word(True, True, True, True), pc.flag_word(True, True, False, False),
                   pc.flag_word(True, False, True, False)):
            _terms_check(E, M, tab, triple, fl)
    _LINE.append(f"bmm-terms E{E}M{M}-{name} {_class(name, E, M)} 3 triples x 4 flag words")


# ------------------------------------------------------------------------------------------ self-checks
@pytest.mark.parametrize("E,M", wt.FORMATS)
@pytest.mark.parametrize("tb", [False, True], ids=["int", "tb"])
def test_self_check_kernels_every_code_pair(E, M, tb):
    """approx_matmul_check and approx_bmm_check at K = 1: their C is the term of every code pair, their G the
    golden product; one signed wide table per format."""
    import fp8_quantization_amd as fa
    name = SIGNED[(E, M)]
    tab = wt.tables(E, M)[name]
    bA, bB, bR = (wt.tb_triples if tb else wt.v9_triples)(E, M)[0]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bB)
    A, B = a.reshape(-1, 1), b.reshape(1, -1)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")  # noqa: E731
    for s2n, qbma in ((True, True), (False, True), (True, False)):
        flags = fa.make_flags(True, s2n, qbma, False, tensor_bias=tb)
        ref = orc.terms(A, B, E, M, bA, bB, bR, tab, flags)[:, 0, :]
        g = (A * B).astype(np.float32)
        gold = orc.quant(g, E, M, bR, tb=tb, clip=False) if qbma else g
        bBt = torch.tensor([bB], dtype=torch.int32)
        C, G, st = fa.approx_matmul_check(dev(A), dev(B), E, M, bA, bBt, bR, torch.from_numpy(tab), flags=flags)
        _terms_equal(C.cpu().numpy(), ref, a, b, f"matmul_check E{E}M{M} {name} tb={tb} s2n={s2n} qbma={qbma}")
        _terms_equal(G.cpu().numpy(), gold, a, b, f"matmul_check golden E{E}M{M} tb={tb}")
        if not tb:  # (the batched check has no tensor-bias form)
            C2, G2, st2 = fa.approx_bmm_check(dev(A[None, None]), dev(B[None, None]), E, M, bA, bBt, bR, torch.from_numpy(tab),
                                              flags=flags)
            _terms_equal(C2.cpu().numpy()[0, 0], ref, a, b, f"bmm_check E{E}M{M} {name} s2n={s2n} qbma={qbma}")
            assert st2.max_err == st.max_err
    _LINE.append(f"self-check E{E}M{M}-{name} {'tb' if tb else 'int'} {_class(name, E, M)} 3 flag words")


# ------------------------------------------------------------------------------------------ operator level
def test_e3m4_operator_with_a_mixed_table_equals_direct_op_call():
    """test_gpu_custom_table.py's operator test for E3M4 and a `mixed` table (gemm_fast_kernel<TM_LUT>: the table
    has negative V): QCustomLinearTorch's run_forward equals the direct op call on the same operands by bits,
    and differs from the built-in table's result."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    from fp8_quantization_amd.error_tables import get_error_table_NN
    from fp8_quantization_amd.resnet_workload import approx_qparams
    from tests.test_gpu_custom_table import _calibrate, _record_operands
    tab = wt.tables(3, 4)["mixed"]
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    mod = QCustomLinearTorch(in_features=72, out_features=24, bias=False,
                             **approx_qparams(expo_width=3, mant_width=4, error_table=tab.tolist()))
    mod = mod.to("cuda:0").eval()
    _calibrate(mod, torch.randn((37, 72), generator=g).to("cuda:0"))
    rec = _record_operands([("m", mod)])
    with torch.no_grad():
        mod(torch.randn((37, 72), generator=g).to("cuda:0"))
    x, w = rec["m"]
    E, M, t, flags = mod._approx_config()
    assert (E, M) == (3, 4) and t.numpy().tolist() == tab.tolist() and flags == make_flags(True, True, True)
    bA = mod._default_bias(mod.get_acts_fp_bias(), E, x.device)
    bW, bR = mod.get_weights_fp_bias(), mod._default_bias(mod.get_res_fp_bias(), E, x.device)
    _lib.path_stats(reset=True)
    with torch.no_grad():
        got = mod.run_forward(x, w, None)
    paths = _lib.path_stats(reset=True)
    assert _only(paths, "fast"), paths
    direct = approx_matmul(x, w.t(), E, M, bA, bW, bR, torch.as_tensor(tab), flags=flags)
    other = approx_matmul(x, w.t(), E, M, bA, bW, bR, get_error_table_NN(3, 4, False, 3), flags=flags)
    assert torch.equal(got.view(torch.int32), direct.view(torch.int32))
    assert not torch.equal(got, other), "the custom table computes what the built-in one does"
    _LINE.append("operator E3M4-mixed QCustomLinearTorch fastx1")
