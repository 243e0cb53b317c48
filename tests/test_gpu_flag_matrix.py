"""Every kernel instance the flags select, against the CPU oracle.

The exhaustive code-pair tests of the matrix-core, tile-table and depthwise table forms all run with
s2n = 1, qbma = 1, gclip = 0, the only combination those forms take.  Every other combination goes to
gemm_fast_kernel<S2N, QBMA, GCLIP, TMODE> (k_fast.hip: 8 flag combinations x 7 table modes of separately
compiled code), to gemm_exact_kernel, to the depthwise VALU form conv_tb_fast_kernel or to
conv_tb_direct_kernel.  Here, through the production entry points fp8a_matmul / fp8a_conv2d with a
caller-owned workspace, the path counters read back per launch:

  * terms: A [256, 1] x B [1, 256], K = 1 (all 256 x 256 code pairs, one term per output) for every
    format x table x bias triple of tests/pairs_cases.py -- the cases on which the oracle is pinned to the
    reference (tests/test_oracle_pairs_cpu.py) -- under all 8 (s2n, qbma, gclip) combinations with approx on
    and, once per triple, with approx off; bit-exact against oracle.terms, zeros by value.  The fallback
    flag is not asserted (a term beyond the fp8 range reruns the exact kernel: still bit-exact); the path
    counter is: it must say what fp8approx.hip's dispatch rules say (pairs_cases.expected_matmul_path);
  * table modes: built-in and synthetic tables make every TMode of pack_table run under every flag
    combination (the coverage guard below restates the mode rule);
  * sums through the same instances: (65, 17, 63) and (130, 300, 129), grid operands with zeros,
    per-column bB, one table per mode, all 8 combinations, within 1e-5 * sum|term| of oracle.matmul and
    bit-identical run to run;
  * tensor bias: a 1 x 1 depthwise convolution over 256 channels, channel c carrying weight code c and
    one 16 x 16 plane the 256 activation codes -- every output is a single term -- against
    oracle.terms(..., flags | TB) under all 16 flag combinations (s2n & !gclip: conv_tb_fast_kernel with
    the gated conv_tb_direct_kernel behind it; else conv_tb_direct_kernel alone);
  * v5 off the matrix core: gemm_fast_kernel<TM_V5> on every code pair for E4M3 / E3M4 / E2M5 under the
    five OF / UF switch sets, and E5M2 with the adder wrap off; bit-exact, path_stats["v5mx"] == 0.

Every test prints one "FM ..." line with a token per launch (_one_log_line_per_test; run with -s to keep
them: profiles/flag_matrix/flag_matrix.log).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import golden_io as gio
from tests import pairs_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


# ------------------------------------------------------------------------------------------ launches
def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype=dtype, device=DEV)


def _stop_on_device_error(fn):
    """A HIP error (not a wrong value) ends the session: nothing more is started on a device that faulted."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kw):
        try:
            return fn(*args, **kw)
        except RuntimeError as ex:
            pytest.exit(f"device error in {fn.__name__}: {ex}", returncode=3)
    return run


@_stop_on_device_error
def _matmul_raw(A, B, E, M, bA, bB, bR, table, flags):
    """fp8a_matmul with a caller-owned workspace of the queried size: (C, flag word, path counters,
    fallback counters) of this one launch."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    Mr, K = A.shape
    N = B.shape[1]
    At, Bt = _dev(A), _dev(B)
    C = torch.empty((Mr, N), dtype=torch.float32, device=DEV)
    ws = torch.zeros(max(int(L.fp8a_matmul_workspace_size_mnk(Mr, N, K)), 256), dtype=torch.uint8, device=DEV)
    bB = np.asarray(bB, np.int32).reshape(-1)
    tA, tB, tR = _dev([bA], torch.int32), _dev(bB, torch.int32), _dev([bR], torch.int32)
    tab = torch.as_tensor(np.ascontiguousarray(table, np.int32))
    _lib.path_stats(reset=True)
    _lib.fallback_stats(reset=True)
    rc = L.fp8a_matmul(_lib.dev_ptr(At), K, _lib.dev_ptr(Bt), N, 1, _lib.dev_ptr(C), N, Mr, N, K, E, M,
                       _lib.dev_ptr(tA), _lib.dev_ptr(tB), 0 if bB.size == 1 else 1, _lib.dev_ptr(tR),
                       _lib.host_ptr(tab), flags, _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "fp8a_matmul")
    torch.cuda.synchronize()
    flag = int(ws[:4].view(torch.int32).item())
    return C.cpu().numpy(), flag, _lib.path_stats(reset=True), _lib.fallback_stats(reset=True)


@_stop_on_device_error
def _dw1x1_raw(x, w, E, M, bA, bW, bR, table, flags):
    """fp8a_conv2d on a 1 x 1 depthwise layer with a caller-owned workspace: (y, gate word, path counters,
    fallback counters)."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    Bn, C, H, W = x.shape
    xt, wt = _dev(x), _dev(w)
    y = torch.empty((Bn, C, H, W), dtype=torch.float32, device=DEV)
    n = int(L.fp8a_conv2d_workspace_size(Bn, C, H, W, C, 1, 1, 1, 1, 0, 0, 1, 1, C))
    ws = torch.zeros(max(n, 256), dtype=torch.uint8, device=DEV)
    tA, tW, tR = _dev([bA], torch.int32), _dev(bW, torch.int32), _dev([bR], torch.int32)
    tab = torch.as_tensor(np.ascontiguousarray(table, np.int32))
    _lib.path_stats(reset=True)
    _lib.fallback_stats(reset=True)
    rc = L.fp8a_conv2d(_lib.dev_ptr(xt), _lib.dev_ptr(wt), _lib.dev_ptr(y), Bn, C, H, W, C, 1, 1, 1, 1, 0, 0, 1, 1, C,
                       E, M, _lib.dev_ptr(tA), _lib.dev_ptr(tW), _lib.dev_ptr(tR), _lib.host_ptr(tab), flags,
                       _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "fp8a_conv2d")
    torch.cuda.synchronize()
    gate = int(ws[:4].view(torch.int32).item())
    return y.cpu().numpy(), gate, _lib.path_stats(reset=True), _lib.fallback_stats(reset=True)


def _flag_text(fl):
    if fl & pc.V5:
        return f"v5 ofuf{int(bool(fl & pc.OFUF))} of{int(bool(fl & pc.OF_OPT))} uf{int(bool(fl & pc.UF_OPT))}"
    return (f"a{fl & 1} s{(fl >> 1) & 1} q{(fl >> 2) & 1} g{(fl >> 3) & 1}" + (" tb" if fl & pc.TB else ""))


_LINE = []


@pytest.fixture(autouse=True)
def _one_log_line_per_test():
    """`FM <test> <format-table-biases> <TMode> <flags>:<what ran> ...`, one token a launch.  <flags>: the
    bits approx, s2n, qbma, gclip (v5: v, then ofuf, of_opt, uf_opt); <what ran>: the path counter that
    moved (fast, f8mx, tt, tt16; `!` after it: the flag word came back nonzero, e.g. the gated exact kernel
    reran flagged tiles), or for the tensor-bias layer valu (conv_tb_fast_kernel, gate 0), valu>direct (its
    gate raised: conv_tb_direct_kernel recomputed the launch) or direct (conv_tb_direct_kernel alone)."""
    del _LINE[:]
    yield
    if _LINE:
        print("FM", *_LINE)


def _log(head, fl, paths, flag, tb=False):
    if not _LINE:
        _LINE.append(head)
    bits = "v" + "".join(str(int(bool(fl & f))) for f in (pc.OFUF, pc.OF_OPT, pc.UF_OPT)) if fl & pc.V5 else \
        "".join(str(int(bool(fl & f))) for f in (pc.APPROX, pc.S2N, pc.QBMA, pc.GCLIP))
    if tb:
        ran = "direct" if not fl & pc.S2N or fl & pc.GCLIP else "valu>direct" if flag else "valu"
    else:
        ran = "+".join(f"{k}" if v == 1 else f"{k}x{v}" for k, v in paths.items() if v) + ("!" if flag else "")
    _LINE.append(f"{bits}:{ran}")


def _terms_equal(got, ref, a, b, what):
    same = pc.same_bits(got, ref)
    if not same.all():
        i, j = (int(v) for v in np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} terms differ; first a={a[i]!r} b={b[j]!r}: "
                             f"got {got[i, j]!r} oracle {ref[i, j]!r}")


def _only(paths, name):
    return paths[name] == 1 and sum(v for k, v in paths.items() if k != name) == 0


# ------------------------------------------------------------------------------------------ coverage guard
def test_parametrisation_covers_every_table_mode():
    """Not a check of any kernel: the tables the tests below run give, per mantissa width, every packing
    mode of pack_table that exists for it (pairs_cases.table_mode restates the rule), seven in all, and the
    sum tests pick one table of each."""
    seen = set()
    for (E, M) in pc.FORMATS:
        modes = {pc.table_mode(t, M) for t in pc.tables(E, M).values()}
        assert modes == pc.modes_of_width(M), (E, M, modes)
        assert {pc.table_mode(pc.tables(E, M)[n], M) for n in _one_table_per_mode(E, M)} == modes
        seen |= modes
    assert seen == set(pc.TM_NAMES)
    syn = pc.synthetic_tables(5)
    assert syn["s_w2s"].min() == -2 and syn["s_w2s"].max() == 1 and syn["s_w2u"].max() == 3 and syn["s_w2u"].min() == 0
    assert syn["s_lut"].min() == -3 and syn["s_lut"].max() == 4 and set(np.unique(syn["s_w1u"])) == {0, 1}


def _one_table_per_mode(E, M):
    out = {}
    for name, t in pc.tables(E, M).items():
        out.setdefault(pc.table_mode(t, M), name)
    return list(out.values())


# ------------------------------------------------------------------------------------------ terms (v9)
V9_PARAMS = [(E, M, name, tr) for (E, M) in pc.FORMATS for name in pc.tables(E, M) for tr in pc.V9_TRIPLES[(E, M)]]
V9_IDS = [f"E{E}M{M}-{name}-{'_'.join(map(str, tr))}" for (E, M, name, tr) in V9_PARAMS]


def _run_term_case(E, M, tname, biases, fl):
    bA, bB, bR = biases
    tab = pc.tables(E, M)[tname]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bB)
    A, B = a.reshape(-1, 1), b.reshape(1, -1)
    C, flag, paths, fb = _matmul_raw(A, B, E, M, bA, bB, bR, tab, fl)
    mode = pc.table_mode(tab, M, bool(fl & pc.APPROX))
    _log(f"terms E{E}M{M}-{tname}-{'_'.join(map(str, biases))} {mode}", fl, paths, flag)
    ref = orc.terms(A, B, E, M, bA, bB, bR, tab, fl)[:, 0, :]
    _terms_equal(C, ref, a, b, f"E{E}M{M} {tname} {mode} {biases} [{_flag_text(fl)}]")
    want = pc.expected_matmul_path(E, M, tab, fl, K=1)
    assert _only(paths, want), f"[{_flag_text(fl)}] expected one `{want}` launch, counters say {paths}"
    if not (fl & pc.S2N and fl & pc.QBMA) or fl & pc.GCLIP:
        assert want == "fast"


@pytest.mark.parametrize("E,M,tname,biases", V9_PARAMS, ids=V9_IDS)
def test_terms_every_code_pair_all_flags(E, M, tname, biases):
    for fl in pc.v9_flag_words(False):  # approx on: the 8 (s2n, qbma, gclip) combinations
        _run_term_case(E, M, tname, biases, fl)


@pytest.mark.parametrize("E,M,biases", [(E, M, tr) for (E, M) in pc.FORMATS for tr in pc.V9_TRIPLES[(E, M)]],
                         ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_terms_every_code_pair_approx_off(E, M, biases):
    tname = next(iter(pc.tables(E, M)))  # (the table is irrelevant with approx off)
    for fl in pc.v9_flag_words(True)[8:]:
        _run_term_case(E, M, tname, biases, fl)


# ------------------------------------------------------------------------------------------ sums
def _grid(rng, E, M, shape, bias, zero_frac):
    """Values of the (E, M, bias) grid, exponent field in the top 9 codes (subnormals included where E is
    small), random signs, a fraction of zeros."""
    emax = (1 << E) - 1
    bias = np.broadcast_to(np.asarray(bias), shape)
    expo = rng.integers(max(0, emax - 8), emax + 1, size=shape)
    mant = rng.integers(0, 1 << M, size=shape)
    v = np.where(expo == 0, np.ldexp(mant / 2.0 ** M, 1 - bias), np.ldexp(1.0 + mant / 2.0 ** M, expo - bias))
    v = v * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(shape) < zero_frac] = 0.0
    return v.astype(np.float32)


SUM_PARAMS = [(E, M, name, shape) for (E, M) in pc.FORMATS for name in _one_table_per_mode(E, M)
              for shape in ((65, 17, 63), (130, 300, 129))]


@pytest.mark.parametrize("E,M,tname,shape", SUM_PARAMS,
                         ids=[f"E{E}M{M}-{n}-{'x'.join(map(str, s))}" for (E, M, n, s) in SUM_PARAMS])
def test_sums_all_flags_within_bar_and_deterministic(E, M, tname, shape):
    Mr, K, N = shape
    rng = np.random.default_rng(Mr * 1000 + K * 10 + N + E)
    h = 1 << (E - 1)
    bA, bR = h + 2, h + 4
    bB = rng.integers(h + 4, h + 7, size=N).astype(np.int32)
    A = _grid(rng, E, M, (Mr, K), bA, 0.4)
    B = _grid(rng, E, M, (K, N), bB[None, :], 0.1)
    tab = pc.tables(E, M)[tname]
    mode = pc.table_mode(tab, M)
    flags = pc.v9_flag_words(False)
    with ThreadPoolExecutor(len(flags)) as ex:  # the oracle's 8 references, once each
        refs = list(ex.map(lambda fl: orc.matmul(A, B, E, M, bA, bB, bR, tab, fl, with_abs=True), flags))
    for fl, (Cref, S) in zip(flags, refs):
        C, flag, paths, fb = _matmul_raw(A, B, E, M, bA, bB, bR, tab, fl)
        _log(f"sums E{E}M{M}-{tname}-{Mr}x{K}x{N} {mode}", fl, paths, flag)
        want = pc.expected_matmul_path(E, M, tab, fl, K=K)
        assert _only(paths, want), f"[{_flag_text(fl)}] expected one `{want}` launch, counters say {paths}"
        err = np.abs(C.astype(np.float64) - Cref)
        tol = gio.sum_tolerance(S.astype(np.float64))
        assert np.all(err <= tol), f"[{_flag_text(fl)}] {np.count_nonzero(err > tol)} sums outside the bar, " \
                                   f"worst {np.max(err / tol):.3g} x the bar"
        C2 = _matmul_raw(A, B, E, M, bA, bB, bR, tab, fl)[0]
        assert np.array_equal(C.view(np.uint32), C2.view(np.uint32)), f"[{_flag_text(fl)}] not deterministic"


# ------------------------------------------------------------------------------------------ tensor bias
TB_PARAMS = [(E, M, name, tr) for (E, M) in pc.FORMATS for name in pc.tables(E, M) for tr in pc.TB_TRIPLES[(E, M)]]


@pytest.mark.parametrize("E,M,tname,biases", TB_PARAMS,
                         ids=[f"E{E}M{M}-{n}-{'_'.join(map(str, tr))}" for (E, M, n, tr) in TB_PARAMS])
def test_tensor_bias_depthwise_1x1_every_code_pair(E, M, tname, biases):
    """Every output of the 1 x 1 depthwise layer is one tensor-bias term: no assumption about the terms of
    zero weights.  approx off runs with the format's first table only (the table is irrelevant)."""
    bA, bW_, bR = biases
    names = list(pc.tables(E, M))
    tab = pc.tables(E, M)[tname]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bW_)
    C = 256
    x = np.broadcast_to(a.reshape(1, 1, 16, 16), (1, C, 16, 16)).copy()
    w = b.reshape(C, 1, 1, 1).copy()
    bW = np.full(C, bW_, np.int32)
    for fl in pc.v9_flag_words(tname == names[0]):
        y, gate, paths, fb = _dw1x1_raw(x, w, E, M, bA, bW, bR, tab, fl)
        form = "conv_tb_fast_kernel+gated_direct" if fl & pc.S2N and not fl & pc.GCLIP else "conv_tb_direct_kernel"
        _log(f"tb1x1 E{E}M{M}-{tname}-{'_'.join(map(str, biases))} {pc.table_mode(tab, M)}", fl, paths, gate,
             tb=True)
        ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, bA, bW, bR, tab, fl | orc.TB)[:, 0, :]
        got = y[0].reshape(C, 256).T  # [pixel = a index, channel = b index]
        _terms_equal(got, ref, a, b, f"E{E}M{M} {tname} {biases} [{_flag_text(fl | pc.TB)}] {form}")
        # the gated direct kernel recomputes only what the VALU form flagged; without the VALU form no gate exists
        assert (fb["tb_launches"] != 0) == (gate != 0), (gate, fb)
        if not (fl & pc.S2N) or fl & pc.GCLIP:
            assert gate == 0


# ------------------------------------------------------------------------------------------ v5 off the matrix core
V5_PARAMS = [(E, M, name, b) for (E, M) in pc.FORMATS for name in pc.v5_tables(E, M) for b in pc.v5_biases(E)]


@pytest.mark.parametrize("E,M,tname,b", V5_PARAMS, ids=[f"E{E}M{M}-{n}-b{b}" for (E, M, n, b) in V5_PARAMS])
def test_v5_fast_kernel_every_code_pair(E, M, tname, b):
    """gemm_fast_kernel<TM_V5>: E4M3 / E3M4 / E2M5 under the five switch sets; E5M2 only with the adder wrap
    off (with it on, gemm_v5mx_kernel runs: tests/test_gpu_v5.py)."""
    tab = pc.v5_tables(E, M)[tname]
    a = pc.all_codes(E, M, b)
    A, B = a.reshape(-1, 1), a.reshape(1, -1)
    for sw in pc.V5_FLAGS:
        if (E, M) == (5, 2) and sw[0]:
            continue
        fl = pc.v5_flag_word(*sw)
        C, flag, paths, fb = _matmul_raw(A, B, E, M, b, b, b, tab, fl)
        _log(f"v5 E{E}M{M}-{tname}-b{b} TM_V5", fl, paths, flag)
        ref = orc.terms(A, B, E, M, b, b, b, tab, fl)[:, 0, :]
        _terms_equal(C, ref, a, a, f"v5 E{E}M{M} {tname} b={b} [{_flag_text(fl)}]")
        assert paths["v5mx"] == 0 and _only(paths, "fast"), paths


# ------------------------------------------------------------------------------------------ regressions
# What the matrix found when it first ran, each narrowed to the one launch that showed it.
def _tb_case(E, M, tname, biases, fl):
    bA, bW_, bR = biases
    tab = pc.tables(E, M)[tname]
    a, b = pc.all_codes(E, M, bA), pc.all_codes(E, M, bW_)
    x = np.broadcast_to(a.reshape(1, 1, 16, 16), (1, 256, 16, 16)).copy()
    y, gate, paths, fb = _dw1x1_raw(x, b.reshape(256, 1, 1, 1).copy(), E, M, bA, np.full(256, bW_, np.int32), bR, tab, fl)
    _log(f"tb1x1-regression E{E}M{M}-{tname}-{'_'.join(map(str, biases))} {pc.table_mode(tab, M)}", fl, paths, gate,
         tb=True)
    ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, bA, bW_, bR, tab, fl | orc.TB)[:, 0, :]
    return y[0].reshape(256, 256).T, ref, a, b, gate


@pytest.mark.parametrize("biases", [(7, 9, 8), (9, 9, 12)])
def test_regression_tb_valu_form_keeps_the_sign_without_qbma(biases):
    """conv_tb_fast_kernel applied the F7 sign rule (a negative g whose Q_R(g) is 0 gives a positive term)
    with quant_btw_mult_accu off as well, where g is never quantized and keeps its sign: E4M3, s2n on,
    qbma off, gclip off, every product with |g| = 2^-bR came back positive.  Gate 0: the VALU form itself
    (not the direct kernel behind it) produced these terms."""
    fl = pc.flag_word(True, True, False, False)
    got, ref, a, b, gate = _tb_case(4, 3, "nocomp", biases, fl)
    assert gate == 0, "the VALU form did not produce these terms"
    g = np.outer(a.astype(np.float64), b.astype(np.float64))
    assert np.count_nonzero(g == -2.0 ** -biases[2]) > 0, "the case must hold products equal to -2^-bR"
    _terms_equal(got, ref, a, b, f"E4M3 nocomp {biases} [{_flag_text(fl | pc.TB)}]")


@pytest.mark.parametrize("biases,every", [((10, 10, -13), False), ((16, 17, 0), True)])
def test_regression_tb_golden_clip_with_wrapped_max_norm(biases, every):
    """Tensor-bias max_norm is the reference's int32 power 2**(max_expo - bR) times (2 - 2^-M): 0 once
    max_expo - bR >= 32 and -2^31 * 1.75 at 31.  With golden_clip_OF and per-product quantization every
    nonzero product (at 31: every product, zeros included) then decodes as the grid's largest code.  The
    oracle and dfmt() computed a float power there (found by the oracle-vs-reference pin)."""
    fl = pc.flag_word(True, False, True, True)
    got, ref, a, b, _ = _tb_case(5, 2, "zero", biases, fl)
    top = np.float32(1.75 * 2.0 ** (31 - biases[2]))
    hit = np.ones(ref.shape, bool) if every else np.outer(a, b) != 0
    assert np.all(np.abs(ref[hit]) == top) and np.all(ref[~hit] == 0)
    _terms_equal(got, ref, a, b, f"E5M2 zero {biases} [{_flag_text(fl | pc.TB)}]")
