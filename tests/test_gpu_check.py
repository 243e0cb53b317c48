"""The fused self-check on the GPU (fp8a_matmul_check / fp8a_conv2d_check, gemm_check.h): the
approx sum C and its scale S against the CPU oracle, the golden sum G against a host golden built
from its definition (v9:30-36), the statistics against a recomputation from the returned tensors,
the counts against numpy + oracle.decompose, the F9 known answer, off-grid operands, determinism,
the prod= comparison, the convolution form against per-group matmul checks, the operators'
self_check_mode and the per-layer report.

Tolerances: C and S carry the project's bar 1e-5 * S + tiny (fp32 sums of <= 67 terms in another
order move by far less); G the same bar on its own scale sum_k |g_k|; the double sums are sums of
at most 10^4 doubles, so any reordering moves them by at most n 2^-53 < 1e-9 relative; max and
counts are order-free and must be exact."""
import itertools

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = 1e-30
FORMATS = {"e4m3": (4, 3), "e3m4": (3, 4), "e2m5": (2, 5), "e5m2": (5, 2)}
FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def _table(E, M, zero=False):
    from fp8_quantization_amd.error_tables import get_error_table_NN
    if zero or (E, M) == (5, 2):  # (the reference ships no E5M2 table: the zero table)
        return torch.zeros((2 ** M, 2 ** M), dtype=torch.int32)
    return get_error_table_NN(E, M, withComp=False, dnsmp_factor=3)


def _qbias(mx, E, M):
    return int(np.rint(2.0 ** E - np.log2(mx) + np.log2(2.0 - 2.0 ** -M) - 1.0))


def _quantized(rng, shape, E, M, mx, zeros):
    """FP8-quantized values (the project's quantizer on the GPU): `zeros` of them zero, ~15 % below
    the grid's min_norm (subnormals).  Returns (float32 numpy array, its int bias)."""
    import fp8_quantization_amd as fa
    b = _qbias(mx, E, M)
    v = rng.standard_normal(shape).astype(np.float32)
    small = rng.random(shape) < 0.15
    v[small] = (np.sign(v[small]) * 2.0 ** (1 - b) * rng.uniform(0.1, 1.5, size=int(small.sum()))).astype(np.float32)
    v[rng.random(shape) < zeros] = 0.0
    q, bias = fa.fp8_fake_quantize(torch.from_numpy(v).to(DEV), torch.tensor([mx], dtype=torch.float32), 1 + E + M, M)
    assert int(bias.item()) == b
    return q.cpu().numpy(), b


def _min_norm(b, tb):
    return np.float32(2.0 ** (1 - b)) if (not tb or 1 - b >= 0) else np.float32(0.0)


def _reference(A, B, E, M, bA, bB, bR, table, flags):
    """Oracle C / S, host golden G and its scale, and the exact counts."""
    from fp8_quantization_amd import _lib
    from oracle import oracle as orc
    tb, s2n, qbma, gclip = (bool(flags & f) for f in (_lib.TB, _lib.S2N, _lib.QBMA, _lib.GCLIP))
    N = B.shape[1]
    bBv = np.broadcast_to(np.asarray(bB, dtype=np.int64).reshape(-1), (N,)) if np.size(bB) in (1, N) else None
    C, S = orc.matmul(A, B, E, M, bA, bBv, bR, table.numpy(), flags, with_abs=True)
    g = (A[:, :, None] * B[None]).astype(np.float32)
    if qbma:
        g = orc.quant(g, E, M, bR, tb=tb, clip=gclip)
    ref = dict(C=C, S=S, G=g.astype(np.float64).sum(axis=1), Gabs=np.abs(g).astype(np.float64).sum(axis=1))
    ref["a_norm"] = int((np.abs(A) >= _min_norm(bA, tb)).sum())
    mnB = np.array([_min_norm(int(b), tb) for b in bBv], dtype=np.float32)
    ref["b_norm"] = int((np.abs(B) >= mnB[None, :]).sum())
    if not s2n:  # v9:87
        eA, _ = orc.decompose(A, E, M, bA, tb=tb)
        eB = np.empty(B.shape, np.int32)
        for b in np.unique(bBv):
            cols = bBv == b
            eB[:, cols] = orc.decompose(B[:, cols], E, M, int(b), tb=tb)[0]
        ref["r_norm"] = int(((eA[:, :, None] > 0) & (eB[None] > 0) & (np.abs(g) >= _min_norm(bR, tb))).sum())
    return ref


def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def _check_stats_against_tensors(st, C, G):
    """max_err bit for bit, the double sums within 1e-9 relative, from the returned fp32 C / G."""
    e = np.abs(G - C)
    assert e.dtype == np.float32
    assert st.n_out == C.size
    assert np.float32(st.max_err).tobytes() == e.max().tobytes()
    e64, g64 = e.astype(np.float64), G.astype(np.float64)
    assert _close(st.sum_err, e64.sum()), (st.sum_err, e64.sum())
    assert _close(st.sum_err2, (e64 * e64).sum()), (st.sum_err2, (e64 * e64).sum())
    assert _close(st.sum_gold2, (g64 * g64).sum()), (st.sum_gold2, (g64 * g64).sum())


def _run_matmul_case(rng, fmt, s2n, qbma, gclip, shape, tb, quantize=True, table=None):
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    E, M = FORMATS[fmt]
    Mr, K, N = shape
    if quantize:
        A, bA = _quantized(rng, (Mr, K), E, M, 4.0, 0.5)
        B, b0 = _quantized(rng, (K, N), E, M, 2.0, 0.2)
    else:  # unquantized operands: off every FP8 grid
        A, bA = rng.standard_normal((Mr, K)).astype(np.float32), _qbias(4.0, E, M)
        B, b0 = rng.standard_normal((K, N)).astype(np.float32), _qbias(2.0, E, M)
    bB = b0 + (np.arange(N) % 3) - 1 if N > 1 else np.array([b0])  # (every column its own bias)
    bR = bA
    table = _table(E, M) if table is None else table
    flags = fa.make_flags(True, s2n, qbma, gclip, tensor_bias=tb)
    C, G, st = fa.approx_matmul_check(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), E, M, bA,
                                      torch.from_numpy(bB.astype(np.int32)), bR, table, flags=flags)
    C, G, S = C.cpu().numpy(), G.cpu().numpy(), st.S.cpu().numpy()
    ref = _reference(A, B, E, M, bA, bB, bR, table, flags)
    tag = (fmt, s2n, qbma, gclip, shape, tb)
    dC, dS, dG = np.abs(C - ref["C"]), np.abs(S - ref["S"]), np.abs(G - ref["G"])
    print(tag, "max |C-oracle|/S", float((dC / np.maximum(ref["S"], TINY)).max()),
          "max |S-oracle|/S", float((dS / np.maximum(ref["S"], TINY)).max()),
          "max |G-golden|/sum|g|", float((dG / np.maximum(ref["Gabs"], TINY)).max()), "max_err", st.max_err)
    assert np.all(dC <= 1e-5 * ref["S"] + TINY), tag
    assert np.all(dS <= 1e-5 * ref["S"] + TINY), tag
    assert np.all(dG <= 1e-5 * ref["Gabs"] + TINY), tag
    _check_stats_against_tensors(st, C, G)
    assert (st.a_norm, st.a_total) == (ref["a_norm"], Mr * K), tag
    assert (st.b_norm, st.b_total) == (ref["b_norm"], K * N), tag
    if s2n:
        assert (st.r_norm, st.r_total) == (0, 0) and st.r_norm_pct is None
    else:
        assert (st.r_norm, st.r_total) == (ref["r_norm"], Mr * K * N), tag
    assert st.has_prod == 0 and st.prod_max_abs == 0.0 and st.prod_max_rel == 0.0
    return st


SHAPES = [((70, 37, 67), False), ((1, 1, 1), False), ((130, 16, 3), False), ((65, 9, 1), True)]


@pytest.mark.parametrize("s2n,qbma,gclip", list(itertools.product((False, True), repeat=3)),
                         ids=lambda v: str(int(v)))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_matmul_check_matrix(fmt, s2n, qbma, gclip):
    rng = np.random.default_rng(1000 * sorted(FORMATS).index(fmt) + 4 * s2n + 2 * qbma + gclip)
    for shape, tb in SHAPES:
        _run_matmul_case(rng, fmt, s2n, qbma, gclip, shape, tb)


@pytest.mark.parametrize("tb", (False, True), ids=("int", "tb"))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_known_answer_zero_table(fmt, tb):
    """F9: on-grid operands and a zero table give G == C bit for bit."""
    import fp8_quantization_amd as fa
    E, M = FORMATS[fmt]
    rng = np.random.default_rng(7)
    Mr, K, N = (65, 9, 1) if tb else (70, 37, 67)
    A, bA = _quantized(rng, (Mr, K), E, M, 4.0, 0.5)
    B, bB = _quantized(rng, (K, N), E, M, 2.0, 0.2)
    flags = fa.make_flags(True, True, True, False, tensor_bias=tb)
    C, G, st = fa.approx_matmul_check(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), E, M, bA, bB, bA,
                                      _table(E, M, zero=True), flags=flags)
    assert np.abs(C.cpu().numpy()).max() > 0
    assert C.cpu().numpy().tobytes() == G.cpu().numpy().tobytes()
    assert st.max_err == 0.0 and st.sum_err == 0.0 and st.sum_err2 == 0.0


def test_no_comp_table_has_error():
    import fp8_quantization_amd as fa
    rng = np.random.default_rng(8)
    A, bA = _quantized(rng, (70, 37), 4, 3, 4.0, 0.5)
    B, bB = _quantized(rng, (37, 67), 4, 3, 2.0, 0.2)
    _, _, st = fa.approx_matmul_check(torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV), 4, 3, bA, bB, bA,
                                      _table(4, 3), flags=fa.make_flags(True, True, True, False))
    assert st.max_err > 0 and st.rmse > 0 and np.isfinite(st.sqnr_db)


@pytest.mark.parametrize("s2n,qbma", list(itertools.product((False, True), repeat=2)), ids=lambda v: str(int(v)))
def test_offgrid_operands(s2n, qbma):
    """Unquantized randn operands: G is the definition, not a zero-table approx launch."""
    rng = np.random.default_rng(9)
    st = _run_matmul_case(rng, "e4m3", s2n, qbma, False, (70, 37, 67), False, quantize=False)
    # off the grid even a zero table leaves golden != approx (F9 needs on-grid operands)
    z = _run_matmul_case(rng, "e4m3", s2n, qbma, False, (70, 37, 67), False, quantize=False,
                         table=_table(4, 3, zero=True))
    assert st.max_err > 0 and z.max_err > 0


def test_determinism():
    import fp8_quantization_amd as fa
    rng = np.random.default_rng(10)
    A, bA = _quantized(rng, (130, 40), 4, 3, 4.0, 0.5)
    B, bB = _quantized(rng, (40, 70), 4, 3, 2.0, 0.2)
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    fl = fa.make_flags(True, False, True, False)
    r1 = fa.approx_matmul_check(a, b, 4, 3, bA, bB, bA, _table(4, 3), flags=fl)
    r2 = fa.approx_matmul_check(a, b, 4, 3, bA, bB, bA, _table(4, 3), flags=fl)
    assert len(r1[2].raw) == 96 and r1[2].raw == r2[2].raw
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and torch.equal(r1[2].S, r2[2].S)


def test_prod_comparison():
    import fp8_quantization_amd as fa
    rng = np.random.default_rng(11)
    A, bA = _quantized(rng, (70, 37), 4, 3, 4.0, 0.5)
    B, bB = _quantized(rng, (37, 67), 4, 3, 2.0, 0.2)
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    fl = fa.make_flags(True, True, True, False)
    tab = _table(4, 3)
    prod = fa.approx_matmul(a, b, 4, 3, bA, bB, bA, tab, flags=fl)
    C, _, st = fa.approx_matmul_check(a, b, 4, 3, bA, bB, bA, tab, flags=fl, prod=prod)
    print("prod_max_rel", st.prod_max_rel, "prod_max_abs", st.prod_max_abs)
    assert st.has_prod == 1 and st.prod_max_rel <= 1e-5
    Cn, S, P = C.cpu().numpy(), st.S.cpu().numpy(), prod.cpu().numpy()
    assert np.float32(st.prod_max_abs).tobytes() == np.abs(P - Cn).max().tobytes()
    # one element moved by a known delta (a quarter of its scale: far above the bar everywhere else)
    i, j = np.unravel_index(np.argmax(S), S.shape)
    P2 = P.copy()
    P2[i, j] = np.float32(P2[i, j] + np.float32(0.25) * S[i, j])
    _, _, st2 = fa.approx_matmul_check(a, b, 4, 3, bA, bB, bA, tab, flags=fl, prod=torch.from_numpy(P2).to(DEV))
    d = np.abs(P2 - Cn)
    assert (i, j) == np.unravel_index(np.argmax(d), d.shape)
    assert np.float32(st2.prod_max_abs).tobytes() == d.max().tobytes()
    want = np.float32(d[i, j]) / np.maximum(S[i, j], FLT_MIN)
    assert abs(np.float32(st2.prod_max_rel) - want) <= np.spacing(want)


# ------------------------------------------------------------------------------------ conv
CONV_CASES = {
    "s2p1": dict(x=(2, 5, 9, 9), w=(6, 5, 3, 3), stride=(2, 2), padding=(1, 1), groups=1),
    "groups2": dict(x=(2, 4, 9, 9), w=(6, 2, 3, 3), stride=(1, 1), padding=(1, 1), groups=2),
    "depthwise": dict(x=(2, 5, 9, 9), w=(5, 1, 3, 3), stride=(1, 1), padding=(1, 1), groups=5),
    # non-square (tests/exact_sums.py: GEO_CONVS dense-geo, GEO_TBDW kh5-s2): every (h, w) pair differs somewhere
    "dense-geo": dict(x=(2, 16, 15, 17), w=(24, 16, 3, 3), stride=(2, 1), padding=(1, 2), dilation=(1, 2), groups=1),
    "kh5-s2": dict(x=(2, 8, 13, 10), w=(8, 1, 5, 3), stride=(2, 2), padding=(2, 1), groups=8),
}


@pytest.mark.parametrize("s2n", (False, True), ids=("nos2n", "s2n"))
@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv_check_equals_per_group_matmul_check(case, s2n):
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_calculation import ApproxConv2dMixin
    c = CONV_CASES[case]
    E, M = 4, 3
    rng = np.random.default_rng(12)
    xq, bA = _quantized(rng, c["x"], E, M, 4.0, 0.5)
    w = rng.standard_normal(c["w"]).astype(np.float32) * 0.5
    Cout, cig, kh, kw = c["w"]
    wq, wb = fa.fp8_fake_quantize(torch.from_numpy(w).to(DEV), torch.from_numpy(np.abs(w).reshape(Cout, -1).max(1)),
                                  1 + E + M, M, per_row=True)
    bW = wb.reshape(-1).to(torch.int32)
    x = torch.from_numpy(xq).to(DEV)
    tab = _table(E, M)
    fl = fa.make_flags(True, s2n, True, False)
    dil = c.get("dilation", (1, 1))
    geo = dict(stride=c["stride"], padding=c["padding"], dilation=dil, groups=c["groups"])
    prod = fa.approx_conv2d(x, wq, E, M, bA, bW, bA, tab, flags=fl, **geo)
    y, G, st = fa.approx_conv2d_check(x, wq, E, M, bA, bW, bA, tab, flags=fl, prod=prod, **geo)
    print(case, "prod_max_rel", st.prod_max_rel, "max_err", st.max_err)
    assert st.prod_max_rel <= 1e-5
    groups, cog = c["groups"], Cout // c["groups"]
    Bn, _, Ho, Wo = y.shape
    tot = dict(n_out=0, a_norm=0, a_total=0, b_norm=0, b_total=0, r_norm=0, r_total=0, sum_err=0.0, sum_err2=0.0,
               sum_gold2=0.0, max_err=0.0)
    for g in range(groups):
        rows = ApproxConv2dMixin.im2col(None, x[:, g * cig:(g + 1) * cig], kh, kw, c["stride"], c["padding"], dil)
        wg = wq[g * cog:(g + 1) * cog].reshape(cog, -1).t()
        Cg, Gg, sg = fa.approx_matmul_check(rows, wg, E, M, bA, bW[g * cog:(g + 1) * cog], bA, tab,
                                            flags=fl | (_lib.TB if cog == 1 else 0))
        nchw = lambda t: t.reshape(Bn, Ho, Wo, cog).permute(0, 3, 1, 2)  # noqa: E731
        assert torch.equal(y[:, g * cog:(g + 1) * cog], nchw(Cg))
        assert torch.equal(G[:, g * cog:(g + 1) * cog], nchw(Gg))
        assert torch.equal(st.S[:, g * cog:(g + 1) * cog], nchw(sg.S))
        for k in tot:
            tot[k] = max(tot[k], getattr(sg, k)) if k == "max_err" else tot[k] + getattr(sg, k)
    for k in ("n_out", "a_norm", "a_total", "b_norm", "b_total", "r_norm", "r_total"):
        assert getattr(st, k) == tot[k], k
    assert np.float32(st.max_err).tobytes() == np.float32(tot["max_err"]).tobytes()
    for k in ("sum_err", "sum_err2", "sum_gold2"):
        assert _close(getattr(st, k), tot[k]), k
    _check_stats_against_tensors(st, y.cpu().numpy(), G.cpu().numpy())
    assert st.n_out == y.numel() and st.a_total == groups * Bn * Ho * Wo * cig * kh * kw


# ------------------------------------------------------------------------------------ operators
LABELS = ["====== Self-Checking Mode ======", "With Approximation    =", "With S2N & N2S Opt    =",
          "Quant btw Mult & Accu =", "Normal Values in A_2d :", "Normal Values in B_2d :", "Normal Values in R_3d :",
          "MatMul Max  Error     :", "MatMul Mean Error     :", "MatMul RMSE           :"]


def _calibrated(mod, shape, seed):
    g = torch.Generator().manual_seed(seed)
    mod = mod.to(DEV).eval()
    mod.quantized()
    mod.estimate_ranges()
    with torch.no_grad():
        mod(torch.randn(shape, generator=g).to(DEV))
    mod.fix_ranges()
    return mod, torch.randn(shape, generator=g).to(DEV)


def _on_off(mod, x, capsys):
    """(output with the mode off and the fusion switches off, output with the mode on, printed lines)."""
    mod.fuse_bn_act = mod.fuse_input_quant = mod.fuse_linear_block = False
    with torch.no_grad():
        y_off = mod(x)
    assert mod.last_self_check is None
    capsys.readouterr()
    del mod.fuse_bn_act, mod.fuse_input_quant, mod.fuse_linear_block  # (the class defaults: fusions on)
    mod.custom_approx_params["self_check_mode"] = True
    with torch.no_grad():
        y_on = mod(x)
    lines = [ln for ln in capsys.readouterr().out.split("\n") if ln]
    mod.custom_approx_params["self_check_mode"] = False
    return y_off, y_on, lines


def _assert_block(lines, s2n):
    want = [lab for lab in LABELS if not (s2n and "R_3d" in lab)]
    assert [ln[:len(lab)] for ln, lab in zip(lines, want)] == want and len(lines) == len(want)


NONPROD = ("n_out", "sum_err", "sum_err2", "sum_gold2", "a_norm", "a_total", "b_norm", "b_total", "r_norm", "r_total",
           "max_err")


@pytest.mark.parametrize("s2n", (False, True), ids=("nos2n", "s2n"))
def test_linear_operator_self_check(s2n, capsys):
    import fp8_quantization_amd as fa
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    from fp8_quantization_amd.resnet_workload import approx_qparams
    torch.manual_seed(3)
    mod = QCustomLinearTorch(in_features=37, out_features=19, bias=True,
                             **approx_qparams(with_s2nn2s_opt=s2n, withComp=False))
    mod, x = _calibrated(mod, (11, 37), 4)
    with torch.no_grad():  # (a trainable bias under autograd keeps the separate passes)
        assert mod.supports_input_quant_fusion
    y_off, y_on, lines = _on_off(mod, x, capsys)
    assert torch.equal(y_off, y_on)
    _assert_block(lines, s2n)
    st = mod.last_self_check
    assert st.has_prod == 1 and st.prod_max_rel <= 1e-5 and st.n_out == 11 * 19 and st.a_total == 11 * 37
    with torch.no_grad():
        xq = mod.activation_quantizer(x)
        wq, _ = mod.get_params()
    E, M, table, flags = mod._approx_config()
    _, _, direct = fa.approx_matmul_check(xq, wq.t(), E, M, mod.get_acts_fp_bias(), mod.get_weights_fp_bias(),
                                          mod.get_res_fp_bias(), table, flags=flags)
    for k in NONPROD:
        assert getattr(st, k) == getattr(direct, k), k
    with torch.no_grad():
        assert mod.supports_input_quant_fusion  # (the mode is off again)
        mod.custom_approx_params["self_check_mode"] = True
        assert not mod.supports_input_quant_fusion and not mod.tail_ok()


@pytest.mark.parametrize("groups", (1, 8), ids=("dense", "depthwise"))
def test_bnconv_operator_self_check(groups, capsys):
    import fp8_quantization_amd as fa
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch
    from fp8_quantization_amd.resnet_workload import approx_qparams
    torch.manual_seed(5)
    mod = QCustomBNConv2dTorch(in_channels=8, out_channels=8 if groups > 1 else 12, kernel_size=3, stride=1, padding=1,
                               groups=groups, bias=False, activation=nn.ReLU(), **approx_qparams(withComp=False))
    nn.init.kaiming_normal_(mod.weight, mode="fan_out", nonlinearity="relu")
    mod, x = _calibrated(mod, (2, 8, 9, 9), 6)
    assert mod.supports_bn_act_epilogue and mod.supports_input_quant_fusion
    y_off, y_on, lines = _on_off(mod, x, capsys)
    assert torch.equal(y_off, y_on)
    _assert_block(lines, True)
    st = mod.last_self_check
    assert st.has_prod == 1 and st.prod_max_rel <= 1e-5 and st.n_out == y_on.numel()
    with torch.no_grad():
        xq = mod.activation_quantizer(x)
        wq, _ = mod.get_params()
    E, M, table, flags = mod._approx_config()
    _, _, direct = fa.approx_conv2d_check(xq, wq, E, M, mod.get_acts_fp_bias(), mod.get_weights_fp_bias(),
                                          mod.get_res_fp_bias(), table, flags=flags, stride=mod.stride,
                                          padding=mod.padding, dilation=mod.dilation, groups=mod.groups)
    for k in NONPROD:
        assert getattr(st, k) == getattr(direct, k), k
    mod.custom_approx_params["self_check_mode"] = True
    assert not mod.supports_bn_act_epilogue and not mod.supports_input_quant_fusion
    assert mod._fused_epilogue() is None and not mod.block_epilogue_ok()


def test_custom_matmul_vectorize_self_check_block(capsys):
    import fp8_quantization_amd as fa
    rng = np.random.default_rng(13)
    A, bA = _quantized(rng, (70, 37), 4, 3, 4.0, 0.5)
    B, bB = _quantized(rng, (37, 67), 4, 3, 2.0, 0.2)
    a, b = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    for s2n in (False, True):
        capsys.readouterr()
        out = fa.custom_matmul_vectorize(a, b, 4, 3, bA, bB, bA, _table(4, 3), with_s2nn2s_opt=s2n,
                                         self_check_mode=True)
        lines = [ln for ln in capsys.readouterr().out.split("\n") if ln]
        _assert_block(lines, s2n)
        assert torch.equal(out, fa.custom_matmul_vectorize(a, b, 4, 3, bA, bB, bA, _table(4, 3), with_s2nn2s_opt=s2n))
        ref = _reference(A, B, 4, 3, bA, bB, bA, _table(4, 3), fa.make_flags(True, s2n, True, False))
        assert f"Normal Values in A_2d : {ref['a_norm']}/{A.size} = {100.0 * ref['a_norm'] / A.size:.1f}%" in lines


def test_capturing_stream_is_rejected():
    """A diagnostic, not for graphs: nothing is launched on a capturing stream."""
    import fp8_quantization_amd as fa
    from fp8_quantization_amd.error_report import layer_error_report
    a = torch.ones((4, 4), device=DEV)
    tab = _table(4, 3)
    fa.approx_matmul_check(a, a, 4, 3, 7, 7, 7, tab, flags=fa.make_flags())  # (warm: biases cached, library loaded)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a + 1.0  # (a node of its own: the graph is not empty)
        with pytest.raises(AssertionError, match="capturing"):
            fa.approx_matmul_check(a, a, 4, 3, 7, 7, 7, tab, flags=fa.make_flags())
        with pytest.raises(RuntimeError, match="capturing"):
            layer_error_report(nn.Identity(), a)


# ------------------------------------------------------------------------------------ report
def test_layer_error_report_resnet18():
    from fp8_quantization_amd.error_report import approx_layers, build_workload, format_report, layer_error_report
    from fp8_quantization_amd.resnet_workload import approx_layer_shapes, approx_macs_per_image
    torch.manual_seed(0)
    cfg = dict(expo_width=4, mant_width=3, dnsmp_factor=3, withComp=False, with_approx=True, with_s2nn2s_opt=True,
               quant_btw_mult_accu=True)
    model = build_workload("resnet18", 32, cfg, bn_stats_batches=1, cal_batch=2, device=DEV)
    x = torch.randn((2, 3, 32, 32), generator=torch.Generator().manual_seed(10)).to(DEV)
    with torch.no_grad():
        y_plain = model(x)
    shapes, hooks = approx_layer_shapes(model, 32)
    rows = layer_error_report(model, x)
    for h in hooks:
        h.remove()
    print(format_report(rows))
    assert [r["kind"] for r in rows].count("conv") == 20 and [r["kind"] for r in rows].count("linear") == 1
    assert len(rows) == 21 == len(approx_layers(model))
    for r in rows:
        M, N, K = r["shape"]
        assert r["macs"] == M * N * K * r["groups"] and M % 2 == 0
        assert r["prod_max_rel"] <= 1.0, r  # (units of the 1e-5 bar)
        assert r["r_norm_pct"] is None and 0.0 <= r["a_norm_pct"] <= 100.0 and 0.0 <= r["b_norm_pct"] <= 100.0
    assert sum(r["macs"] for r in rows) == 2 * approx_macs_per_image(shapes)
    assert rows[0]["shape"] == (2 * 16 * 16, 64, 3 * 7 * 7) and rows[-1]["shape"] == (2, 1000, 512)
    assert any(r["max"] > 0 for r in rows)
    assert all(not m.custom_approx_params["self_check_mode"] for _, m in approx_layers(model))
    with torch.no_grad():
        assert torch.equal(model(x), y_plain)  # (fused again, same network)
    # E4M3 withComp=True: the all-zero table of F3 -- golden == approx in every layer (F9)
    for _, m in approx_layers(model):
        m.custom_approx_params["withComp"] = True
    zero = layer_error_report(model, x)
    assert len(zero) == 21 and all(r["max"] == 0.0 for r in zero), [r["max"] for r in zero]
    assert all(r["prod_max_rel"] <= 1.0 for r in zero)
    assert all(not m.custom_approx_params["self_check_mode"] for _, m in approx_layers(model))
