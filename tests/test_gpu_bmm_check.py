"""The batched self-check on the GPU (fp8a_bmm_check, gemm_check_kernel over batch items): per batch item
the approx sum C and its scale S against the CPU oracle and the golden sum G against a host golden built from
its definition (v9:30-36); the counts against numpy + oracle.decompose; the whole call against per-item
fp8a_matmul_check calls bit for bit; the statistics against a recomputation from the returned tensors; off-grid
operands; the F9 known answer; determinism; the production cross-check of fp8a_bmm's clean and recomputed
tiles; the capturing stream; QCustomMatMul's self_check_mode and error_report's ``matmul`` rows.

Operands are head views cut from [nb0, M, nb1*K] / [nb0, K or N, nb1*...] buffers, so every batch stride is live.
Shapes: 2 x 3 items of 70 x 37 x 67 -- two row and two column tiles, both ragged, a K tail of 5 after two
16-steps -- plus 1 x 1 x 1 and N = 1.

Tolerances (test_gpu_check.py's): C and S carry the project's bar 1e-5 * S + tiny (fp32 sums of <= 37 terms in
another order move by far less), G the same bar on its own scale sum_k |g_k|; the double sums are sums of at
most 3 10^4 doubles, so any reordering moves them by at most n 2^-53 < 1e-9 relative; maxima and counts are
order-free and must be exact."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = 1e-30
FORMATS = {"e4m3": (4, 3), "e3m4": (3, 4), "e2m5": (2, 5), "e5m2": (5, 2)}
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
NB0, NB1, MR, K, N = 2, 3, 70, 37, 67
COUNTS = ("n_out", "a_norm", "a_total", "b_norm", "b_total", "r_norm", "r_total")
SUMS = ("sum_err", "sum_err2", "sum_gold2")


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    from oracle import oracle as orc
    _lib.load()
    orc.lib()


# ------------------------------------------------------------------------------------ helpers
def _table(E, M, zero=False):
    from fp8_quantization_amd.error_tables import get_error_table_NN
    if zero or (E, M) == (5, 2):  # (the reference ships no E5M2 table: the zero table)
        return torch.zeros((2 ** M, 2 ** M), dtype=torch.int32)
    return get_error_table_NN(E, M, withComp=False, dnsmp_factor=3)


def _qbias(mx, E, M):
    return int(np.rint(2.0 ** E - np.log2(mx) + np.log2(2.0 - 2.0 ** -M) - 1.0))


def _quantized(rng, shape, E, M, mx, zeros):
    """FP8-quantized values (the project's quantizer on the GPU): `zeros` of them zero, ~15 % below the grid's
    min_norm (subnormals).  Returns (float32 device tensor, its int bias)."""
    import fp8_quantization_amd as fa
    b = _qbias(mx, E, M)
    v = rng.standard_normal(shape).astype(np.float32)
    small = rng.random(shape) < 0.15
    v[small] = (np.sign(v[small]) * 2.0 ** (1 - b) * rng.uniform(0.1, 1.5, size=int(small.sum()))).astype(np.float32)
    v[rng.random(shape) < zeros] = 0.0
    q, bias = fa.fp8_fake_quantize(torch.from_numpy(v).to(DEV), torch.tensor([mx], dtype=torch.float32), 1 + E + M, M)
    assert int(bias.item()) == b
    return q, b


def _heads(buf, nb1):
    """[nb0, R, nb1 * c] -> the head view [nb0, nb1, R, c] (no copy)."""
    return buf.view(buf.shape[0], buf.shape[1], nb1, -1).permute(0, 2, 1, 3)


def _operands(rng, E, M, transposed, quantize=True, shape=(NB0, NB1, MR, K, N)):
    """(A [nb0, nb1, M, K], B [nb0, nb1, K, N], bA, bB per column) as head views; transposed: B is the
    transpose of an [.., N, K] head view (k stride 1, as K^T in QK^T)."""
    nb0, nb1, Mr, Kk, Nn = shape
    sa, sb = (nb0, Mr, nb1 * Kk), ((nb0, Nn, nb1 * Kk) if transposed else (nb0, Kk, nb1 * Nn))
    if quantize:
        abuf, bA = _quantized(rng, sa, E, M, 4.0, 0.5)
        bbuf, b0 = _quantized(rng, sb, E, M, 2.0, 0.2)
    else:  # unquantized operands: off every FP8 grid
        abuf, bA = torch.from_numpy(rng.standard_normal(sa).astype(np.float32)).to(DEV), _qbias(4.0, E, M)
        bbuf, b0 = torch.from_numpy(rng.standard_normal(sb).astype(np.float32)).to(DEV), _qbias(2.0, E, M)
    A, B = _heads(abuf, nb1), _heads(bbuf, nb1)
    if transposed:
        B = B.transpose(-1, -2)
    assert A.shape == (nb0, nb1, Mr, Kk) and B.shape == (nb0, nb1, Kk, Nn) and A.stride(-1) == 1
    assert B.stride(-2 if transposed else -1) == 1 and (nb1 == 1 or not A.is_contiguous())
    bB = b0 + (np.arange(Nn) % 3) - 1 if Nn > 1 else np.array([b0])  # (every column its own bias; bB[1] = b0)
    return A, B, bA, bB.astype(np.int32)


def _items(t):
    """The batch items of a [..., r, c] tensor as contiguous numpy matrices, in (i0, i1) order."""
    a = t.detach().cpu().numpy()
    return [np.ascontiguousarray(x) for x in a.reshape((-1,) + a.shape[-2:])]


def _min_norm(b):
    return np.float32(2.0 ** (1 - b))


def _reference(A, B, E, M, bA, bB, bR, table, flags):
    """One item: oracle C / S, host golden G and its scale, and the exact counts (int biases)."""
    from fp8_quantization_amd import _lib
    from oracle import oracle as orc
    s2n, qbma, gclip = (bool(flags & f) for f in (_lib.S2N, _lib.QBMA, _lib.GCLIP))
    Nn = B.shape[1]
    bBv = np.broadcast_to(np.asarray(bB, dtype=np.int64).reshape(-1), (Nn,))
    C, S = orc.matmul(A, B, E, M, bA, bBv, bR, table.numpy(), flags, with_abs=True)
    g = (A[:, :, None] * B[None]).astype(np.float32)
    if qbma:
        g = orc.quant(g, E, M, bR, tb=False, clip=gclip)
    ref = dict(C=C, S=S, G=g.astype(np.float64).sum(axis=1), Gabs=np.abs(g).astype(np.float64).sum(axis=1))
    ref["a_norm"] = int((np.abs(A) >= _min_norm(bA)).sum())
    mnB = np.array([_min_norm(int(b)) for b in bBv], dtype=np.float32)
    ref["b_norm"] = int((np.abs(B) >= mnB[None, :]).sum())
    ref["r_norm"] = 0
    if not s2n:  # v9:87
        eA, _ = orc.decompose(A, E, M, bA)
        eB = np.empty(B.shape, np.int32)
        for b in np.unique(bBv):
            cols = bBv == b
            eB[:, cols] = orc.decompose(np.ascontiguousarray(B[:, cols]), E, M, int(b))[0]
        ref["r_norm"] = int(((eA[:, :, None] > 0) & (eB[None] > 0) & (np.abs(g) >= _min_norm(bR))).sum())
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


def _run_case(tag, A, B, E, M, bA, bB, bR, table, flags):
    """approx_bmm_check on the views against the per-item references; returns its CheckStats."""
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    C, G, st = fa.approx_bmm_check(A, B, E, M, bA, torch.from_numpy(bB), bR, table, flags=flags)
    assert C.shape == A.shape[:-1] + B.shape[-1:] == G.shape == st.S.shape and C.is_contiguous()
    nb, (Mr, Kk), Nn = int(np.prod(A.shape[:-2])), A.shape[-2:], B.shape[-1]
    tot = dict(a_norm=0, b_norm=0, r_norm=0)
    worst = [0.0, 0.0, 0.0]
    for z, (a, b, c, g, s) in enumerate(zip(_items(A), _items(B), _items(C), _items(G), _items(st.S))):
        ref = _reference(a, b, E, M, bA, bB, bR, table, flags)
        dC, dS, dG = np.abs(c - ref["C"]), np.abs(s - ref["S"]), np.abs(g - ref["G"])
        for i, (d, scale) in enumerate(((dC, ref["S"]), (dS, ref["S"]), (dG, ref["Gabs"]))):
            worst[i] = max(worst[i], float((d / np.maximum(scale, TINY)).max()))
        assert np.all(dC <= 1e-5 * ref["S"] + TINY), (tag, z)
        assert np.all(dS <= 1e-5 * ref["S"] + TINY), (tag, z)
        assert np.all(dG <= 1e-5 * ref["Gabs"] + TINY), (tag, z)
        for k in tot:
            tot[k] += ref[k]
    print(tag, "max |C-oracle|/S", worst[0], "max |S-oracle|/S", worst[1], "max |G-golden|/sum|g|", worst[2],
          "max_err", st.max_err)
    _check_stats_against_tensors(st, C.cpu().numpy(), G.cpu().numpy())
    assert (st.a_norm, st.a_total) == (tot["a_norm"], nb * Mr * Kk), tag
    assert (st.b_norm, st.b_total) == (tot["b_norm"], nb * Kk * Nn), tag
    if flags & _lib.S2N:
        assert (st.r_norm, st.r_total) == (0, 0) and st.r_norm_pct is None
    else:
        assert (st.r_norm, st.r_total) == (tot["r_norm"], nb * Mr * Kk * Nn), tag
    assert st.has_prod == 0 and st.prod_max_abs == 0.0 and st.prod_max_rel == 0.0
    return st


# ------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("s2n,qbma,gclip", list(itertools.product((False, True), repeat=3)),
                         ids=lambda v: str(int(v)))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_bmm_check_matrix(fmt, s2n, qbma, gclip):
    import fp8_quantization_amd as fa
    E, M = FORMATS[fmt]
    rng = np.random.default_rng(2000 * sorted(FORMATS).index(fmt) + 4 * s2n + 2 * qbma + gclip)
    transposed = bool(s2n) != bool(gclip)  # (half of the cases read a transposed B: sbk = 1)
    A, B, bA, bB = _operands(rng, E, M, transposed)
    flags = fa.make_flags(True, s2n, qbma, gclip)
    _run_case((fmt, s2n, qbma, gclip, transposed), A, B, E, M, bA, bB, bA, _table(E, M), flags)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_bmm_check_without_approx_and_small_shapes(fmt):
    import fp8_quantization_amd as fa
    E, M = FORMATS[fmt]
    rng = np.random.default_rng(77 + sorted(FORMATS).index(fmt))
    A, B, bA, bB = _operands(rng, E, M, False)
    st = _run_case((fmt, "no approx"), A, B, E, M, bA, bB, bA, _table(E, M), fa.make_flags(False, True, True, False))
    assert st.n_out == NB0 * NB1 * MR * N
    # one item of 1 x 1 x 1 behind one leading batch dim; N = 1 with int biases (no tensor-bias semantics)
    for shape, s2n in (((1, 1, 1, 1, 1), True), ((1, 2, 65, 9, 1), False), ((1, 2, 65, 9, 1), True)):
        A, B, bA, bB = _operands(rng, E, M, False, shape=shape)
        st = _run_case((fmt, shape, s2n), A[0], B[0], E, M, bA, bB, bA, _table(E, M),
                       fa.make_flags(True, s2n, True, False))
        assert st.n_out == shape[1] * shape[2] * shape[4]


# ------------------------------------------------------------------------------------ 2. the single-product check
@pytest.mark.parametrize("transposed", (False, True), ids=("v", "kt"))
@pytest.mark.parametrize("s2n", (False, True), ids=("nos2n", "s2n"))
def test_equals_per_item_matmul_check(s2n, transposed):
    """Same k order and per-output arithmetic: C, G, S bit for bit per item; the counts are the sums of the
    per-item counts (A or B counted per tile instead of per item, or a wrong batch stride, fails here)."""
    import fp8_quantization_amd as fa
    E, M = 4, 3
    rng = np.random.default_rng(21 + s2n)
    A, B, bA, bB = _operands(rng, E, M, transposed)
    bBt, tab, fl = torch.from_numpy(bB), _table(E, M), fa.make_flags(True, s2n, True, False)
    C, G, st = fa.approx_bmm_check(A, B, E, M, bA, bBt, bA, tab, flags=fl)
    tot = dict.fromkeys(COUNTS + SUMS, 0)
    mx = np.float32(0.0)
    for i0 in range(NB0):
        for i1 in range(NB1):
            Ci, Gi, si = fa.approx_matmul_check(A[i0, i1], B[i0, i1], E, M, bA, bBt, bA, tab, flags=fl)
            assert torch.equal(C[i0, i1].view(torch.int32), Ci.view(torch.int32)), (i0, i1)
            assert torch.equal(G[i0, i1].view(torch.int32), Gi.view(torch.int32)), (i0, i1)
            assert torch.equal(st.S[i0, i1].view(torch.int32), si.S.view(torch.int32)), (i0, i1)
            for k in tot:
                tot[k] += getattr(si, k)
            mx = max(mx, np.float32(si.max_err))
    for k in COUNTS:
        assert getattr(st, k) == tot[k], k
    assert np.float32(st.max_err).tobytes() == np.float32(mx).tobytes()
    for k in SUMS:
        assert _close(getattr(st, k), tot[k]), (k, getattr(st, k), tot[k])
    assert st.n_out == NB0 * NB1 * MR * N and st.a_total == NB0 * NB1 * MR * K and st.b_total == NB0 * NB1 * K * N
    assert st.r_total == (0 if s2n else NB0 * NB1 * MR * K * N)
    # 3. the statistics from the returned tensors
    _check_stats_against_tensors(st, C.cpu().numpy(), G.cpu().numpy())


# ------------------------------------------------------------------------------------ 4. off-grid operands
@pytest.mark.parametrize("s2n,qbma", list(itertools.product((False, True), repeat=2)), ids=lambda v: str(int(v)))
def test_offgrid_operands(s2n, qbma):
    """Unquantized randn operands: G is the definition, not a zero-table approx launch."""
    import fp8_quantization_amd as fa
    rng = np.random.default_rng(9)
    A, B, bA, bB = _operands(rng, 4, 3, bool(qbma), quantize=False)
    fl = fa.make_flags(True, s2n, qbma, False)
    st = _run_case(("offgrid", s2n, qbma), A, B, 4, 3, bA, bB, bA, _table(4, 3), fl)
    # off the grid even a zero table leaves golden != approx (F9 needs on-grid operands)
    z = _run_case(("offgrid zero table", s2n, qbma), A, B, 4, 3, bA, bB, bA, _table(4, 3, zero=True), fl)
    assert st.max_err > 0 and z.max_err > 0


# ------------------------------------------------------------------------------------ 5. known answer
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_known_answer_zero_table(fmt):
    """F9: on-grid operands and a zero table give G == C bit for bit."""
    import fp8_quantization_amd as fa
    E, M = FORMATS[fmt]
    A, B, bA, bB = _operands(np.random.default_rng(7), E, M, True)
    bB = bB[1:2]  # (B's own bias for every column: on its grid)
    fl = fa.make_flags(True, True, True, False)
    C, G, st = fa.approx_bmm_check(A, B, E, M, bA, torch.from_numpy(bB), bA, _table(E, M, zero=True), flags=fl)
    assert C.abs().max().item() > 0
    assert torch.equal(C.view(torch.int32), G.view(torch.int32))
    assert st.max_err == 0.0 and st.sum_err == 0.0 and st.sum_err2 == 0.0
    if fmt == "e4m3":  # the no-comp table has an error
        _, _, nc = fa.approx_bmm_check(A, B, E, M, bA, torch.from_numpy(bB), bA, _table(E, M), flags=fl)
        assert nc.max_err > 0 and nc.rmse > 0 and np.isfinite(nc.sqnr_db)


# ------------------------------------------------------------------------------------ 6. determinism
def test_determinism():
    import fp8_quantization_amd as fa
    A, B, bA, bB = _operands(np.random.default_rng(10), 4, 3, False)
    fl, bBt = fa.make_flags(True, False, True, False), torch.from_numpy(bB)
    r1 = fa.approx_bmm_check(A, B, 4, 3, bA, bBt, bA, _table(4, 3), flags=fl)
    r2 = fa.approx_bmm_check(A, B, 4, 3, bA, bBt, bA, _table(4, 3), flags=fl)
    assert len(r1[2].raw) == 96 and r1[2].raw == r2[2].raw
    for x, y in ((r1[0], r2[0]), (r1[1], r2[1]), (r1[2].S, r2[2].S)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------ 7. production cross-check
@pytest.mark.parametrize("fmt,transposed", [("e4m3", True), ("e5m2", False), ("e3m4", True)],
                         ids=("e4m3-f8", "e5m2-bf8", "e3m4"))
def test_production_cross_check(fmt, transposed):
    import fp8_quantization_amd as fa
    from fp8_quantization_amd import _lib
    E, M = FORMATS[fmt]
    A, B, bA, bB = _operands(np.random.default_rng(11), E, M, transposed)
    # B's own bias for every column and a result grid that holds every product (bR = bA + bB - 2^E - 3, the
    # rule of tests/test_gpu_bmm.py): nothing leaves fp8a_bmm's fast forms, so their tiles are what is compared
    bBt, tab, fl = torch.from_numpy(bB[1:2]), _table(E, M), fa.make_flags(True, True, True, False)
    bR = bA + int(bB[1]) - 2 ** E - 3
    _lib.bmm_stats(reset=True)
    prod = fa.approx_bmm(A, B, E, M, bA, bBt, bR, tab, flags=fl)
    bs = _lib.bmm_stats(reset=True)
    assert bs["launches"] == 1 and bs["tiles"] == NB0 * NB1 * 4 and bs["recomputed"] == 0, bs  # the clean path ran
    C, _, st = fa.approx_bmm_check(A, B, E, M, bA, bBt, bR, tab, flags=fl, prod=prod)
    print(fmt, "prod_max_rel", st.prod_max_rel, "prod_max_abs", st.prod_max_abs)
    assert st.has_prod == 1 and st.prod_max_rel <= 1e-5
    Cn, S, P = C.cpu().numpy(), st.S.cpu().numpy(), prod.cpu().numpy()
    assert np.float32(st.prod_max_abs).tobytes() == np.abs(P - Cn).max().tobytes()
    assert _lib.bmm_stats(reset=True)["launches"] == 0  # (the check is no fp8a_bmm launch)
    if fmt != "e4m3":
        return
    # one element moved by a known delta (a quarter of its scale: far above the bar everywhere else)
    idx = np.unravel_index(np.argmax(S), S.shape)
    P2 = P.copy()
    P2[idx] = np.float32(P2[idx] + np.float32(0.25) * S[idx])
    _, _, st2 = fa.approx_bmm_check(A, B, E, M, bA, bBt, bR, tab, flags=fl, prod=torch.from_numpy(P2).to(DEV))
    d = np.abs(P2 - Cn)
    assert idx == np.unravel_index(np.argmax(d), d.shape)
    assert np.float32(st2.prod_max_abs).tobytes() == d.max().tobytes()
    want = np.float32(d[idx]) / np.maximum(S[idx], FLT_MIN)
    assert abs(np.float32(st2.prod_max_rel) - want) <= np.spacing(want)
    # one off-grid value in one item: that item's tiles are recomputed exactly inside fp8a_bmm, and still agree
    A2 = A.clone(memory_format=torch.preserve_format)
    assert A2.stride() == A.stride()
    A2[1, 2, 3, 5] = 0.3  # (1.2 * 2^-2: between two E4M3 codes)
    prod2 = fa.approx_bmm(A2, B, E, M, bA, bBt, bR, tab, flags=fl)
    bs = _lib.bmm_stats(reset=True)
    assert bs["launches"] == 1 and bs["recomputed"] == 2, bs  # row tile 0 of item (1, 2): its column tiles
    _, _, st3 = fa.approx_bmm_check(A2, B, E, M, bA, bBt, bR, tab, flags=fl, prod=prod2)
    print("planted off-grid value: prod_max_rel", st3.prod_max_rel)
    assert st3.has_prod == 1 and st3.prod_max_rel <= 1e-5


# ------------------------------------------------------------------------------------ 8. capturing stream
def test_capturing_stream_is_rejected():
    """A diagnostic, not for graphs: nothing is launched on a capturing stream."""
    import fp8_quantization_amd as fa
    a = torch.ones((2, 4, 4), device=DEV)
    tab = _table(4, 3)
    fa.approx_bmm_check(a, a, 4, 3, 7, 7, 7, tab, flags=fa.make_flags())  # (warm: biases cached, library loaded)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a + 1.0  # (a node of its own: the graph is not empty)
        with pytest.raises(AssertionError, match="the self-check does not run on a capturing stream"):
            fa.approx_bmm_check(a, a, 4, 3, 7, 7, 7, tab, flags=fa.make_flags())


# ------------------------------------------------------------------------------------ 9. the operator
LABELS = ["====== Self-Checking Mode ======", "With Approximation    =", "With S2N & N2S Opt    =",
          "Quant btw Mult & Accu =", "Normal Values in A_2d :", "Normal Values in B_2d :", "Normal Values in R_3d :",
          "MatMul Max  Error     :", "MatMul Mean Error     :", "MatMul RMSE           :"]


def _pv_operands(seed):
    """probs [2, 2, 17, 17] (softmax rows) and v [2, 2, 17, 16] as a head view of a [2, 17, 32] buffer."""
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(torch.randn((2, 2, 17, 17), generator=g) * 2.0, dim=-1).to(DEV)
    v = _heads(torch.randn((2, 17, 32), generator=g).to(DEV), 2)
    return probs, v


def _calibrated_matmul(run_method=None, **cfg):
    from fp8_quantization_amd.approx_calculation import QCustomMatMul
    from fp8_quantization_amd.resnet_workload import approx_qparams
    mod = QCustomMatMul(**approx_qparams(withComp=False, run_method=run_method, **cfg)).to(DEV).eval()
    mod.quantized()
    mod.estimate_ranges()
    with torch.no_grad():
        mod(*_pv_operands(4))
    mod.fix_ranges()
    return mod


@pytest.mark.parametrize("s2n", (False, True), ids=("nos2n", "s2n"))
def test_matmul_operator_self_check(s2n, capsys):
    from fp8_quantization_amd import _lib
    mod = _calibrated_matmul(with_s2nn2s_opt=s2n)
    probs, v = _pv_operands(5)

    def forward():
        ctx = torch.full((2, 17, 2, 16), float("nan"), device=DEV)
        _lib.bmm_stats(reset=True)
        with torch.no_grad():
            out = mod(probs, v, out=ctx.permute(0, 2, 1, 3))
        assert out.data_ptr() == ctx.data_ptr() and out.shape == (2, 2, 17, 16)
        assert _lib.bmm_stats(reset=True)["launches"] == 1  # exactly one fp8a_bmm launch per forward
        return ctx
    y_off = forward()
    assert mod.last_self_check is None
    capsys.readouterr()
    mod.custom_approx_params["self_check_mode"] = True
    y_on = forward()
    lines = [ln for ln in capsys.readouterr().out.split("\n") if ln]
    mod.custom_approx_params["self_check_mode"] = False
    assert torch.isfinite(y_on).all() and torch.equal(y_off.view(torch.int32), y_on.view(torch.int32))
    want = [lab for lab in LABELS if not (s2n and "R_3d" in lab)]
    assert [ln[:len(lab)] for ln, lab in zip(lines, want)] == want and len(lines) == len(want)  # printed once
    st = mod.last_self_check
    assert st.has_prod == 1 and st.prod_max_rel <= 1e-5
    assert st.n_out == 4 * 17 * 16 and st.a_total == 4 * 17 * 17 and st.b_total == 4 * 17 * 16
    assert st.r_total == (0 if s2n else 4 * 17 * 17 * 16) and st.S.shape == (2, 2, 17, 16)


def test_matmul_operator_without_approx_has_no_self_check(capsys):
    mod = _calibrated_matmul(run_method=dict(approx_flag=False, quantize_after_mult_and_add=False,
                                             res_quantizer_flag=True, original_quantize_res=True))
    mod.custom_approx_params["self_check_mode"] = True
    capsys.readouterr()
    with torch.no_grad():
        out = mod(*_pv_operands(5))
    assert out.shape == (2, 2, 17, 16) and capsys.readouterr().out == "" and mod.last_self_check is None


# ------------------------------------------------------------------------------------ 10. the report
TINY_VIT = dict(image_size=32, patch_size=8, hidden=32, layers=2, heads=2, mlp=64, num_labels=10)


def _tiny_vit(**kw):
    from fp8_quantization_amd.vit_workload import vit_b16_approx
    m = vit_b16_approx(seed=43, expo_width=4, mant_width=3, withComp=False, **kw, **TINY_VIT).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    m.quantized()
    m.estimate_ranges()
    with torch.no_grad():
        m(torch.randn((4, 3, 32, 32), generator=g).to(DEV))
    m.fix_ranges()
    return m, torch.randn((2, 3, 32, 32), generator=g).to(DEV)


def test_layer_error_report_with_attention_rows():
    from fp8_quantization_amd.error_report import approx_layers, format_report, layer_error_report
    base, x = _tiny_vit()
    base_rows = layer_error_report(base, x)
    assert len(base_rows) == len(approx_layers(base)) and all(r["kind"] == "linear" for r in base_rows)
    assert all("batch" not in r for r in base_rows)
    on, _ = _tiny_vit(approx_attention=True)
    rows = layer_error_report(on, x)
    print(format_report(rows))
    mm = [r for r in rows if r["kind"] == "matmul"]
    rest = [r for r in rows if r["kind"] != "matmul"]
    assert [(r["name"], r["kind"], r["shape"], r["groups"], r["macs"]) for r in rest] == \
        [(r["name"], r["kind"], r["shape"], r["groups"], r["macs"]) for r in base_rows]
    assert [r["name"] for r in rows] == [n for n, _ in approx_layers(on)]  # module order
    assert len(mm) == 2 * TINY_VIT["layers"]
    for i, r in enumerate(mm):
        qk = i % 2 == 0
        assert r["name"].endswith("qk_matmul" if qk else "pv_matmul") and f"layer.{i // 2}." in r["name"], r["name"]
        assert r["shape"] == ((17, 17, 16) if qk else (17, 16, 17)) and r["batch"] == 4 and r["groups"] == 1
        assert r["macs"] == 4 * 17 * 17 * 16
        assert r["r_norm_pct"] is None and 0.0 <= r["a_norm_pct"] <= 100.0 and 0.0 <= r["b_norm_pct"] <= 100.0
    for r in rows:
        assert r["prod_max_rel"] <= 1.0, r  # (units of the 1e-5 bar)
    assert any(r["max"] > 0 for r in mm)  # the no-comp table
    assert all(not m.custom_approx_params.get("self_check_mode") for _, m in approx_layers(on))
    # E4M3 withComp=True: the all-zero table of F3 -- golden == approx in every row (F9)
    for _, m in approx_layers(on):
        m.custom_approx_params["withComp"] = True
    zero = layer_error_report(on, x)
    assert len(zero) == len(rows) and all(r["max"] == 0.0 for r in zero), [(r["name"], r["max"]) for r in zero]
    assert all(r["prod_max_rel"] <= 1.0 for r in zero)
    assert all(not m.custom_approx_params.get("self_check_mode") for _, m in approx_layers(on))
    assert len(layer_error_report(base, x)) == len(base_rows)
