"""fp8a_bmm (gemm_bmm_kernel, DESIGN.md §3z'): the batched approx product against the CPU oracle.

  * terms: K = 1 makes every output one term.  A = the 256 magnitudes of the format as [256, 1], B = the
    same as [1, 256], batch (2, 2) = the four sign pairings; bit-exact against oracle.terms (zeros by value)
    for E4M3 (built-in nocomp, zero table), E5M2 (zero table, a non-negative custom table), E3M4 and E2M5
    (built-in comp and nocomp) at three bias triples of tests/pairs_cases.py each, and E4M3 / E3M4 under all
    16 flag combinations at one triple;
  * sums and indexing: operands on the FP8 grid cut as head views from [B, S, H*d] buffers (B = 2, H = 3),
    written into a sentinel-filled [B, S, H*slot] output: QK^T (M = N = 37, K = 16, sbk = 1), PV (M = 37,
    N = 16, K = 37: ragged K, sbn = 1) and a tile-crossing shape (M = 70, N = 130, K = 64); every (b, h)
    within 1e-5 * sum|term| of oracle.matmul, two calls bit-identical, 0 recomputed tiles;
  * off-grid: one off-grid value in one item's A -- that item still meets the oracle, the others' bytes
    equal the clean run, exactly the tiles that staged it are counted;
  * F9: zero table, qbma off, s2n on equals torch.matmul within the bar;
  * empty extents and graph capture.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import pairs_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77.25


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(DEV)


def _bmm(*args, **kw):
    from fp8_quantization_amd.approx_ops import approx_bmm
    return approx_bmm(*args, **kw)


def _stats(reset=False):
    from fp8_quantization_amd import _lib
    return _lib.bmm_stats(reset)


def _bar(S):
    return 1e-5 * S.astype(np.float64) + 1e-30


# ------------------------------------------------------------------------------------------ terms
TERM_CASES = [((4, 3), "nocomp"), ((4, 3), "zero"), ((5, 2), "zero"), ((5, 2), "s_w2u"),
              ((3, 4), "comp3"), ((3, 4), "nocomp"), ((2, 5), "comp3"), ((2, 5), "nocomp")]
SIGNS = [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)]


def _terms_check(E, M, table, triple, flags):
    bA, bB, bR = triple
    a = pc.all_codes(E, M, bA)[:256]
    b = pc.all_codes(E, M, bB)[:256]
    A = np.stack([s[0] * a for s in SIGNS]).reshape(2, 2, 256, 1)
    B = np.stack([s[1] * b for s in SIGNS]).reshape(2, 2, 1, 256)
    C = _bmm(_dev(A), _dev(B), E, M, bA, bB, bR, torch.from_numpy(table), flags=flags).cpu().numpy()
    for z, (sa, sb) in enumerate(SIGNS):
        ref = orc.terms(A[z // 2, z % 2], B[z // 2, z % 2], E, M, bA, bB, bR, table, flags)[:, 0, :]
        ok = pc.same_bits(C[z // 2, z % 2], ref)
        assert ok.all(), (f"E{E}M{M} {triple} flags {flags} signs {sa, sb}: {np.count_nonzero(~ok)} terms differ, "
                          f"first at {np.argwhere(~ok)[0]}")


@pytest.mark.parametrize("fmt,name", TERM_CASES, ids=[f"E{f[0]}M{f[1]}-{n}" for f, n in TERM_CASES])
def test_terms_bit_exact(fmt, name):
    E, M = fmt
    table = pc.tables(E, M)[name]
    for triple in pc.V9_TRIPLES[fmt][:3]:
        _terms_check(E, M, table, triple, pc.flag_word(True, True, True, False))


@pytest.mark.parametrize("fmt,name", [((4, 3), "nocomp"), ((3, 4), "nocomp")], ids=["E4M3", "E3M4"])
def test_terms_all_16_flag_combinations(fmt, name):
    E, M = fmt
    table = pc.tables(E, M)[name]
    for ap, s2n, qbma, gc in itertools.product((True, False), repeat=4):
        _terms_check(E, M, table, pc.V9_TRIPLES[fmt][0], pc.flag_word(ap, s2n, qbma, gc))


# ------------------------------------------------------------------------------------------ sums
def _grid(rng, shape, E, M, zeros=0.05):
    """Random values on the (E, M) FP8 grid of their own maxval (some exact zeros), and the int bias."""
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < zeros] = 0.0
    q, bias = orc.fp8_fake_quant(x, np.abs(x).max(), E, M)
    return q, int(bias[0])


# (name, M, N, K, "kt": B is K^T cut from a [B, N, H*K] buffer (sbk = 1); "v": B cut from [B, K, H*N] (sbn = 1))
SHAPES = [("qk", 37, 37, 16, "kt"), ("pv", 37, 16, 37, "v"), ("cross", 70, 130, 64, "v")]
SUM_FORMATS = [((4, 3), "nocomp"), ((5, 2), "zero"), ((3, 4), "nocomp")]
NB, NH = 2, 3


def _head_views(shape, E, M, seed):
    """Device head views A [2, 3, M, K], B [2, 3, K, N], the sentinel-filled output buffer with its view, and the
    host operands per (b, h) with the biases."""
    _, Mr, N, K, kind = shape
    rng = np.random.default_rng(seed)
    qa, bA = _grid(rng, (NB, Mr, NH * K), E, M)
    A = _dev(qa).view(NB, Mr, NH, K).permute(0, 2, 1, 3)
    if kind == "kt":
        qb, bB = _grid(rng, (NB, N, NH * K), E, M)
        B = _dev(qb).view(NB, N, NH, K).permute(0, 2, 3, 1)
    else:
        qb, bB = _grid(rng, (NB, K, NH * N), E, M)
        B = _dev(qb).view(NB, K, NH, N).permute(0, 2, 1, 3)
    slot = N + 3  # the output's per-head slot is wider than N: the pad columns must keep the sentinel
    buf = torch.full((NB, Mr, NH * slot), SENT, device=DEV)
    out = buf.view(NB, Mr, NH, slot)[..., :N].permute(0, 2, 1, 3)
    return A, B, buf, out, bA, bB


def _check_items(A, B, C, E, M, bA, bB, bR, table, flags, items=None):
    Ah, Bh, Ch = A.cpu().numpy(), B.cpu().numpy(), C.cpu().numpy()
    for b, h in (items or itertools.product(range(NB), range(NH))):
        ref, S = orc.matmul(Ah[b, h], Bh[b, h], E, M, bA, bB, bR, table, flags, with_abs=True)
        err = np.abs(Ch[b, h].astype(np.float64) - ref)
        assert (err <= _bar(S)).all(), f"item {b, h}: max excess {(err - _bar(S)).max():.3e}"


def _pad_untouched(buf, N):
    slot = buf.shape[-1] // NH
    pad = buf.view(NB, -1, NH, slot)[..., N:]
    return bool((pad == SENT).all())


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("fmt,name", SUM_FORMATS, ids=[f"E{f[0]}M{f[1]}" for f, _ in SUM_FORMATS])
def test_sums_and_indexing(shape, fmt, name):
    E, M = fmt
    table = pc.tables(E, M)[name]
    flags = pc.flag_word(True, True, True, False)
    A, B, buf, out, bA, bB = _head_views(shape, E, M, seed=11)
    bR = bA + bB - 2 ** E - 3  # (pairs_cases' rule: the products stay inside the result grid)
    _stats(reset=True)
    _bmm(A, B, E, M, bA, bB, bR, torch.from_numpy(table), flags=flags, out=out)
    first = buf.clone()
    _check_items(A, B, out, E, M, bA, bB, bR, table, flags)
    assert _pad_untouched(buf, shape[2])
    buf2 = torch.full_like(buf, SENT)
    _bmm(A, B, E, M, bA, bB, bR, torch.from_numpy(table), flags=flags,
         out=buf2.view(NB, shape[1], NH, -1)[..., :shape[2]].permute(0, 2, 1, 3))
    assert torch.equal(first.view(torch.int32), buf2.view(torch.int32))
    st = _stats()
    tiles = NB * NH * ((shape[1] + 63) // 64) * ((shape[2] + 63) // 64)
    assert st["launches"] == 2 and st["tiles"] == 2 * tiles and st["recomputed"] == 0, st


def test_per_column_bias_and_single_batch_dim():
    """bB per column n (stride 1) and 3-D operands ([b, M, K] @ [b, K, N])."""
    E, M = 4, 3
    table = pc.tables(E, M)["nocomp"]
    flags = pc.flag_word(True, True, True, False)
    rng = np.random.default_rng(5)
    qa, bA = _grid(rng, (3, 33, 21), E, M)
    qb, bB0 = _grid(rng, (3, 21, 70), E, M)
    bB = (bB0 + np.arange(70) % 3).astype(np.int32)
    qb = (qb * np.exp2(-(np.arange(70) % 3))).astype(np.float32)  # column n on the grid of its own bias
    bR = bA + bB0 - 2 ** E - 3
    C = _bmm(_dev(qa), _dev(qb), E, M, bA, torch.from_numpy(bB).to(DEV), bR, torch.from_numpy(table), flags=flags)
    assert C.shape == (3, 33, 70)
    assert _stats(reset=True)["recomputed"] == 0
    for b in range(3):
        ref, S = orc.matmul(qa[b], qb[b], E, M, bA, bB, bR, table, flags, with_abs=True)
        assert (np.abs(C[b].cpu().numpy().astype(np.float64) - ref) <= _bar(S)).all()


@pytest.mark.parametrize("fmt,name", SUM_FORMATS, ids=[f"E{f[0]}M{f[1]}" for f, _ in SUM_FORMATS])
def test_off_grid_value_recomputes_only_its_tiles(fmt, name):
    E, M = fmt
    table = pc.tables(E, M)[name]
    flags = pc.flag_word(True, True, True, False)
    shape = SHAPES[2]
    A, B, buf, out, bA, bB = _head_views(shape, E, M, seed=23)
    bR = bA + bB - 2 ** E - 3  # (pairs_cases' rule: the products stay inside the result grid)
    _bmm(A, B, E, M, bA, bB, bR, torch.from_numpy(table), flags=flags, out=out)
    clean = out.clone()
    A[1, 2, 5, 3] = 0.1234567  # not on any (E, M) grid: 24 significant bits
    _stats(reset=True)
    _bmm(A, B, E, M, bA, bB, bR, torch.from_numpy(table), flags=flags, out=out)
    st = _stats()
    assert st["recomputed"] == (shape[2] + 63) // 64, st  # row tile 0 of item (1, 2): one tile per column tile
    _check_items(A, B, out, E, M, bA, bB, bR, table, flags, items=[(1, 2)])
    others = [(b, h) for b in range(NB) for h in range(NH) if (b, h) != (1, 2)]
    for b, h in others:
        assert torch.equal(out[b, h].contiguous().view(torch.int32), clean[b, h].contiguous().view(torch.int32))
    assert torch.equal(out[1, 2, 64:].contiguous().view(torch.int32), clean[1, 2, 64:].contiguous().view(torch.int32))
    assert _pad_untouched(buf, shape[2])


def test_known_answer_without_the_oracle_f9():
    """Zero table, qbma off, s2n on: every term is the exact product a * b, so the result is
    torch.matmul of the same operands within the bar (S = |A| @ |B|)."""
    E, M = 4, 3
    A, B, buf, out, bA, bB = _head_views(SHAPES[2], E, M, seed=31)
    table = np.zeros((8, 8), np.int32)
    C = _bmm(A, B, E, M, bA, bB, bA + bB - 2 ** E, torch.from_numpy(table), flags=pc.flag_word(True, True, False, False))
    ref = torch.matmul(A.double(), B.double())
    S = torch.matmul(A.double().abs(), B.double().abs())
    assert torch.all((C.double() - ref).abs() <= 1e-5 * S + 1e-30)


def test_empty_extents():
    E, M = 4, 3
    A = torch.zeros((2, 3, 5, 0), device=DEV)
    B = torch.zeros((2, 3, 0, 7), device=DEV)
    C = torch.full((2, 3, 5, 7), SENT, device=DEV)
    _bmm(A, B, E, M, 8, 8, 8, None, out=C)
    assert bool((C == 0).all())  # K = 0: the empty sum
    C0 = _bmm(torch.zeros((0, 3, 5, 4), device=DEV), torch.zeros((0, 3, 4, 7), device=DEV), E, M, 8, 8, 8, None)
    assert C0.shape == (0, 3, 5, 7)
    keep = torch.full((2, 5, 0), SENT, device=DEV)
    _bmm(torch.zeros((2, 5, 4), device=DEV), torch.zeros((2, 4, 0), device=DEV), E, M, 8, 8, 8, None, out=keep)
    torch.cuda.synchronize()


def test_rejects_overlap_and_bad_flags():
    from fp8_quantization_amd import _lib
    E, M = 4, 3
    A = torch.zeros((2, 8, 8), device=DEV)
    B = torch.zeros((2, 8, 8), device=DEV)
    with pytest.raises(AssertionError):
        _bmm(A, B, E, M, 8, 8, 8, None, out=A)
    with pytest.raises(AssertionError):
        _bmm(A, B, E, M, 8, 8, 8, None, flags=_lib.APPROX | _lib.TB)
    with pytest.raises(AssertionError):
        _bmm(A, B, E, M, 8, 8, 8, None, flags=_lib.V5)
    with pytest.raises(RuntimeError):
        _bmm(A.cpu(), B.cpu(), E, M, 8, 8, 8, None)


def test_graph_capture_replays_bit_identical():
    E, M = 4, 3
    table = torch.from_numpy(pc.tables(E, M)["nocomp"])
    flags = pc.flag_word(True, True, True, False)
    A, B, buf, out, bA, bB = _head_views(SHAPES[0], E, M, seed=41)
    bR = bA + bB - 2 ** E - 3  # (pairs_cases' rule: the products stay inside the result grid)
    eager = _bmm(A, B, E, M, bA, bB, bR, table, flags=flags).clone()
    got = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _bmm(A, B, E, M, bA, bB, bR, table, flags=flags, out=got)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _bmm(A, B, E, M, bA, bB, bR, table, flags=flags, out=got)
    for _ in range(3):
        got.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), eager.view(torch.int32))
