"""gemm_f8mx_kernel's tile-table build by the sign of A (option "xm_sign_rows", fp8a_xm_sign_stats).

The kernel's per-tile table holds the c_b-applied pairs for both signs of A; the rows of s_a = 1
are built only for launches one of whose A words is negative.  That is known on the device alone:
the A pre-pass records it in the launch's flag words, an emitting producer in header word [6] of
the word image, which the consumer's gated pre-pass copies.  Checked here, all bit for bit (int32
views) between "xm_sign_rows" = 1 and = 0 (always both halves: the previous behaviour), with the
device counter telling which build each launch ran:
  * matmul M = 130, K = 19, N = 70 (a ragged last row tile, a K tail inside a staged tile, a second
    ragged column tile), E4M3 and E5M2, on the 128 x 64 and the 256 x 16 tile: A non-negative,
    mixed, non-negative but for one element (last row and K-step / first), all zero, with -0.0;
  * a 3x3 convolution chained to a second one through the word image: a ReLU producer (half), a
    signed producer (full), the image flagged invalid with negative values present (full), and the
    same through a split-K producer (the reduction emits: fp8a_splitk_stats says it ran split);
  * a depthwise producer (the staged table-form kernel) emitting a 1x1 convolution's words, signed
    and non-negative;
  * one captured convolution replayed over non-negative, mixed, mixed again (a word raised twice in a
    row through the same captured flag words), non-negative and mixed input.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF, FULL = dict(half=1, full=0), dict(half=0, full=1)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


@pytest.fixture
def opts():
    """set(name, value) for library options, restored afterwards."""
    from fp8_quantization_amd import _lib
    old = []

    def set_(name, value):
        old.append((name, _lib.set_option(name, value)))

    yield set_
    for name, value in reversed(old):
        _lib.set_option(name, value)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _table(E, M):
    from fp8_quantization_amd.error_tables import get_error_table_NN
    return get_error_table_NN(E, M, False, 3, zero_table_ext=(E, M) == (5, 2))


def _counted(fn):
    """(fn(), the sign-build counters of its launches)"""
    from fp8_quantization_amd import _lib
    _lib.xm_sign_stats(reset=True)
    out = fn()
    return out, _lib.xm_sign_stats(reset=True)


def _both_ways(fn, expect):
    """fn() with the option on (its launches' counters == expect) and off (all full): equal bits."""
    from fp8_quantization_amd import _lib
    on, st = _counted(fn)
    assert st == expect, st
    old = _lib.set_option("xm_sign_rows", 0)
    try:
        off, st0 = _counted(fn)
    finally:
        _lib.set_option("xm_sign_rows", old)
    assert st0 == dict(half=0, full=expect["half"] + expect["full"]), st0
    assert torch.equal(_bits(on), _bits(off)), "output differs between the half and the full table build"
    return on


# --------------------------------------------------------------------------------------- matmul
MM, MK, MN = 130, 19, 70
VARIANTS = {"nonneg": HALF, "mixed": FULL, "neg_last": FULL, "neg_first": FULL, "zero": HALF, "negzero": HALF}


def _operands(E, M, variant):
    """A [130, 19], B [19, 70] on the (M, bias) grids, every term inside the result format's range
    (as the helpers of test_gpu_f8.py / test_gpu_f8_e5m2.py build them)."""
    rng = np.random.default_rng(5)
    if M == 3:
        bA, bB, bR, ea, eb = 9, 12, 3, (3, 12), (5, 12)
    else:
        bA, bB, bR, ea, eb = 20, 20, 7, (21, 28), (21, 28)
    A = np.ldexp(1.0 + rng.integers(0, 2 ** M, (MM, MK)) / 2.0 ** M, rng.integers(*ea, (MM, MK)) - bA)
    B = np.ldexp(1.0 + rng.integers(0, 2 ** M, (MK, MN)) / 2.0 ** M, rng.integers(*eb, (MK, MN)) - bB)
    B *= rng.choice([-1.0, 1.0], B.shape)
    A[rng.random(A.shape) < 0.3] = 0.0
    A = A.astype(np.float32)
    if variant == "mixed":
        A *= rng.choice([-1.0, 1.0], A.shape).astype(np.float32)
    elif variant == "neg_last":
        A[129, 18] = -np.float32(np.ldexp(1.25, ea[0] - bA))
    elif variant == "neg_first":
        A[0, 0] = -np.float32(np.ldexp(1.25, ea[0] - bA))
    elif variant == "zero":
        A[:] = 0.0
    elif variant == "negzero":
        A[A == 0.0] = -0.0
        assert np.signbit(A).any() and not (A < 0).any()
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B.astype(np.float32)).to(DEV), bA, bB, bR


@pytest.mark.parametrize("ncg", [4, 1])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_matmul_sign_build(E, M, variant, ncg, opts):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    opts("xm_ncg", ncg)
    A, B, bA, bB, bR = _operands(E, M, variant)
    tab, fl = _table(E, M), make_flags(True, True, True)
    _lib.path_stats(reset=True)
    _lib.fallback_stats(reset=True)
    _both_ways(lambda: approx_matmul(A, B, E, M, bA, bB, bR, tab, flags=fl), VARIANTS[variant])
    st = _lib.path_stats(reset=True)
    assert st["f8mx"] == 2 and sum(v for k, v in st.items() if k != "f8mx") == 0, st
    assert _lib.fallback_stats(reset=True)["exact_launches"] == 0, "the operands left the matrix-core range"


# --------------------------------------------------------------------------------- chained convs
def _pair(E, M, relu, splitk=False, seed=21):
    from tests.test_gpu_chain import _run_pair
    kw = dict(cin=8, cmid=16, cout=16, hw=12, Bn=2, k1=3, k2=3, p1=1, p2=1, epilogue=relu, post=False, seed=seed)
    if splitk:  # long K, few output tiles: the reduction kernel stores y and emits the words
        kw.update(cin=512, cmid=128, cout=64, hw=7, Bn=2)
    from fp8_quantization_amd import _lib
    _lib.splitk_stats(reset=True)
    z, z2, _, header, ctx = _run_pair(E, M, **kw)
    # _run_pair: the producer twice (plain, emitting) and the consumer twice -- more than two split
    # launches means the producer's were split (its reduction kernel is the emitter); none otherwise
    nsplit = _lib.splitk_stats(reset=True)
    assert (nsplit >= 3) if splitk else (nsplit == 0), f"{nsplit} split-K launches: not the route this case is about"
    assert header == 0, "the emitted image was flagged invalid"
    assert torch.equal(_bits(z), _bits(z2)), "consumer output differs with the word image"
    return z, ctx


def _consume(E, M, ctx, chained):
    from fp8_quantization_amd.approx_ops import approx_conv2d
    y2, w2, bW2, bR2t, qin2, args2, img, tab = ctx
    return approx_conv2d(y2, w2, E, M, None, bW2, bR2t, tab, qin=qin2, chain=(img, None) if chained else None,
                         **args2)[0]


@pytest.mark.parametrize("splitk", [False, True])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_chained_consumer_sign_build(E, M, relu, splitk, opts):
    opts("xm_ncg", 4)  # the 128 x 64 tile: M = 288 is three row tiles, the last ragged
    z, ctx = _pair(E, M, relu, splitk)
    y2 = ctx[0]
    assert bool((y2 < 0).any()) != relu
    expect = HALF if relu else FULL
    # the consumer alone, reading the image the producer left (header word [6]) and unchained (its
    # own pre-pass records): the same build, the same bits as the always-full build
    zc = _both_ways(lambda: _consume(E, M, ctx, True), expect)
    zu = _both_ways(lambda: _consume(E, M, ctx, False), expect)
    assert torch.equal(_bits(zc), _bits(z)) and torch.equal(_bits(zu), _bits(z))


def test_invalid_image_with_negative_values_is_full(opts):
    opts("xm_ncg", 4)
    z, ctx = _pair(4, 3, relu=False, seed=22)
    img = ctx[6]
    img[4:].zero_()  # garbage words (header word [6] with them) ...
    img[:4].view(torch.int32).fill_(1)  # ... flagged invalid: the gated pre-pass re-decodes y and records
    z3 = _both_ways(lambda: _consume(4, 3, ctx, True), FULL)
    assert torch.equal(_bits(z3), _bits(z))


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_depthwise_producer_records_the_sign(E, M, signed, opts):
    """The staged table-form depthwise kernel as the emitter of the next 1x1 convolution's matrix-core
    words (as test_gpu_chain.test_depthwise_handoff_to_matrix_core): signed outputs -> the consumer
    builds both halves; non-negative input and weights -> the positive rows only."""
    from fp8_quantization_amd.approx_ops import approx_conv2d, make_flags, new_word_image
    from tests.test_gpu_chain import _grid
    g = torch.Generator().manual_seed(41 + M)
    C, H, b = 24, 15, 2 ** (E - 1)
    x = _grid(g, (2, C, H, H), M).to(DEV)
    wd = _grid(g, (C, 1, 3, 3), M, -8, 0, 0.0).to(DEV)
    wp = _grid(g, (40, C, 1, 1), M, -8, 0, 0.0).to(DEV)
    if not signed:
        x, wd = x.abs(), wd.abs()
    tab, fl = _table(E, M), make_flags(True, True, True)
    bWd = torch.full((C,), b + 6, dtype=torch.int32, device=DEV)
    bWp = torch.full((40,), b + 6, dtype=torch.int32, device=DEV)
    bR = torch.tensor([b], dtype=torch.int32, device=DEV)
    qin1 = (torch.tensor([9.0], device=DEV), 8, M, 1)
    qin2 = (torch.tensor([3.5], device=DEV), 8, M, 1)
    img = new_word_image(2, C, H, H, 0, 0, DEV)
    y, _, _ = approx_conv2d(x, wd, E, M, None, bWd, bR, tab, qin=qin1, chain=(None, (img, (0, 0), qin2, bR, M)),
                            flags=fl, stride=(1, 1), padding=(1, 1), groups=C)
    torch.cuda.synchronize()
    assert int(img[:4].view(torch.int32).item()) == 0, "the staged depthwise producer did not emit"
    neg = bool((y < 0).any())
    assert neg or not signed
    opts("af32_maxct", 0)  # the unchained consumer through its A pre-pass too (not the fp32-staging form)
    z = approx_conv2d(y, wp, E, M, None, bWp, bR, tab, qin=qin2, flags=fl)[0]
    z2 = _both_ways(lambda: approx_conv2d(y, wp, E, M, None, bWp, bR, tab, qin=qin2, flags=fl, chain=(img, None))[0],
                    FULL if neg else HALF)
    assert torch.equal(_bits(z), _bits(z2))


# --------------------------------------------------------------------------------- graph capture
def test_captured_conv_follows_the_input_sign(opts):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_conv2d, make_flags
    from tests.test_gpu_chain import _grid
    from tests.test_gpu_graph import _capture
    opts("xm_ncg", 4)
    E, M = 4, 3
    g = torch.Generator().manual_seed(31)
    tab, fl = _table(E, M), make_flags(True, True, True)
    mixed = _grid(g, (2, 8, 12, 12), M).to(DEV)
    nonneg = _grid(g, (2, 8, 12, 12), M).abs().to(DEV)
    nonneg2 = _grid(g, (2, 8, 12, 12), M).abs().to(DEV)
    w = _grid(g, (16, 8, 3, 3), M, -8, 0, 0.0).to(DEV)
    bW = torch.full((16,), 14, dtype=torch.int32, device=DEV)
    x = nonneg.clone()

    def fn():
        return approx_conv2d(x, w, E, M, 10, bW, 7, tab, flags=fl, padding=(1, 1))  # bA + bW - bR = 17

    graph, out, _ = _capture(fn)
    mixed2 = -mixed.flip(0)
    # (signed twice in a row: a raised word must be raised again, not remembered, on the next replay)
    for data, expect in ((nonneg, HALF), (mixed, FULL), (mixed2, FULL), (nonneg2, HALF), (mixed, FULL)):
        x.copy_(data)
        ref, st = _counted(lambda: fn().clone())
        assert st == expect, st
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        _lib.xm_sign_stats(reset=True)
        graph.replay()
        torch.cuda.synchronize()
        assert _lib.xm_sign_stats(reset=True) == expect
        assert torch.equal(_bits(ref), _bits(out)), "replay differs from the eager launch"
        old = _lib.set_option("xm_sign_rows", 0)
        try:
            ref0 = fn()
        finally:
            _lib.set_option("xm_sign_rows", old)
        assert torch.equal(_bits(ref), _bits(ref0)), "half and full table builds differ"
