"""The matrix-core path's stores and pre-passes with option "fq_fast" = 1 against = 0 (the literal fake
quantizer and xm_word_a everywhere: the previous code), bit for bit: the fp32 outputs as int32, the
emitted word image -- its words and its header words [0] (invalid), [5] (scale-exponent extreme) and
[6] (a negative word was written) -- the consumer's output read from that image, the quantizer
biases and the fallback counters.  In the chained cases it is the PRODUCER whose split count is asserted (its
store, or its reduction, carries the quantizers); the consumer launches of these shapes run split, with nothing
but raw sums in their stores.

Chained 3x3 pairs (padding 1, stride 1 / 2; batch 2 of 8x8 and 9x9 inputs, so the output plane is a
multiple of 4 or not -- the 16-byte and the scalar store -- and the row count is no multiple of the
128-row tile; 16 -> 64 / 72 channels, a column tail), E4M3 and E5M2, with a ReLU producer, a signed
producer and a block tail (residual + post quantizer).  The producer's BatchNorm scale plants, per
case, a channel that rounds to zero under the next quantizer (-0.0 where it is signed), one in its
subnormal band and one beyond its maxval.  One case more puts the next quantizer's grid outside the
exactness window, so the image comes back invalid and the consumer re-decodes y (through the pre-pass's
own fast word, which then marks rows for the exact kernel).  Then 1x1 launches and matrix launches with a
fused input quantizer: pre-decoded A (the pre-pass's fast forms) and fp32-staged A (whose staging keeps the
literal forms: only its store changes).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _grid(g, shape, M, lo=-6, hi=3, zero=0.3):
    e = torch.randint(lo, hi, shape, generator=g).float()
    m = torch.randint(0, 2 ** M, shape, generator=g).float()
    v = torch.ldexp(1.0 + m / 2 ** M, e.int()) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    v[torch.rand(shape, generator=g) < zero] = 0.0
    return v


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _image(Bn, C, H, W):
    """new_word_image (padding 1) on a zeroed buffer: the bytes between the last word and the
    allocation's 256-byte end are not part of the image, and are compared along with it below."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import word_image_bytes
    n = word_image_bytes(Bn, C, H, W, 1, 1)
    buf = torch.zeros(n + 256, dtype=torch.uint8, device=DEV)
    off = (-buf.data_ptr()) % 256
    img = buf[off:off + n]
    _lib.check(_lib.load().fp8a_word_image_init(_lib.dev_ptr(img), Bn, C, H, W, 1, 1, _lib.stream_ptr(torch.device(DEV))),
               "fp8a_word_image_init")
    return img


def _both(fn, launches, quantizers, may_split=False):
    """fn() under fq_fast = 0 and = 1: the two result tuples and the fallback counters of each.
    That the comparison is between the two forms, and not of the literal form with itself, is checked
    too: every one of fn's `launches` GEMMs ran on the matrix-core path (none on the VALU kernel), and none
    split along K -- except with may_split, where fn itself checks the one launch whose store the case is about
    (the producer: unsplit, or split where the reduction's tail is meant) and the consumer may run split -- and
    each (maxval, E, M) of `quantizers` passes the guard the kernels evaluate (fq_fast_ok, as
    fp8a_fq_selfcheck reports it for the same constants)."""
    from fp8_quantization_amd import _lib
    for mx, E, M in quantizers:
        assert _lib.fq_selfcheck(mx, E, M, 1, count=1)["fast"], f"maxval {mx} E{E}M{M} is outside the guard"
    out = []
    old = _lib.set_option("fq_fast", 0)
    try:
        for v in (0, 1):
            _lib.set_option("fq_fast", v)
            _lib.fallback_stats(reset=True)
            _lib.path_stats(reset=True)
            _lib.splitk_stats(reset=True)
            r = fn()
            torch.cuda.synchronize()
            paths = _lib.path_stats(reset=True)
            assert paths["f8mx"] == launches and paths["fast"] == 0, paths
            assert may_split or _lib.splitk_stats(reset=True) == 0, "a launch ran split along K"
            out.append((r, _lib.fallback_stats(reset=True)))
    finally:
        _lib.set_option("fq_fast", old)
    return out


def _same(a, b):
    (ra, sa), (rb, sb) = a, b
    assert sa == sb, f"fallback counters differ: {sa} vs {sb}"
    assert len(ra) == len(rb)
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert torch.equal(_bits(x), _bits(y)), f"result {i} differs between fq_fast 0 and 1"


def _pair(E, M, hw, stride, cout, producer, next_mx=5.5, big=2.0 ** 6, seed=3, cin=16, split=False):
    from fp8_quantization_amd.approx_ops import approx_conv2d, make_flags, bn_act_epilogue
    from fp8_quantization_amd.error_tables import get_error_table_NN
    g = torch.Generator().manual_seed(seed + hw + 7 * stride + cout)
    tab = get_error_table_NN(E, M, False, 3, zero_table_ext=(E, M) == (5, 2))
    fl = make_flags(True, True, True)
    b = 2 ** (E - 1)
    Bn, cout2 = 2, 64
    x = _grid(g, (Bn, cin, hw, hw), M).to(DEV)
    w1 = _grid(g, (cout, cin, 3, 3), M, -8, 0, 0.0).to(DEV)
    w2 = _grid(g, (cout2, cout, 3, 3), M, -8, 0, 0.0).to(DEV)
    bA, bR1, bR2 = b + 2, b + 1, b
    bW1 = torch.full((cout,), b + 6, dtype=torch.int32, device=DEV)
    bW2 = torch.full((cout2,), b + 6, dtype=torch.int32, device=DEV)
    # BatchNorm scale per channel: 1 rounds to (+-) zero under the next quantizer, 2 lands in its
    # subnormal band, 3 beyond its maxval; the rest of order one
    gam = torch.rand(cout, generator=g) + 0.5
    gam[1], gam[2], gam[3] = 2.0 ** -44, (2.0 ** -13 if E == 4 else 2.0 ** -29), big
    act = torch.nn.ReLU() if producer in ("relu", "tail") else None
    ep = bn_act_epilogue(torch.zeros(cout), torch.ones(cout), gam, torch.zeros(cout), 0.0, act)
    ep = (ep[0].to(DEV),) + tuple(ep[1:])
    ho = (hw + 2 - 3) // stride + 1
    post = None
    if producer == "tail":
        res = _grid(g, (Bn, cout, ho, ho), M).to(DEV)
        res[:, 1:3] *= 2.0 ** -14  # (the planted channels stay small through the residual add)
        post = (res, 1, -4.0, float("inf"), (torch.tensor([6.0], device=DEV), 8, M, 1))
    qin2 = (torch.tensor([next_mx], device=DEV), 8, M, 1)
    bR2t = torch.tensor([bR2], dtype=torch.int32, device=DEV)

    def run():
        from fp8_quantization_amd import _lib
        img = _image(Bn, cout, ho, ho)
        kw = dict(flags=fl, stride=(stride, stride), padding=(1, 1), epilogue=ep)
        if post is not None:
            kw["post"] = post
        _lib.splitk_stats(reset=True)
        y = approx_conv2d(x, w1, E, M, bA, bW1, bR1, tab, chain=(None, (img, (1, 1), qin2, bR2t, M)), **kw)[0]
        # (cin 16, K = 144: the producer's own store emits; split: cin 64, K = 576, the producer runs split and
        # splitk_reduce_kernel runs its tail and emits.  The consumer, K = 9 cout, may run split either way -- its
        # store and its reduction carry no quantizer)
        assert _lib.splitk_stats(reset=True) == (1 if split else 0), "the producer's store is not the one meant"
        z, ib, _ = approx_conv2d(y, w2, E, M, None, bW2, bR2t, tab, qin=qin2, chain=(img, None), flags=fl,
                                 padding=(1, 1))
        words = img.view(torch.int32)
        return y, words, words[[0, 5, 6]], z, ib

    return run


@pytest.mark.parametrize("producer", ["relu", "signed", "tail"])
@pytest.mark.parametrize("cout", [64, 72])
@pytest.mark.parametrize("hw,stride", [(8, 1), (9, 1), (8, 2), (9, 2)])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_chained_pair_bit_identical(E, M, hw, stride, cout, producer):
    lit, fast = _both(_pair(E, M, hw, stride, cout, producer), 2, [(5.5, 8 - 1 - M, M), (6.0, 8 - 1 - M, M)],
                      may_split=True)
    _same(lit, fast)
    y, _, header, _, _ = fast[0]
    assert int(header[0]) == 0, "the emitted image was flagged invalid"
    if producer == "relu":
        assert int(header[2]) == 0, "a negative word recorded after a ReLU"
    if producer == "signed":  # the planted channel really holds negative values, all rounding to -0.0
        assert int(header[2]) != 0
        assert bool((y[:, 1] < 0).any()) and float(y[:, 1].abs().max()) < 2.0 ** -31


@pytest.mark.parametrize("producer", ["relu", "signed", "tail"])
@pytest.mark.parametrize("hw", [8, 9])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_split_producer_bit_identical(E, M, hw, producer):
    """The same pairs with 64 input channels (K = 576): the producer runs split along K, so the BN / activation,
    the residual tail with its post quantizer and the emission all run in splitk_reduce_kernel -- its 16-byte form
    (8 x 8) and its scalar form (9 x 9) -- under fq_fast 0 against 1."""
    lit, fast = _both(_pair(E, M, hw, 1, 72, producer, cin=64, split=True), 2,
                      [(5.5, 8 - 1 - M, M), (6.0, 8 - 1 - M, M)], may_split=True)
    _same(lit, fast)
    assert int(fast[0][2][0]) == 0, "the emitted image was flagged invalid"


@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_window_miss_takes_the_invalid_route(E, M):
    # next maxval 2^52: its grid's top lies above the window's 2^50, and channel 3 is scaled up to reach it
    lit, fast = _both(_pair(E, M, 9, 1, 72, "signed", next_mx=2.0 ** 52, big=2.0 ** 52), 2, [(2.0 ** 52, 8 - 1 - M, M)],
                      may_split=True)
    _same(lit, fast)
    assert int(fast[0][2][0]) != 0, "no element left the window: the case does not test the invalid route"
    assert fast[1]["exact_launches"] >= 1


@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
@pytest.mark.parametrize("cout", [64, 160])
def test_pointwise_with_fused_quantizer(E, M, cout):
    """1x1, unpadded: the fp32-staging form (one column tile, A quantized and decoded while staged) and
    the pre-decoded form (160 channels: five 32-column tiles) -- unquantized input with values that round to -0.0, in the
    subnormal band and beyond maxval."""
    from fp8_quantization_amd.approx_ops import approx_conv2d, make_flags
    from fp8_quantization_amd.error_tables import get_error_table_NN
    g = torch.Generator().manual_seed(5 + cout)
    tab = get_error_table_NN(E, M, False, 3, zero_table_ext=(E, M) == (5, 2))
    b = 2 ** (E - 1)
    x = torch.randn((2, 24, 9, 9), generator=g) * torch.ldexp(torch.ones(1), torch.randint(-26, 4, (2, 24, 9, 9), generator=g))
    x = x.to(DEV)
    w = _grid(g, (cout, 24, 1, 1), M, -8, 0, 0.0).to(DEV)
    bW = torch.full((cout,), b + 6, dtype=torch.int32, device=DEV)
    bR = torch.tensor([b], dtype=torch.int32, device=DEV)
    qin = (torch.tensor([3.5], device=DEV), 8, M, 1)

    def run():
        y, ib, _ = approx_conv2d(x, w, E, M, None, bW, bR, tab, qin=qin, flags=make_flags(True, True, True))
        return y, ib

    _same(*_both(run, 1, [(3.5, 8 - 1 - M, M)]))


@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
@pytest.mark.parametrize("N", [64, 96])
def test_matrix_with_fused_quantizers(E, M, N):
    """fq_in(A) @ B + bias + residual through the output quantizer: M = 200 rows (no multiple of the
    tile), N = 64 (A staged as fp32) and 96 (A pre-decoded), unsigned and signed input quantizers."""
    from fp8_quantization_amd.approx_ops import approx_matmul_block, make_flags
    from fp8_quantization_amd.error_tables import get_error_table_NN
    g = torch.Generator().manual_seed(9 + N)
    tab = get_error_table_NN(E, M, False, 3, zero_table_ext=(E, M) == (5, 2))
    b = 2 ** (E - 1)
    A = (torch.randn((200, 72), generator=g) * torch.ldexp(torch.ones(1), torch.randint(-26, 4, (200, 72), generator=g))).to(DEV)
    B = _grid(g, (72, N), M, -8, 0, 0.0).to(DEV)
    bB = torch.full((N,), b + 6, dtype=torch.int32, device=DEV)
    bR = torch.tensor([b], dtype=torch.int32, device=DEV)
    res = (torch.randn((200, N), generator=g) * 2.0).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)

    def run(sign):
        def f():
            C, ib, ob = approx_matmul_block(A, B, E, M, None, bB, bR, tab, flags=make_flags(True, True, True), bias=bias,
                                            qin=(torch.tensor([3.5], device=DEV), 8, M, sign),
                                            post=(res, 0, 0.0, 0.0, (torch.tensor([2.5], device=DEV), 8, M, 1)))
            return C, ib, ob
        return f

    for sign in (0, 1):
        _same(*_both(run(sign), 1, [(3.5, 8 - sign - M, M), (2.5, 8 - 1 - M, M)]))
