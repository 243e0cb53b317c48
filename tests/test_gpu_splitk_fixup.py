"""The in-launch split-K sum (option "splitk_fixup", gemm_f8mx_kernel's E4M3 launches): the tile's
last-arriving block sums the partial tiles and runs the final store, instead of splitk_reduce_kernel.
Option 1 against 0 (the separate reduce pass), bit for bit, with the split count forced per case (option
"splitk"):

  * matrix launches M = 200, N = 96, K = 800 / 1600 with S = 2, 3 and 6 (K-step chunks that do not divide: a
    ragged last chunk), plain and with bias + residual + output quantizer;
  * a convolution 2 x 32 x 7 x 7 -> 96 channels, 3 x 3 (K = 288), with BN + ReLU, with the residual tail and
    post quantizer, and as the producer of a word image (the emitting instance finishes the tile: image words
    and header compared, and the consumer's output);
  * every case launched twice in a row (the second launch finds the counters the first one left), and
    captured into a graph and replayed three times -- one workspace, so the arrival counters must be
    re-zeroed by every replay's own pre-pass;
  * an off-grid B operand: unit marks are raised and gemm_exact_kernel recomputes units after the sum; outputs
    and fallback counters identical.

Each run also checks that the launch really ran split on the matrix-core path.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, M = 4, 3


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _grid(g, shape, lo=-6, hi=3, zero=0.3):
    e = torch.randint(lo, hi, shape, generator=g).float()
    m = torch.randint(0, 2 ** M, shape, generator=g).float()
    v = torch.ldexp(1.0 + m / 2 ** M, e.int()) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    v[torch.rand(shape, generator=g) < zero] = 0.0
    return v


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tensors(r):
    return [t for t in (r if isinstance(r, (tuple, list)) else (r,)) if isinstance(t, torch.Tensor)]


def _capture(fn, warm=2):
    gs = torch.cuda.Stream()
    gs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(gs):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(gs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=gs, capture_error_mode="thread_local"):
        out = fn()
    return g, out


def _compare(fn, S, launches=1, split_launches=1):
    """fn() with the reduce pass (splitk_fixup 0) as the reference, then with the in-launch sum: twice eagerly,
    then captured and replayed three times; outputs and fallback counters equal every time."""
    from fp8_quantization_amd import _lib
    old = (_lib.set_option("splitk", S), _lib.set_option("splitk_fixup", 0))
    try:
        def run():
            _lib.fallback_stats(reset=True)
            _lib.path_stats(reset=True)
            _lib.splitk_stats(reset=True)
            r = fn()
            torch.cuda.synchronize()
            paths = _lib.path_stats(reset=True)
            assert paths["f8mx"] == launches and paths["fast"] == 0, paths
            assert _lib.splitk_stats(reset=True) == split_launches, "the launch did not run split"
            return [_bits(t) for t in _tensors(r)], _lib.fallback_stats(reset=True)

        ref, fb = run()
        _lib.set_option("splitk_fixup", 1)
        for again in range(2):
            got, fb1 = run()
            assert fb1 == fb, f"fallback counters differ: {fb1} vs {fb}"
            for i, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a, b), f"launch {again}: result {i} differs from the reduce pass"
        g, out = _capture(fn)
        outs = _tensors(out)
        for rep in range(3):
            for o in outs:  # scribble over the captured outputs: the replay must rewrite them
                if o.dtype == torch.float32:
                    o.fill_(float("nan"))
            _lib.fallback_stats(reset=True)
            g.replay()
            torch.cuda.synchronize()
            for i, (a, o) in enumerate(zip(ref, outs)):
                assert torch.equal(a, _bits(o)), f"replay {rep}: result {i} differs from the reduce pass"
            assert _lib.fallback_stats(reset=True) == fb, f"replay {rep} left other fallback counters"
        return fb
    finally:
        _lib.set_option("splitk", old[0])
        _lib.set_option("splitk_fixup", old[1])


def _table():
    from fp8_quantization_amd.error_tables import get_error_table_NN
    return get_error_table_NN(E, M, False, 3)


@pytest.mark.parametrize("tail", ["plain", "block"])
@pytest.mark.parametrize("S", [2, 3, 6])
@pytest.mark.parametrize("K", [800, 1600])
def test_matrix_sum_in_launch(K, S, tail):
    from fp8_quantization_amd.approx_ops import approx_matmul, approx_matmul_block, make_flags
    g = torch.Generator().manual_seed(K + S)
    b = 2 ** (E - 1)
    A = _grid(g, (200, K)).to(DEV)
    B = _grid(g, (K, 96), -8, 0, 0.0).to(DEV)
    bB = torch.full((96,), b + 6, dtype=torch.int32, device=DEV)
    res = (torch.randn((200, 96), generator=g) * 2.0).to(DEV)
    bias = torch.randn(96, generator=g).to(DEV)
    fl, tab = make_flags(True, True, True), _table()
    post = (res, 0, 0.0, 0.0, (torch.tensor([2.5], device=DEV), 8, M, 1))

    def fn():
        if tail == "plain":
            return approx_matmul(A, B, E, M, b + 2, bB, b + 1, tab, flags=fl)
        return approx_matmul_block(A, B, E, M, b + 2, bB, b + 1, tab, flags=fl, bias=bias, post=post)

    _compare(fn, S)


def _conv(g, producer, bad=False):
    from fp8_quantization_amd.approx_ops import approx_conv2d, make_flags, bn_act_epilogue
    b = 2 ** (E - 1)
    x = _grid(g, (2, 32, 7, 7)).to(DEV)
    w1 = _grid(g, (96, 32, 3, 3), -8, 0, 0.0).to(DEV)
    if bad:  # off-grid weights: their column unit is marked, the exact kernel recomputes it
        w1[3, 0, 0, 0] = 0.3333
    w2 = _grid(g, (64, 96, 3, 3), -8, 0, 0.0).to(DEV)
    bW1 = torch.full((96,), b + 6, dtype=torch.int32, device=DEV)
    bW2 = torch.full((64,), b + 6, dtype=torch.int32, device=DEV)
    fl, tab = make_flags(True, True, True), _table()
    gam = torch.rand(96, generator=g) + 0.5
    ep = bn_act_epilogue(torch.randn(96, generator=g) * 0.1, torch.rand(96, generator=g) + 0.5, gam,
                         torch.randn(96, generator=g) * 0.1, 1e-5, torch.nn.ReLU())
    ep = (ep[0].to(DEV),) + tuple(ep[1:])
    res = _grid(g, (2, 96, 7, 7)).to(DEV)
    post = (res, 1, 0.0, float("inf"), (torch.tensor([6.0], device=DEV), 8, M, 1))
    qin2 = (torch.tensor([5.5], device=DEV), 8, M, 1)
    bR2 = torch.tensor([b], dtype=torch.int32, device=DEV)
    from fp8_quantization_amd.approx_ops import word_image_bytes
    nimg = word_image_bytes(2, 96, 7, 7, 1, 1)

    def fn():
        from fp8_quantization_amd import _lib
        kw = dict(flags=fl, padding=(1, 1), epilogue=ep)
        if producer == "bn_relu":
            return approx_conv2d(x, w1, E, M, b + 2, bW1, b + 1, tab, **kw)
        if producer == "tail":
            return approx_conv2d(x, w1, E, M, b + 2, bW1, b + 1, tab, post=post, **kw)[0]
        buf = torch.zeros(nimg + 256, dtype=torch.uint8, device=DEV)
        img = buf[(-buf.data_ptr()) % 256:][:nimg]
        _lib.check(_lib.load().fp8a_word_image_init(_lib.dev_ptr(img), 2, 96, 7, 7, 1, 1,
                                                    _lib.stream_ptr(torch.device(DEV))), "fp8a_word_image_init")
        y = approx_conv2d(x, w1, E, M, b + 2, bW1, b + 1, tab, post=post,
                          chain=(None, (img, (1, 1), qin2, bR2, M)), **kw)[0]
        z, ib, _ = approx_conv2d(y, w2, E, M, None, bW2, bR2, tab, qin=qin2, chain=(img, None), flags=fl,
                                 padding=(1, 1))
        return y, img.view(torch.int32), z, ib

    return fn


@pytest.mark.parametrize("S", [2, 3, 6])
@pytest.mark.parametrize("producer", ["bn_relu", "tail", "emit"])
def test_conv_sum_in_launch(producer, S):
    fn = _conv(torch.Generator().manual_seed(11 + S), producer)
    n = 2 if producer == "emit" else 1  # (the consumer, K = 864, runs split as well)
    _compare(fn, S, launches=n, split_launches=n)


def test_marks_and_exact_recompute_after_the_sum():
    fb = _compare(_conv(torch.Generator().manual_seed(5), "tail", bad=True), 3)
    assert fb["exact_launches"] >= 1 and fb["exact_units"] >= 1
