"""gemm_f8mx_kernel's 128 x 64 math loop with its waves mapped by rows (option "xm_wave_rows").

With "xm_wave_rows" = 1 (the default, under "xm_pipe" = 1) the word-staged 128 x 64 launches run the instances
in which wave w converts tile rows 32 w .. 32 w + 31 for all 64 columns -- one table address per (row block,
K-step) for the four column groups -- instead of 16 columns of all 128 rows.  Every accumulator still takes one
MFMA per staged tile, in K order, over the same codes, so every output must be bit-identical to
"xm_wave_rows" = 0 (waves by columns).  Checked here with "xm_ncg" forced to 4, all as int32 views, with the
fallback counters and the launch's path (f8mx) read back:
  * matmul M = 130, N = 70 (two row tiles, the second with 2 live rows; two column tiles, the second with 6
    live columns) with K = 5, 8, 16, 19, 24 (a partial staged tile, exactly one, two, a K tail inside the third,
    three), E4M3 and E5M2, A non-negative (half table build), mixed-sign (full build) and all zero;
  * split-K: matmul 200 x 96 x 800 with "splitk" forced to 2 and 3, summed by the reduction kernel (the plain
    instance's raw partial stores);
  * a 3x3 convolution (pad 1, 3 -> 20 channels, 2 images of 9 x 9: K = 27, M = 162) chained to a second 3x3
    through the word image, so the emitting instance runs: a ReLU producer and a signed one; outputs, the
    word image and its header compared;
  * a tile that takes the exact kernel (one term past the e4m3 range), an off-grid A element, and an E5M2
    launch that raises FB_HALF (the halved-block rerun, which keeps its mapping, follows it);
  * one captured launch replayed three times with the option on.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MM, MN = 130, 70


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    assert _lib.set_option("xm_pipe", 1) == 1, "the waves-by-rows instances exist only under xm_pipe = 1"


@pytest.fixture
def opts():
    """set(name, value) for library options, restored afterwards; "xm_ncg" = 4 (the 128 x 64 tile) throughout."""
    from fp8_quantization_amd import _lib
    old = []

    def set_(name, value):
        old.append((name, _lib.set_option(name, value)))

    set_("xm_ncg", 4)
    yield set_
    for name, value in reversed(old):
        _lib.set_option(name, value)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _table(E, M):
    from fp8_quantization_amd.error_tables import get_error_table_NN
    return get_error_table_NN(E, M, False, 3, zero_table_ext=(E, M) == (5, 2))


def _run(fn, rows):
    """fn() under "xm_wave_rows" = rows: (its tensors, path counters, fallback counters)."""
    from fp8_quantization_amd import _lib
    old = _lib.set_option("xm_wave_rows", rows)
    try:
        _lib.path_stats(reset=True)
        _lib.fallback_stats(reset=True)
        out = fn()
        torch.cuda.synchronize()
        return out, _lib.path_stats(reset=True), _lib.fallback_stats(reset=True)
    finally:
        _lib.set_option("xm_wave_rows", old)


def _both(fn, names=None):
    """fn() (a tensor or a tuple of tensors) with the waves by rows and by columns: equal bits, equal counters,
    every launch on the f8mx path.  Returns (the by-rows outputs, fallback counters)."""
    on, paths1, fb1 = _run(fn, 1)
    off, paths0, fb0 = _run(fn, 0)
    on = on if isinstance(on, tuple) else (on,)
    off = off if isinstance(off, tuple) else (off,)
    for paths in (paths1, paths0):
        assert paths["f8mx"] >= 1 and sum(v for k, v in paths.items() if k not in ("f8mx", "exact")) == 0, paths
    assert paths1 == paths0, (paths1, paths0)
    assert fb1 == fb0, (fb1, fb0)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        what = names[i] if names else f"output {i}"
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what} differs between xm_wave_rows = 1 and 0"
    return on, fb1


# --------------------------------------------------------------------------------------- matmul
def _operands(E, M, Mr, K, N, variant, seed=5):
    """A [Mr, K], B [K, N] on the (M, bias) grids, every term inside the result format's range."""
    rng = np.random.default_rng(seed)
    if M == 3:
        bA, bB, bR, ea, eb = 9, 12, 3, (3, 12), (5, 12)
    else:
        bA, bB, bR, ea, eb = 20, 20, 7, (21, 28), (21, 28)
    A = np.ldexp(1.0 + rng.integers(0, 2 ** M, (Mr, K)) / 2.0 ** M, rng.integers(*ea, (Mr, K)) - bA)
    B = np.ldexp(1.0 + rng.integers(0, 2 ** M, (K, N)) / 2.0 ** M, rng.integers(*eb, (K, N)) - bB)
    B *= rng.choice([-1.0, 1.0], B.shape)
    A[rng.random(A.shape) < 0.3] = 0.0
    if variant == "mixed":
        A *= rng.choice([-1.0, 1.0], A.shape)
    elif variant == "zero":
        A[:] = 0.0
    return A.astype(np.float32), B.astype(np.float32), bA, bB, bR


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("variant", ["nonneg", "mixed", "zero"])
@pytest.mark.parametrize("K", [5, 8, 16, 19, 24])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_matmul_wave_rows_bit_identical(E, M, K, variant, opts):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    A, B, bA, bB, bR = _operands(E, M, MM, K, MN, variant)
    A, B = _dev(A), _dev(B)
    tab, fl = _table(E, M), make_flags(True, True, True)
    _lib.xm_sign_stats(reset=True)
    (C,), fb = _both(lambda: approx_matmul(A, B, E, M, bA, bB, bR, tab, flags=fl))
    # the table build each case is about: positive rows only / both halves, in both runs
    st = _lib.xm_sign_stats(reset=True)
    assert st == (dict(half=0, full=2) if variant == "mixed" else dict(half=2, full=0)), st
    assert fb["exact_launches"] == 0, "the operands left the matrix-core range"
    assert tuple(C.shape) == (MM, MN) and bool((C != 0).any()) != (variant == "zero")
    if variant != "zero":  # the ragged edges are live: the last row (tile 2, row 1) and column (tile 2, column 5)
        assert bool((C[MM - 1] != 0).any()) and bool((C[:, MN - 1] != 0).any())


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_splitk_reduce_wave_rows_bit_identical(E, M, splits, opts):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    opts("splitk", splits)
    opts("splitk_fixup", 0)
    A, B, bA, bB, bR = _operands(E, M, 200, 800, 96, "mixed", seed=9)
    A, B = _dev(A), _dev(B)
    tab, fl = _table(E, M), make_flags(True, True, True)
    _lib.splitk_stats(reset=True)
    _, fb = _both(lambda: approx_matmul(A, B, E, M, bA, bB, bR, tab, flags=fl))
    assert _lib.splitk_stats(reset=True) == 2, "the launches did not run split along K"
    assert fb["exact_launches"] == 0


# --------------------------------------------------------------------------------- chained convs
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_chained_convs_wave_rows_bit_identical(E, M, relu, opts):
    from fp8_quantization_amd import _lib
    from tests.test_gpu_chain import _run_pair
    kw = dict(cin=3, cmid=20, cout=24, hw=9, Bn=2, k1=3, k2=3, p1=1, p2=1, epilogue=relu, post=False, seed=33)

    def fn():
        z, z2, _, header, ctx = _run_pair(E, M, **kw)
        assert header == 0, "the emitted image was flagged invalid"
        return z, z2, ctx[0], ctx[6]

    _lib.splitk_stats(reset=True)
    (z, z2, y2, img), fb = _both(fn, ("the unchained consumer's output", "the chained consumer's output",
                                      "the emitting producer's output", "the word image (header and words)"))
    assert _lib.splitk_stats(reset=True) == 0, "a split launch: the reduction kernel emitted, not gemm_f8mx_kernel"
    assert tuple(y2.shape) == (2, 20, 9, 9) and bool((y2 < 0).any()) != relu
    assert torch.equal(_bits(z), _bits(z2))
    assert fb["exact_launches"] == 0


# ------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("case", ["term_out_of_range", "off_grid_a"])
def test_fallback_wave_rows_bit_identical(case, opts):
    """E4M3: one term past the e4m3 range of bR (its tile converts to NaN and takes the exact kernel) /
    one A element off the grid (the pre-pass marks its row): the same outputs and counters."""
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    E, M, K = 4, 3, 19
    A, B, bA, bB, bR = _operands(E, M, MM, K, MN, "mixed", seed=13)
    r, k0, n = 77, 11, 66
    if case == "term_out_of_range":
        # row k0 of B small but for column n, A[r, k0] = 2^14: the product with B[k0, n] = 1 is past
        # 1.75 x 2^(15 - bR), every other one of the row stays in range
        B[k0, :] /= 16.0
        B[k0, n] = 1.0
        A[:, k0] = np.abs(A[:, k0])
        A[r, k0] = 2.0 ** 14
    else:
        A[r, k0] = 1.0 + 2.0 ** -10
    A, B = _dev(A), _dev(B)
    tab, fl = _table(E, M), make_flags(True, True, True)
    (C,), fb = _both(lambda: approx_matmul(A, B, E, M, bA, bB, bR, tab, flags=fl))
    assert fb["exact_launches"] == 1 and fb["exact_units"] >= 1, fb
    assert bool(torch.isfinite(C).all())


def test_e5m2_halved_block_rerun_follows_the_wave_rows_launch(opts):
    """The E5M2 grid's top binade: the plain launch (waves by rows) raises FB_HALF and the halved-block form
    -- which keeps the mapping by columns -- recomputes its tiles; no exact fallback."""
    from fp8_quantization_amd import _lib
    from oracle import oracle as orc
    from tests.test_gpu_f8_e5m2 import FB_ANY, FB_HALF, _all_codes, _codes_from, _matmul_raw
    from tests.test_gpu_f8_e5m2 import _table as e5m2_table
    bA, bB, bR = 20, 20, 8
    A = _all_codes(bA).reshape(-1, 1)
    B = _codes_from(bB, 16).reshape(1, -1)
    tab = e5m2_table("zero")
    fl = orc.flags_of(approx=True, s2n=True, qbma=True)
    res = []
    for rows in (1, 0):
        old = _lib.set_option("xm_wave_rows", rows)
        try:
            res.append(_matmul_raw(A, B, bA, bB, bR, tab, fl))
        finally:
            _lib.set_option("xm_wave_rows", old)
    (C1, flag1, paths1), (C0, flag0, paths0) = res
    assert paths1 == paths0 and paths1["f8mx"] == 1, (paths1, paths0)
    assert flag1 == flag0 and flag1 & FB_HALF and flag1 & FB_ANY == 0, (flag1, flag0)
    assert np.array_equal(C1.view(np.int32), C0.view(np.int32))


# ------------------------------------------------------------------------------------- captured
def test_captured_launch_replays_bit_identical(opts):
    """One launch captured with the option on and replayed three times: every replay's output equals the
    eager by-columns output."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_matmul, make_flags
    E, M, K = 4, 3, 19
    A, B, bA, bB, bR = _operands(E, M, MM, K, MN, "mixed", seed=21)
    A, B = _dev(A), _dev(B)
    tab, fl = _table(E, M), make_flags(True, True, True)

    def fn():
        return approx_matmul(A, B, E, M, bA, bB, bR, tab, flags=fl)

    ref, paths0, fb0 = _run(fn, 0)
    assert paths0["f8mx"] == 1 and fb0["exact_launches"] == 0, (paths0, fb0)
    ref = _bits(ref)
    old = _lib.set_option("xm_wave_rows", 1)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()  # (warm: allocations and the workspace exist before the capture)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            C = fn()
        for i in range(3):
            C.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(_bits(C), ref), f"replay {i} differs from the by-columns output"
    finally:
        _lib.set_option("xm_wave_rows", old)
