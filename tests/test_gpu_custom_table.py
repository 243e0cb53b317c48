"""Custom error tables on the GPU fast paths.

A table without negative entries whose V' = sig_a sig_b - T 2^-M stay positive (xm_table_form,
csrc/fp8approx.hip) runs the E4M3 / E5M2 matrix-core kernel, the depthwise table form and the word-image
hand-off like the built-in table; a table with a negative entry stays on gemm_fast_kernel.  Checked here,
against the CPU oracle:
  * every E4M3 / E5M2 code pair as a K = 1 term, bit-exact, with the matrix-core launch counter, the
    fallback counters and the launch's flag word read back (E5M2: the halved-block form of the grid's
    top binade included, with V' below 0.5 in the table);
  * the VALU TM_F8 form (an E4M3 launch whose workspace lacks the pre-decoded operands) on the same
    table: it builds V' from the raw table, so it takes the same tables -- bit-exact terms;
  * sums within the 1e-5 sum|v| bar, bit-identical run to run;
  * the depthwise table form, the expo-0 binade included, gate word 0;
  * the hand-off between two convolutions; the operators and ResNet-18 with
    custom_approx_params["error_table"]; the validate driver's --error-table.
"""
import json

import numpy as np
import pytest
import torch
from torch import nn

from oracle import oracle as orc
from tests import golden_io as gio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T_POS = np.array([[(ma + 2 * mb + 3) % 4 for mb in range(8)] for ma in range(8)], np.int32)  # 0..3; (0,0) = 3
T_SGN = T_POS - 1                                                                             # negative entries
T_E5 = np.array([[(ma + mb + 2) % 3 for mb in range(4)] for ma in range(4)], np.int32)       # E5M2; (0,0) = 2
FL = orc.flags_of(approx=True, s2n=True, qbma=True)
FB_ANY, FB_HALF = 1, 64  # the flag word's exact-fallback / halved-block bits (csrc/fp8approx_common.h)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def test_fixture_tables_keep_every_significand_product_positive():
    for tab, n in ((T_POS, 8), (T_SGN, 8), (T_E5, 4)):
        N = (n + np.arange(n))[:, None] * (n + np.arange(n))[None, :] - n * tab
        assert N.min() >= 1
    assert 64 - 8 * T_POS[0, 0] == 40 and 16 - 4 * T_E5[0, 0] == 8 and T_SGN.min() < 0


def _all_codes(bias, E, M, min_field=0):
    """The values of the (E, M, bias) grid with exponent field >= min_field, both signs (both zeros)."""
    n = 1 << M
    e = np.repeat(np.arange(min_field, 1 << E), n)
    m = np.tile(np.arange(n), (1 << E) - min_field)
    v = np.where(e == 0, np.ldexp(m / n, 1 - bias), np.ldexp(1.0 + m / n, e - bias))
    return np.concatenate([v, -v]).astype(np.float32)


def _matmul_raw(A, B, E, M, bA, bB, bR, table, flags, ws_bytes=None):
    """fp8a_matmul through ctypes with a caller-owned workspace (ws_bytes: smaller than the size query, so
    that the launch finds no room for its pre-decoded operands): (C, flag word, paths, matrix-core launches)."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    A = torch.from_numpy(np.ascontiguousarray(A)).to(DEV)
    B = torch.from_numpy(np.ascontiguousarray(B)).to(DEV)
    Mr, K = A.shape
    N = B.shape[1]
    C = torch.empty((Mr, N), dtype=torch.float32, device=DEV)
    n = max(int(L.fp8a_matmul_workspace_size_mnk(Mr, N, K)), 256) if ws_bytes is None else ws_bytes
    ws = torch.zeros(n, dtype=torch.uint8, device=DEV)
    tA = torch.tensor([bA], dtype=torch.int32, device=DEV)
    tB = torch.as_tensor(np.asarray(bB, np.int32).reshape(-1)).to(DEV)
    tR = torch.tensor([bR], dtype=torch.int32, device=DEV)
    tab = torch.as_tensor(np.ascontiguousarray(table, np.int32))
    _lib.path_stats(reset=True)
    _lib.xm_sign_stats(reset=True)
    rc = L.fp8a_matmul(_lib.dev_ptr(A), K, _lib.dev_ptr(B), N, 1, _lib.dev_ptr(C), N, Mr, N, K, E, M,
                       _lib.dev_ptr(tA), _lib.dev_ptr(tB), 0 if tB.numel() == 1 else 1, _lib.dev_ptr(tR),
                       _lib.host_ptr(tab), flags, _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "fp8a_matmul")
    torch.cuda.synchronize()
    flag = int(ws[:4].view(torch.int32).item())
    xm = _lib.xm_sign_stats(reset=True)
    return C.cpu().numpy(), flag, _lib.path_stats(reset=True), xm["half"] + xm["full"]


def _terms_equal(got, ref, what=""):
    """bit-exact up to the sign of zero (as tests/test_gpu_f8.py)"""
    same = (got.view(np.uint32) == ref.view(np.uint32)) | ((got == 0) & (ref == 0))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} terms differ; first at {i}: got {got[i]!r} ref {ref[i]!r}")


_ZERO_FB = dict(exact_launches=0, exact_units=0, f32_reruns=0, tb_launches=0)
E4M3_BIASES = [(12, 12, 8), (10, 13, 7), (9, 9, 2), (12, 14, 0), (8, 8, -14), (20, 18, 22)]  # tests/test_gpu_f8.py's


# ------------------------------------------------------------------------------ 1. all code pairs, E4M3
@pytest.mark.parametrize("biases", E4M3_BIASES)
def test_e4m3_every_code_pair_on_the_matrix_core(biases):
    from fp8_quantization_amd import _lib
    bA, bB, bR = biases
    A = _all_codes(bA, 4, 3).reshape(-1, 1)
    B = _all_codes(bB, 4, 3).reshape(1, -1)
    _lib.fallback_stats(reset=True)
    C, flag, paths, xm = _matmul_raw(A, B, 4, 3, bA, bB, bR, T_POS, FL)
    _terms_equal(C, orc.terms(A, B, 4, 3, bA, bB, bR, T_POS, FL)[:, 0, :], f"T_pos {biases}")
    assert xm >= 1, "the matrix-core launch counter did not advance"
    assert paths["f8mx"] == 1 and paths["fast"] == 0, paths
    assert flag == 0 and _lib.fallback_stats(reset=True) == _ZERO_FB


@pytest.mark.parametrize("biases", E4M3_BIASES)
def test_e4m3_signed_table_stays_off_the_matrix_core(biases):
    bA, bB, bR = biases
    A = _all_codes(bA, 4, 3).reshape(-1, 1)
    B = _all_codes(bB, 4, 3).reshape(1, -1)
    C, _, paths, xm = _matmul_raw(A, B, 4, 3, bA, bB, bR, T_SGN, FL)
    _terms_equal(C, orc.terms(A, B, 4, 3, bA, bB, bR, T_SGN, FL)[:, 0, :], f"T_sgn {biases}")
    assert xm == 0 and paths["f8mx"] == 0 and paths["fast"] == 1, (xm, paths)


@pytest.mark.parametrize("biases", E4M3_BIASES)
def test_e4m3_valu_f8_form_takes_the_same_table(biases):
    """An E4M3 launch whose workspace holds the flag block only: gemm_fast_kernel's TM_F8 form, which builds
    V' from the raw table in fp32."""
    bA, bB, bR = biases
    A = _all_codes(bA, 4, 3).reshape(-1, 1)
    B = _all_codes(bB, 4, 3).reshape(1, -1)
    C, flag, paths, xm = _matmul_raw(A, B, 4, 3, bA, bB, bR, T_POS, FL, ws_bytes=256)
    _terms_equal(C, orc.terms(A, B, 4, 3, bA, bB, bR, T_POS, FL)[:, 0, :], f"T_pos {biases} (VALU)")
    assert xm == 0 and paths["fast"] == 1 and paths["f8mx"] == 0 and flag == 0, (xm, paths, flag)


# ------------------------------------------------------------------------------ 2. all code pairs, E5M2
# (tests/test_gpu_f8_e5m2.py's triples: bA + bB - bR >= 33, every product inside the e5m2 range)
@pytest.mark.parametrize("biases", [(20, 20, 7), (18, 22, 5), (16, 17, 0), (10, 10, -13), (30, 12, 9)])
def test_e5m2_every_code_pair_on_the_matrix_core(biases):
    from fp8_quantization_amd import _lib
    bA, bB, bR = biases
    A = _all_codes(bA, 5, 2).reshape(-1, 1)
    B = _all_codes(bB, 5, 2).reshape(1, -1)
    _lib.fallback_stats(reset=True)
    C, flag, paths, xm = _matmul_raw(A, B, 5, 2, bA, bB, bR, T_E5, FL)
    _terms_equal(C, orc.terms(A, B, 5, 2, bA, bB, bR, T_E5, FL)[:, 0, :], f"T_e5 {biases}")
    assert xm >= 1 and paths["f8mx"] == 1 and paths["fast"] == 0, (xm, paths)
    assert flag == 0 and _lib.fallback_stats(reset=True) == _ZERO_FB


def test_e5m2_top_binade_with_the_halved_block_form():
    """bA + bB - bR = 32: products reach the grid's top binade 31 - bR, which the plain form hands to the
    halved-block instance (FB_HALF); its `tok` threshold reads the table's true lowest V' binade (-1 here:
    V'(0, 0) = 8 / 16).  No exact fallback."""
    from fp8_quantization_amd import _lib
    bA, bB, bR = 20, 20, 8
    A = _all_codes(bA, 5, 2).reshape(-1, 1)
    B = _all_codes(bB, 5, 2, min_field=16).reshape(1, -1)
    ref = orc.terms(A, B, 5, 2, bA, bB, bR, T_E5, FL)[:, 0, :]
    assert np.abs(ref).max() >= 2.0 ** (31 - bR), "the case must reach the top binade"
    _lib.fallback_stats(reset=True)
    C, flag, paths, xm = _matmul_raw(A, B, 5, 2, bA, bB, bR, T_E5, FL)
    _terms_equal(C, ref, "T_e5 top binade")
    assert xm >= 1 and paths["f8mx"] == 1 and flag & FB_ANY == 0 and flag & FB_HALF, (xm, paths, flag)
    assert _lib.fallback_stats(reset=True)["exact_launches"] == 0


# ------------------------------------------------------------------------------ 3. sums
def _sum_operands(Mr, K, N, seed):
    """(tests/test_gpu_f8.py's: no product reaches the result grid's top binade, bR <= bA + min bB - 16)"""
    rng = np.random.default_rng(seed)
    bA, bR = 9, 3
    bB = rng.integers(11, 15, size=N).astype(np.int32)
    e = rng.integers(3, 16, size=(Mr, K))
    m = rng.integers(0, 8, size=(Mr, K))
    A = np.ldexp(1.0 + m / 8.0, e - bA) * rng.choice([-1.0, 1.0], size=(Mr, K))
    A[rng.random((Mr, K)) < 0.4] = 0.0
    e = rng.integers(5, 16, size=(K, N))
    m = rng.integers(0, 8, size=(K, N))
    B = np.ldexp(1.0 + m / 8.0, e - bB[None, :]) * rng.choice([-1.0, 1.0], size=(K, N))
    return A.astype(np.float32), B.astype(np.float32), bA, bB, bR


# (257 x 33, K = 100: ragged tiles, the narrow column tile; 200 x 96, K = 800 split 3 ways:
# tests/test_gpu_splitk_fixup.py's matrix shape, with the reduce pass and with the in-launch sum; 1 x 1 x 1)
@pytest.mark.parametrize("shape,split,fixup", [((257, 100, 33), 0, 0), ((200, 800, 96), 3, 0), ((200, 800, 96), 3, 1),
                                               ((1, 1, 1), 0, 0)])
def test_sums_within_bar_and_run_to_run_identical(shape, split, fixup):
    from fp8_quantization_amd import _lib
    Mr, K, N = shape
    A, B, bA, bB, bR = _sum_operands(Mr, K, N, Mr + K + N)
    Cref, S = orc.matmul(A, B, 4, 3, bA, bB, bR, T_POS, FL, with_abs=True)
    old = (_lib.set_option("splitk", split), _lib.set_option("splitk_fixup", fixup))
    try:
        _lib.splitk_stats(reset=True)
        C, flag, paths, xm = _matmul_raw(A, B, 4, 3, bA, bB, bR, T_POS, FL)
        assert _lib.splitk_stats(reset=True) == (1 if split else 0)
        C2 = _matmul_raw(A, B, 4, 3, bA, bB, bR, T_POS, FL)[0]
    finally:
        _lib.set_option("splitk", old[0])
        _lib.set_option("splitk_fixup", old[1])
    assert flag == 0 and paths["f8mx"] == 1 and xm >= 1, (flag, paths, xm)
    assert np.all(np.abs(C.astype(np.float64) - Cref) <= gio.sum_tolerance(S.astype(np.float64)))
    assert np.array_equal(C.view(np.uint32), C2.view(np.uint32)), "two runs differ"


# ------------------------------------------------------------------------------ 4. depthwise table form
def _dw_raw(x, w, bA, bW, bR, table, flags, stride, pad, fmt):
    """fp8a_conv2d on a depthwise layer with a caller-owned workspace: (y, gate word)."""
    from fp8_quantization_amd import _lib
    L = _lib.load()
    Bn, C, H, W = x.shape
    kh, kw = w.shape[2], w.shape[3]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    xt = torch.as_tensor(np.ascontiguousarray(x)).to(DEV)
    wt = torch.as_tensor(np.ascontiguousarray(w)).to(DEV)
    y = torch.empty((Bn, C, Ho, Wo), dtype=torch.float32, device=DEV)
    n = int(L.fp8a_conv2d_workspace_size(Bn, C, H, W, C, kh, kw, stride, stride, pad, pad, 1, 1, C))
    ws = torch.zeros(n, dtype=torch.uint8, device=DEV)
    tA = torch.tensor([bA], dtype=torch.int32, device=DEV)
    tW = torch.as_tensor(np.asarray(bW, np.int32)).to(DEV)
    tR = torch.tensor([bR], dtype=torch.int32, device=DEV)
    tab = torch.as_tensor(np.ascontiguousarray(table, np.int32))
    rc = L.fp8a_conv2d(_lib.dev_ptr(xt), _lib.dev_ptr(wt), _lib.dev_ptr(y), Bn, C, H, W, C, kh, kw, stride, stride,
                       pad, pad, 1, 1, C, fmt[0], fmt[1], _lib.dev_ptr(tA), _lib.dev_ptr(tW), _lib.dev_ptr(tR),
                       _lib.host_ptr(tab), flags, _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "fp8a_conv2d")
    torch.cuda.synchronize()
    return y.cpu().numpy(), int(ws[:4].view(torch.int32).item())


# (the one-nonzero-tap construction of tests/test_gpu_tbx.py and its bias triples: products near 2^-bR, so
# every case holds terms in the expo-0 binade [2^-bR, 2^(1-bR)) and the F7 band)
@pytest.mark.parametrize("fmt,tab,biases", [((4, 3), T_POS, (12, 12, 8)), ((4, 3), T_POS, (9, 9, 2)),
                                            ((4, 3), T_POS, (14, 14, 20)), ((4, 3), T_POS, (8, 8, 3)),
                                            ((5, 2), T_E5, (20, 20, 9)), ((5, 2), T_E5, (28, 28, 40))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_table_form_every_code_pair(fmt, tab, biases, stride):
    from fp8_quantization_amd import _lib
    bA, bW_, bR = biases
    a, b = _all_codes(bA, *fmt), _all_codes(bW_, *fmt)
    C = 256
    if stride == 1:
        x = np.broadcast_to(a.reshape(1, 1, 16, 16), (1, C, 16, 16)).copy()
    else:  # stride 2 with padding 1: output (i, j) centres on input (2i, 2j)
        x = np.zeros((1, C, 32, 32), np.float32)
        x[:, :, 0::2, 0::2] = a.reshape(1, 1, 16, 16)
    w = np.zeros((C, 1, 3, 3), np.float32)
    w[:, 0, 1, 1] = b
    bW = np.full(C, bW_, np.int32)
    ref = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), fmt[0], fmt[1], bA, bW, bR, tab, FL | orc.TB)[:, 0, :]
    expo0 = (np.abs(ref) >= 2.0 ** -bR) & (np.abs(ref) < 2.0 ** (1 - bR))
    assert expo0.any(), "the case must hold terms in the expo-0 binade"
    _lib.fallback_stats(reset=True)
    y, gate = _dw_raw(x, w, bA, bW, bR, tab, FL, stride, 1, fmt)
    assert gate == 0, "gate raised: the table form did not produce these terms"
    assert _lib.fallback_stats(reset=True)["tb_launches"] == 0
    _terms_equal(y[0].reshape(C, 256).T, ref, f"depthwise {fmt} {biases} stride {stride}")


def test_wants_image_follows_the_table_predicate():
    """fp8a_conv2d_wants_image (the hand-off's question "would this convolution read a word image?") is
    the matrix-core form's predicate: 1 for the zero, the built-in and the non-negative custom tables,
    0 for a negative entry or a V' that would not stay positive."""
    from fp8_quantization_amd.approx_ops import conv2d_wants_image
    wants = lambda tab: conv2d_wants_image(32, (3, 3), (1, 1), 1, 4, 3, torch.as_tensor(tab), FL)  # noqa: E731
    assert wants(T_POS) == 1 and wants(T_SGN) == 0
    assert wants(np.zeros((8, 8), np.int32)) == 1 and wants(gio.load("g2_matmul.npz")["E4M3_table_nocomp"]) == 1
    none_left = np.zeros((8, 8), np.int32)
    none_left[0, 0] = 8  # N = 64 - 64 = 0: V' would be zero
    assert wants(none_left) == 0
    assert conv2d_wants_image(32, (3, 3), (1, 1), 1, 5, 2, torch.as_tensor(T_E5), FL) == 1


# ------------------------------------------------------------------------------ 5. hand-off
def test_hand_off_between_two_convolutions():
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import conv2d_wants_image
    from tests.test_gpu_chain import _bits, _run_pair
    tab = torch.as_tensor(T_POS)
    assert conv2d_wants_image(16, (3, 3), (1, 1), 1, 4, 3, tab, FL) == 1, "the consumer would not read an image"
    _lib.path_stats(reset=True)
    _lib.fallback_stats(reset=True)
    z, z2, (ib, ib2), header, _ = _run_pair(4, 3, cin=8, cmid=16, cout=16, hw=12, Bn=2, k1=3, k2=3, p1=1, p2=1,
                                            epilogue=False, post=False, seed=21, fmt_table=tab)
    paths = _lib.path_stats(reset=True)
    assert header == 0, "the image was not emitted (flagged invalid)"
    assert paths["f8mx"] == 4 and paths["fast"] == 0, paths  # producer and consumer, unchained and chained
    assert torch.equal(_bits(z), _bits(z2)), "consumer output differs with the word image"
    assert torch.equal(ib, ib2)
    assert _lib.fallback_stats(reset=True)["exact_launches"] == 0


# ------------------------------------------------------------------------------ 6. operator and model
def _record_operands(mods):
    """Wrap run_forward of every module: keep the (quantized input, quantized weight) it was called with."""
    rec = {}

    def wrap(name, mod):
        orig = mod.run_forward

        def run_forward(x, weight, bias, *a, **kw):
            assert kw.get("qin") is None, "the input quantizer was fused: x is not the quantized operand"
            rec[name] = (x.detach().clone(), weight.detach().clone())
            return orig(x, weight, bias, *a, **kw)
        mod.run_forward = run_forward
    for name, mod in mods:
        mod.fuse_input_quant = False  # the hijacker quantizes x before run_forward
        wrap(name, mod)
    return rec


def _calibrate(mod, x_cal):
    mod.quantized()
    mod.estimate_ranges()
    with torch.no_grad():
        mod(x_cal)
    mod.fix_ranges()


@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_operator_equals_direct_op_call(kind):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_calculation import QCustomBNConv2dTorch, QCustomLinearTorch
    from fp8_quantization_amd.approx_ops import approx_conv2d, approx_matmul, make_flags
    from fp8_quantization_amd.error_tables import get_error_table_NN
    from fp8_quantization_amd.resnet_workload import approx_qparams
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    qp = approx_qparams(error_table=T_POS.tolist())
    if kind == "linear":
        mod = QCustomLinearTorch(in_features=72, out_features=24, bias=False, **qp)
        shape = (37, 72)
    else:
        mod = QCustomBNConv2dTorch(in_channels=8, out_channels=16, kernel_size=3, padding=1, bias=False,
                                   activation=nn.ReLU(), **qp)
        shape = (2, 8, 12, 12)
    mod = mod.to(DEV).eval()
    _calibrate(mod, torch.randn(shape, generator=g).to(DEV))
    rec = _record_operands([("m", mod)])
    with torch.no_grad():
        mod(torch.randn(shape, generator=g).to(DEV))
    x, w = rec["m"]
    E, M, tab, flags = mod._approx_config()
    assert tab.numpy().tolist() == T_POS.tolist() and flags == make_flags(True, True, True)
    bA = mod._default_bias(mod.get_acts_fp_bias(), E, x.device)
    bW, bR = mod.get_weights_fp_bias(), mod._default_bias(mod.get_res_fp_bias(), E, x.device)
    _lib.path_stats(reset=True)
    with torch.no_grad():
        got = mod.run_forward(x, w, None)
    assert _lib.path_stats(reset=True)["f8mx"] == 1
    builtin = get_error_table_NN(4, 3, False, 3)
    if kind == "linear":
        direct = approx_matmul(x, w.t(), E, M, bA, bW, bR, torch.as_tensor(T_POS), flags=flags)
        other = approx_matmul(x, w.t(), E, M, bA, bW, bR, builtin, flags=flags)
    else:
        direct = approx_conv2d(x, w, E, M, bA, bW, bR, torch.as_tensor(T_POS), flags=flags, padding=(1, 1))
        other = approx_conv2d(x, w, E, M, bA, bW, bR, builtin, flags=flags, padding=(1, 1))
    assert torch.equal(got.view(torch.int32), direct.view(torch.int32))
    assert not torch.equal(got, other), "the custom table computes what the built-in one does"


@pytest.fixture(scope="module")
def resnet18_pair():
    """ResNet-18 at 2 x 3 x 32 x 32 with the built-in table and with error_table = T_pos: the same weights and
    BN statistics, each through estimate -> fix; (custom model, logits custom, logits built-in, input)."""
    from fp8_quantization_amd import resnet_workload as rw
    g = torch.Generator().manual_seed(2)
    x_cal = torch.randn((2, 3, 32, 32), generator=g).to(DEV)
    x = torch.randn((2, 3, 32, 32), generator=g).to(DEV)
    out = []
    for cfg in (dict(error_table=torch.as_tensor(T_POS)), {}):
        torch.manual_seed(1)
        fp = rw.ResNet(rw.BasicBlock, (2, 2, 2, 2))
        rw.estimate_bn_statistics(fp, 1, batch_size=4, input_shape=(3, 32, 32), device=torch.device("cpu"))
        m = rw.QuantizedResNet(fp, input_size=(1, 3, 32, 32), **rw.approx_qparams(**cfg)).to(DEV).eval()
        _calibrate(m, x_cal)
        with torch.no_grad():
            out.append((m, m(x).cpu().numpy()))
    return out[0][0], out[0][1], out[1][1], x


def test_resnet18_logits_differ_from_the_builtin_tables(resnet18_pair):
    _, custom, builtin, _ = resnet18_pair
    assert np.isfinite(custom).all() and np.isfinite(builtin).all()
    assert not np.array_equal(custom, builtin)


def test_resnet18_layers_match_the_oracle(resnet18_pair):
    """Every approx layer, teacher-forced (the pattern of tests/test_gpu_model.py): the layer's run_forward on
    the quantized operands the model's own forward gave it, against the double-accumulated oracle on the same
    operands with the same table, within 1e-5 sum|v|."""
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_calculation import ApproxOpMixin
    m, _, _, x = resnet18_pair
    layers = [(n, mod) for n, mod in m.named_modules() if isinstance(mod, ApproxOpMixin) and mod.approx_flag]
    assert len(layers) == 21  # 20 convolutions and the classifier
    rec = _record_operands(layers)
    with torch.no_grad():
        m(x)
    assert set(rec) == {n for n, _ in layers}
    _lib.path_stats(reset=True)
    worst = 0.0
    for name, mod in layers:
        xq, wq = rec[name]
        E, M, tab, flags = mod._approx_config()
        assert tab.numpy().tolist() == T_POS.tolist()
        with torch.no_grad():
            y = mod.run_forward(xq, wq, None).cpu().numpy().astype(np.float64)
        bA, bB, bR = (np.asarray(t.reshape(-1).cpu().numpy(), np.int32) for t in
                      (mod.get_acts_fp_bias(), mod.get_weights_fp_bias(), mod.get_res_fp_bias()))
        xc, wc = xq.cpu(), wq.cpu()
        if wc.dim() == 2:
            ref, S = orc.matmul(xc.numpy(), wc.t().contiguous().numpy(), E, M, int(bA[0]), bB, int(bR[0]), T_POS,
                                int(flags), with_abs=True)
        else:
            cols = torch.nn.functional.unfold(xc, wc.shape[2:], dilation=mod.dilation, padding=mod.padding,
                                              stride=mod.stride)
            A = cols.transpose(1, 2).reshape(-1, cols.shape[1]).numpy()
            ref, S = orc.matmul(A, wc.reshape(wc.shape[0], -1).t().contiguous().numpy(), E, M, int(bA[0]), bB,
                                int(bR[0]), T_POS, int(flags), with_abs=True)
            y = y.transpose(0, 2, 3, 1).reshape(-1, y.shape[1])
        tol = gio.sum_tolerance(S.astype(np.float64))
        bad = np.abs(y - ref) > tol
        assert not bad.any(), f"{name}: {np.count_nonzero(bad)} of {y.size} outputs outside 1e-5 sum|v|"
        worst = max(worst, float(np.max(np.abs(y - ref) / np.maximum(tol, 1e-30))))
    paths = _lib.path_stats(reset=True)
    assert paths["f8mx"] == len(layers) and paths["fast"] == 0, paths  # every layer on the matrix core
    print(f"ResNet-18, T_pos: worst |y - oracle| / bar = {worst:.3g} over {len(layers)} layers")


def test_cli_writes_the_digest(tmp_path):
    from fp8_quantization_amd import imagenet as inet
    from fp8_quantization_amd.error_tables import format_error_table, table_digest
    tab = tmp_path / "t_pos.txt"
    tab.write_text("\n".join(format_error_table(torch.as_tensor(T_POS))) + "\n")
    out = tmp_path / "res.json"
    common = ["--synthetic", "8", "--arch", "resnet18", "--image-size", "32", "--batch-size", "4", "--num-workers", "0"]
    inet.main(common + ["--error-table", str(tab), "--output", str(out)])
    res = json.loads(out.read_text())
    assert res["images"] == 8 and res["error_table_digest"] == table_digest(T_POS)
    assert "error_table" not in res["approx_params"]
    inet.main(common + ["--output", str(out)])
    assert json.loads(out.read_text())["error_table_digest"] is None
