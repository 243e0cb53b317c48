"""The batched self-check's host side (no GPU): fp8a_bmm_check's surface, its workspace formula, its argument
validation -- every case with its code and text, in the order the header documents, each call wrong in that
respect and in every later one -- and error_report's ``matmul`` rows from a hand-made CheckStats."""
import ctypes
import os
import re

import pytest

from fp8_quantization_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART = 64  # bytes of one workgroup's partial (gemm_check.h CheckPart)


def _a256(x):
    return (x + 255) // 256 * 256


def test_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "fp8approx.h")).read()
    declared = set(re.findall(r"\b(fp8a_[a-z0-9_]+)\s*\(", src))
    L = _lib.load()
    for name in ("fp8a_bmm_check_workspace_size", "fp8a_bmm_check"):
        assert name in declared and name in _lib.SYMBOLS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    assert len(L.fp8a_bmm_check.argtypes) == 29  # the header's argument list
    import fp8_quantization_amd as fa
    assert callable(fa.approx_bmm_check)


def test_workspace_formula():
    L = _lib.load()
    tiles = lambda M, N: ((M + 63) // 64) * ((N + 63) // 64)  # noqa: E731
    for nb0, nb1, M, N, K in ((1, 1, 1, 1, 1), (2, 3, 70, 67, 37), (2, 12, 197, 197, 64)):
        nb = nb0 * nb1
        assert L.fp8a_bmm_check_workspace_size(nb0, nb1, M, N, K) == \
            _a256(4 * nb * M * N) + _a256(PART * nb * tiles(M, N))
    assert L.fp8a_bmm_check_workspace_size(2, 3, 70, 67, 1) == L.fp8a_bmm_check_workspace_size(2, 3, 70, 67, 999)
    for bad in ((0, 3, 4, 4, 4), (2, 0, 4, 4, 4), (2, 3, 0, 4, 4), (2, 3, 4, -1, 4), (2, 3, 4, 4, 0), (-2, -3, 4, 4, 4)):
        assert L.fp8a_bmm_check_workspace_size(*bad) == 0, bad


# Every argument wrong at once; the steps below mend them one by one, in the documented order.  Pointers are
# dummies: every call here must be rejected before anything dereferences them (the last step still fails).
ALL_WRONG = dict(E=0, nb0=0, nb1=1 << 11, M=5, N=-1, K=4, lda=2, sa0=-1, flags=_lib.TB | _lib.V5 | (1 << 20), bBs=2,
                 ptr=None, stats=None, ws=None, wsb=16)
STEPS = [
    (dict(), _lib.EFORMAT, None),
    (dict(E=4), _lib.EINVAL, "fp8a_bmm_check: negative extent"),
    (dict(N=7), _lib.EINVAL, "fp8a_bmm_check: negative stride"),
    (dict(sa0=None), _lib.EINVAL, "fp8a_bmm: no tensor-bias semantics (FP8A_TB) for a batched product"),
    (dict(flags=_lib.V5 | (1 << 20)), _lib.EINVAL, "fp8a_bmm: the v5 model is not implemented for a batched product"),
    (dict(flags=_lib.APPROX | (1 << 20)), _lib.EINVAL, "fp8a_bmm_check: unknown flag bits"),
    (dict(flags=_lib.APPROX | _lib.S2N | _lib.QBMA), _lib.EINVAL, "fp8a_bmm_check: bB_stride must be 0 or 1"),
    (dict(bBs=1), _lib.EINVAL, "leading dimension smaller than extent"),
    (dict(lda=4), _lib.EINVAL, "self-check extents must be positive"),
    (dict(nb0=1 << 20), _lib.EINVAL, "null pointer"),
    (dict(ptr=4096), _lib.EINVAL, "null pointer"),  # (stats alone)
    (dict(stats=12), _lib.EINVAL, "self-check workspace missing, misaligned or too small"),
    (dict(ws=264, wsb=1 << 62), _lib.EINVAL, "self-check workspace missing, misaligned or too small"),
    (dict(ws=256, wsb=16), _lib.EINVAL, "self-check workspace missing, misaligned or too small"),
    (dict(wsb=1 << 62), _lib.EINVAL, "stats must be 8-byte aligned"),
    (dict(stats=8), _lib.EINVAL, "self-check grid too large"),  # 2^31 items x 1 tile
]


def _call(E, nb0, nb1, M, N, K, lda, sa0, flags, bBs, ptr, stats, ws, wsb):
    L = _lib.load()
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    sa0 = nb1 * M * K if sa0 is None else sa0
    return L.fp8a_bmm_check(p(ptr), p(ptr), p(ptr), nb0, nb1, M, N, K, lda, sa0, M * K, N, 1, nb1 * K * N, K * N, E, 3,
                            p(ptr), p(ptr), bBs, p(ptr), None, flags, None, None, p(stats), p(ws), wsb, None)


@pytest.mark.parametrize("upto", range(len(STEPS)), ids=lambda i: f"step{i:02d}")
def test_validation_order(upto):
    kw = dict(ALL_WRONG)
    for fix, _, _ in STEPS[:upto + 1]:
        kw.update(fix)
    _, code, text = STEPS[upto]
    rc = _call(**kw)
    assert rc == code, (rc, _lib.load().fp8a_last_error().decode())
    if text is not None:
        assert _lib.load().fp8a_last_error().decode() == text
    with pytest.raises(ValueError if code == _lib.EFORMAT else AssertionError):
        _lib.check(rc, "fp8a_bmm_check")


@pytest.mark.parametrize("kw", [dict(nb0=-1), dict(nb1=-1), dict(M=-1), dict(K=-1), dict(nb1=0), dict(M=0), dict(N=0),
                                dict(K=0)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_every_extent_is_checked(kw):
    good = dict(ALL_WRONG)
    for fix, _, _ in STEPS:
        good.update(fix)
    good.update(nb0=2, nb1=3)
    good.update(kw)
    assert _call(**good) == _lib.EINVAL
    want = "fp8a_bmm_check: negative extent" if min(kw.values()) < 0 else "self-check extents must be positive"
    assert _lib.load().fp8a_last_error().decode() == want


def test_python_entry_rejects_bad_shapes_and_cpu_tensors():
    import torch
    from fp8_quantization_amd.approx_ops import approx_bmm_check
    A, B = torch.zeros(2, 3, 4), torch.zeros(2, 4, 5)
    with pytest.raises(AssertionError):
        approx_bmm_check(A, torch.zeros(2, 5, 5), 4, 3, 8, 8, 8)
    with pytest.raises(AssertionError):
        approx_bmm_check(A, torch.zeros(3, 4, 5), 4, 3, 8, 8, 8)
    with pytest.raises(AssertionError):
        approx_bmm_check(A[0], B[0], 4, 3, 8, 8, 8)
    with pytest.raises(RuntimeError):
        approx_bmm_check(A, B, 4, 3, 8, 8, 8)


# ------------------------------------------------------------------------------------ report
def _stub_matmul():
    from fp8_quantization_amd.approx_calculation import ApproxMatMulMixin

    class Stub(ApproxMatMulMixin):  # (no quantizers: _row reads the CheckStats alone)
        pass
    return Stub()


def test_report_row_of_a_batched_product():
    import torch
    from fp8_quantization_amd.approx_ops import CheckStats
    from fp8_quantization_amd.error_report import _row, format_report
    nb, M, N, K = 4, 17, 16, 17  # the PV orientation of 2 images x 2 heads
    st = CheckStats(S=torch.empty(2, 2, M, N), n_out=nb * M * N, sum_err=2.0, sum_err2=0.5, sum_gold2=50.0,
                    a_norm=100, a_total=nb * M * K, b_norm=544, b_total=nb * K * N, max_err=0.75, prod_max_rel=2e-6,
                    has_prod=1)
    row = _row("encoder.layer.0.attention.attention.pv_matmul", _stub_matmul(), st)
    assert row["kind"] == "matmul" and row["shape"] == (M, N, K) and row["batch"] == nb and row["groups"] == 1
    assert row["macs"] == nb * M * N * K
    assert row["prod_max_rel"] == pytest.approx(0.2) and row["max"] == 0.75 and row["r_norm_pct"] is None
    assert row["b_norm_pct"] == pytest.approx(50.0)
    # the other kinds gain no key
    lin = type("Lin", (), dict(out_features=N, in_features=K))()
    other = _row("fc", lin, CheckStats(n_out=M * N, a_total=M * K, b_total=K * N))
    assert other["kind"] == "linear" and "batch" not in other and set(row) - set(other) == {"batch"}
    lines = format_report([row, other]).split("\n")
    assert len(lines) == 4 and len(lines[2]) == len(lines[0]) == len(lines[3])
    cols = lines[2].split()
    assert cols[0].endswith("pv_matmul") and cols[1] == "matmul" and cols[2:5] == [str(M), str(N), str(K)]
    assert cols[-1] == "0.2" and cols[-2] == "-"


def test_approx_attention_needs_vit(capsys):
    from fp8_quantization_amd.error_report import build_workload, main
    with pytest.raises(SystemExit) as ex:
        main(["--arch", "resnet18", "--approx-attention"])
    assert ex.value.code == 2
    assert "--approx-attention needs --arch vit_b16" in capsys.readouterr().err
    with pytest.raises(ValueError, match="vit_b16"):
        build_workload("resnet18", 32, {}, approx_attention=True)
