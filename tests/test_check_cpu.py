"""The fused self-check's host side (no GPU): the workspace queries, the argument validation of
fp8a_matmul_check / fp8a_conv2d_check, the fp8a_check_stats layout and CheckStats' arithmetic."""
import ctypes
import math
import re
import os

import pytest

from fp8_quantization_amd import _lib
from fp8_quantization_amd.approx_ops import (CHECK_STATS_BYTES, SELF_CHECK_LABELS, CheckStats, _CheckStatsStruct,
                                             format_self_check)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PART = 64  # bytes of one workgroup's partial (gemm_check.h CheckPart)


def _a256(x):
    return (x + 255) // 256 * 256


def test_workspace_queries_are_host_only_and_grow_with_mn():
    L = _lib.load()
    tiles = lambda M, N: ((M + 63) // 64) * ((N + 63) // 64)  # noqa: E731
    for M, N, K in ((1, 1, 1), (70, 67, 37), (130, 3, 16), (4096, 512, 4608)):
        assert L.fp8a_check_workspace_size(M, N, K) == _a256(M * N * 4) + _a256(tiles(M, N) * PART)
    assert L.fp8a_check_workspace_size(70, 67, 1) == L.fp8a_check_workspace_size(70, 67, 999)  # (no K term)
    assert L.fp8a_check_workspace_size(128, 128, 8) > L.fp8a_check_workspace_size(64, 128, 8) > \
        L.fp8a_check_workspace_size(64, 64, 8)
    assert L.fp8a_check_workspace_size(0, 4, 4) == 0 and L.fp8a_check_workspace_size(4, 4, -1) == 0
    # conv: S in y's layout + a partial per (64-row tile, 64-channel tile, group)
    Bn, Cin, H, W, Cout, g = 2, 4, 9, 9, 6, 2
    Mrows = Bn * 9 * 9
    assert L.fp8a_conv2d_check_workspace_size(Bn, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, g) == \
        _a256(Bn * Cout * 81 * 4) + _a256(tiles(Mrows, Cout // g) * g * PART)
    assert L.fp8a_conv2d_check_workspace_size(Bn, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, 4) == 0  # 6 % 4
    assert L.fp8a_conv2d_check_workspace_size(Bn, Cin, 2, 2, Cout, 5, 5, 1, 1, 0, 0, 1, 1, 1) == 0  # empty output


def _matmul_check(L, A=1, B=1, C=1, M=3, N=4, K=5, lda=5, ldc=4, E=4, Mw=3, bias=1, stats=8, ws=256, wsb=1 << 20,
                  flags=0):
    """Dummy non-null pointers: every case here must be rejected before anything dereferences them."""
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return L.fp8a_matmul_check(p(A), lda, p(B), 1, 1, p(C), ldc, M, N, K, E, Mw, p(bias), p(bias), 0, p(bias), None,
                               flags, None, None, p(stats), p(ws), wsb, None)


@pytest.mark.parametrize("kw", [dict(A=0), dict(B=0), dict(C=0), dict(bias=0), dict(stats=0), dict(ws=0),
                                dict(M=0), dict(N=-1), dict(K=0), dict(lda=4), dict(ldc=3), dict(wsb=16),
                                dict(ws=264), dict(flags=_lib.V5)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_matmul_check_rejects_bad_arguments(kw):
    rc = _matmul_check(_lib.load(), **kw)
    with pytest.raises(AssertionError):
        _lib.check(rc, "fp8a_matmul_check")


def test_matmul_check_bad_format_is_value_error():
    rc = _matmul_check(_lib.load(), E=0)
    with pytest.raises(ValueError):
        _lib.check(rc, "fp8a_matmul_check")


def _conv_check(L, x=1, w=1, y=1, Bn=2, Cin=4, H=9, W=9, Cout=6, k=3, s=1, groups=2, E=4, stats=8, ws=256,
                wsb=1 << 20):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return L.fp8a_conv2d_check(p(x), p(w), p(y), Bn, Cin, H, W, Cout, k, k, s, s, 1, 1, 1, 1, groups, E, 3, p(1), p(1),
                               p(1), None, 0, None, None, p(stats), p(ws), wsb, None)


@pytest.mark.parametrize("kw", [dict(x=0), dict(w=0), dict(y=0), dict(stats=0), dict(ws=0), dict(groups=4),
                                dict(groups=0), dict(H=1, k=5), dict(s=0), dict(wsb=1024), dict(Bn=0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_conv_check_rejects_bad_arguments(kw):
    rc = _conv_check(_lib.load(), **kw)
    with pytest.raises(AssertionError):
        _lib.check(rc, "fp8a_conv2d_check")


def test_conv_check_bad_format_is_value_error():
    rc = _conv_check(_lib.load(), E=0)
    with pytest.raises(ValueError):
        _lib.check(rc, "fp8a_conv2d_check")


def test_stats_struct_layout_matches_header():
    """The ctypes mirror has the offsets include/fp8approx.h documents."""
    src = open(os.path.join(ROOT, "include", "fp8approx.h")).read()
    doc = dict((name, int(off)) for off, name in re.findall(r"^ \*\s+(?:offset\s+)?(\d+)\s+([a-z_0-9]+)\s", src, re.M)
               if name in CheckStats.FIELDS)
    assert set(doc) == set(CheckStats.FIELDS)
    for name in CheckStats.FIELDS:
        assert getattr(_CheckStatsStruct, name).offset == doc[name], name
    assert CHECK_STATS_BYTES == 96


def test_check_stats_arithmetic():
    st = _CheckStatsStruct(n_out=8, sum_err=2.0, sum_err2=0.5, sum_gold2=50.0, a_norm=3, a_total=12, b_norm=5,
                           b_total=20, r_norm=7, r_total=28, max_err=0.75, prod_max_abs=1e-7, prod_max_rel=2e-8,
                           has_prod=1)
    s = CheckStats.from_bytes(bytes(st))
    assert (s.n_out, s.a_norm, s.a_total, s.b_norm, s.b_total, s.r_norm, s.r_total, s.has_prod) == \
        (8, 3, 12, 5, 20, 7, 28, 1)
    assert s.max == s.max_err == 0.75
    assert s.mean == 0.25
    assert s.rmse == 0.25
    assert s.sqnr_db == pytest.approx(20.0, abs=1e-12)
    assert (s.a_norm_pct, s.b_norm_pct, s.r_norm_pct) == (25.0, 25.0, 25.0)
    assert s.raw == bytes(st)
    # s2n: the reference has no R_3d mask; an exact product has an infinite SQNR
    z = CheckStats(n_out=4, sum_gold2=3.0, a_norm=1, a_total=2, b_norm=1, b_total=2)
    assert z.r_norm_pct is None and z.sqnr_db == math.inf and z.mean == 0.0 and z.rmse == 0.0
    with pytest.raises(TypeError):
        CheckStats(bogus=1)


def test_printed_block_has_the_reference_labels():
    s = CheckStats(n_out=8, sum_err=2.0, sum_err2=0.5, a_norm=3, a_total=12, b_norm=5, b_total=20, r_norm=7,
                   r_total=28, max_err=0.75)
    no_s2n = format_self_check(s, _lib.APPROX | _lib.QBMA).split("\n")
    assert no_s2n[0] == ""
    assert [ln[:len(lab)] for ln, lab in zip(no_s2n[1:], SELF_CHECK_LABELS)] == list(SELF_CHECK_LABELS)
    assert len(no_s2n) == 1 + len(SELF_CHECK_LABELS)
    assert "Normal Values in A_2d : 3/12 = 25.0%" in no_s2n and "With Approximation    = True" in no_s2n
    assert "With S2N & N2S Opt    = False" in no_s2n and "MatMul Mean Error     : 0.25" in no_s2n
    s2n = format_self_check(s, _lib.APPROX | _lib.QBMA | _lib.S2N)
    assert "R_3d" not in s2n and "With S2N & N2S Opt    = True" in s2n
