"""Custom error tables on the host: the loader and its notation, the table of a
multiplier function, the digest, and the operator plumbing of custom_approx_params["error_table"]."""
import hashlib

import numpy as np
import pytest
import torch

from fp8_quantization_amd import error_tables as et
from fp8_quantization_amd.error_tables import (format_error_table, get_error_table_NN, load_error_table,
                                               table_digest, table_from_multiplier)

T_POS = [[(ma + 2 * mb + 3) % 4 for mb in range(8)] for ma in range(8)]   # E4M3, entries 0..3
T_SGN = [[v - 1 for v in row] for row in T_POS]                           # E4M3, negative entries
T_E5 = [[(ma + mb + 2) % 3 for mb in range(4)] for ma in range(4)]        # E5M2


def _params(E=4, M=3, **extra):
    p = dict(expo_width=E, mant_width=M, dnsmp_factor=3, withComp=False, with_approx=True, with_s2nn2s_opt=True,
             sim_hw_add_OFUF=False, with_OF_opt=False, with_UF_opt=False, golden_clip_OF=False,
             quant_btw_mult_accu=True, debug_mode=False, self_check_mode=False)
    p.update(extra)
    return p


def _qparams(E=4, M=3, **extra):
    from fp8_quantization_amd.quantization import FPQuantizer, RangeEstimators
    return dict(method=FPQuantizer, act_method=FPQuantizer, n_bits=8, per_channel_weights=True,
                weight_range_method=RangeEstimators.current_minmax.cls,
                act_range_method=RangeEstimators.allminmax.cls, quantize_input=True,
                fp8_kwargs=dict(maxval=None, mantissa_bits=M, set_maxval=True),
                custom_approx_params=_params(E, M, **extra),
                run_method=dict(approx_flag=True, quantize_after_mult_and_add=False, res_quantizer_flag=True,
                                original_quantize_res=False))


# ------------------------------------------------------------------------------------ loader
@pytest.mark.parametrize("tab,M", [(T_POS, 3), (T_SGN, 3), (T_E5, 2)])
def test_loader_round_trips(tab, M, tmp_path):
    ref = torch.tensor(tab, dtype=torch.int32)
    t = load_error_table(tab, M)                                  # nested list
    assert t.dtype == torch.int32 and t.device.type == "cpu" and t.is_contiguous() and t.shape == (2 ** M, 2 ** M)
    assert torch.equal(t, ref)
    np.save(tmp_path / "t.npy", np.asarray(tab, dtype=np.int64))  # .npy
    assert torch.equal(load_error_table(str(tmp_path / "t.npy"), M), ref)
    rows = format_error_table(t)                                  # text notation
    assert len(rows) == 2 ** M and all(len(r) == 2 ** M and set(r) <= set(".-0123456789") for r in rows)
    (tmp_path / "t.txt").write_text("# a comment\n" + "\n".join(rows) + "\n\n")
    assert torch.equal(load_error_table(tmp_path / "t.txt", M), ref)
    assert torch.equal(load_error_table(np.asarray(tab, dtype=np.int8), M), ref)            # ndarray
    assert torch.equal(load_error_table(torch.tensor(tab, dtype=torch.int64).t().t(), M), ref)  # int tensor
    assert torch.equal(load_error_table(np.asarray(tab, dtype=np.float32), M), ref)         # whole-number floats


def test_format_is_the_modules_own_notation():
    for key, rows in et._TABLES.items():
        t = et.table(*key)
        assert tuple(format_error_table(t)) == rows
    assert format_error_table(load_error_table(T_SGN, 3))[0] == "2.2.2.2."
    assert format_error_table(load_error_table(T_SGN, 3))[1] == "-1-1-1-1"
    with pytest.raises(ValueError, match=r"\[0\]\[1\]"):
        format_error_table(torch.tensor([[0, 10], [0, 0]]))


def test_loader_errors_name_the_entry(tmp_path):
    with pytest.raises(ValueError, match=r"shape \(4, 4\).*\(8, 8\)"):
        load_error_table(T_E5, 3)
    with pytest.raises(ValueError, match="shape"):
        load_error_table([0] * 64, 3)
    frac = np.zeros((8, 8))
    frac[2, 5] = 0.5
    with pytest.raises(ValueError, match=r"\[2\]\[5\].*0\.5.*not an integer"):
        load_error_table(frac, 3)
    with pytest.raises(ValueError, match="integers"):
        load_error_table([["a"] * 8] * 8, 3)
    big = np.zeros((8, 8), dtype=np.int64)
    big[7, 1] = 128
    with pytest.raises(ValueError, match=r"\[7\]\[1\] = 128.*int8"):
        load_error_table(big, 3)
    big[7, 1] = -129
    with pytest.raises(ValueError, match=r"\[7\]\[1\] = -129.*int8"):
        load_error_table(torch.from_numpy(big), 3)
    big[7, 1] = -128  # the range's ends are accepted
    big[0, 0] = 127
    assert load_error_table(big, 3)[7, 1] == -128
    (tmp_path / "bad.txt").write_text("....\n..x.\n....\n....\n")
    with pytest.raises(ValueError, match=r"line 2, column 3.*'x'"):
        load_error_table(tmp_path / "bad.txt", 2)
    (tmp_path / "ragged.txt").write_text("....\n...\n....\n....\n")
    with pytest.raises(ValueError, match="row 1 has 3 entries"):
        load_error_table(tmp_path / "ragged.txt", 2)


def test_digest_is_sha256_of_int8_bytes():
    t = load_error_table(T_SGN, 3)
    want = hashlib.sha256(np.asarray(T_SGN, dtype=np.int8).tobytes()).hexdigest()
    assert table_digest(t) == want == table_digest(np.asarray(T_SGN)) and len(want) == 64
    assert table_digest(load_error_table(T_POS, 3)) != want


# ------------------------------------------------------------------------------------ multiplier
def test_exact_multiplier_gives_zero_table():
    for M in (2, 3, 4, 5):
        n = 2 ** M
        t = table_from_multiplier(lambda ma, mb, n=n: (n + ma) * (n + mb), M)
        assert t.shape == (n, n) and not t.any()


def test_truncating_multiplier():
    """A multiplier whose cross-term adder is M bits wide: of (8 + ma)(8 + mb) = 64 + 8 (ma + mb) + ma mb
    it keeps only the low 3 bits of ma mb and drops the rest, 8 floor(ma mb / 8) units of 2^-6 -- whole
    units of 2^-3, so the entry is floor(ma mb / 8); the table below is written out by hand."""
    trunc = lambda ma, mb: 64 + 8 * (ma + mb) + (ma * mb) % 8  # noqa: E731
    hand = [[0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 1, 1, 1, 1],
            [0, 0, 0, 1, 1, 1, 2, 2],
            [0, 0, 1, 1, 2, 2, 3, 3],
            [0, 0, 1, 1, 2, 3, 3, 4],
            [0, 0, 1, 2, 3, 3, 4, 5],
            [0, 0, 1, 2, 3, 4, 5, 6]]
    assert table_from_multiplier(trunc, 3).tolist() == hand
    # a multiplier that drops the product's low 3 bits instead: (9 x 9 = 81 -> 80) the error is one unit of
    # 2^-6, not a whole number of 2^-3 units
    with pytest.raises(ValueError, match=r"multiplier\(1, 1\) = 80"):
        table_from_multiplier(lambda ma, mb: ((8 + ma) * (8 + mb)) // 8 * 8, 3)
    with pytest.raises(ValueError, match="not an integer"):
        table_from_multiplier(lambda ma, mb: (8 + ma) * (8 + mb) + 0.5, 3)


# ------------------------------------------------------------------------------------ operator plumbing
def _linear(**extra):
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    return QCustomLinearTorch(in_features=8, out_features=4, bias=False, **_qparams(**extra))


def test_approx_config_returns_the_custom_table():
    from fp8_quantization_amd import _lib
    # withComp / dnsmp_factor are not consulted: (E3M4, withComp, dnsmp 2) raises without a custom table
    tab16 = [[(a * b) % 3 for b in range(16)] for a in range(16)]
    lin = _linear(E=3, M=4, withComp=True, dnsmp_factor=2, error_table=tab16)
    E, M, table, flags = lin._approx_config()
    assert (E, M) == (3, 4) and table.tolist() == tab16 and table.dtype == torch.int32 and table.is_contiguous()
    assert flags == _lib.APPROX | _lib.S2N | _lib.QBMA
    with pytest.raises(UnboundLocalError):
        _linear(E=3, M=4, withComp=True, dnsmp_factor=2)._approx_config()
    # E5M2 without zero_table_ext
    lin5 = _linear(E=5, M=2, error_table=T_E5)
    assert lin5._approx_config()[2].tolist() == T_E5
    with pytest.raises(ValueError):
        _linear(E=5, M=2)._approx_config()
    # a wrong-shape table is the loader's ValueError
    with pytest.raises(ValueError, match="shape"):
        _linear(error_table=T_E5)._approx_config()


def test_custom_table_is_normalised_once_per_operator(monkeypatch):
    from fp8_quantization_amd import approx_calculation as ac
    calls = []
    real = ac.load_error_table
    monkeypatch.setattr(ac, "load_error_table", lambda spec, M: calls.append(1) or real(spec, M))
    lin = _linear(error_table=T_POS)
    a = lin._approx_config()[2]
    b = lin._approx_config()[2]
    assert a is b and len(calls) == 1
    lin.custom_approx_params["error_table"] = [row[:] for row in T_SGN]  # a new object: read again
    assert lin._approx_config()[2].tolist() == T_SGN and len(calls) == 2


def test_version_5_with_custom_table_raises():
    lin = _linear(error_table=T_POS, approx_version=5)
    with pytest.raises(ValueError, match="v5"):
        lin._approx_config()


def test_absent_or_none_key_is_todays_table():
    for extra in ({}, {"error_table": None}):
        t = _linear(**extra)._approx_config()[2]
        assert t is get_error_table_NN(4, 3, withComp=False, dnsmp_factor=3)
    t5 = _linear(E=5, M=2, zero_table_ext=True, error_table=None)._approx_config()[2]
    assert t5.shape == (4, 4) and not t5.any()


def test_key_passes_through_the_workloads_and_bound_classes():
    from fp8_quantization_amd import resnet_workload as rw
    from fp8_quantization_amd.approx_calculation import ApproxOpMixin, bind_operator_classes
    from fp8_quantization_amd.quantization.hijacker import QuantizationHijacker
    from fp8_quantization_amd.quantization.quantized_folded_bn import BNFusedHijacker
    spec = load_error_table(T_POS, 3)
    qp = rw.approx_qparams(error_table=spec)
    assert qp["custom_approx_params"]["error_table"] is spec
    assert "error_table" not in rw.approx_qparams()["custom_approx_params"]
    model = rw.QuantizedResNet(rw.ResNet(rw.BasicBlock, (1, 1, 1, 1)), input_size=(1, 3, 32, 32), **qp)
    ops = [m for m in model.modules() if isinstance(m, ApproxOpMixin)]
    assert len(ops) >= 10
    for m in ops:
        assert m.custom_approx_params["error_table"] is spec
        assert torch.equal(m._approx_config()[2], spec)
    _, linear, _ = bind_operator_classes(QuantizationHijacker, BNFusedHijacker)
    lin = linear(in_features=8, out_features=4, bias=False, **_qparams(error_table=T_SGN))
    assert lin._approx_config()[2].tolist() == T_SGN


def test_cli_reads_the_table_once_and_reports_the_digest(tmp_path):
    from fp8_quantization_amd import imagenet
    (tmp_path / "t.txt").write_text("\n".join(format_error_table(load_error_table(T_POS, 3))) + "\n")
    args = imagenet.parse(["--synthetic", "8", "--error-table", str(tmp_path / "t.txt")])
    cfg = imagenet.approx_cfg(args)
    assert cfg["error_table"].tolist() == T_POS
    assert "error_table" not in imagenet.approx_cfg(imagenet.parse(["--synthetic", "8"]))
