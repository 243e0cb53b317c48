"""fp8a_bmm's C-ABI surface without a GPU: declared, bound and exported; host-side argument validation
answers before any launch, with the exception types fp8a_matmul's codes map to."""
import ctypes
import os
import re

import pytest

from fp8_quantization_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "fp8approx.h")).read()
    declared = set(re.findall(r"\b(fp8a_[a-z0-9_]+)\s*\(", src))
    L = _lib.load()
    for name in ("fp8a_bmm", "fp8a_bmm_stats"):
        assert name in declared and name in _lib.SYMBOLS
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value
    assert len(L.fp8a_bmm.argtypes) == 27  # the header's argument list


def test_build_lists_the_unit():
    from fp8_quantization_amd import build_native
    assert any(u[0] == "k_bmm.hip" for u in build_native.UNITS)


def _call(nb0=2, nb1=3, M=5, N=7, K=4, E=4, Mw=3, flags=_lib.APPROX | _lib.S2N | _lib.QBMA, ptr=None, bBs=0):
    """fp8a_bmm with dense strides; ptr: the value of every pointer argument (None = NULL)."""
    L = _lib.load()
    p = ctypes.c_void_p(ptr) if ptr else None
    return L.fp8a_bmm(p, p, p, nb0, nb1, M, N, K, K, nb1 * M * K, M * K, N, 1, nb1 * K * N, K * N, N, nb1 * M * N,
                      M * N, E, Mw, p, p, bBs, p, None, flags, None)


def test_negative_extents_are_einval():
    for kw in (dict(nb0=-1), dict(nb1=-1), dict(M=-1), dict(N=-1), dict(K=-1)):
        assert _call(**kw) == _lib.EINVAL, kw
        with pytest.raises(AssertionError):
            _lib.check(_call(**kw), "fp8a_bmm")


def test_null_pointer_with_a_non_empty_shape_is_einval():
    assert _call() == _lib.EINVAL
    assert "null pointer" in _lib.load().fp8a_last_error().decode()
    with pytest.raises(AssertionError):
        _lib.check(_call(), "fp8a_bmm")


def test_empty_extents_are_ok_without_pointers():
    for kw in (dict(nb0=0), dict(nb1=0), dict(M=0), dict(N=0)):
        assert _call(**kw) == _lib.OK, kw


def test_tensor_bias_and_v5_flags_are_einval():
    for fl in (_lib.TB, _lib.APPROX | _lib.TB, _lib.V5, _lib.V5 | _lib.OFUF, _lib.APPROX | _lib.OF_OPT, _lib.UF_OPT,
               1 << 20):
        assert _call(flags=fl) == _lib.EINVAL, fl
        assert _lib.load().fp8a_last_error().decode().startswith("fp8a_bmm")
        with pytest.raises(AssertionError):
            _lib.check(_call(flags=fl), "fp8a_bmm")
    assert _call(bBs=2) == _lib.EINVAL


def test_bad_format_raises_like_fp8a_matmul():
    """check_format's code, shared with fp8a_matmul: a ValueError through _lib.check."""
    L = _lib.load()
    for E, Mw in ((0, 3), (4, 0), (4, 6), (6, 3)):
        rc = _call(E=E, Mw=Mw)
        rcm = L.fp8a_matmul(None, 4, None, 1, 1, None, 4, 3, 4, 4, E, Mw, None, None, 0, None, None, 0, None, 0, None)
        assert rc != _lib.OK and rc == rcm
        with pytest.raises(ValueError):
            _lib.check(rc, "fp8a_bmm")


def test_stats_null_pointer_is_einval():
    assert _lib.load().fp8a_bmm_stats(None, 0) == _lib.EINVAL


def test_python_entry_rejects_cpu_tensors_and_bad_shapes():
    import torch
    from fp8_quantization_amd.approx_ops import approx_bmm
    A, B = torch.zeros(2, 3, 4), torch.zeros(2, 4, 5)
    with pytest.raises(RuntimeError):
        approx_bmm(A, B, 4, 3, 8, 8, 8)
    with pytest.raises(AssertionError):
        approx_bmm(A, torch.zeros(2, 5, 5), 4, 3, 8, 8, 8)
    with pytest.raises(AssertionError):
        approx_bmm(A, torch.zeros(3, 4, 5), 4, 3, 8, 8, 8)
    with pytest.raises(AssertionError):
        approx_bmm(A, B, 4, 3, 8, 8, 8, out=torch.zeros(2, 3, 6))
