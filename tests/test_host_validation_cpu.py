"""Host-side argument validation and the option table of libfp8approx.so, without a GPU: every call here
is rejected (or answered) before the library touches a device.  The return codes and fp8a_last_error()
texts are the library's contract with approx_ops.py (EINVAL -> AssertionError, EFORMAT -> ValueError);
the option triples pin each option's default and its normalisation in fp8a_set_option."""
import ctypes
import os

import pytest

from fp8_quantization_amd import _lib

FL = _lib.APPROX | _lib.S2N | _lib.QBMA
BASE = dict(Bn=2, Cin=4, H=8, W=8, Cout=4, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, groups=1)
PTR = ctypes.c_void_p(4096)  # a non-null, aligned pointer value the host side never dereferences


def geo(**kw):
    d = dict(BASE, **kw)
    return [d[k] for k in ("Bn", "Cin", "H", "W", "Cout", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")], d["groups"]


def err(rc):
    return rc, _lib.load().fp8a_last_error().decode()


def conv2d(E=4, Mw=3, **kw):
    g, groups = geo(**kw)
    return err(_lib.load().fp8a_conv2d(None, None, None, *g, groups, E, Mw, None, None, None, None, FL, None, 0, None))


def quantizers(in_q, out_q):
    """(maxval, nbits, mbits, sign_bits, bias_out, ibias_out) of the input quantizer, the null block tail,
    then the same six of the output quantizer."""
    return [*in_q, None, 0, 0.0, 0.0, *out_q]


NOQ = (None, 8, 3, 1, None, None)


def block(name, bA=PTR, post_act=0, in_q=NOQ, out_q=NOQ, in_image=None):
    L = _lib.load()
    g, groups = geo()
    args = [None, None, None, *g, groups, 4, 3, bA, None, None, None, FL, None, 0, 0.0, 0.0]
    args += quantizers(in_q, out_q)
    args[-9] = post_act
    if name == "fp8a_conv2d_chain":
        args += [in_image, None, 0, 0, None, 8, 3, 1, None, 3, 0]
    return err(getattr(L, name)(*args, None, 0, None))


def test_conv2d_validation_order():
    assert conv2d(E=0) == (_lib.EFORMAT, "Invalid combination of expo_width and mant_width")
    assert conv2d(groups=3) == (_lib.EINVAL, "bad groups")
    assert conv2d(H=1, W=1, ph=0, pw=0) == (_lib.EINVAL, "empty convolution output")
    assert conv2d() == (_lib.EINVAL, "conv2d workspace too small")


def test_conv2d_qin_null_maxval():
    g, groups = geo()
    rc = _lib.load().fp8a_conv2d_qin(None, None, None, *g, groups, 4, 3, None, None, None, FL, None, 0, 0.0, 0.0,
                                     None, 8, 3, 1, None, None, None, 0, None)
    assert err(rc) == (_lib.EINVAL, "null pointer")


@pytest.mark.parametrize("name,prefix", [("fp8a_conv2d_block", "conv2d_block"), ("fp8a_conv2d_chain", "conv2d_chain")])
def test_block_and_chain_validation(name, prefix):
    assert block(name, post_act=2) == (_lib.EINVAL, prefix + ": post_act is 0 or 1")
    assert block(name, bA=None) == (_lib.EINVAL, "null pointer")  # no input quantizer and no bA
    bad = (PTR, 8, 0, 1, PTR, PTR)  # mbits = 0
    assert block(name, in_q=bad) == (_lib.EFORMAT, "bad FP8 quantizer format")
    assert block(name, out_q=bad) == (_lib.EFORMAT, "bad FP8 quantizer format")
    assert block(name) == (_lib.EINVAL, prefix + " workspace too small")


def test_chain_misaligned_image():
    assert block("fp8a_conv2d_chain", in_image=ctypes.c_void_p(4096 + 8)) == (
        _lib.EINVAL, "word images must be 256-byte aligned")


def test_matmul_block_leading_dimension():
    rc = _lib.load().fp8a_matmul_block(None, 3, None, 1, 1, None, 4, 2, 4, 5, 4, 3, None, None, 0, None, None, FL, None,
                                       0, 0.0, 0.0, *quantizers(NOQ, NOQ), None, 0, None)
    assert err(rc) == (_lib.EINVAL, "leading dimension smaller than extent")


# (name, default, value read back after setting -5, after setting 70000)
OPTIONS = [("xm_ncg", 0, -5, 70000)] + \
          [(n, d, -5, 70000) for n, d in (("tt_band", 1), ("tbx_rw", 2), ("tbs", 2), ("dn_direct", 1), ("v5ds", 1),
                                          ("dw3", 2))] + \
          [(n, 1, 1, 1) for n in ("xm_sign_rows", "xm_pipe", "xm_wave_rows", "fq_fast", "mse_group")] + \
          [("splitk_fixup", 0, 1, 1), ("splitk", 0, 0, 70000), ("af32_maxct", 1, 0, 70000), ("tt16_mink", 64, 0, 70000),
           ("dw_lds", 40960, 4096, 65536), ("dw_target", 4096, 256, 70000)]


@pytest.mark.parametrize("name,default,low,high", OPTIONS)
def test_option_default_and_normalisation(name, default, low, high):
    L = _lib.load()
    prev = L.fp8a_set_option(name.encode(), -5)
    try:
        after_low = L.fp8a_set_option(name.encode(), 70000)
        after_high = L.fp8a_set_option(name.encode(), prev)
    finally:
        L.fp8a_set_option(name.encode(), prev)
    if "FP8A_" + name.upper() not in os.environ:  # (the environment sets the value at load)
        assert prev == default
    assert (after_low, after_high) == (low, high)
    assert L.fp8a_set_option(name.encode(), prev) == prev  # restored


def test_unknown_option():
    assert err(_lib.load().fp8a_set_option(b"nope", 1)) == (_lib.EINVAL, "unknown option nope")


# A kernel size, stride or dilation below 1 or a negative padding: rejected by every entry point that
# derives the output size (before: an integer division by zero in those without a check of their own).
BAD_GEOMETRY = [dict(sh=0), dict(kh=0), dict(dh=0), dict(ph=-1)]


@pytest.mark.parametrize("bad", BAD_GEOMETRY, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_bad_geometry_is_rejected(bad):
    L = _lib.load()
    want = (_lib.EINVAL, "bad convolution geometry")
    assert conv2d(**bad) == want
    g, groups = geo(**bad)
    assert err(L.fp8a_im2col(None, None, *g[:4], *g[5:], None)) == want
    assert err(L.fp8a_conv2d_qamaa(None, None, None, *g, groups, None, 8, 3, 1, None)) == want
    assert L.fp8a_conv2d_workspace_size(*g, groups) == 0
    assert L.fp8a_conv2d_check_workspace_size(*g, groups) == 0
    assert L.fp8a_dense_conv2d_workspace_size(*g) == 0
