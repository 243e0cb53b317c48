"""The fast fake quantizer and the direct A word (option "fq_fast") against the literal
forms, exhaustively: fp8a_fq_selfcheck runs both on the device over EVERY fp32 bit pattern (2^32, in
four slices) and compares the results as bits -- NaN payloads, infinities, float subnormals, both
zeros, ties and grid points are all among the patterns.

  * fq_apply_fast against fq_apply_lit: the four formats x sign_bits 0 / 1 x maxval 3.7, 0.013, 911,
    448, 2^-120, 1e30.  The last two lie outside the guard (fq_fast_ok) and must take the literal
    form through it -- the entry reports which form ran -- and still match.
  * the word formed from the quantized value's bits against xm_word_a(fq_apply_lit(..)), its ok bit
    included, for M = 3 and M = 2: result biases that put the quantizer's whole exponent range inside
    the window and the scale range (no per-element test: the hoisted decision itself is what is
    checked) and outside them (per-element test), maxvals whose grid leaves the exactness window on
    either side, and the per-element test forced on.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMATS = [(4, 3), (5, 2), (3, 4), (2, 5)]
MAXVALS = [3.7, 0.013, 911.0, 448.0, 2.0 ** -120, 1e30]
SLICE = 1 << 30


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()


def _sweep(mx, E, M, sign_bits, mode=0, bR=0):
    from fp8_quantization_amd import _lib
    bad, first, fast, per = 0, None, set(), set()
    for s in range(4):
        r = _lib.fq_selfcheck(mx, E, M, sign_bits, mode=mode, bR=bR, first=s * SLICE, count=SLICE)
        bad += r["mismatches"]
        if first is None:
            first = r["first_bad"]
        fast.add(r["fast"])
        per.add(r["per_element"])
    assert len(fast) == 1 and len(per) == 1
    return bad, first, fast.pop(), per.pop()


@pytest.mark.parametrize("mx", MAXVALS)
@pytest.mark.parametrize("sign_bits", [0, 1])
@pytest.mark.parametrize("E,M", FORMATS)
def test_fast_quantizer_matches_literal_on_every_float(E, M, sign_bits, mx):
    bad, first, fast, _ = _sweep(mx, E, M, sign_bits)
    print(f"E{E}M{M} sign_bits={sign_bits} maxval={mx!r}: mismatches={bad} first_bad={first} fast={fast}")
    assert fast == (mx not in (2.0 ** -120, 1e30)), "the guard chose the other form"
    assert bad == 0, f"first mismatching pattern 0x{first:08x}"


# (maxval, bR, the window test runs per element): E4M3 maxval 3.7 has bias 14, E5M2 bias 30
WORD_CASES = [(3.7, 14, False), (3.7, 9, False), (0.013, 20, False), (911.0, 6, False), (448.0, 8, False),
              (911.0, 140, True),    # scale exponent below 1 at the top of the grid
              (0.013, -110, True),    # ... above 252 at its bottom
              (2.0 ** 60, 0, True),   # grid values above the window's 2^50
              (2.0 ** -70, 100, True),  # ... below its 2^-62
              (2.0 ** -120, 14, None), (1e30, 14, None)]  # outside the guard: the literal forms


@pytest.mark.parametrize("mx,bR,per_element", WORD_CASES)
@pytest.mark.parametrize("sign_bits", [0, 1])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_direct_word_matches_xm_word_a_on_every_float(E, M, sign_bits, mx, bR, per_element):
    bad, first, fast, per = _sweep(mx, E, M, sign_bits, mode=1, bR=bR)
    print(f"E{E}M{M} sign_bits={sign_bits} maxval={mx!r} bR={bR}: mismatches={bad} first_bad={first} fast={fast} "
          f"per_element={per}")
    assert fast == (per_element is not None)
    if per_element is not None:
        assert per == per_element, "the hoisted window decision is not the expected one"
    assert bad == 0, f"first mismatching pattern 0x{first:08x}"


@pytest.mark.parametrize("mx,bR", [(3.7, 14), (911.0, 6)])
@pytest.mark.parametrize("E,M", [(4, 3), (5, 2)])
def test_per_element_window_test_agrees_inside_the_window(E, M, mx, bR):
    bad, first, fast, per = _sweep(mx, E, M, 1, mode=2, bR=bR)
    assert fast and per
    assert bad == 0, f"first mismatching pattern 0x{first:08x}"
