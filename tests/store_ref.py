"""The fused store on the CPU: what a launch writes from its fp32 accumulator on.  numpy only; no
import from the library under test.

From the accumulator on, a launch's store is a fixed chain of fp32 operations (csrc/fp8approx_common.h):

    epi         v = fmaf(acc, scale[c], shift[c]); fminf(fmaxf(v, lo), hi) when the activation is set
    post1/4     v += res[o]                                   (one fp32 add)
    post_tail   the post clamp, then the block's output quantizer fq_apply
    emit_word   the next convolution's A word of fq_next(v), into its zero-bordered word image; the header
                words [0] invalid, [5] scale-exponent extreme, [6] "a negative word was written"

Every function here restates one of these steps from the comments that define it, in float64 or on the fp32 bit
pattern, where each step is exact; tests/test_store_ref_cpu.py checks them against exact rationals, the oracle and
the committed reference outputs.  With an accumulator that is known by bits (tests/exact_sums.py) the stored value,
the emitted word and the header follow by bits, and the GPU comparison needs no tolerance.

Out of scope: the GELU tail (post_act 2) calls the device's erff and has no bit-exact CPU twin -- its tests stay in
tests/test_gpu_linear_block.py on their tolerance; word form 2 (the v5 words, v5_word_a) has no written layout in
the kernel comments beyond "the v5 matrix-core form's words" and is left out.

Zeros.  compare() states the rule of every comparison with a kernel:
  * by value (a zero of either sign equals a zero: pairs_cases.same_bits / exact_sums.assert_same) wherever the sign
    of a zero depends on an accumulator's zero (a sum of products with zero operands), on fmaxf / fminf of two zeros
    (IEEE leaves that sign open) or on the clamp of a zero;
  * by bits where the kernel comments define the sign: fq_apply_fast "copies xc's sign bit onto q", as the literal
    form's rint(-0.3) = -0.0 does -- a NEGATIVE NONZERO value that a signed quantizer rounds to zero is stored as
    -0.0.  fake_quant() returns that -0.0 and signed_zero() marks those elements.
"""
import numpy as np

F32, F64, U32, I64 = np.float32, np.float64, np.uint32, np.int64
XM_ZERO_WORD = 253 << 23      # fp8approx_common.h: A = 0 as a matrix-core word
XM_SIGN_BIT = 0x40            # word bit 6: the tile-table row of s_a = 1
HEADER_WORDS = 64             # the image's 256-byte header


# ------------------------------------------------------------------------------------------ fma
def fma32(x, s, t):
    """The correctly rounded float32 of x * s + t (all float32): __fmaf_rn.

    float64(x) * float64(s) is exact (48 bits).  The float64 sum with t is formed by TwoSum (sum + err exactly);
    where err != 0 the sum is rounded to odd -- of the two float64 neighbours of the exact value the one with an odd
    last bit -- and a round-to-odd value of 53 bits rounds to float32's 24 (to nearest even) like the exact value."""
    x, s, t = (np.asarray(v, F32).astype(F64) for v in (x, s, t))
    p = x * s
    with np.errstate(over="ignore", invalid="ignore"):
        sm = p + t
        bb = sm - p
        err = (p - (sm - bb)) + (t - bb)
        even = (np.asarray(sm).reshape(-1).view(I64).reshape(np.shape(sm)) & 1) == 0
        adj = (err != 0) & even & np.isfinite(sm)
        toward = np.where(err > 0, np.inf, -np.inf)
        sm = np.where(adj, np.nextafter(sm, toward), sm)
        return sm.astype(F32)


def mul_add32(x, s, t):
    """x * s rounded to float32, then + t rounded again: what a store without the fused multiply-add would give."""
    x, s, t = (np.asarray(v, F32) for v in (x, s, t))
    return ((x * s).astype(F32) + t).astype(F32)


def _clamp32(v, lo, hi):
    """fminf(fmaxf(v, lo), hi) on float32 values (no NaN among them)."""
    return np.minimum(np.maximum(np.asarray(v, F32), F32(lo)), F32(hi)).astype(F32)


def bn_act(acc, scale_shift, act, lo, hi, channel_axis):
    """epi: fma32(acc, scale[c], shift[c]) along channel_axis, then the clamp when act is set.  scale_shift [C, 2]."""
    acc = np.asarray(acc, F32)
    ss = np.asarray(scale_shift, F32)
    shape = [1] * acc.ndim
    shape[channel_axis] = ss.shape[0]
    v = fma32(acc, ss[:, 0].reshape(shape), ss[:, 1].reshape(shape))
    return _clamp32(v, lo, hi) if act else v


# ------------------------------------------------------------------------------------------ the quantizer
def fq_bias(maxval, n_bits, M, sign_bits):
    """fq_bias: rint(2^E - log2(maxval) + log2(2 - 2^-M) - 1), E = n_bits - sign_bits - M.  Evaluated in float64;
    the float32 chain of the kernel gives the same integer unless the unrounded value is within 1e-3 of a half,
    which this refuses (a condition on maxval, not on any kernel)."""
    E = n_bits - sign_bits - M
    raw = float(2 ** E) - np.log2(float(F32(maxval))) + np.log2(2.0 - 2.0 ** -M) - 1.0
    if abs(raw - np.floor(raw) - 0.5) < 1e-3:
        raise ValueError(f"maxval {maxval}: the quantizer bias {raw} is too close to a rounding tie")
    return float(np.rint(raw))


def fake_quant(v, maxval, n_bits, M, sign_bits):
    """quantize_to_fp8_ste_MM's forward as fq_apply states it: xc = clamp(v) to [-maxval or 0, maxval],
    ls = max(floor(log2 |xc|) + bias, 1) (1 for xc = 0), k = ls - M - bias, q = rint(xc / 2^k) 2^k -- every step
    exact in float64.  Returns (q float32, the float bias).  A negative xc that rounds to zero gives -0.0."""
    v = np.asarray(v, F32)
    mx = F32(maxval)
    bias = fq_bias(mx, n_bits, M, sign_bits)
    lo = -mx if sign_bits else F32(0.0)
    xc = np.minimum(np.maximum(v, lo), mx).astype(F64)
    _, e = np.frexp(xc)                                   # |xc| = m 2^e, m in [0.5, 1): floor(log2 |xc|) = e - 1
    ls = np.where(xc == 0, 1.0, np.maximum(e - 1 + bias, 1.0))
    k = (ls - M - bias).astype(np.int32)
    q = np.ldexp(np.rint(np.ldexp(xc, -k)), k)
    return q.astype(F32), F32(bias)


def signed_zero(v, maxval, n_bits, M, sign_bits):
    """Where fake_quant's zero carries a defined sign: a negative nonzero value under a signed quantizer."""
    q, _ = fake_quant(v, maxval, n_bits, M, sign_bits)
    return (q == 0) & (np.asarray(v, F32) < 0) & bool(sign_bits)


def tail(v, res, post_act, lo, hi, post_fq):
    """post1 / post_tail: v + res as one float32 add, the clamp (post_act 1), then fake_quant(*post_fq)
    (post_fq = (maxval, n_bits, M, sign_bits) or None).  Returns (value, the quantizer's float bias or None).
    GELU (post_act 2) is out of scope: it calls the device erff and has no bit-exact CPU twin."""
    if post_act not in (0, 1):
        raise ValueError("store_ref.tail models post_act 0 and 1 only (GELU has no bit-exact CPU twin)")
    v = np.asarray(v, F32)
    if res is not None:
        v = (v + np.asarray(res, F32)).astype(F32)
    if post_act == 1:
        v = _clamp32(v, lo, hi)
    if post_fq is None:
        return v, None
    return fake_quant(v, *post_fq)


# ------------------------------------------------------------------------------------------ words
def xbias(Mw):
    """xm_xbias: the OCP format's bias, 7 for e4m3 words (Mw 3), 15 for e5m2 (Mw 2)."""
    return 15 if Mw == 2 else 7


def words(y_final, next_fq, bR_next, Mw, form):
    """The emitted words of fake_quant(y_final, *next_fq), by the layouts the kernel comments give.

    form 0 (xm_word_a / XM_ZERO_WORD, gemm_f8mx.h): bits 23-30 the scale exponent se = 254 + xbias - bR - (exponent
    field of q), bits 3-6 the row 8 s + m (s the sign, m the top Mw mantissa bits); a zero of either sign is
    253 << 23.  ok = q on the (Mw, min normal 2^(1 - bias)) grid, |q| in [2^-62, 2^50] and 1 <= se <= 252; se is
    clamped to that range in the word.
    form 1 (emit_word's tbx_decode_a form): q's sign and exponent bits | m << 3; a zero is 0.  ok = q has no
    mantissa bit below the top Mw and lies in the window.

    Returns (words uint32, ok bool, header) with header = {0: any word not ok, 5: max(255 - se) over the nonzero
    words (0 if none), 6: whether any word carries bit 6}.  Header words 5 and 6 are defined for form 0 only."""
    q, fb = fake_quant(y_final, *next_fq)
    u = q.view(U32).astype(I64)
    ua = u & 0x7FFFFFFF
    sign = u >> 31
    field = ua >> 23
    m = (ua >> (23 - Mw)) & ((1 << Mw) - 1)
    win = (ua == 0) | ((ua >= 0x20800000) & (ua <= 0x58800000))
    if form == 1:
        ok = (ua == 0) | (((ua & ((1 << (23 - Mw)) - 1)) == 0) & win)
        w = np.where(ua == 0, 0, (u & 0xFF800000) | (m << 3))
        return w.astype(U32), ok, {0: int(not ok.all())}
    if form != 0:
        raise ValueError("store_ref.words models forms 0 and 1 (form 2, the v5 words, has no written layout)")
    emn = (128 - int(fb)) << 23                           # bits of 2^(1 - bias): the grid's smallest normal
    sub = ua < emn
    sh = (23 - Mw) + np.where(sub, (emn - (ua & 0x7F800000)) >> 23, 0)
    grid = np.where(sh < 24, (ua & ((1 << np.minimum(sh, 23)) - 1)) == 0, ua == 0)
    se = 254 + xbias(Mw) - int(bR_next) - field
    ok = np.where(ua == 0, True, grid & win & (se >= 1) & (se <= 252))
    w = np.where(ua == 0, XM_ZERO_WORD, (np.clip(se, 1, 252) << 23) | ((sign * 8 + m) << 3))
    nz = ua != 0
    sehi = int((255 - (w[nz] >> 23)).max()) if nz.any() else 0
    return w.astype(U32), ok.astype(bool), {0: int(not ok.all()), 5: sehi, 6: int(bool((w & XM_SIGN_BIT).any()))}


def decode_words(w, bR_next, Mw, form):
    """The value a word stands for (the round trip of words()): form 0 sign (1 + m / 2^Mw) 2^(field - 127) with
    field = 254 + xbias - bR - se; form 1 the same from the word's own sign and exponent bits."""
    w = np.asarray(w, U32).astype(I64)
    m = (w >> 3) & ((1 << Mw) - 1)
    if form == 1:
        field = (w >> 23) & 0xFF
        sign = np.where(w >> 31, -1.0, 1.0)
        zero = w == 0
    else:
        field = 254 + xbias(Mw) - int(bR_next) - (w >> 23)
        sign = np.where(w & XM_SIGN_BIT, -1.0, 1.0)
        zero = w == XM_ZERO_WORD
    v = sign * np.ldexp(1.0 + m / 2.0 ** Mw, (field - 127).astype(np.int32))
    return np.where(zero, 0.0, v).astype(F32)


# ------------------------------------------------------------------------------------------ the image
def image(Bn, C, H, W, ph, pw):
    """The layout comment of csrc/fp8approx.hip (word_image): a 256-byte header (64 words), then
    [Bn][C][H + 2 ph][W'] words rounded up to 256 bytes; every plane sits inside a zero border, ph rows above and
    below, pw columns on the left -- widened to 4 when 0 < pw <= 4 and W % 4 == 0, with the row length
    (W + 4 + pw) rounded up to a multiple of 4 -- else W' = W + 2 pw.  Returns dict(words = all words of the image,
    header included; index = the word index [Bn, C, H, W] of every element of the plane)."""
    if 0 < pw <= 4 and W % 4 == 0:
        left, Wp = 4, (W + 4 + pw + 3) // 4 * 4
    else:
        left, Wp = pw, W + 2 * pw
    Hp = H + 2 * ph
    body = Bn * C * Hp * Wp
    total = HEADER_WORDS + (body * 4 + 255) // 256 * 64
    b, c, h, w = np.meshgrid(np.arange(Bn), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    index = HEADER_WORDS + ((b * C + c) * Hp + h + ph) * Wp + w + left
    return dict(words=total, index=index, Hp=Hp, Wp=Wp, left=left)


# ------------------------------------------------------------------------------------------ comparison
def compare(got, want, defined_zero_sign=None):
    """Boolean array: got equals want by bits, zeros by value -- and, where defined_zero_sign marks an element, by
    bits also for the zero (the module docstring's rule)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    gb, wb = got.view(U32), want.view(U32)
    same = (gb == wb) | ((got == 0) & (want == 0))
    if defined_zero_sign is not None:
        same &= ~defined_zero_sign | (gb == wb)
    return same
