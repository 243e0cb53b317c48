"""The CPU model of the fused store (tests/store_ref.py) against exact rationals, the oracle and the committed
reference outputs -- and the conditions on the store cases (tests/exact_sums.py: store_cases) that make the GPU
comparison (tests/test_gpu_store_exact.py) tell a wrong store from a right one, proved from the CPU model alone:

  * every store case sits on an exact-sum case, whose budget tests/test_exact_sums_cpu.py proves (here: membership,
    and the budget again for one base per family): its accumulator is known by bits;
  * BN: at least 10 % of the BN outputs separate fma32 from the float32 multiply-then-add, and where no quantizer
    follows at least 20 final values do (so a store that rounds twice fails the case);
  * BN on more than one channel: every pair of adjacent channels differs in the final value on at least one pixel
    (a shifted channel index fails);
  * an activation: at least 5 % of the BN outputs are clamped at each bound it has, and planted channels sit
    exactly on each bound;
  * a post clamp: it lies strictly inside the quantizer's range; at least 20 values sit exactly on each bound after
    the residual, at least 5 % are cut at each bound, and dropping the clamp changes at least 20 outputs;
  * a quantizer: at least 20 values in each planted class the case can hold (exact_sums.CLASSES_Q without those a
    preceding clamp cuts off) and more than 50 distinct outputs.

Each case prints `SC <case> fma_sep=<share on the BN output>/<on the final value> clamp=<lo>/<hi> classes=<min
count> distinct=<n>` (run with -s).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from tests import exact_sums as xs
from tests import golden_io as gio
from tests import store_ref as sr

F32 = np.float32


# ------------------------------------------------------------------------------------------ fma32
def _round_f32(fr):
    """The float32 nearest (ties to even) to an exact rational, by integer arithmetic."""
    if fr == 0:
        return F32(0.0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    e = max(e, -126)                                      # (float32's subnormals share the smallest normal's step)
    q = a / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** (e - 23)
    return F32(float(v) if fr > 0 else -float(v))         # (n <= 2^24: exact in float64)


def _exact(x, s, t):
    return [_round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in zip(x, s, t)]


def _assert_fma(x, s, t, what):
    x, s, t = (np.asarray(v, F32) for v in (x, s, t))
    got, want = sr.fma32(x, s, t), np.array(_exact(x, s, t), F32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {x.size} differ; first x={x[bad[0]]!r} s={s[bad[0]]!r} " \
                          f"t={t[bad[0]]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def test_fma32_random_triples():
    rng = np.random.default_rng(1)
    n = 6000
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(F32)
    s = (rng.standard_normal(n) * np.exp2(rng.integers(-6, 6, n))).astype(F32)
    t = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(F32)
    _assert_fma(x, s, t, "random")
    t2 = (-(x.astype(np.float64) * s) * (1 + rng.integers(-3, 4, n) * 2.0 ** -22)).astype(F32)  # cancellation
    _assert_fma(x, s, t2, "cancelling")


def test_fma32_on_float32_ties():
    """x s + t exactly halfway between two float32 values: x s = an odd multiple of 2^-24 in [1, 2) (x = 1 + k 2^-12,
    s = 1 + 2^-12 gives 24 fractional bits), t a multiple of 2^-23: the sums that stay in [1, 2) keep bit -24 set."""
    rng = np.random.default_rng(2)
    k = rng.integers(0, 1 << 11, 3000) * 2 + 1            # odd k: (1 + k 2^-12)(1 + 2^-12) has bit -24 set
    x = (1.0 + k * 2.0 ** -12).astype(F32)
    s = np.full(x.shape, 1.0 + 2.0 ** -12, F32)
    t = (rng.integers(-1 << 20, 1 << 20, x.size) * 2.0 ** -23).astype(F32)
    p = x.astype(np.float64) * s.astype(np.float64) + t
    lsb = np.round(p * 2.0 ** 24).astype(np.int64)
    tie = (np.abs(p) >= 1) & (np.abs(p) < 2) & (lsb % 2 != 0)
    assert tie.sum() > 500, tie.sum()                     # exact sums with 25 significant bits: float32 ties
    _assert_fma(x[tie], s[tie], t[tie], "ties")
    got = sr.fma32(x[tie], s[tie], t[tie])
    assert np.all((got.view(np.uint32) & 1) == 0), "a tie did not go to the even neighbour"


def test_fma32_where_the_float64_sum_is_inexact_at_a_tie():
    """The float64 sum p + t itself rounds, onto a float32 tie, while the exact sum lies just below it: a plain float64
    add and cast then goes to the even neighbour above; round-to-odd keeps the sum off the tie and the cast goes down.
    x = 2^3 (1 + a 2^-23), s = 2^3 (1 - a 2^-23): p = 2^6 (1 - a^2 2^-46), just below 2^6; t = 2^30 + 2^7, a float32
    with an odd last bit (float32's step at 2^30 is 2^7), so t + 2^6 is the tie between t and the even t + 2^7; the
    exact sum misses it by a^2 2^-40 < 2^-24, below half of float64's step 2^-22 there."""
    a = np.arange(1, 256)
    x = (2.0 ** 3 * (1 + a * 2.0 ** -23)).astype(F32)
    s = (2.0 ** 3 * (1 - a * 2.0 ** -23)).astype(F32)
    t = np.full(a.size, 2.0 ** 30 + 2.0 ** 7, F32)
    assert np.all(t.view(np.uint32) & 1 == 1)
    plain = (x.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(F32)
    assert np.all(plain == F32(2.0 ** 30 + 2.0 ** 8)), "the plain float64 sum was expected to round the wrong way"
    _assert_fma(x, s, t, "inexact float64 sum below a tie")
    assert np.all(sr.fma32(x, s, t) == t)
    _assert_fma(x, -s, -t, "the mirrored sums")


# ------------------------------------------------------------------------------------------ fake_quant
def test_fake_quant_equals_the_oracle_signed():
    rng = np.random.default_rng(4)
    v = (rng.standard_normal(200000) * np.exp2(rng.integers(-24, 6, 200000))).astype(F32)
    for (E, M, mx) in ((4, 3, 5.5), (5, 2, 3.5), (3, 4, 6.0), (4, 3, 0.37), (4, 3, 3.0), (2, 5, 1.7), (5, 2, 5.5)):
        want, wb = orc.fp8_fake_quant(v, mx, E, M)
        got, gb = sr.fake_quant(v, mx, 1 + E + M, M, 1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (E, M, mx)   # by bits, -0.0 included
        assert float(gb) == float(wb[0])
    neg = sr.fake_quant(F32(-1e-9), 3.0, 8, 3, 1)[0]
    assert neg == 0 and np.signbit(neg), "a negative value that rounds to zero keeps its sign (rint(-0.3) = -0.0)"


def test_fake_quant_equals_the_committed_reference_outputs():
    """tests/golden/ste_quant.npz: the reference quantizer's outputs y for sign_bits 0 and 1, per tensor and per
    channel (tests/golden/learn_maxval.npz records gradients only: it holds no forward output to compare)."""
    g = gio.load("ste_quant.npz")
    names = sorted({k.split("/")[0] for k in g})
    assert any("_s0_" in n for n in names) and any("_s1_" in n for n in names)
    for n in names:
        nb, mb, sb, per_channel = (int(v) for v in g[n + "/meta"])
        x, y, mx = g[n + "/x"], g[n + "/y"], g[n + "/maxval"]
        for r in range(x.shape[0]):
            got, _ = sr.fake_quant(x[r], mx[r] if per_channel else mx[0], nb, mb, sb)
            assert np.array_equal(got.view(np.uint32), y[r].view(np.uint32)), (n, r)


# ------------------------------------------------------------------------------------------ words
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("Mw,S", [(3, 1), (3, 0), (2, 1), (2, 0)])
def test_words_round_trip(Mw, S, form):
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(50000) * np.exp2(rng.integers(-24, 4, 50000))).astype(F32)
    nq, bR = (xs.NEXT_MX, 8, Mw, S), xs.NEXT_BR[Mw]
    w, ok, hdr = sr.words(v, nq, bR, Mw, form)
    q, _ = sr.fake_quant(v, *nq)
    assert ok.all() and hdr[0] == 0
    back = sr.decode_words(w, bR, Mw, form)
    assert np.array_equal(back, q) and np.count_nonzero(q) > 10000      # (zeros by value: a zero's word has no sign)
    if form == 0:
        assert np.all(w[q == 0] == sr.XM_ZERO_WORD) and np.all((w & ~np.uint32(0x7FF80078)) == 0)
        assert hdr[6] == int(S == 1) and bool((w & 0x40).any()) == (S == 1)
        assert hdr[5] == 255 - int((w[q != 0] >> 23).min())
    wi, oki, hi = sr.words(v, (2.0 ** -70, 8, Mw, S), bR, Mw, form)     # a grid below the window 2^-62
    assert hi[0] == 1 and not oki[v > 0].any()


def test_image_matches_the_size_rule():
    for (Bn, C, H, W, ph, pw) in ((2, 24, 9, 16, 0, 0), (2, 24, 9, 16, 1, 1), (2, 24, 9, 16, 0, 3), (2, 24, 9, 10, 1, 1),
                                  (1, 3, 5, 8, 2, 5), (2, 12, 7, 14, 0, 0)):
        im = sr.image(Bn, C, H, W, ph, pw)
        assert im["words"] * 4 == xs.word_image_bytes(Bn, C, H, W, ph, pw)
        idx = im["index"]
        assert idx.shape == (Bn, C, H, W) and np.unique(idx).size == idx.size and idx.min() >= sr.HEADER_WORDS
        assert idx.max() < sr.HEADER_WORDS + Bn * C * im["Hp"] * im["Wp"]
        assert np.all(np.diff(idx, axis=3) == 1) and np.all(np.diff(idx, axis=2) == im["Wp"])
        if 0 < pw <= 4 and W % 4 == 0:
            assert np.all(idx[..., 0] % 4 == 0), "the interior rows start 16-byte aligned"


# ------------------------------------------------------------------------------------------ the store cases
def _bcast(ss, col, ndim):
    return ss[:, col].reshape((1, -1) + (1,) * (ndim - 2))


def _groups():
    out = {}
    for c in xs.store_cases():
        out.setdefault(c["base"], []).append(c)
    return out


GROUPS = _groups()


def test_every_store_case_is_an_exact_sum_case():
    """Each base is a case of exact_sums.CASES, whose budget (max sum |T| <= 2^22 u)
    tests/test_exact_sums_cpu.py::test_budget_oracle_and_shares proves for every case; here only membership is checked
    for all, and the budget once more for one base per (kind, family).  A forced split along K leaves the accumulator
    proved: under the budget the sum does not depend on its order."""
    seen = set()
    for c in xs.store_cases():
        b = xs.CASES[c["base"]]
        assert b["kind"] in ("mat", "conv", "tbdw"), b["kind"]
        if (b["kind"], b["fam"]) not in seen:
            seen.add((b["kind"], b["fam"]))
            assert xs.case_budget_log2(xs.problem_of(b["pkey"])) <= xs.BUDGET_LOG2, c["base"]
    sites = {c["site"] for c in xs.store_cases()}
    assert {"f8mx", "tt", "tt16", "fast", "v5mx", "v5fast", "exact+f8mx", "exact+tt", "exact+fast", "splitk-f8mx",
            "splitk-f8mx-fixup", "splitk-tt", "splitk-fast", "tbx", "tb_fast", "tb_direct", "v5dw", "tbx-emit"} <= sites


@pytest.mark.parametrize("base", list(GROUPS), ids=list(GROUPS))
def test_store_case_conditions(base):
    for c in GROUPS[base]:
        sp = xs.store_problem(c["id"])
        acc, ss, y = sp["acc"], sp["ss"], sp["y"]
        C = acc.shape[1]
        line = f"SC {c['id']}"
        if c["bn"] == "rand":
            twice = sr.mul_add32(acc, _bcast(ss, 0, acc.ndim), _bcast(ss, 1, acc.ndim))
            sep = float(np.mean(twice != sp["bn_raw"]))
            act, lo, hi = sp["act"]
            y2 = sr.tail(sr._clamp32(twice, lo, hi) if act else twice, sp["res"], *sp["post"])[0]
            sep_final = float(np.mean(~sr.compare(y2, y)))
            line += f" fma_sep={sep:.3f}/{sep_final:.3f}"
            assert sep >= 0.10, f"{c['id']}: only {sep:.3f} of the BN outputs tell a twice-rounded store"
            # (the 10 % is a condition on the BN output; behind a clamp fewer final values differ -- the clamped ones are
            # those with the largest products -- and behind a quantizer only those next to a tie.  One differing value
            # fails a comparison by bits: 20 of them, spread over the tiles, are asked of every case without a quantizer)
            if sp["post"][3] is None and not c["emit"]:
                assert np.sum(~sr.compare(y2, y)) >= 20, f"{c['id']}: {sep_final:.3f} of the final values tell it"
            if act:
                at_lo, at_hi = float(np.mean(sp["bn_raw"] <= F32(lo))), float(np.mean(sp["bn_raw"] >= F32(hi)))
                line += f" clamp={at_lo:.3f}/{at_hi:.3f}"
                assert at_lo >= 0.05 and at_hi >= 0.05, f"{c['id']}: clamped shares {at_lo:.3f} / {at_hi:.3f}"
                if not c["emit"]:   # (an emitting case spends its planted channels on the quantizer's classes first)
                    assert {"lo", "hi"} <= set(sp["chan_targets"].values())
                if "hi" in sp["chan_targets"].values():
                    assert np.sum(sp["bn_raw"] == F32(lo)) >= 20 and np.sum(sp["bn_raw"] == F32(hi)) >= 20, \
                        f"{c['id']}: no BN output exactly on a clamp bound"
        if ss is not None and C > 1:
            yc = np.moveaxis(y, 1, 0).reshape(C, -1)
            same = [ch for ch in range(C - 1) if not (~sr.compare(yc[ch], yc[ch + 1])).any()]
            assert not same, f"{c['id']}: channels {same} equal their right neighbour in every pixel"
        q = sp["q_first"]
        req_q = [k for k in sp["required"] if k in xs.CLASSES_Q]
        if q is not None and req_q:
            cl = xs.store_classes(sp["xin"], q)
            low = {k: cl[k] for k in req_q if cl[k] < 20}
            distinct = int(np.unique(y).size)
            line += f" classes={min(cl[k] for k in req_q)} distinct={distinct}"
            assert not low, f"{c['id']}: planted classes with fewer than 20 values: {low}"
            assert distinct > 50, f"{c['id']}: {distinct} distinct outputs"
            if q[3] and sp["q_clamp"] is None and (C >= 16 or sp["res"] is not None) and \
                    not (sp["act"][0] and sp["res"] is None):
                assert set(req_q) == set(xs.CLASSES_Q), f"{c['id']}: a signed quantizer misses {req_q}"
            if "tiny_n" in req_q:   # (a signed quantizer with the class planted: those values must store -0.0)
                assert sr.signed_zero(sp["xin"], *q).sum() >= 20
        if sp["q_clamp"] is not None:
            # the post clamp decides values: both bounds are planted, each cuts at least 5 % of the values that reach
            # it, and a store without the clamp (the quantizer's own clamp to maxval alone) differs in 20 outputs or more
            plo, phi = sp["q_clamp"]
            cc = xs.clamp_classes(sp["xpre"], plo, phi)
            no_clamp = sr.tail(sp["bn_out"], sp["res"], 0, 0.0, 0.0, sp["post"][3])[0]
            changed = int((~sr.compare(no_clamp, y)).sum())
            line += f" post_clamp={cc['below']:.3f}/{cc['above']:.3f} on_bounds={cc['plo']}/{cc['phi']} unclamped_differs={changed}"
            assert {"plo", "phi"} <= set(sp["required"]), f"{c['id']}: the post clamp's bounds are not planted"
            assert cc["plo"] >= 20 and cc["phi"] >= 20, f"{c['id']}: values on the post clamp's bounds: {cc}"
            assert cc["below"] >= 0.05 and cc["above"] >= 0.05, f"{c['id']}: post clamp shares {cc}"
            assert changed >= 20, f"{c['id']}: dropping the post clamp changes {changed} outputs"
        if c["emit"]:
            line += f" header={sp['header']}"
            if c["emit"].get("q"):
                assert sp["header"][0] == 1, f"{c['id']}: the image was to come back invalid"
            else:
                assert sp["header"][0] == 0 and sp["ok"].all()
                back = sr.decode_words(sp["words"], sp["bR_next"], sp["Mw"], sp["form"])
                assert np.array_equal(back, sr.fake_quant(y, *sp["nextq"])[0])
        print(line)


def test_the_literal_quantizer_case_lies_outside_fq_fast_ok():
    """fq_fast_ok (fp8approx_common.h): -100 <= bias <= 120, 2^-100 <= maxval <= 2^64."""
    mx, nb, M, S = xs.Q_LITERAL
    assert mx > 2.0 ** 64 and -100 <= sr.fq_bias(mx, nb, M, S) <= 120
    for q in xs.OUT_Q.values():
        assert 2.0 ** -100 <= q[0] <= 2.0 ** 64 and -100 <= sr.fq_bias(*q) <= 120
