"""Conditions on the inputs of tests/test_gpu_grad_exact.py, checked without a GPU (tests/grad_exact.py).

  * every family case meets the exact-sum budget (tests/exact_sums.py: sum_k |T| <= 2^22 u); a case that misses
    it fails;
  * the plain model of the kernel's arithmetic equals expected(T) on every case;
  * every named mutant of the model -- a bug the old bar 1e-5 S would let pass -- changes at least one output of
    the cases named in CATCHES: the evidence that the GPU tests would fail on that bug;
  * the gap the new tests close: with tests/test_gpu_grad.py's own operands the model with the third piece
    dropped stays inside 1e-5 S;
  * the padded buffers hold NaN exactly outside the views;
  * the STE operator problems meet the budget: the same backward on absolute values, in units of u.
"""
import numpy as np
import pytest

from tests import exact_sums as xs
from tests import grad_exact as gx
from tests import pairs_cases as pc

FAMILY_CASES = [c for c in gx.CASES if gx.CASES[c]["fam"] in "WG"]

# mutant -> the cases that must catch it
CATCHES = {
    "drop_p2": ["W-2x37-130x40", "W-1x7-64x64", "W-1x1-64x64", "W-1x5-1x1", "routing"],
    "drop_p1": ["W-2x37-40x130", "W-1x96-70x67", "routing"],
    "b7": ["G-2x37-130x40", "G-1x1-64x64", "G-1x96-70x67"],
    "drop_last_k": ["W-1x33-64x65", "W-1x64-64x64", "W-1x32-65x64", "W-1x1-64x64", "G-2x37-40x130"],
    "swap_tile_counts": ["W-2x37-130x40", "W-2x37-40x130", "G-2x37-130x40", "G-2x37-40x130"],
    "no_wrap": [f"W-pad-{K0}x{K1}/{lay}" for (K0, K1) in gx.PAD_K for lay in ("k1", "m")],
}


def _views(cid):
    """(A, B) of a case: contiguous, or for "<pad case>/<layout>" the views of its padded buffers."""
    name, _, layout = cid.partition("/")
    p = gx.problem(name)
    if not layout:
        return p["A"], p["B"], p
    ba, bb = gx.padded(p["A"], p["B"], layout)
    M, K1, N = p["A"].shape[1], p["A"].shape[3], p["B"].shape[3]
    return gx.a_view(ba, layout, M, K1), gx.b_view(bb, layout, K1, N), p


@pytest.mark.parametrize("cid", FAMILY_CASES)
def test_case_meets_the_budget_and_the_model_is_exact(cid):
    p = gx.problem(cid)
    lg = xs.budget_log2(p["T"], axis=2)
    print(f"{cid}: u = 2^{np.log2(xs.unit(p['T'])):g}, budget 2^{lg:.2f}")
    assert xs.within_budget(p["T"], axis=2), f"{cid}: sum |T| = 2^{lg:.2f} u exceeds 2^{xs.BUDGET_LOG2} u"
    xs.assert_same(gx.model(p["A"], p["B"]), p["want"], cid, None)
    assert np.isfinite(p["want"]).all() and np.count_nonzero(p["want"]) > 0


def test_family_w_rows_have_three_full_width_elements():
    p = gx.problem("W-2x37-130x40")
    a = np.abs(p["A"].reshape(2, 130, 74).astype(np.float64)) / gx.A_SCALE
    wide = a >= 2 ** 17
    assert (wide.sum(axis=2) == 3).all() and (a[wide] % 2 == 1).all() and (a[wide] < 2 ** 18).all()
    from tests.test_grad_cpu import split3
    for q in split3(p["A"]):
        assert (q[wide.reshape(p["A"].shape)] != 0).all()          # all three pieces are nonzero there
    assert (np.abs(gx.problem("W-1x1-64x64")["A"]) >= 2 ** 17 * gx.A_SCALE).all()  # K < 3: every entry


def test_family_g_b_has_full_significands():
    B = gx.problem("G-2x37-130x40")["B"]
    u = B.view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()                          # bf16-exact: the kernel's contract
    assert (u[B != 0] & np.uint32(0x10000)).any()                     # ... with the eighth bit in use
    assert 0.05 < np.mean(B == 0) < 0.15


def test_routing_case():
    p = gx.problem("routing")
    A, B = p["A"], p["B"]
    K = A.shape[2] * A.shape[3]
    b = B.reshape(B.shape[0], K, -1)
    assert (np.count_nonzero(b, axis=1) == 1).all()                   # one nonzero per column
    assert (np.count_nonzero(b, axis=2) >= 1).all()                   # every k chosen by a column
    m, e = np.frexp(np.abs(b[b != 0]))
    assert (m == 0.5).all()                                           # powers of two
    sig = np.abs(A.astype(np.float64))
    m, e = np.frexp(sig)
    assert ((m * 2.0 ** 22) % 1 == 0).all() and e.min() >= -60 and e.max() <= 61
    from tests.test_grad_cpu import kernel_accepts
    assert kernel_accepts(A).all()
    xs.assert_same(gx.model(A, B), p["want"], "routing")
    # every output is the one product, which fp32 holds
    k_of = np.argmax(b != 0, axis=1)                                  # [nb, N]
    a = A.reshape(A.shape[0], -1, K)
    for i in range(A.shape[0]):
        want = a[i][:, k_of[i]].astype(np.float64) * b[i][k_of[i], np.arange(b.shape[2])].astype(np.float64)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        assert np.array_equal(p["want"][i], want.astype(np.float32))


@pytest.mark.parametrize("sign", [1, -1])
def test_pairs_case(sign):
    A, B, want = gx.pairs(sign)
    xs.assert_same(gx.model(A, B), want, f"pairs {sign:+d}")
    assert np.array_equal(gx.product64(A, B), want)
    assert want[3, 5, 0] == np.float32(1 + sign * 2.0 ** -21) and want[3, 3, 0] == 1.0


@pytest.mark.parametrize("mutant", gx.MUTANTS)
def test_every_mutant_is_caught_by_its_named_cases(mutant):
    for cid in CATCHES[mutant]:
        A, B, p = _views(cid)
        got = gx.model(A, B, mutant)
        n = int(np.count_nonzero(~(pc.same_bits(got, p["want"]))))
        print(f"{mutant} on {cid}: {n} of {got.size} outputs differ ({100.0 * n / got.size:.1f} %)")
        assert n >= 1, f"mutant {mutant} changes no output of case {cid}: the GPU test of that case would not see it"
        xs.assert_same(gx.model(A, B), p["want"], cid)                # (the unmutated model on the same views)


def test_mutants_the_old_shapes_cannot_see():
    """Square tile grids hide a swap of the tile counts, contiguous operands hide a missing k0 step."""
    A, B = gx.family("W", 2, 70, 2, 37, 67)                           # tests/test_gpu_grad.py's extents
    want = xs.expected(gx.terms(A, B), axis=2)
    for mutant in ("swap_tile_counts", "no_wrap"):
        xs.assert_same(gx.model(A, B, mutant), want, mutant)


def test_dropping_the_third_piece_passes_the_old_bar_on_the_old_operands():
    """The gap: tests/test_gpu_grad.py's operands (seed 0) and its bar 1e-5 S accept a kernel without p2."""
    from tests.test_gpu_grad import _operands, _ref
    A, B = _operands()
    ref, S = _ref(A, B)
    got = gx.model(A.numpy(), B.numpy(), "drop_p2")
    full = gx.model(A.numpy(), B.numpy())
    worst = float((np.abs(got.astype(np.float64) - ref.numpy()) / S.numpy()).max())
    exact = float((np.abs(full.astype(np.float64) - ref.numpy()) / S.numpy()).max())
    print(f"p2 dropped: worst err / S = {worst:.3e}; the full model: {exact:.3e}")
    assert worst <= 1e-5, worst                                       # inside the old bar: not caught
    assert worst > 20 * max(exact, 6e-8)                              # ... though far outside the kernel's own error
    assert np.count_nonzero(got != full) > 0.5 * got.size


@pytest.mark.parametrize("layout", ["k1", "m"])
@pytest.mark.parametrize("k0,k1", gx.PAD_K)
def test_padded_buffers_hold_nan_exactly_outside_the_views(k0, k1, layout):
    p = gx.problem(f"W-pad-{k0}x{k1}")
    A, B = p["A"], p["B"]
    M, N = A.shape[1], B.shape[3]
    ba, bb = gx.padded(A, B, layout)
    va, vb = gx.a_view(ba, layout, M, k1), gx.b_view(bb, layout, k1, N)
    assert va.shape == A.shape and vb.shape == B.shape
    assert np.array_equal(va, A) and np.array_equal(vb, B) and not np.isnan(va).any() and not np.isnan(vb).any()
    assert np.isnan(ba).sum() == ba.size - A.size and np.isnan(bb).sum() == bb.size - B.size
    st = lambda v: [s // 4 for s in v.strides]  # noqa: E731
    sa, sb = st(va), st(vb)
    assert sa[2] != k1 * sa[3] and sb[1] != k1 * sb[2]                # the k0 step does not collapse
    assert (sa[3] == 1) == (layout == "k1") and (sa[1] == 1) == (layout == "m")
    assert (sb[2] == 1) == (layout == "k1") and (sb[3] == 1) == (layout == "m")
    cb = gx.c_buffer(A.shape[0], M, N, layout)
    vc = gx.c_view(cb, layout)
    assert vc.shape == (A.shape[0], M, N) and (vc.strides[2] == 4) == (layout == "k1")
    vc[...] = 0.0
    assert np.count_nonzero(cb == gx.SENTINEL) == cb.size - vc.size   # a frame of sentinels all around


# ------------------------------------------------------------------------------------------ window edges
def test_window_values_sit_on_the_fields_they_are_named_for():
    assert gx.exponent_field(gx.GOOD_A) == 24
    assert [gx.exponent_field(gx.A_REJECTED[k]) for k in ("field23", "field1", "field0")] == [23, 1, 0]
    from tests.test_grad_cpu import kernel_accepts
    assert kernel_accepts(np.array([gx.GOOD_A, 0.0, -0.0], np.float32)).all()
    assert not kernel_accepts(np.array(list(gx.A_REJECTED.values()), np.float32)).any()
    sub = gx.B_REJECTED["bf16-subnormal"]
    assert sub != 0 and not (sub.view(np.uint32) & np.uint32(0xFFFF)) and gx.exponent_field(sub) == 0
    assert gx.B_REJECTED["1+2^-12"].view(np.uint32) & np.uint32(0xFFFF)


@pytest.mark.parametrize("M,N", gx.TWO_LEVEL)
def test_window_cases_have_one_exact_product_per_output(M, N):
    num_mt, num_nt = -(-M // 64), -(-N // 64)
    for operand in ("A", "B"):
        c = gx.window_case(M, N, operand)
        assert not c["tiles"] and np.isfinite(c["want"]).all() and (c["want"] != 0).all()
        xs.assert_same(gx.model(c["A"], c["B"]), c["want"], f"clean window case {operand}")
    for name in gx.A_REJECTED:
        w = gx.window_case(M, N, "A", name)
        assert len(w["tiles"]) == num_nt and w["spot"][2] >= 64       # the last, ragged stage
        assert np.count_nonzero(w["A"][1, w["spot"][1]]) == 1
    for name in gx.B_REJECTED:
        w = gx.window_case(M, N, "B", name)
        assert len(w["tiles"]) == num_mt
        if name == "bf16-subnormal":                                  # meets a = 2^100 in some row: 2^-30
            assert (np.abs(w["want"][1, :, w["spot"][2]]) == np.float32(2.0 ** -30)).any()


def test_small_product_cases():
    c = gx.small_case("piece-term-subnormal")
    a, b = gx.SMALL["piece-term-subnormal"]
    from tests.test_grad_cpu import split3
    assert [float(q[0]) for q in split3(np.array([a]))] == [2.0 ** -100, 2.0 ** -121, 0.0]
    assert 0 < 2.0 ** -121 * float(b) < 2.0 ** -126                   # the second piece's term is an fp32 subnormal
    assert (np.abs(c["want"]) == np.float32(2.0 ** -110 * (1 + 2.0 ** -21))).all()
    a3, b3 = gx.SMALL["third-piece-term-subnormal"]
    assert [float(q[0]) for q in split3(np.array([a3]))] == [2.0 ** -100, 2.0 ** -109, 2.0 ** -121] and b3 == b
    want3 = np.float32(2.0 ** -110 * (1 + 2.0 ** -9 + 2.0 ** -21))
    assert (np.abs(gx.small_case("third-piece-term-subnormal")["want"]) == want3).all()
    from tests.test_grad_cpu import kernel_accepts
    assert kernel_accepts(np.array([a, a3, gx.SMALL["product-subnormal"][0]], np.float32)).all()
    d = gx.small_case("product-subnormal")
    assert (np.abs(d["want"]) == np.float32(2.0 ** -140)).all() and np.float32(2.0 ** -140) != 0
    ks = {int(np.flatnonzero(r)[0]) for r in c["A"].reshape(70, 74)}
    assert len(ks) > 8 and max(ks) >= 64                              # several k positions, the tail included


# ------------------------------------------------------------------------------------------ STE operators
@pytest.mark.parametrize("stride", gx.CONV_STRIDES)
@pytest.mark.parametrize("groups", gx.CONV_GROUPS)
def test_conv_problem_meets_the_budget(groups, stride):
    x, w, dy = gx.conv_problem(groups, stride)
    L = dy.shape[2] * dy.shape[3]
    assert L == (117 if stride == (1, 1) else 63)
    for t, u in ((x, 2.0 ** -3), (w, 2.0 ** -3), (dy, 2.0 ** -20)):
        v = t.double().numpy() / u
        assert (v == np.round(v)).all()
    sx, sw = gx.conv_backward64(x, w, dy, groups, stride, use_abs=True)
    bx, bw = gx.budget_of(sx, gx.CONV_U), gx.budget_of(sw, gx.CONV_U)
    print(f"G = {groups}, stride {stride}: dX 2^{bx:.2f} u, dW 2^{bw:.2f} u")
    assert bx <= xs.BUDGET_LOG2 and bw <= xs.BUDGET_LOG2
    dx, dw = gx.conv_backward64(x, w, dy, groups, stride)
    for g in (dx, dw):                                                # ... so the float64 gradients are fp32 values
        assert np.array_equal(g.numpy().astype(np.float32).astype(np.float64), g.numpy())
        assert np.count_nonzero(g.numpy()) > 0.5 * g.numel()


def test_linear_and_bmm_problems_meet_the_budget():
    xq, wq, dy = gx.linear_problem()
    a = np.abs(dy.astype(np.float64))
    for name, S in (("linear dX", a @ np.abs(wq.astype(np.float64))), ("linear dW", a.T @ np.abs(xq.astype(np.float64)))):
        lg = gx.budget_of(S, gx.GRID_U)
        print(f"{name}: 2^{lg:.2f} u")
        assert lg <= xs.BUDGET_LOG2, name
    q, k, dc = gx.bmm_problem()
    qh, kh, a = (np.abs(gx.heads(q).astype(np.float64)), np.abs(gx.heads(k).astype(np.float64)),
                 np.abs(dc.astype(np.float64)))
    for name, S in (("bmm dA", a @ kh), ("bmm dB", np.swapaxes(a, -1, -2) @ qh)):
        lg = gx.budget_of(S, gx.GRID_U)
        print(f"{name}: 2^{lg:.2f} u")
        assert lg <= xs.BUDGET_LOG2, name
    for t in (xq, wq, q, k):
        v = t.astype(np.float64) / 2.0 ** -8
        assert (v == np.round(v)).all() and not (t.view(np.uint32) & np.uint32(0xFFFF)).any()
    for t in (dy, dc):
        v = t.astype(np.float64) / gx.A_SCALE
        assert (v == np.round(v)).all()
