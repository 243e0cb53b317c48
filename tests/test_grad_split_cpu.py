"""The gradient GEMM's split along K (fp8a_grad_bmm_split) without a GPU: the two exports, every
new argument check -- answered before the library touches a device --, the split plan of the C entry against the
Python restatement (tests/grad_split.py), and the model the GPU tests compare with: its cases meet the exact-sum
budget, it equals expected(T) for every split count, and each of its mutants changes the outputs of named cases.

Which mutant shows where (outputs that differ from expected(T), of nb M N = 9380 at 70 x 67 and 10400 on the 130 x
40 / 40 x 130 grids; mutant_shows() states the pattern, test_mutants_change_named_cases the counts' lower bounds):
  drop_part, stage_overlap  every case at every split count >= 2: more than 8000 outputs (a whole part's terms are
                            missing, or a stage's are summed twice);
  tail_dropped              only where K is ragged, K = 1 x 129 (the stage of one element): its 8004 .. 8400 outputs
                            whose lost term is nonzero; nothing where K is a multiple of 32;
  per_floor                 where max(1, floor(nst / splits)) < ceil: splits 2, 3, 4 at five stages (5 divides);
                            K = 1 x 96 (three stages) at splits = 2 only;
  ws_item_stride            every case with S >= 2: 5266 outputs at 70 x 67 (items and tiles exchanged in a 2 x 4
                            index, and ragged tiles read their neighbours' zeros), 7760 on the 3-tile grids.
"""
import ctypes

import numpy as np
import pytest

from fp8_quantization_amd import _lib
from tests import exact_sums as xs
from tests import grad_split as gs
from tests.test_grad_cpu import GOOD, ORDER, PTR

WHO = "fp8a_grad_bmm_split: "
BIG = ctypes.c_void_p(1 << 40)   # a workspace pointer far from the operands, 16-byte aligned, never dereferenced


def call(A=PTR, B=ctypes.c_void_p(8192), C=ctypes.c_void_p(16384), splits=2, ws=BIG, ws_bytes=1 << 30, **kw):
    d = dict(GOOD, **kw)
    L = _lib.load()
    rc = L.fp8a_grad_bmm_split(A, B, C, *[d[k] for k in ORDER], splits, ws, ws_bytes, None)
    return rc, L.fp8a_last_error().decode()


def size(nb, M, N, K0, K1, splits):
    L = _lib.load()
    S, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = L.fp8a_grad_bmm_split_workspace_size(nb, M, N, K0, K1, splits, ctypes.byref(S), ctypes.byref(nbytes))
    return rc, int(S.value), int(nbytes.value)


def test_exports():
    L = _lib.load()
    for name in ("fp8a_grad_bmm_split_workspace_size", "fp8a_grad_bmm_split"):
        assert name in _lib.SYMBOLS and callable(getattr(L, name))
    from fp8_quantization_amd import approx_ops
    assert "grad_split_auto" in approx_ops.__all__ and callable(approx_ops.grad_split_auto)
    assert callable(_lib.grad_split_plan)


def test_the_checks_of_the_unsplit_entry_under_the_new_name():
    for ext in ("nb", "M", "N", "K0", "K1"):
        assert call(**{ext: -1}) == (_lib.EINVAL, WHO + "negative extent")
    for st in ORDER[5:]:
        assert call(**{st: -1}) == (_lib.EINVAL, WHO + "negative stride")
    assert call(K0=1 << 20, K1=1 << 11) == (_lib.EINVAL, WHO + "K0 * K1 exceeds 2^31 - 1")
    for null in ("A", "B", "C"):
        assert call(**{null: None}) == (_lib.EINVAL, WHO + "null pointer")
    for st in ("sc_i", "sc_m", "sc_n"):
        assert call(**{st: 0}) == (_lib.EINVAL, WHO + "a zero stride of C over an extent above 1")
    assert call(C=PTR) == (_lib.EINVAL, WHO + "C overlaps an operand")
    assert call(C=ctypes.c_void_p(4096 + 4 * 80)) == (_lib.EINVAL, WHO + "C overlaps an operand")
    assert call(M=1 << 38, N=64, sc_m=64) == (_lib.EINVAL, WHO + "more than 2^31 - 1 tiles")
    for ext in ("nb", "M", "N"):
        assert call(A=None, B=None, C=None, ws=None, **{ext: 0})[0] == _lib.OK


def test_every_new_check_returns_before_a_hip_call():
    """(Where there is no HIP device, a call that got as far as HIP would not return FP8A_EINVAL.)"""
    wide = dict(K0=1, K1=96, sa_i=288, sa_m=96, sa_k0=96, sb_i=480, sb_k0=480)     # three stages: S = 2 at splits = 2
    for s in (0, -3):
        assert call(splits=s, **wide) == (_lib.EINVAL, WHO + "splits below 1")
    # tiles nb S: 2^20 x 2^9 tiles x 2 items fit (2^30), times S = 2 they do not
    assert call(splits=2, **dict(wide, M=64 << 20, N=64 << 9, sc_m=64 << 9, sc_i=1 << 50, sa_i=1 << 50)) == \
        (_lib.EINVAL, WHO + "more than 2^31 - 1 blocks")
    need = gs.workspace_bytes(2, 3, 5, 96, 2)
    assert need == 2 * 2 * 4096 * 4
    assert call(ws=None, **wide) == (_lib.EINVAL, WHO + "null workspace")
    assert call(ws_bytes=need - 1, **wide) == (_lib.EINVAL, WHO + f"workspace of {need - 1} bytes, {need} needed")
    assert call(ws=ctypes.c_void_p((1 << 40) + 8), **wide) == (_lib.EINVAL, WHO + "workspace not 16-byte aligned")
    overlap = WHO + "the workspace overlaps A, B or C"
    assert call(ws=PTR, **wide) == (_lib.EINVAL, overlap)                           # A's base
    assert call(ws=ctypes.c_void_p(8192), **wide) == (_lib.EINVAL, overlap)         # B's base
    assert call(ws=ctypes.c_void_p(16384), **wide) == (_lib.EINVAL, overlap)        # C's base
    # dense spans that meet: A's 576 floats end inside a workspace that starts 16 bytes below it; C's 30 floats
    assert call(ws=ctypes.c_void_p(4096 - 16), **wide) == (_lib.EINVAL, overlap)
    assert call(ws=ctypes.c_void_p(16384 + 16), **wide) == (_lib.EINVAL, overlap)
    # (S = 1 asks for no workspace: tests/test_gpu_grad_split.py runs it with none, on real operands)


KS = (1, 5, 32, 33, 64, 74, 96, 129, 160)
REQUESTED = (1, 2, 3, 4, 5, 7, 64)


@pytest.mark.parametrize("K", KS)
def test_workspace_size_equals_the_python_plan(K):
    for splits in REQUESTED:
        per, S = gs.plan(K, splits)
        nst = -(-K // 32)
        assert 1 <= S <= min(splits, max(nst, 1)) and per * S >= nst and per * (S - 1) < nst     # no part is empty
        assert (S == 1) == (nst <= 1 or splits == 1 or per == nst)
        for (nb, M, N) in ((2, 70, 67), (1, 130, 40), (3, 64, 64)):
            for (K0, K1) in ((1, K), (K, 1)):
                assert size(nb, M, N, K0, K1, splits) == (_lib.OK, S, gs.workspace_bytes(nb, M, N, K, splits)), \
                    (K, splits, nb, M, N)
                assert _lib.grad_split_plan(nb, M, N, K0, K1, splits) == (S, gs.workspace_bytes(nb, M, N, K, splits))
    assert gs.plan(33, 7) == (1, 2) and gs.plan(5, 4) == (1, 1) and gs.plan(129, 4) == (2, 3)
    assert size(2, 70, 67, 0, 9, 5) == (_lib.OK, 1, 0)                               # K = 0: no stage
    L = _lib.load()
    assert size(2, 70, 67, 1, 96, 0)[0] == _lib.EINVAL
    assert L.fp8a_last_error().decode() == "fp8a_grad_bmm_split_workspace_size: splits below 1"
    assert L.fp8a_grad_bmm_split_workspace_size(2, 70, 67, 1, 96, 2, None, None) == _lib.EINVAL


def test_the_parts_cover_k_once():
    for K in KS:
        for splits in REQUESTED:
            rs = gs.ranges(K, splits)
            assert rs[0][0] == 0 and rs[-1][1] == K and all(a < b for a, b in rs)
            assert all(rs[i][1] == rs[i + 1][0] and rs[i + 1][0] % 32 == 0 for i in range(len(rs) - 1))
            assert len(rs) == gs.plan(K, splits)[1]


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("cid", list(gs.CASES))
def test_cases_meet_the_budget_and_the_model_is_exact_for_every_split(cid):
    p = gs.problem(cid)
    b = xs.budget_log2(p["T"], axis=2)
    print(f"{cid}: sum |T| <= 2^{b:.2f} u")
    assert b <= xs.BUDGET_LOG2
    for splits in (1,) + gs.SPLITS:
        xs.assert_same(gs.model_split(p["A"], p["B"], splits), p["want"], f"{cid} splits {splits}", p["T"])


def test_family_g_at_k_256_is_over_the_budget():
    """(Why no case is longer: the next K that is a power of two does not fit.)"""
    from tests import grad_exact as gx
    A, B = gx.family("G", 2, 70, 1, 256, 67)
    assert xs.budget_log2(gx.terms(A, B), axis=2) > xs.BUDGET_LOG2


def _stages(cid):
    c = gs.CASES[cid]
    return -(-(c["K0"] * c["K1"]) // 32)


def mutant_shows(mutant, cid, splits):
    """Whether a mutant changes a case's outputs at a requested split count (the docstring's table)."""
    c = gs.CASES[cid]
    K, nst = c["K0"] * c["K1"], _stages(cid)
    if gs.plan(K, splits)[1] == 1:
        return False
    if mutant == "tail_dropped":
        return K % 32 != 0
    if mutant == "per_floor":
        return max(1, nst // splits) != -(-nst // splits)
    return True


@pytest.mark.parametrize("mutant", gs.MUTANTS)
def test_mutants_change_named_cases(mutant):
    shown = 0
    for cid in gs.CASES:
        p = gs.problem(cid)
        for splits in (1,) + gs.SPLITS:
            bad = len(xs.mismatches(gs.model_split(p["A"], p["B"], splits, mutant), p["want"]))
            if mutant_shows(mutant, cid, splits):
                floor = 5000 if mutant == "ws_item_stride" else 8000
                assert bad >= floor, f"{mutant} changes only {bad} outputs of {cid} at splits = {splits}"
                shown += 1
            else:
                assert bad == 0, f"{mutant} changes {bad} outputs of {cid} at splits = {splits}"
    # each of the 13 cases shows the three mutants that need no special K at all four split counts; tail_dropped only
    # the two ragged cases; per_floor the eleven five-stage cases at 2, 3, 4 and the two three-stage ones at 2
    want = {"drop_part": 52, "stage_overlap": 52, "ws_item_stride": 52, "tail_dropped": 8, "per_floor": 35}[mutant]
    assert shown == want, (mutant, shown)


def test_the_first_three_mutants_change_nothing_unsplit():
    p = gs.problem("W-1x129-70x67")
    for mutant in gs.MUTANTS[:3]:
        assert np.array_equal(gs.model_split(p["A"], p["B"], 1, mutant).view(np.uint32),
                              gs.model_split(p["A"], p["B"], 1).view(np.uint32))


def test_the_order_of_the_adds_matters_on_the_slice_operands():
    """The slice identity's data (GPU test 4) tells index order from another order and from one float64 sum."""
    A, B = gs.slice_operands(1, 160)
    parts = [gs.gx.model(*gs.k_slice(A, B, kb, ke)) for (kb, ke) in gs.ranges(160, 5)]
    fwd, rev = gs.slice_sum(parts), gs.slice_sum(parts[::-1])
    assert (fwd.view(np.uint32) != rev.view(np.uint32)).sum() > 100
    assert (fwd.view(np.uint32) != gs.gx.model(A, B).view(np.uint32)).sum() > 100


def test_the_operator_key_is_checked_at_construction():
    from fp8_quantization_amd.resnet_workload import approx_qparams
    from fp8_quantization_amd.approx_calculation import QCustomLinearTorch
    for bad in (0, -1, 1.5, "8", True, None):
        qp = approx_qparams(ste_backward=True)
        qp["custom_approx_params"]["grad_split_k"] = bad
        with pytest.raises(ValueError, match="grad_split_k"):
            QCustomLinearTorch(8, 4, **qp)
    for good in (1, 2, 7, "auto"):
        qp = approx_qparams(ste_backward=True, grad_split_k=good)
        assert qp["custom_approx_params"].get("grad_split_k", 1) == good
        QCustomLinearTorch(8, 4, **qp)
    assert "grad_split_k" not in approx_qparams(ste_backward=True)["custom_approx_params"]


def test_split_k_values_are_checked_before_any_launch():
    import torch
    from fp8_quantization_amd.approx_ops import grad_bmm, ste_linear
    a, b = torch.zeros(2, 3), torch.zeros(3, 4)
    for bad in (0, -2, 2.0, "all", True):
        with pytest.raises(ValueError, match="split_k"):
            grad_bmm(a, b, split_k=bad)
        with pytest.raises(ValueError, match="split_k"):
            ste_linear(a, b.t(), torch.nn.functional.linear, split_k=bad)
