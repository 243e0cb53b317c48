"""The cases of tests/reduce_plan.py without a GPU: that each reaches the branch it is there for, and that each can
tell a kernel with an index error in it from a right one.

Conditions, from the built library and not only from the Python restatement:
  * fp8a_bn_train_workspace_size / (16 C) and (fp8a_fp8_mse_workspace_size - rows nc 16) / (rows nc 8) are the
    planned parts, for the new cases and for every shape of the two older GPU files;
  * per case what its `expect` claims -- parts < tiles, the uneven split, the ragged last tile, the image boundary
    inside a tile, more apply work than the grid has threads;
  * the older shapes reach none of it: parts == tiles for each, and one apply iteration per thread.
Mutants (reduce_plan.MUTANTS; a condition, not a measurement): for every case and every mutant that applies to it,
at least one checked quantity -- save_mean, save_var, scale, shift under the S1 / S2 bars; a sse under B -- leaves
the GPU test's bar by a factor of 100 or more, and the unmutated model stays inside the bar.
"""
import numpy as np
import pytest

from fp8_quantization_amd import _lib
from tests import reduce_plan as rp

NC = {"m3": 111, "m1to6": 666}


def bn_parts_of_library(pl):
    nbytes = _lib.load().fp8a_bn_train_workspace_size(pl["N"], pl["C"], pl["inner"])
    assert nbytes > 0 and nbytes % (16 * pl["C"]) == 0
    return nbytes // (16 * pl["C"])


def mse_parts_of_library(pl, n_mbits):
    nc = 111 * n_mbits
    rest = _lib.load().fp8a_fp8_mse_workspace_size(pl["rows"], pl["inner"], 111, n_mbits) - pl["rows"] * nc * 16
    assert rest > 0 and rest % (pl["rows"] * nc * 8) == 0
    return rest // (pl["rows"] * nc * 8)


def test_constants_are_the_headers():
    k = rp.K
    assert set(k) == {"BN_TILE", "BN_LIN_TILE", "BN_LIN_INNER", "BN_TARGET_WGS", "MSE_TILE", "MSE_TARGET_WGS",
                      "APPLY_THREADS"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    # the library agrees with each of them where a workspace size can show it: one more value than a tile holds is
    # a second part, one channel more than the target halves what a channel may have
    L = _lib.load()
    f = L.fp8a_bn_train_workspace_size
    assert f(1, 1, k["BN_TILE"]) == 16 and f(1, 1, k["BN_TILE"] + 1) == 32
    assert f(k["BN_LIN_TILE"], 1, 1) == 16 and f(k["BN_LIN_TILE"] + 1, 1, 1) == 32
    N, li = k["BN_LIN_TILE"] + 1, k["BN_LIN_INNER"]
    assert f(N, 1, li - 1) == 16 * rp.cdiv(N * (li - 1), k["BN_LIN_TILE"])                 # lin: tiles of 256
    assert f(N, 1, li) == 16 * rp.cdiv(N * li, k["BN_TILE"]) < f(N, 1, li - 1)             # tiles of BN_TILE
    C = k["BN_TARGET_WGS"]
    assert f(1, C, 8 * k["BN_TILE"]) == 16 * C and f(1, C - 1, 8 * k["BN_TILE"]) == 16 * (C - 1) * 2
    g = L.fp8a_fp8_mse_workspace_size
    assert g(1, k["MSE_TILE"], 111, 1) == 111 * 24 and g(1, k["MSE_TILE"] + 1, 111, 1) == 111 * 32
    R = k["MSE_TARGET_WGS"]
    assert g(R, 8 * k["MSE_TILE"], 1, 1) == R * 24 and g(R - 1, 8 * k["MSE_TILE"], 1, 1) == (R - 1) * 32


@pytest.mark.parametrize("cid", list(rp.BN_CASES))
def test_bn_case_reaches_its_branch(cid):
    case = rp.BN_CASES[cid]
    pl, ex = rp.bn_plan(case["shape"]), case["expect"]
    assert bn_parts_of_library(pl) == pl["parts"]
    sizes = tuple(t1 - t0 for (t0, t1) in pl["split"])
    for k, v in ex.items():
        assert (sizes if k == "sizes" else pl[k]) == v, (cid, k)
    assert pl["parts"] < pl["tiles"] and sum(sizes) == pl["tiles"] and min(sizes) >= 1 and max(sizes) >= 2
    if "uneven" in cid:
        assert pl["tiles"] % pl["parts"] != 0 and len(set(sizes)) > 1
    if cid == "bn-one-part":
        assert pl["want"] == 1 and pl["parts"] == 1
    assert 0 < pl["last"] < pl["tile"]                                  # the last tile is ragged ...
    assert pl["split"][-1][1] - pl["split"][-1][0] >= 2                 # ... at the end of a several-tile part
    assert pl["work"] > rp.K["APPLY_THREADS"] and pl["strides"] >= 4    # later grid-stride iterations of apply
    assert pl["N"] * pl["C"] * pl["inner"] < 2 ** 31                    # (the uint32_t instance)
    wraps = rp.wrap_tiles(pl)
    late = [t for (t, first) in wraps if not first]
    if pl["lin"]:
        assert pl["groups"] == 65 and pl["C"] % 64 == 4                 # a last group with 4 live channels
        assert late                                                     # (inner = 1: every value is an image)
    else:
        assert wraps, "no image boundary inside a tile"
        # every part's later tiles start inside an image (off0 != 0) ...
        assert all((t * pl["tile"]) % pl["inner"] != 0 for (t0, t1) in pl["split"] for t in range(t0 + 1, t1))
    if cid == "bn-vec-uneven":
        assert (1, True) in wraps                                       # the table's claim: inside tile 1
    if cid == "bn-wrap-late":
        assert late == [2]                                              # ... and here one holds a boundary too


@pytest.mark.parametrize("cid", list(rp.MSE_CASES))
def test_mse_case_reaches_its_branch(cid):
    case = rp.MSE_CASES[cid]
    pl, ex = rp.mse_plan(case["shape"]), case["expect"]
    from tests.test_gpu_mse import WIDTHS
    assert NC[case["widths"]] == 111 * len(WIDTHS[case["widths"]])
    assert mse_parts_of_library(pl, len(WIDTHS[case["widths"]])) == pl["parts"]
    sizes = tuple(t1 - t0 for (t0, t1) in pl["split"])
    for k, v in ex.items():
        assert (sizes if k == "sizes" else pl[k]) == v, (cid, k)
    assert pl["parts"] < pl["tiles"] and sum(sizes) == pl["tiles"] and min(sizes) >= 1
    assert 0 < pl["last"] < pl["tile"] and sizes[-1] >= 2               # a ragged tile ends a several-tile part
    if cid == "mse-rows-uneven":
        assert pl["tiles"] % pl["parts"] != 0
    if cid == "mse-one-part":
        assert pl["want"] == 1
    if cid == "mse-tensor":
        assert sorted(sizes) == [1] * 2044 + [2] * 4


def test_the_older_shapes_reach_none_of_it():
    from tests.test_gpu_bn_train import SHAPES as BN_OLD
    from tests.test_gpu_mse import SHAPES as MSE_OLD, WIDTHS
    for shape in BN_OLD:
        pl = rp.bn_plan(shape)
        assert bn_parts_of_library(pl) == pl["parts"] == pl["tiles"], shape
        assert all(t1 - t0 == 1 for (t0, t1) in pl["split"])
        assert pl["work"] <= rp.K["APPLY_THREADS"] and pl["strides"] == 0, shape
        assert not [t for (t, first) in rp.wrap_tiles(pl) if not first]
    for shape in MSE_OLD:
        pl = rp.mse_plan(shape)
        for w in WIDTHS.values():
            assert mse_parts_of_library(pl, len(w)) == pl["parts"] == pl["tiles"], shape
        assert all(t1 - t0 == 1 for (t0, t1) in pl["split"])


def test_the_bars_are_those_of_the_bn_train_file():
    """bn_reference / bn_bars / ulp32 restate case() and ulp32 of tests/test_gpu_bn_train.py in numpy: equal on
    that file's own cases up to the float64 rounding of the two libraries' sums and powers."""
    from tests import test_gpu_bn_train as old
    assert rp.EPS == old.EPS and rp.U == old.U
    for shape in old.SHAPES:
        c = old.case(shape)
        r = rp.bn_reference(c["x"].numpy(), c["gamma"].numpy(), c["beta"].numpy())
        assert r["n"] == c["n"] and r["C"] == c["C"]
        for k in ("dm", "dv", "ds", "dsh", "scale", "shift", "mean", "var"):
            want = c[k].numpy()
            assert np.all(np.abs(r[k] - want) <= 1e-12 * np.abs(want) + 1e-300 + (1e-15 if k in ("mean", "shift") else 0)), \
                (shape, k)
        assert np.array_equal(rp.ulp32(r["scale"]), old.ulp32(c["scale"]).numpy())


def _caught(pairs):
    """At least one checked quantity is 100 bars or more away (and away at all: a bar may be 0)."""
    return any(bool(((err >= 100 * bar) & (err > 0)).any()) for (err, bar) in pairs)


@pytest.mark.parametrize("cid", list(rp.BN_CASES))
def test_bn_model_inside_the_bars_and_every_mutant_outside(cid):
    c = rp.bn_case(cid)
    pl = c["plan"]
    assert pl == rp.bn_plan(rp.BN_CASES[cid]["shape"])
    x = c["x"]
    assert np.all(x[:, 0] == -2.625) and np.all(x[:, 2] == 0) and np.all(np.abs(x[:, 1] - 4096) <= 2.0 ** -8)
    assert c["var"][0] == 0 and c["var"][2] == 0 and 0 < c["var"][1] < 2.0 ** -16
    for (err, bar) in rp.bn_errors_over_bars(c, *rp.bn_model(cid)):
        assert (err <= bar).all(), cid
    shown = []
    for mutant in rp.MUTANTS:
        if not rp.mutant_applies(pl, mutant, bn=True):
            continue
        pairs = rp.bn_errors_over_bars(c, *rp.bn_model(cid, mutant))
        worst = max(float((err[bar > 0] / bar[bar > 0]).max()) for (err, bar) in pairs)
        print(f"{cid} {mutant}: worst error / bar {worst:.3g}")
        assert _caught(pairs), f"{cid} cannot tell {mutant}"
        shown.append(mutant)
    want = {"bn-one-part": ["tail_short", "no_wrap"], "bn-lin-uneven": ["t1_floor", "tile_twice", "tail_short",
                                                                        "lin_unclamped"]}
    assert shown == want.get(cid, ["t1_floor", "tile_twice", "tail_short", "no_wrap"]), shown


@pytest.mark.parametrize("sign_bits", [1, 0])
@pytest.mark.parametrize("cid", list(rp.MSE_CASES))
def test_mse_model_inside_the_bar_and_every_mutant_outside(cid, sign_bits):
    from tests.test_gpu_mse import B
    c = rp.mse_case(cid)
    pl = c["plan"]
    x = c["x"]
    assert (x[:, ::7][:, :-1] == 0).all() and (x < 0).any() and (x[:, -1] > 0).all()
    model, straight = rp.mse_model(cid, sign_bits)
    assert np.isfinite(straight).all() and (straight > 0).all()
    assert (np.abs(model - straight) <= B * straight).all()
    shown = []
    for mutant in rp.MUTANTS:
        if not rp.mutant_applies(pl, mutant, bn=False) or mutant in rp.MSE_CASES[cid]["exempt"]:
            continue
        got, _ = rp.mse_model(cid, sign_bits, mutant)
        rel = np.abs(got - straight) / straight
        print(f"{cid} sign_bits={sign_bits} {mutant}: worst relative error {rel.max():.3g}, bar {B:.3g}")
        assert (rel >= 100 * B).any(), f"{cid} cannot tell {mutant}"
        shown.append(mutant)
    want = {"mse-rows-uneven": ["t1_floor", "tile_twice", "tail_short", "row_base"],
            "mse-one-part": ["tail_short", "row_base"], "mse-tensor": ["t1_floor", "tile_twice"]}
    assert shown == want[cid], shown
