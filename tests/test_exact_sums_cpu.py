"""Every case of tests/test_gpu_exact_sums.py, on the CPU oracle alone (tests/exact_sums.py):

  * the budget: max over outputs of sum_k |T| <= 2^22 u, u the largest power of two dividing every nonzero
    term -- the condition under which a float32 sum of the terms is the same in every order;
  * oracle.matmul (a float64 accumulation, rounded once) equals expected(oracle.terms) bit for bit (the exact
    product: the float64 matrix product; qamaa: oracle.matmul_qamaa's float32 k-order sums of the fq terms);
  * the case is not vacuous: with per-product quantization, among products of two nonzero operands at least
    5 % are flushed to zero, 15 % lie in the result grid's subnormal band and 15 % are normal; without it (and
    for the v5 model) the nonzero terms occupy at least 3 binades.  The constructed wave-tile cases assert their
    construction instead: exactly one product at the grid's smallest normal / at half the quantum, every other
    product below it, at a K position that is not the first of a staged tile.

It also writes what the old tolerance 1e-5 sum|T| had allowed per case, in units of u, to
profiles/exact_sums/old_bar.txt.
"""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from tests import exact_sums as xs
from tests import pairs_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_BAR = os.path.join(ROOT, "profiles", "exact_sums", "old_bar.txt")
FLOORS = dict(flushed=0.05, band=0.15, normal=0.15)

PROBLEMS = collections.OrderedDict()  # problem key -> its first case (cases that differ in options share it)
for _c in xs.CASES.values():
    PROBLEMS.setdefault(_c["pkey"], _c)
GROUPS = collections.OrderedDict()
for _k, _c in PROBLEMS.items():
    shape = "x".join(map(str, _c["shape"])) if "shape" in _c else _c["kind"]
    GROUPS.setdefault(f"{_c['kind']}-{_c['fam']}-{shape}", []).append(_k)

_BARS = {}


@pytest.fixture(scope="module", autouse=True)
def _old_bar_file():
    orc.lib()
    yield
    if set(_BARS) == set(PROBLEMS):  # (a partial run leaves the file alone)
        os.makedirs(os.path.dirname(OLD_BAR), exist_ok=True)
        with open(OLD_BAR, "w") as f:
            f.write("# case  K  log2(max sum|T| / u)  old bar 1e-5 sum|T| in u: median max\n")
            for k in PROBLEMS:
                f.write(_BARS[k] + "\n")


def _check_band_construction(c, p):
    A, B, T, _ = p["parts"][0]
    M, bR = c["M"], p["bR"]
    r, k, n = xs.BAND_SPOT
    level = 2.0 ** (1 - bR) if c["regime"] == "band" else 2.0 ** (-bR - M)
    g = np.abs(A[:, :, None].astype(np.float64) * B[None, :, :])
    at = np.argwhere(g >= level)
    assert [tuple(v) for v in at] == [(r, k, n)], f"products at or above the level: {at[:5]}"
    assert g[r, k, n] == level * (1 + (1 / 32 if c["regime"] == "zero1" else 0))
    assert k % 2 == 1, "an odd K position is the first of no staged tile (XK = 4 for E2M5; any even XK)"
    want = {"band": level, "zero": 0.0, "zero1": 2.0 ** (1 - bR - M)}[c["regime"]] if c["table"] == "zero" else None
    if want is not None:
        assert abs(float(T[r, k, n])) == want, (T[r, k, n], want)
    if c["regime"] != "band":
        others = np.abs(T).sum() - abs(float(T[r, k, n]))
        assert others == 0, "every other term of the zero regime must be flushed"


def _check(pkey):
    c = PROBLEMS[pkey]
    p = xs.problem_of.__wrapped__(pkey)  # (no cache: the groups run their problems in parallel)
    E, M, fl = c["E"], c["M"], c["flags"]
    lb = xs.case_budget_log2(p)
    assert lb <= xs.BUDGET_LOG2, f"{pkey}: max sum|T| = 2^{lb:.2f} u is over the 2^22 u budget"
    for (A, B, T, sl) in p["parts"]:
        if c["fam"] == "dense":    # the reference of the exact product: the float64 product, rounded once
            C = (A.astype(np.float64) @ B.astype(np.float64)).astype(np.float32)
        elif c["fam"] == "qamaa":  # the oracle's own float32 k-order sums before the final quantizer
            C = orc.matmul_qamaa(A, B, c["maxval"], 8, M)[1]
        else:
            bB = p["bB"][sl] if isinstance(sl, slice) else p["bB"]
            C = orc.matmul(A, B, E, M, p["bA"], bB, p["bR"], p["table"], p.get("flags", fl))
        xs.assert_same(C, xs.expected(T), f"{pkey}: the oracle's sum against the summed terms", T)
    if c["kind"] == "band":
        _check_band_construction(c, p)
    elif c["fam"] == "qamaa":
        sh = xs.shares(p["parts"][0][2], p["parts"][0][0], p["parts"][0][1], M, p["bR"])
        for name, floor in FLOORS.items():
            assert sh[name] >= floor, f"{pkey}: {name} share {sh[name]:.3f} is under {floor}"
    elif c["fam"] == "dense":
        nz = np.concatenate([np.abs(T[T != 0]).ravel() for (_, _, T, _) in p["parts"]])
        assert np.unique(np.frexp(nz)[1]).size >= 3, f"{pkey}: the products occupy fewer than 3 binades"
    else:
        sh = [xs.shares(T, A, B, M, p["bR"]) for (A, B, T, _) in p["parts"]]
        if c["kind"] == "tbdw":  # no subnormal floor: the binades around 2^-bR (expo field 0, F7) must all occur
            nz = np.concatenate([np.abs(T[T != 0]).ravel() for (_, _, T, _) in p["parts"]])
            assert np.unique(np.frexp(nz)[1]).size >= 8, f"{pkey}: the terms occupy fewer than 8 binades"
            if not fl & pc.V5:
                for lo_, hi_ in ((-p["bR"] - 2, -p["bR"]), (-p["bR"], 1 - p["bR"]), (1 - p["bR"], 3 - p["bR"])):
                    share = np.mean((nz >= 2.0 ** lo_) & (nz < 2.0 ** hi_))
                    assert share >= 0.03, f"{pkey}: {share:.3f} of the terms in [2^{lo_}, 2^{hi_})"
        elif fl & pc.QBMA and not fl & pc.V5:
            for name, floor in FLOORS.items():  # (per part: each group of a convolution, each batch item)
                got = min(s[name] for s in sh)
                assert got >= floor, f"{pkey}: {name} share {got:.3f} is under {floor}"
        else:
            assert min(s["binades"] for s in sh) >= 3, f"{pkey}: the terms occupy {sh[0]['binades']} binades"
    med, mx = xs.case_old_bar(p)
    return f"{pkey}  {xs.case_K(c)}  {lb:.2f}  {med:.3g} {mx:.3g}"


@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_budget_oracle_and_shares(group):
    keys = GROUPS[group]
    with ThreadPoolExecutor(min(8, len(keys))) as ex:
        futs = [(k, ex.submit(_check, k)) for k in keys]
    errs = []
    for k, f in futs:
        if f.exception() is not None:
            errs.append(str(f.exception()))
        else:
            _BARS[k] = f.result()
    assert not errs, f"{len(errs)} of {len(keys)} cases:\n" + "\n".join(errs)


GEO_PROBLEMS = collections.OrderedDict()  # the non-square geometry problems, by geometry name
for _c in xs.geo_cases() + [xs.QAMAA_CONV]:
    _g = _c["cfg"] if _c["kind"] == "conv" else _c["geo"]
    GEO_PROBLEMS.setdefault(_g["name"], collections.OrderedDict()).setdefault(_c["pkey"], (_c, _g))


def _check_exchanges(c, geo):
    """The case's expected output against what a kernel would give that took one (h, w) pair the wrong way round."""
    p = xs.problem_of.__wrapped__(c["pkey"])
    if c["fam"] == "qamaa":
        def mm(A, B, sl):
            return orc.matmul_qamaa(A, B, c["maxval"], 8, c["M"])[1]
    else:
        def mm(A, B, sl):
            return orc.matmul(A, B, c["E"], c["M"], p["bA"], p["bB"][sl], p["bR"], p["table"], p.get("flags", c["flags"]))
    want = np.concatenate([xs.expected(T) for (_, _, T, _) in p["parts"]], axis=1)
    mine = xs.conv_output(geo, p["x"], p["w"], mm)
    xs.assert_same(mine.reshape(want.shape), want, f"{c['pkey']}: conv_output against the terms")
    want = want.reshape(mine.shape)
    told = []
    for which in xs.EXCHANGES:
        ex = xs.exchanged(geo, p["x"], p["w"], which)
        if ex is None:
            continue
        got = xs.conv_output(*ex, mm)
        differ = 1.0 if got.shape != want.shape else float(np.mean(~pc.same_bits(got, want)))
        assert differ >= 0.5, f"{c['pkey']}: with `{which}` exchanged only {differ:.2f} of the outputs differ"
        told.append(which)
    return told


@pytest.mark.parametrize("name", list(GEO_PROBLEMS), ids=list(GEO_PROBLEMS))
def test_geometry_cases_tell_an_exchanged_pair(name):
    """Every non-square case: exchanging ph / pw, sh / sw, dh / dw, the taps' kh / kw or the planes' H / W -- each
    exchange that changes the problem at all -- gives another output shape or differs in at least half of the
    outputs.  A condition on the drawn data and sizes: a kernel with a transposed index cannot pass the case."""
    items = list(GEO_PROBLEMS[name].values())
    with ThreadPoolExecutor(min(8, len(items))) as ex:
        futs = [(c["pkey"], ex.submit(_check_exchanges, c, g)) for c, g in items]
    errs = [str(f.exception()) for _, f in futs if f.exception() is not None]
    assert not errs, f"{len(errs)} of {len(items)} problems:\n" + "\n".join(errs)
    for k, f in futs:  # H <-> W changes every case here, and so does at least one other pair
        assert "hw" in f.result() and len(f.result()) >= 2, (k, f.result())


@pytest.mark.parametrize("cid", [c["id"] for c in xs.chain_cases()])
def test_chained_consumers_meet_the_budget_and_tell_an_exchange(cid):
    """The consumer of each chained pair, on the oracle's quantizer of the producer's expected output: the budget, the
    oracle's sum against the summed terms, at least 8 binades of terms and few zero outputs, and the exchanged pairs."""
    c = next(v for v in xs.chain_cases() if v["id"] == cid)
    p = xs.chain_problem(c)
    lb = xs.case_budget_log2(p)
    assert lb <= xs.BUDGET_LOG2, f"{cid}: max sum|T| = 2^{lb:.2f} u is over the 2^22 u budget"

    def mm(A, B, sl):
        return orc.matmul(A, B, c["E"], c["M"], p["bA"], p["bB"][sl], p["bR"], p["table"], p["flags"])
    want = np.concatenate([xs.expected(T) for (_, _, T, _) in p["parts"]], axis=1)
    for (A, B, T, sl) in p["parts"]:
        xs.assert_same(mm(A, B, sl), xs.expected(T), f"{cid}: the oracle's sum against the summed terms", T)
    nz = np.concatenate([np.abs(T[T != 0]).ravel() for (_, _, T, _) in p["parts"]])
    assert np.unique(np.frexp(nz)[1]).size >= 8 and np.mean(want == 0) < 0.05
    want = want.reshape(xs.conv_output(p["geo"], p["q"], p["w"], mm).shape)
    told = 0
    for which in xs.EXCHANGES:
        ex = xs.exchanged(p["geo"], p["q"], p["w"], which)
        if ex is not None:
            got = xs.conv_output(*ex, mm)
            differ = 1.0 if got.shape != want.shape else float(np.mean(~pc.same_bits(got, want)))
            assert differ >= 0.5, f"{cid}: with `{which}` exchanged only {differ:.2f} of the outputs differ"
            told += 1
    assert told >= 1


def test_unit_and_expected_on_known_values():
    T = np.array([[[0.75], [0.0], [-2.5]]], np.float32)  # multiples of 0.25
    assert xs.unit(T) == 0.25 and xs.unit(np.zeros(3, np.float32)) == 0.0
    assert xs.budget_log2(T) == np.log2(3.25 / 0.25)
    assert xs.expected(T)[0, 0] == np.float32(-1.75)
    big = np.array([[[2.0 ** 23], [1.0]]], np.float32)   # 2^23 + 1 units: over the budget
    assert not xs.within_budget(big) and xs.within_budget(np.array([[[2.0 ** 22 - 1.0], [1.0]]], np.float32))
    assert len(xs.mismatches(np.array([0.0, 1.0], np.float32), np.array([-0.0, 1.0], np.float32))) == 0


def test_case_list_reaches_every_listed_path():
    fams = collections.Counter((c["kind"], c["fam"]) for c in xs.CASES.values())
    for key in (("mat", "f8mx"), ("mat", "tt"), ("mat", "tt16"), ("mat", "fast"), ("mat", "v5mx"), ("mat", "v5fast"),
                ("conv", "f8mx"), ("conv", "tt"), ("conv", "tt16"), ("conv", "fast"), ("band", "tt"), ("bmm", "bmm"),
                ("dense", "dense"), ("dconv", "dense"), ("ddw", "dense"), ("qamaa", "qamaa"), ("tbdw", "tbx"),
                ("tbdw", "tb_fast"), ("tbdw", "tb_direct"), ("tbdw", "v5dw")):
        assert fams[key] > 0, key
    modes = {pc.table_mode(pc.tables(E, M)[n], M) for (E, M, n) in xs.one_table_per_mode()}
    assert modes == set(pc.TM_NAMES)
    for c in xs.CASES.values():  # what the family names say is what the dispatch rule says
        if c["kind"] in ("mat", "conv", "band") and c["fam"] != "fast":
            want = {"v5fast": "fast"}.get(c["fam"], c["fam"])
            got = pc.expected_matmul_path(c["E"], c["M"], xs.case_table(c), c["flags"], K=xs.case_K(c))
            assert got == want, c["id"]
