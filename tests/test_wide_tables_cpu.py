"""The CPU oracle against the reference on error tables over the full int8 range (tests/wide_tables.py:
V >= 4, 0 < V < 1/2, V == 0, V < 0 with |V| below and above the golden significand product, negative V above
Q_R's pre-clamp bound, a signed mix, entries that wrap through uint8_t), for every format.

  * live: where the reference checkout is mounted, tests/golden/gen_golden_wide.py --check recomputes the
    reference's K = 1 terms of every case, compares them with oracle.terms value by value (zeros by value) and
    confirms the recorded digests.
  * digest: everywhere, oracle.terms' SHA-256 per case, combined per group, against
    tests/golden/wide_digest.json.
  * non-vacuity, from the oracle alone: every table's class is reached by at least 20 K = 1 terms of some
    triple (flags approx + s2n + qbma, both operands normal), each class with its own witness, and at least
    5 % of a case's terms of nonzero operands differ from the same case under the table clipped to -3 .. 4.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from tests import pairs_cases as pc
from tests import wide_tables as wt

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
JOBS = max(1, min(16, os.cpu_count() or 1))
FL = pc.flag_word(True, True, True, False)


def _recorded():
    with open(os.path.join(HERE, "golden", "wide_digest.json")) as f:
        return json.load(f)["groups"]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "approx")), reason="reference checkout not mounted")
def test_oracle_equals_reference_on_wide_tables_live():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONWARNINGS="ignore")
    out = subprocess.run([sys.executable, os.path.join(HERE, "golden", "gen_golden_wide.py"), "--check",
                          "--jobs", str(JOBS)], capture_output=True, text=True, timeout=900, env=env,
                         cwd=os.path.dirname(HERE))
    assert out.stdout.strip(), out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] == len(wt.all_cases())
    assert res["n_oracle_mismatches"] == 0, "oracle != reference, first differing pair per case: " + \
        json.dumps(res["oracle_mismatches"], indent=1)
    assert res["n_stale"] == 0, f"wide_digest.json is not what the reference gives now: {res['stale_digests']}"
    assert out.returncode == 0, out.stderr[-3000:]


def test_digest_file_lists_exactly_the_cases():
    rec, groups = _recorded(), wt.groups()
    assert [{k: r[k] for k in g} for r, g in zip(rec, groups)] == groups and len(rec) == len(groups)
    assert all(len(r["sha256"]) == 64 for r in rec)
    cases = wt.all_cases()
    assert sum(len(g["flags"]) for g in groups) == len(cases) == len({pc.case_id(c) for c in cases})


@pytest.mark.parametrize("part,E,M", [(p, E, M) for p in ("v9", "tb") for (E, M) in wt.FORMATS],
                         ids=lambda v: str(v))
def test_oracle_digests_match_the_recorded_reference(part, E, M):
    rec = [r for r in _recorded() if (r["part"], r["E"], r["M"]) == (part, E, M)]
    assert rec, "no recorded group for this part and format"
    orc.lib()  # (built before the threads start)
    cases = [c for r in rec for c in pc.group_cases(r)]
    with ThreadPoolExecutor(JOBS) as ex:
        got = iter(list(ex.map(lambda c: pc.digest(wt.oracle_terms(c)), cases)))
    bad = [pc.case_id(dict(r, flags="*")) for r in rec
           if pc.group_digest([next(got) for _ in r["flags"]]) != r["sha256"]]
    assert not bad, f"{len(bad)} of {len(rec)} groups of cases differ from the reference's digest: {bad[:8]}"


# ------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("E,M", wt.FORMATS)
def test_tables_are_what_their_docstrings_say(E, M):
    n = 1 << M
    tabs = wt.tables(E, M)
    assert list(tabs) == list(wt.NAMES) and set(wt.TABLES) == set(tabs)
    N = {k: wt.numerators(t, M) for k, t in tabs.items()}
    ss = wt.numerators(np.zeros((n, n), np.int32), M)
    assert tabs["hi"].min() == -128 and tabs["hi"].max() < 0 and N["hi"][0, 0] == 4 * n * n
    assert (N["hi"] == 8 * n * n).any() == (M <= 4)  # (E2M5: V tops out at 7.88, see wide_tables.hi)
    assert tabs["lowpos"].min() >= 0 and N["lowpos"].min() == 1 and 2 * N["lowpos"].max() < n * n
    assert tabs["zero_v"].min() >= 0 and tabs["zero_v"][0, 0] == n and np.count_nonzero(N["zero_v"] == 0) >= 2 * n - 1
    assert tabs["neg_small"].min() >= 0 and N["neg_small"].max() < 0 and (-N["neg_small"] <= ss).all()
    assert tabs["neg_big"].min() >= 0 and tabs["neg_big"].max() == 127 and np.count_nonzero(-N["neg_big"] > ss) >= n
    assert tabs["neg_sat"].min() >= 0 and np.count_nonzero(wt.class_mask("neg_sat", M)) >= n
    assert tabs["mixed"].min() < -3 and tabs["mixed"].max() > 4  # signed, outside the narrow tables' range
    assert pc.table_mode(tabs["mixed"], M) == "TM_LUT" and not pc.tt_table_form(tabs["mixed"], M)
    u = tabs["u8wrap"]
    assert ((u >= 64) | (u <= -65)).all() and u.min() < -65 and u.max() > 64
    # the host's table predicates on the family (csrc/fp8approx.hip, restated in pairs_cases)
    assert pc.xm_table_form(tabs["lowpos"], M) and not any(pc.xm_table_form(tabs[k], M) for k in wt.NAMES if k != "lowpos")
    assert {k for k in wt.NAMES if pc.tt_table_form(tabs[k], M)} == {"hi", "lowpos", "zero_v"}


# ------------------------------------------------------------------------------------------ non-vacuity
def _terms(E, M, tr, table, fl=FL):
    a, b = pc.all_codes(E, M, tr[0]), pc.all_codes(E, M, tr[1])
    return orc.terms(a.reshape(-1, 1), b.reshape(1, -1), E, M, tr[0], tr[1], tr[2], table, fl)[:, 0, :], a, b


def _witnesses(E, M, name, tr):
    """(terms in the class, the class's own witness count, share of nonzero-operand terms that differ under
    the clipped table) of one (format, table, triple) under approx + s2n + qbma."""
    n = 1 << M
    tab = wt.tables(E, M)[name]
    T, a, b = _terms(E, M, tr, tab)
    cls = wt.pair_class(name, E, M)
    g = np.outer(a.astype(np.float64), b.astype(np.float64))
    gq = orc.quant(g.astype(np.float32), E, M, tr[2])
    e, m, _ = wt.code_fields(E, M)
    Nn = wt.numerators(tab, M)[m[:, None], m[None, :]].astype(np.float64)
    ss = ((n + m)[:, None] * (n + m)[None, :]).astype(np.float64)
    x = g * Nn / ss  # the unquantized approximate product of a normal pair, exact in double
    if name == "zero_v":  # (the class's terms are zero by construction: counted where the golden product is not)
        in_class = np.count_nonzero(cls & (gq != 0) & (T == 0))
    else:
        in_class = np.count_nonzero(cls & (T != 0))
    own = in_class
    if name == "neg_big":  # the golden product flushed, the approximate term not, s_a s_b = -1
        own = np.count_nonzero(cls & (g < 0) & (gq == 0) & (T != 0))
    elif name == "neg_sat":  # plain round-half-even at the value's own step (carrying) gives another value
        k = np.maximum(np.floor(np.log2(np.maximum(np.abs(x), 1e-300))), 1 - tr[2])
        step = 2.0 ** (k - M)
        carried = np.rint(np.abs(x) / step) * step
        own = np.count_nonzero(cls & (T != 0) & (carried != np.abs(T.astype(np.float64))))
    elif name == "hi":  # finite, nonzero, V >= 4, below max_norm: golden_clip_OF would not clip it
        max_norm = (2.0 - 2.0 ** -M) * 2.0 ** ((1 << E) - 1 - tr[2])
        own = np.count_nonzero(cls & np.isfinite(T) & (T != 0) & (np.abs(T) < max_norm))
    Tn = _terms(E, M, tr, wt.narrow(tab))[0]
    nz = g != 0
    share = np.count_nonzero(~pc.same_bits(T, Tn) & nz) / np.count_nonzero(nz)
    return in_class, own, share


@pytest.mark.parametrize("E,M", wt.FORMATS)
@pytest.mark.parametrize("name", wt.NAMES)
def test_every_class_is_reached(E, M, name):
    """Conditions on the inputs, not on any kernel: one and the same triple of the format reaches the table's
    class with at least 20 terms, holds at least 20 of the class's own witnesses and differs from the clipped
    table on at least 5 % of the terms of nonzero operands (the triples that do are printed; a triple whose
    products all lie in the flush region or far above the grid need not)."""
    per = {tr: _witnesses(E, M, name, tr) for tr in wt.v9_triples(E, M)}
    good = [tr for tr, (c, o, sh) in per.items() if c >= 20 and o >= 20 and sh >= 0.05]
    print(f"WIDE-CLASS E{E}M{M} {name}: {len(good)} of {len(per)} triples meet all three; " +
          " ".join(f"{'_'.join(map(str, tr))}:{c}/{o}/{sh:.3f}" for tr, (c, o, sh) in per.items()))
    assert good, per
