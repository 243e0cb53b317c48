"""The CPU oracle against the reference on every code pair (tests/pairs_cases.py's cases: v9 at every
bias triple of the every-code-pair GPU tests under all 16 flag combinations and every built-in and
synthetic table, the tensor-bias single-column call, v5 with its OF / UF switches).

  * live: where the reference checkout is mounted, tests/golden/gen_golden_pairs.py --check recomputes
    the reference's terms (in subprocesses: the import shim patches torch factories, as
    test_ref_dropin_cpu.py) and compares them with oracle.terms bit for bit, zeros by value; a failure
    names the first differing pair of a case: the two operand values, the reference's and the oracle's
    value.  It also checks that the recorded digests are the reference's.
  * digest: everywhere (the reference absent included), oracle.terms' SHA-256 of every case, combined per
    group of cases that differ only in the flag word, against tests/golden/pairs_digest.json, which the
    generator wrote from the reference's terms.
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

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
JOBS = max(1, min(16, os.cpu_count() or 1))


def _recorded():
    with open(os.path.join(HERE, "golden", "pairs_digest.json")) as f:
        return json.load(f)["groups"]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "approx")), reason="reference checkout not mounted")
def test_oracle_equals_reference_on_every_code_pair_live():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONWARNINGS="ignore")
    out = subprocess.run([sys.executable, os.path.join(HERE, "golden", "gen_golden_pairs.py"), "--check",
                          "--jobs", str(JOBS)], capture_output=True, text=True, timeout=900, env=env,
                         cwd=os.path.dirname(HERE))
    assert out.stdout.strip(), out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] == len(pc.all_cases())
    assert res["n_oracle_mismatches"] == 0, "oracle != reference, first differing pair per case: " + \
        json.dumps(res["oracle_mismatches"], indent=1)
    assert res["n_stale"] == 0, f"pairs_digest.json is not what the reference gives now: {res['stale_digests']}"
    assert out.returncode == 0, out.stderr[-3000:]


def test_digest_file_lists_exactly_the_cases():
    rec = _recorded()
    groups = pc.groups()
    assert [{k: r[k] for k in g} for r, g in zip(rec, groups)] == groups and len(rec) == len(groups)
    assert all(len(r["sha256"]) == 64 for r in rec)
    cases = pc.all_cases()
    assert sum(len(g["flags"]) for g in groups) == len(cases) == len({pc.case_id(c) for c in cases})


def test_case_tables_cover_every_packing_mode():
    """Coverage guard of the case list (not a check of any kernel): per mantissa width every packing
    mode of pack_table that exists for it occurs among the format's tables, seven modes in all."""
    seen = set()
    for (E, M) in pc.FORMATS:
        modes = {pc.table_mode(t, M) for t in pc.tables(E, M).values()}
        assert modes == pc.modes_of_width(M), (E, M, modes)
        seen |= modes
    assert seen == set(pc.TM_NAMES)


def _oracle_digest(c):
    a, b = pc.case_operands(c)
    T = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), c["E"], c["M"], c["bA"], c["bB"], c["bR"], pc.case_table(c),
                  c["flags"])[:, 0, :]
    return pc.digest(T)


GROUPS = [(part, E, M) for part in ("v9", "tb", "v5") for (E, M) in pc.FORMATS]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}-E{g[1]}M{g[2]}")
def test_oracle_digests_match_the_recorded_reference(group):
    part, E, M = group
    rec = [r for r in _recorded() if (r["part"], r["E"], r["M"]) == (part, E, M)]
    assert rec, "no recorded group for this part and format"
    orc.lib()  # (built before the threads start)
    cases = [c for r in rec for c in pc.group_cases(r)]
    with ThreadPoolExecutor(JOBS) as ex:
        got = iter(list(ex.map(_oracle_digest, cases)))
    bad = [pc.case_id(dict(r, flags="*")) for r in rec
           if pc.group_digest([next(got) for _ in r["flags"]]) != r["sha256"]]
    assert not bad, f"{len(bad)} of {len(rec)} groups of cases differ from the reference's digest: {bad[:8]}"


@pytest.mark.parametrize("biases,every", [((10, 10, -13), False), ((16, 17, 0), True)])
def test_tensor_bias_max_norm_is_an_int32_power(biases, every):
    """Found by the live test: in the tensor-bias call the reference's
    max_norm = 2**(max_expo - bR) * (2 - 2^-M) is an int32 power, 0 once max_expo - bR >= 32 and negative at
    31, so with golden_clip_OF and quant_btw_mult_accu every nonzero product (at 31: every product, zero
    included) decodes as the largest code of the grid, (2 - 2^-M) 2^(max_expo - bR).  E5M2, zero table."""
    bA, bB, bR = biases
    a, b = pc.all_codes(5, 2, bA), pc.all_codes(5, 2, bB)
    fl = pc.flag_word(True, False, True, True, tb=True)
    T = orc.terms(a.reshape(-1, 1), b.reshape(1, -1), 5, 2, bA, bB, bR, pc.tables(5, 2)["zero"], fl)[:, 0, :]
    hit = np.ones(T.shape, bool) if every else np.outer(a, b) != 0
    assert np.all(np.abs(T[hit]) == np.float32(1.75 * 2.0 ** (31 - bR))) and np.all(T[~hit] == 0)
    assert any((r["part"], r["E"], r["bR"]) == ("tb", 5, bR) and fl in r["flags"] for r in _recorded())
