#!/usr/bin/env python
"""Every-code-pair digests of the reference's product terms (TEST INFRASTRUCTURE ONLY).

Like gen_golden.py it runs only where the reference checkout is mounted and imports the reference
UNMODIFIED (through gen_golden's import shim).  For every case of tests/pairs_cases.py -- a format, a
bias triple, an error table and a flag word -- it asks the reference for the term of every code pair,
T[i, j] = term(a_i, b_j) over the 256 codes of A's grid and the 256 codes of B's grid:

  v9   custom_matmul_vectorize on A [256, 1] x B [1, 256] (K = 1: one term per output), the table passed
       as an argument (built-in and synthetic tables alike)
  tb   QCustomBNConv2dTorch.approx_multiply's single-column (tensor-bias) call, A [256, 1] against every
       weight code as B [1, 1] -- 256 calls per case (the reference picks the table itself from withComp /
       dnsmp_factor; for E5M2, which its get_error_table_NN rejects, the operator is given gen_golden.table,
       the zero table, as gen_golden's G8 does)
  v5   approx_matmul_whole_v5's custom_matmul_vectorize through gen_golden.v5_call

and writes tests/golden/pairs_digest.json.  Per case it takes the SHA-256 of the term bits (little-endian
uint32, every zero canonicalised to +0); per group of cases that differ only in the flag word it records the
parameters, the flag words and one SHA-256 over those case digests (pairs_cases.group_digest): every term bit
of every case enters a recorded digest, in a file a tenth the size.  The raw terms are tens of MB.

  python tests/golden/gen_golden_pairs.py            write pairs_digest.json (and compare with the oracle)
  python tests/golden/gen_golden_pairs.py --check    recompute, compare with oracle.terms bit for bit and
                                                     with the recorded digests; one JSON line; exit 1 on a
                                                     difference (tests/test_oracle_pairs_cpu.py runs this)
Both spread the cases over worker processes (--jobs, default 8), each a fresh interpreter.
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "pairs_digest.json")
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden as gg  # noqa: E402  (installs the import shim, puts the reference on sys.path)
from oracle import oracle as orc  # noqa: E402
from tests import pairs_cases as pc  # noqa: E402


def _variant(E, M, name):
    """(withComp, dnsmp_factor) of a built-in table name (gen_golden.TABLE_VARIANTS)."""
    return next((wc, dn) for (n, wc, dn) in gg.TABLE_VARIANTS[(E, M)] if n == name)


_checked = set()


def _check_builtin_table(c, tab):
    """The committed fixture table a case names is the reference's own."""
    E, M, name = c["E"], c["M"], c["table"]
    key = (c["part"] == "v5", E, M, name)
    if key in _checked:
        return
    if c["part"] == "v5":
        if name != "zero":
            ref = gg.v5.get_comp_table_NN(E, M, True, int(name[1:]), "cpu")
            assert np.array_equal(ref.numpy().astype(np.int32), tab), f"v5 table {key} differs from the reference's"
    elif name in pc.BUILTIN[(E, M)]:
        ref = gg.table(E, M, *_variant(E, M, name))
        assert np.array_equal(ref.numpy().astype(np.int32), tab), f"table {key} differs from the reference's"
    _checked.add(key)


def ref_terms(c):
    """The reference's terms of a case, float32 [256 a][256 b]."""
    E, M, fl = c["E"], c["M"], c["flags"]
    a, b = pc.case_operands(c)
    tab = pc.case_table(c)
    _check_builtin_table(c, tab)
    A = torch.from_numpy(a.reshape(-1, 1).copy())
    if c["part"] == "v5":
        sw = (bool(fl & pc.OFUF), bool(fl & pc.OF_OPT), bool(fl & pc.UF_OPT))
        T = gg.v5_call(A, torch.from_numpy(b.reshape(1, -1).copy()), E, M, c["bA"], torch.from_numpy(tab.copy()), *sw)
        return T.numpy().astype(np.float32)
    approx, s2n, qbma, gclip = (bool(fl & f) for f in (pc.APPROX, pc.S2N, pc.QBMA, pc.GCLIP))
    if c["part"] == "v9":
        T = gg.cmv(A, torch.from_numpy(b.reshape(1, -1).copy()), E, M, c["bA"], c["bB"], c["bR"],
                   torch.from_numpy(tab.copy()), approx, s2n, qbma, gclip)
        return T.numpy().astype(np.float32)
    wc, dn = _variant(E, M, c["table"])
    op = gg._FakeOp(gg.approx_params(E, M, dn, wc, approx, s2n, qbma, gclip))
    xb = torch.tensor([float(c["bA"])])
    yb = torch.tensor(float(c["bB"]))  # 0-dim, as weight_group_fp_bias.squeeze(): the tensor-bias call
    rb = torch.tensor([float(c["bR"])])
    gg.ac.get_error_table_NN = gg.table if (E, M) == (5, 2) else gg.v9.get_error_table_NN
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cols = [gg.ac.QCustomBNConv2dTorch.approx_multiply(op, A, torch.tensor([[float(w)]]), xb, yb, rb)
                    for w in b]
    finally:
        gg.ac.get_error_table_NN = gg.v9.get_error_table_NN
    return torch.cat(cols, dim=1).numpy().astype(np.float32)


def oracle_terms(c):
    a, b = pc.case_operands(c)
    return orc.terms(a.reshape(-1, 1), b.reshape(1, -1), c["E"], c["M"], c["bA"], c["bB"], c["bR"],
                     pc.case_table(c), c["flags"])[:, 0, :]


def run_shard(index, count):
    """[(case number, digest, mismatch or None)] of the cases index, index + count, ..."""
    torch.set_num_threads(1)
    cases = pc.all_cases()
    out = []
    for k in range(index, len(cases), count):
        c = cases[k]
        T = ref_terms(c)
        R = oracle_terms(c)
        same = pc.same_bits(T, R)
        bad = None
        if not same.all():
            a, b = pc.case_operands(c)
            i, j = (int(v) for v in np.argwhere(~same)[0])
            bad = dict(case=pc.case_id(c), differing=int(np.count_nonzero(~same)), a=float(a[i]), b=float(b[j]),
                       reference=float(T[i, j]), oracle=float(R[i, j]),
                       reference_bits=int(T[i, j:j + 1].view(np.uint32)[0]),
                       oracle_bits=int(R[i, j:j + 1].view(np.uint32)[0]))
        out.append((k, pc.digest(T), bad))
    return out


def run_all(jobs):
    """Every case, spread over `jobs` fresh interpreters: (digests by case number, mismatches)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--shard", f"{i}/{jobs}"],
                              stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT) for i in range(jobs)]
    digests, bad = {}, []
    for p in procs:
        stdout, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"worker failed with status {p.returncode}")
        for k, d, b in json.loads(stdout.strip().splitlines()[-1]):
            digests[k] = d
            if b:
                bad.append(b)
    return digests, bad


def group_records(digests):
    """One record a group: its parameters, its flag words and the digest over its cases' term digests."""
    out, k = [], 0
    for g in pc.groups():
        n = len(g["flags"])
        out.append(dict(g, sha256=pc.group_digest([digests[k + i] for i in range(n)])))
        k += n
    assert k == len(digests)
    return out


def write(digests):
    assert sorted(digests) == list(range(len(pc.all_cases())))
    lines = [json.dumps(r, separators=(",", ":")) for r in group_records(digests)]
    with open(OUT, "w") as f:
        f.write('{"reference":"revollllt/FP8_quantization@2024-11-08",\n'
                '"terms":"per case T[i][j] of all_codes(bA) x all_codes(bB), uint32 little-endian, zeros as +0",\n'
                '"sha256":"of the hex SHA-256 of each case of the group, in the order of flags",\n'
                '"groups":[\n' + ",\n".join(lines) + "\n]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--shard", default=None, help="internal: i/n")
    args = ap.parse_args()
    if args.shard:
        i, n = (int(v) for v in args.shard.split("/"))
        print(json.dumps(run_shard(i, n)))
        return 0
    digests, bad = run_all(max(1, args.jobs))
    if args.check:
        with open(OUT) as f:
            rec = json.load(f)["groups"]
        now = group_records(digests)
        stale = [pc.case_id(dict(g, flags="*")) for k, g in enumerate(now) if k >= len(rec) or rec[k] != g]
        print(json.dumps(dict(cases=len(digests), groups=len(now), oracle_mismatches=bad[:10],
                              n_oracle_mismatches=len(bad), stale_digests=stale[:10],
                              n_stale=len(stale) + abs(len(rec) - len(now)))))
        return 1 if bad or stale or len(rec) != len(now) else 0
    for b in bad:
        print("ORACLE DIFFERS:", json.dumps(b))
    write(digests)
    print(f"{OUT}: {len(digests)} cases, {os.path.getsize(OUT)} bytes, {len(bad)} oracle mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
