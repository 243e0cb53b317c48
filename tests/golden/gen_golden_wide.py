#!/usr/bin/env python
"""Every-code-pair digests of the reference's product terms on error tables over the full int8 range
(TEST INFRASTRUCTURE ONLY).

gen_golden_pairs.py's twin for the cases of tests/wide_tables.py: it runs only where the reference checkout
is mounted, imports the reference UNMODIFIED (through gen_golden's import shim) and asks it for the K = 1
term of every code pair,

  v9   custom_matmul_vectorize on A [codes, 1] x B [1, codes], the wide table passed as the argument
  tb   QCustomBNConv2dTorch.approx_multiply's single-column (tensor-bias) call per weight code, the
       operator's table lookup answered with the wide table (as gen_golden_pairs answers it with the zero
       table for E5M2)

and writes tests/golden/wide_digest.json: per group of cases that differ only in the flag word the
parameters, the flag words and one SHA-256 over the cases' term digests (pairs_cases.group_digest).

  python tests/golden/gen_golden_wide.py            write wide_digest.json (and compare with the oracle)
  python tests/golden/gen_golden_wide.py --check    recompute, compare with oracle.terms value by value and
                                                    with the recorded digests; one JSON line; exit 1 on a
                                                    difference (tests/test_wide_tables_cpu.py runs this)
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
OUT = os.path.join(HERE, "wide_digest.json")
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden as gg  # noqa: E402  (installs the import shim, puts the reference on sys.path)
from tests import pairs_cases as pc  # noqa: E402
from tests import wide_tables as wt  # noqa: E402


def ref_terms(c):
    """The reference's terms of a case, float32 [codes a][codes b]."""
    E, M, fl = c["E"], c["M"], c["flags"]
    a, b = pc.case_operands(c)
    tab = wt.case_table(c)
    A = torch.from_numpy(a.reshape(-1, 1).copy())
    approx, s2n, qbma, gclip = (bool(fl & f) for f in (pc.APPROX, pc.S2N, pc.QBMA, pc.GCLIP))
    if c["part"] == "v9":
        T = gg.cmv(A, torch.from_numpy(b.reshape(1, -1).copy()), E, M, c["bA"], c["bB"], c["bR"],
                   torch.from_numpy(tab.copy()), approx, s2n, qbma, gclip)
        return T.numpy().astype(np.float32)
    op = gg._FakeOp(gg.approx_params(E, M, 3, False, approx, s2n, qbma, gclip))
    xb = torch.tensor([float(c["bA"])])
    yb = torch.tensor(float(c["bB"]))  # 0-dim, as weight_group_fp_bias.squeeze(): the tensor-bias call
    rb = torch.tensor([float(c["bR"])])
    gg.ac.get_error_table_NN = lambda *args, **kw: torch.from_numpy(tab.copy())
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cols = [gg.ac.QCustomBNConv2dTorch.approx_multiply(op, A, torch.tensor([[float(w)]]), xb, yb, rb)
                    for w in b]
    finally:
        gg.ac.get_error_table_NN = gg.v9.get_error_table_NN
    return torch.cat(cols, dim=1).numpy().astype(np.float32)


def run_shard(index, count):
    """[(case number, digest, mismatch or None)] of the cases index, index + count, ..."""
    torch.set_num_threads(1)
    cases = wt.all_cases()
    out = []
    for k in range(index, len(cases), count):
        c = cases[k]
        T = ref_terms(c)
        R = wt.oracle_terms(c)
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
    out, k = [], 0
    for g in wt.groups():
        n = len(g["flags"])
        out.append(dict(g, sha256=pc.group_digest([digests[k + i] for i in range(n)])))
        k += n
    assert k == len(digests)
    return out


def write(digests):
    assert sorted(digests) == list(range(len(wt.all_cases())))
    lines = [json.dumps(r, separators=(",", ":")) for r in group_records(digests)]
    with open(OUT, "w") as f:
        f.write('{"reference":"revollllt/FP8_quantization@2024-11-08",\n'
                '"terms":"per case T[i][j] of all_codes(bA) x all_codes(bB), uint32 little-endian, zeros as +0",\n'
                '"tables":"tests/wide_tables.py",\n'
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
