"""The every-code-pair case list shared by the oracle-vs-reference pin (tests/golden/gen_golden_pairs.py,
tests/test_oracle_pairs_cpu.py) and the kernel-vs-oracle flag matrix (tests/test_gpu_flag_matrix.py).

Data and plain helpers only: no reference code, and nothing here needs the reference or a GPU.  The
built-in error tables are read from the committed fixtures (g2_matmul.npz: the v9 tables of
gen_golden.TABLE_VARIANTS; g7_v5.npz: the v5 compensation tables); the generator checks them against
the reference's own before it uses them.

Cases that differ only in the flag word form a group (groups()): pairs_digest.json records one digest a group.
A case is a dict of plain values (JSON-able):
  part   "v9" | "tb" | "v5"
  E, M   the format;  bA, bB, bR  the bias triple (v5: one bias three times)
  table  a name of tables(E, M) (v9 / tb) or v5_tables(E, M) (v5)
  flags  the oracle's flag word (oracle.py: APPROX | S2N | QBMA | GCLIP | TB, or V5 | OFUF | OF_OPT | UF_OPT)
Every case's terms are T[i, j] = term(a_i, b_j) over all 256 codes a of (E, M, bA) and all 256 codes b
of (E, M, bB), 256 x 256 float32.
"""
import functools
import hashlib
import itertools

import numpy as np

from tests import golden_io as gio

APPROX, S2N, QBMA, GCLIP, TB = 1, 2, 4, 8, 16
V5, OFUF, OF_OPT, UF_OPT = 32, 64, 128, 256

FORMATS = [(4, 3), (3, 4), (2, 5), (5, 2)]
TM_NAMES = ("TM_NONE", "TM_W1U", "TM_W2S1", "TM_W2S2", "TM_W2U1", "TM_W2U2", "TM_LUT")

# gen_golden.TABLE_VARIANTS' names (the reference's get_error_table_NN selections; E5M2: the zero table)
BUILTIN = {(4, 3): ["comp", "nocomp"], (3, 4): ["comp3", "comp4", "nocomp"],
           (2, 5): ["comp3", "comp4", "comp5", "nocomp"], (5, 2): ["zero"]}
# gen_golden.V5_TABLES' down-sampling factors (v5's get_comp_table_NN; none for E5M2)
V5_DNS = {(4, 3): [3], (3, 4): [3, 4], (2, 5): [3, 4, 5], (5, 2): []}

# ------------------------------------------------------------------------------------------ bias triples
# v9: gen_golden.G2_BIASES' triple first, then every triple of the existing every-code-pair GPU tests of
# the format (test_gpu_f8 / _custom_table: E4M3; test_gpu_tt: bA, bB = 2^(E-1) + 2, + 5 and
# bR = bA + bB - 2^E - {0, 3, 6}; test_gpu_f8_e5m2 / _custom_table: E5M2, incl. the out-of-range (16, 16, 5)
# and the top-binade (20, 20, 8)), then E4M3's beyond-the-top-binade (12, 12, 14).
V9_TRIPLES = {
    (4, 3): [(7, 9, 8), (12, 12, 8), (10, 13, 7), (9, 9, 2), (12, 14, 0), (8, 8, -14), (20, 18, 22), (12, 12, 14)],
    (3, 4): [(3, 5, 5), (6, 9, 7), (6, 9, 4), (6, 9, 1)],
    (2, 5): [(1, 2, 2), (4, 7, 7), (4, 7, 4), (4, 7, 1)],
    (5, 2): [(15, 17, 16), (20, 20, 7), (18, 22, 5), (24, 24, 15), (16, 17, 0), (10, 10, -13), (30, 12, 9),
             (16, 16, 5), (20, 20, 8)],
}
# tensor bias: per format the G2 triple (mid range: every band of the result grid occurs), one whose
# products lie in the result grid's subnormal band and flush region, one whose products reach its top
# binade and run beyond it, and one with a negative bR.  E5M2's last two have 31 - bR = 44 and 31: the
# reference's int32 power 2**(max_expo - bR) behind max_norm wraps to 0 and to -2^31 there
TB_TRIPLES = {
    (4, 3): [(7, 9, 8), (9, 9, -2), (9, 9, 12), (8, 8, -14)],
    (3, 4): [(3, 5, 5), (6, 6, 0), (6, 6, 9), (4, 4, -3)],
    (2, 5): [(1, 2, 2), (4, 4, 1), (3, 3, 7), (2, 2, -4)],
    (5, 2): [(15, 17, 16), (20, 20, 4), (28, 28, 40), (10, 10, -13), (16, 17, 0)],
}


def v5_biases(E):
    """v5 has one bias for A, B and the result: the default, and two above it."""
    return [2 ** (E - 1) - 1, 2 ** (E - 1) + 2, 2 ** (E - 1) + 6]


V5_FLAGS = [(False, False, False), (True, False, False), (True, True, False), (True, False, True),
            (True, True, True)]  # (sim_hw_add_OFUF, with_OF_opt, with_UF_opt), gen_golden.V5_FLAGS


# ------------------------------------------------------------------------------------------ operands
def all_codes(E, M, bias):
    """Every value of the (E, M) format at the given bias: 2^(E+M) magnitudes (subnormals and +0
    included), then their negatives (-0 included)."""
    e = np.repeat(np.arange(1 << E), 1 << M)
    m = np.tile(np.arange(1 << M), 1 << E)
    v = np.where(e == 0, np.ldexp(m / 2.0 ** M, 1 - bias), np.ldexp(1.0 + m / 2.0 ** M, e - bias))
    return np.concatenate([v, -v]).astype(np.float32)


# ------------------------------------------------------------------------------------------ tables
def synthetic_tables(M):
    """Small deterministic tables, one per packing mode of pack_table (csrc/fp8approx.hip) that the
    built-in tables do not already give for every format."""
    n = 1 << M
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return {
        "zero": np.zeros((n, n), np.int32),                             # TM_NONE
        "s_w1u": ((i * 3 + j * 5 + 1) // 2 % 2).astype(np.int32),       # {0, 1}: TM_W1U
        "s_w2s": ((i + 2 * j) % 4 - 2).astype(np.int32),                # -2..1: TM_W2S1 (M <= 4) / TM_W2S2 (M = 5)
        "s_w2u": ((i + 2 * j + 3) % 4).astype(np.int32),                # 0..3: TM_W2U1 / TM_W2U2
        "s_lut": ((i * 5 + j * 3) % 8 - 3).astype(np.int32),            # -3..4: TM_LUT
    }


@functools.lru_cache(maxsize=None)
def tables(E, M):
    """name -> int32 [2^M][2^M]: the built-in v9 tables of the format, then the synthetic ones."""
    g2 = gio.load("g2_matmul.npz")
    out = {name: np.ascontiguousarray(g2[f"E{E}M{M}_table_{name}"], np.int32) for name in BUILTIN[(E, M)]}
    for name, tab in synthetic_tables(M).items():
        out.setdefault(name, tab)
    return out


@functools.lru_cache(maxsize=None)
def v5_tables(E, M):
    """name -> int32 table: the zero table and v5's compensation tables (g7_v5.npz)."""
    g7 = gio.load("g7_v5.npz")
    out = {"zero": np.zeros((1 << M, 1 << M), np.int32)}
    for d in V5_DNS[(E, M)]:
        out[f"d{d}"] = np.ascontiguousarray(g7[f"E{E}M{M}_table_d{d}"], np.int32)
    return out


def table_mode(table, M, approx=True):
    """pack_table's mode rule (csrc/fp8approx.hip), restated."""
    if not approx or table is None:
        return "TM_NONE"
    n = 1 << M
    lo, hi = min(0, int(table.min())), max(0, int(table.max()))
    if lo == 0 and hi == 0:
        return "TM_NONE"
    words2 = (n * 2 + 31) // 32
    if lo >= 0 and hi <= 1 and n <= 32:
        return "TM_W1U"
    if lo >= -2 and hi <= 1 and words2 <= 2:
        return "TM_W2S1" if words2 == 1 else "TM_W2S2"
    if lo >= 0 and hi <= 3 and words2 <= 2:
        return "TM_W2U1" if words2 == 1 else "TM_W2U2"
    return "TM_LUT"


def modes_of_width(M):
    """The packing modes that exist for mantissa width M (2-bit rows take one word up to M = 4, two at M = 5)."""
    one = (1 << M) * 2 <= 32
    return {"TM_NONE", "TM_W1U", "TM_W2S1" if one else "TM_W2S2", "TM_W2U1" if one else "TM_W2U2", "TM_LUT"}


def xm_table_form(table, M, approx=True):
    """xm_table_form (csrc/fp8approx.hip), restated: no negative entry and every
    (2^M + m_a)(2^M + m_b) - 2^M t >= 1.  With approx off the kernels see a zero table."""
    if not approx:
        return True
    n = 1 << M
    ma, mb = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return bool(table.min() >= 0 and ((n + ma) * (n + mb) - n * table).min() >= 1)


def expected_matmul_path(E, M, table, flags, K=1):
    """The path counter run_gemm advances (csrc/fp8approx.hip: f8_form, tt_form, tt16_form, v5mx_form) for a
    launch whose workspace holds the pre-decoded operands, with default options: the matrix-core and
    tile-table kernels only for s2n & qbma & !gclip (v5: only E5M2 with the adder wrap), else `fast`."""
    if flags & V5:
        return "v5mx" if M == 2 and flags & OFUF else "fast"
    approx = bool(flags & APPROX)
    if not (flags & S2N and flags & QBMA) or flags & GCLIP:
        return "fast"
    if (E, M) in ((4, 3), (5, 2)):
        return "f8mx" if xm_table_form(table, M, approx) else "fast"
    if M in (4, 5):
        neg = approx and bool(table.min() < 0)
        if M == 5 and neg:
            return "fast"
        return "tt16" if M == 4 and (neg or K >= 64) else "tt"
    return "fast"


# ------------------------------------------------------------------------------------------ cases
def flag_word(approx, s2n, qbma, gclip, tb=False):
    return (APPROX if approx else 0) | (S2N if s2n else 0) | (QBMA if qbma else 0) | (GCLIP if gclip else 0) | \
        (TB if tb else 0)


def v5_flag_word(ofuf, of, uf):
    return V5 | (OFUF if ofuf else 0) | (OF_OPT if of else 0) | (UF_OPT if uf else 0)


def v9_flag_words(first_table):
    """The 8 (s2n, qbma, gclip) combinations with approx on; with approx off (the table is irrelevant)
    only for a format's first table."""
    out = [flag_word(True, s, q, g) for s, q, g in itertools.product((True, False), repeat=3)]
    if first_table:
        out += [flag_word(False, s, q, g) for s, q, g in itertools.product((True, False), repeat=3)]
    return out


def tb_flag_words(first_table):
    """Per table approx on x s2n x qbma; for a format's first table also golden_clip_OF on, and approx off
    (the table is irrelevant) under all 8 combinations: all 16 flag combinations per triple."""
    out = [flag_word(True, s, q, False, tb=True) for s, q in itertools.product((True, False), repeat=2)]
    if first_table:
        out += [flag_word(True, s, q, True, tb=True) for s, q in itertools.product((True, False), repeat=2)]
        out += [flag_word(False, s, q, g, tb=True) for s, q, g in itertools.product((True, False), repeat=3)]
    return out


def v9_cases():
    for (E, M) in FORMATS:
        names = list(tables(E, M))
        for (bA, bB, bR) in V9_TRIPLES[(E, M)]:
            for name in names:
                for fl in v9_flag_words(name == names[0]):
                    yield dict(part="v9", E=E, M=M, bA=bA, bB=bB, bR=bR, table=name, flags=fl)


def tb_cases():
    """The reference picks the table itself (withComp, dnsmp_factor): the built-in tables only (E5M2: the
    zero table, handed to the reference's operator by the generator)."""
    for (E, M) in FORMATS:
        for (bA, bB, bR) in TB_TRIPLES[(E, M)]:
            for name in BUILTIN[(E, M)]:
                for fl in tb_flag_words(name == BUILTIN[(E, M)][0]):
                    yield dict(part="tb", E=E, M=M, bA=bA, bB=bB, bR=bR, table=name, flags=fl)


def v5_cases():
    for (E, M) in FORMATS:
        for b in v5_biases(E):
            for name in v5_tables(E, M):
                for sw in V5_FLAGS:
                    yield dict(part="v5", E=E, M=M, bA=b, bB=b, bR=b, table=name, flags=v5_flag_word(*sw))


def all_cases():
    return list(v9_cases()) + list(tb_cases()) + list(v5_cases())


def groups():
    """The cases grouped by everything but the flag word, in all_cases() order: dicts with the case's
    part, E, M, bA, bB, bR, table and `flags`, the list of the group's flag words."""
    out = []
    for c in all_cases():
        key = {k: v for k, v in c.items() if k != "flags"}
        if out and {k: v for k, v in out[-1].items() if k != "flags"} == key:
            out[-1]["flags"].append(c["flags"])
        else:
            out.append(dict(key, flags=[c["flags"]]))
    return out


def group_cases(g):
    return [dict(g, flags=fl) for fl in g["flags"]]


def group_digest(case_digests):
    """A group's recorded digest: SHA-256 over its cases' term digests (digest()), as hex text, concatenated
    in the order of the group's flag words -- every term bit of every case enters it."""
    return hashlib.sha256("".join(case_digests).encode()).hexdigest()


def case_id(c):
    return f"{c['part']}-E{c['E']}M{c['M']}-{c['bA']}_{c['bB']}_{c['bR']}-{c['table']}-f{c['flags']}"


def case_table(c):
    return (v5_tables if c["part"] == "v5" else tables)(c["E"], c["M"])[c["table"]]


def case_operands(c):
    """(a [256], b [256]) of a case."""
    return all_codes(c["E"], c["M"], c["bA"]), all_codes(c["E"], c["M"], c["bB"])


def digest(T):
    """SHA-256 of the terms' bits as little-endian uint32, every zero canonicalised to +0."""
    T = np.ascontiguousarray(T, np.float32).copy()
    T[T == 0] = 0.0
    return hashlib.sha256(T.view(np.uint32).astype("<u4").tobytes()).hexdigest()


def same_bits(got, ref):
    """The project's term rule: equal bits, zeros compared by value."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    return (got.view(np.uint32) == ref.view(np.uint32)) | ((got == 0) & (ref == 0))
