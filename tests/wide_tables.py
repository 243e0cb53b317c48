"""Error tables over the full int8 range, per format: the case list shared by the oracle-vs-reference pin
(tests/golden/gen_golden_wide.py, tests/test_wide_tables_cpu.py) and the kernel-vs-oracle tests
(tests/test_gpu_wide_tables.py).  Data and plain helpers only, on top of tests/pairs_cases.py.

With n = 2^M, s_a = n + m_a, s_b = n + m_b and an entry t, the reference's table value is
V = sig_a sig_b - t 2^-M = N / n^2 with N = s_a s_b - n t (approx_matmul_whole_v9.py:75-81, 182).  The
built-in and the synthetic tables of pairs_cases keep V inside about [0.75, 3.94]; every table here plants
one class of V outside it (TABLES: name -> the docstring line of its builder).
"""
import functools

import numpy as np

from tests import pairs_cases as pc

FORMATS = pc.FORMATS
NAMES = ("hi", "lowpos", "zero_v", "neg_small", "neg_big", "neg_sat", "mixed", "u8wrap")

# added to pairs_cases.V9_TRIPLES: E3M4 / E2M5 triples whose top products reach the result grid's top binade
# 2^(2^E - 1 - bR) and, with V >= 2 or a `hi` table's V >= 4, run beyond it (E4M3 (12, 12, 14) and E5M2
# (20, 20, 8) are such triples already); the flushed small products of the sign class occur in the triples
# with a low bR of every format ((9, 9, 2), (6, 9, 1), (4, 7, 1), (16, 16, 5)).
EXTRA_V9 = {(4, 3): [], (3, 4): [(6, 9, 9)], (2, 5): [(4, 7, 8)], (5, 2): []}


def v9_triples(E, M):
    return list(pc.V9_TRIPLES[(E, M)]) + EXTRA_V9[(E, M)]


# added to pairs_cases.TB_TRIPLES: E2M5 has one triple with every bias >= 2 there, the premise of the depthwise VALU
# form (conv_tb_fast_kernel; with a smaller bias conv_tb_direct_kernel recomputes the launch) -- a second one
EXTRA_TB = {(4, 3): [], (3, 4): [], (2, 5): [(2, 3, 4)], (5, 2): []}


def tb_triples(E, M):
    return list(pc.TB_TRIPLES[(E, M)]) + EXTRA_TB[(E, M)]


def _grid(M):
    n = 1 << M
    ma, mb = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return n, ma, mb, (n + ma) * (n + mb)


def numerators(table, M):
    """N = s_a s_b - n t per entry: V = N / n^2."""
    n, _, _, ss = _grid(M)
    return ss - n * np.asarray(table, np.int64)


def _sat(N, M):
    """|N|'s significand is at least 2 - 2^-(M+1): rounding to M mantissa bits would carry into the next
    binade where Q_R's pre-clamp (kb = 2 - 2^-M - 2^-22 times the binade) saturates instead."""
    a = np.abs(N).astype(np.int64)
    k = np.floor(np.log2(np.maximum(a, 1))).astype(np.int64)
    return (a > 0) & (a * 2 ** (M + 1) >= 2 ** (k + 1) * (2 ** (M + 1) - 1))


def hi(M):
    """hi: negative entries down to -128, V >= 4 at the large (m_a, m_b); V == 4 at (0, 0), V == 8 at (0, n/2)
    (M <= 4: with M = 5 the largest V is (63^2 + 32 * 128) / 1024 = 7.88)."""
    n, ma, mb, _ = _grid(M)
    t = -(16 + (ma * 7 + mb * 13) % 113)
    t[0, 0] = -3 * n
    if M <= 4:
        t[0, n // 2] = -(13 * n) // 2
    t[n - 1, n - 1] = -128
    return t.astype(np.int32)


def lowpos(M):
    """lowpos: non-negative entries, every N in 1 .. n, so 0 < V <= 2^-M < 1/2 on every pair, N == 1 at (1, 1)."""
    n, _, _, ss = _grid(M)
    return ((ss - 1) // n).astype(np.int32)


def zero_v(M):
    """zero_v: t = s_a s_b / n wherever that is whole (the first row and column, (0, 0) = n): V == 0 exactly;
    0 elsewhere."""
    n, _, _, ss = _grid(M)
    return np.where(ss % n == 0, ss // n, 0).astype(np.int32)


def neg_small(M):
    """neg_small: non-negative entries with V < 0 and |V| <= sig_a sig_b on every pair."""
    n, ma, mb, ss = _grid(M)
    return np.minimum(ss // n + 1 + (ma + 2 * mb) % max(n // 2, 1), 127).astype(np.int32)


def neg_big(M):
    """neg_big: non-negative entries up to 127 with V < -sig_a sig_b (n t > 2 s_a s_b) wherever t <= 127
    allows it ((0, 0) = 127); 0 elsewhere.  The golden product of a small pair is flushed, the approximate
    term survives: the reference then takes the sign +1, not s_a s_b."""
    n, ma, mb, ss = _grid(M)
    t = 2 * ss // n + 1 + (ma + mb) % 3
    t = np.where(2 * ss // n + 1 <= 127, np.minimum(t, 127), 0)
    t[0, 0] = 127
    return t.astype(np.int32)


def neg_sat(M):
    """neg_sat: per pair the smallest entry (0 .. 127) that makes V negative with a significand of at least
    2 - 2^-(M+1), strictly above kb = 2 - 2^-M - 2^-22: Q_R saturates |V|'s mantissa where plain rounding
    would carry; 0 where no entry does."""
    n, _, _, ss = _grid(M)
    t = np.zeros((n, n), np.int64)
    for cand in range(127, 0, -1):
        N = ss - n * cand
        t = np.where((N < 0) & _sat(N, M), cand, t)
    return t.astype(np.int32)


def mixed(M):
    """mixed: the six classes above and a narrow remainder interleaved in one signed table."""
    n, ma, mb, _ = _grid(M)
    parts = [hi(M), lowpos(M), zero_v(M), neg_small(M), neg_big(M), neg_sat(M), pc.synthetic_tables(M)["s_lut"]]
    sel = (ma * 3 + mb) % len(parts)
    return np.choose(sel, parts).astype(np.int32)


def u8wrap(M):
    """u8wrap: entries in 64 .. 127 and -128 .. -65 only: read back through uint8_t without the sign they
    would all be wrong."""
    n, ma, mb, _ = _grid(M)
    r = (ma * 5 + mb * 3) % 64
    return np.where((ma + mb) % 2 == 0, 64 + r, -128 + r).astype(np.int32)


_BUILDERS = dict(hi=hi, lowpos=lowpos, zero_v=zero_v, neg_small=neg_small, neg_big=neg_big, neg_sat=neg_sat,
                 mixed=mixed, u8wrap=u8wrap)
TABLES = {name: _BUILDERS[name].__doc__.split("\n")[0] for name in NAMES}


@functools.lru_cache(maxsize=None)
def tables(E, M):
    """name -> int32 [2^M][2^M], entries in -128 .. 127."""
    out = {name: np.ascontiguousarray(_BUILDERS[name](M), np.int32) for name in NAMES}
    assert all(t.min() >= -128 and t.max() <= 127 for t in out.values())
    return out


def class_mask(name, M):
    """bool [2^M][2^M]: the entries of tables(.., M)[name] that are in the class the table plants."""
    n, _, _, ss = _grid(M)
    t = tables(0, M)[name]
    N = numerators(t, M)
    if name == "hi":
        return N >= 4 * n * n
    if name == "lowpos":
        return (N > 0) & (2 * N < n * n)
    if name == "zero_v":
        return N == 0
    if name == "neg_small":
        return (N < 0) & (-N <= ss)
    if name == "neg_big":
        return -N > ss
    if name == "neg_sat":
        return (N < 0) & _sat(N, M)
    if name == "mixed":
        return (N >= 4 * n * n) | (2 * N < n * n)
    return (t >= 64) | (t <= -65)  # u8wrap


def narrow(table):
    """The table clipped to the -3 .. 4 of pairs_cases.synthetic_tables: what the older tests could cover."""
    return np.clip(table, -3, 4).astype(np.int32)


def code_fields(E, M):
    """(exponent field, mantissa field, sign) of pairs_cases.all_codes' 2^(E+M+1) values, in its order."""
    e = np.repeat(np.arange(1 << E), 1 << M)
    m = np.tile(np.arange(1 << M), 1 << E)
    return np.concatenate([e, e]), np.concatenate([m, m]), np.concatenate([np.ones(e.size), -np.ones(e.size)])


def pair_class(name, E, M):
    """bool [codes a][codes b]: both operands normal (exponent field >= 1, so the decoded mantissa is the
    code's own) and the pair's table entry in the table's class."""
    e, m, _ = code_fields(E, M)
    normal = e >= 1
    return normal[:, None] & normal[None, :] & class_mask(name, M)[m[:, None], m[None, :]]


# ------------------------------------------------------------------------------------------ cases
def v9_cases():
    for (E, M) in FORMATS:
        for tr in v9_triples(E, M):
            for name in NAMES:
                for fl in pc.v9_flag_words(False):
                    yield dict(part="v9", E=E, M=M, bA=tr[0], bB=tr[1], bR=tr[2], table=name, flags=fl)


def tb_cases():
    for (E, M) in FORMATS:
        for tr in tb_triples(E, M):
            for name in NAMES:
                for fl in pc.tb_flag_words(False):
                    yield dict(part="tb", E=E, M=M, bA=tr[0], bB=tr[1], bR=tr[2], table=name, flags=fl)


def all_cases():
    return list(v9_cases()) + list(tb_cases())


def groups():
    """The cases grouped by everything but the flag word, in all_cases() order (as pairs_cases.groups)."""
    out = []
    for c in all_cases():
        key = {k: v for k, v in c.items() if k != "flags"}
        if out and {k: v for k, v in out[-1].items() if k != "flags"} == key:
            out[-1]["flags"].append(c["flags"])
        else:
            out.append(dict(key, flags=[c["flags"]]))
    return out


def case_table(c):
    return tables(c["E"], c["M"])[c["table"]]


def oracle_terms(c, table=None):
    """oracle.terms of a case, float32 [codes a][codes b]."""
    from oracle import oracle as orc
    a, b = pc.case_operands(c)
    return orc.terms(a.reshape(-1, 1), b.reshape(1, -1), c["E"], c["M"], c["bA"], c["bB"], c["bR"],
                     case_table(c) if table is None else table, c["flags"])[:, 0, :]
