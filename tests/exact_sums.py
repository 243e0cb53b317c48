"""K > 1 sums that can be compared bit for bit: data and plain helpers shared by
tests/test_exact_sums_cpu.py and tests/test_gpu_exact_sums.py.  No GPU, no reference code.

Let T[m, k, n] be the oracle's per-product terms of a case (oracle.terms) and u = unit(T) the largest
power of two that divides every nonzero T.  If

    max over outputs of  sum_k |T|  <=  2^22 * u                                       (the budget)

every partial sum of the terms, in any order and any grouping, is an integer multiple of u below 2^22 u:
an exact float32.  The float32 sum is then the same for every summation order, equals
expected(T) = float32(sum_k float64(T)), and a kernel's result can be compared with it by bits
(pairs_cases.same_bits: zeros by value).  2^22 and not float32's 2^24: the two spare bits keep the condition
inside what was measured for the matrix core's own adder.  The budget is a condition on the
inputs, checked on the oracle's terms alone; a case that misses it fails (tests/test_exact_sums_cpu.py).

The operand generator places the operands' exponent codes so that the terms cover the delicate part of the
result quantizer Q_R: with per-product quantization (qbma) the product exponent e_a + e_b - bA - bB runs
from three binades below the flush point 2^(-bR - M) (half the subnormal quantum u = 2^(1 - bR - M)) through
the subnormal band up into the normal range, as far as the budget allows for the case's K; without it the
terms' unit is the product of the operands' own steps and the windows are a few binades per operand.

The non-square geometry cases (GEO_CONVS, GEO_TBDW, QAMAA_CONV, chain_cases; tests/test_gpu_conv_geometry.py) are
ordinary cases of this table whose (h, w) pairs differ; exchanged() / conv_output() serve the CPU file's proof that
each of them tells an exchanged pair.
"""
import functools
import math

import numpy as np

from tests import pairs_cases as pc

BUDGET_LOG2 = 22
SEED = 0  # of every draw; tests/test_exact_sums_cpu.py checks what the draws must hold


# ------------------------------------------------------------------------------------------ the rule
def unit(T):
    """The largest power of two that divides every nonzero element of T (a float32 / float64 array); 0.0
    if T has no nonzero element."""
    v = np.abs(np.asarray(T, np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return 0.0
    m, e = np.frexp(v)                               # v = m 2^e, m in [0.5, 1): m 2^53 is an integer
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)  # trailing zero bits of the significand
    return float(2.0 ** int((e - 53 + tz).min()))


def abs_sum(T, axis=1):
    return np.abs(np.asarray(T, np.float64)).sum(axis=axis)


def budget_log2(T, axis=1):
    """log2(max_outputs sum_k |T| / u): the case meets the budget iff this is <= 22 (-inf: no nonzero term)."""
    u = unit(T)
    if u == 0.0:
        return -math.inf
    return math.log2(float(abs_sum(T, axis).max()) / u)


def within_budget(T, axis=1):
    return budget_log2(T, axis) <= BUDGET_LOG2


def expected(T, axis=1):
    """float32(sum_k float64(T)): under the budget the float64 sum is exact and so is its cast."""
    return np.asarray(T, np.float64).sum(axis=axis).astype(np.float32)


def old_bar_in_units(T, axis=1):
    """What golden_io.sum_tolerance allowed per output, 1e-5 sum|T|, in units of u."""
    u = unit(T)
    return 1e-5 * abs_sum(T, axis) / u if u else np.zeros(np.asarray(T).shape[:axis] + np.asarray(T).shape[axis + 1:])


def mismatches(got, want):
    """Indices where got and want differ under the comparison rule (equal bits, zeros by value)."""
    return np.argwhere(~pc.same_bits(got, want))


def assert_same(got, want, what, T=None):
    """Bit equality; on failure names the first output and, given the terms, the difference in units."""
    bad = mismatches(got, want)
    if len(bad):
        i = tuple(int(v) for v in bad[0])
        extra = ""
        if T is not None:
            u = unit(T)
            diff = (float(np.asarray(got)[i]) - float(np.asarray(want)[i])) / u
            extra = f" (difference {diff:+g} u, u = 2^{math.log2(u):g})"
        raise AssertionError(f"{what}: {len(bad)} of {np.asarray(want).size} sums differ from the oracle; first at "
                             f"{i}: got {np.asarray(got)[i]!r} expected {np.asarray(want)[i]!r}{extra}")


# ------------------------------------------------------------------------------------------ shares
def shares(T, A, B, M, bR):
    """Among products of two nonzero operands: the shares of terms flushed to zero, in the subnormal band
    (0 < |T| < 2^(1 - bR): at most 2^M u) and normal, and the number of binades the nonzero terms occupy."""
    nz = (np.asarray(A)[:, :, None] != 0) & (np.asarray(B)[None, :, :] != 0)
    t = np.abs(np.asarray(T, np.float64))[nz]
    n = max(t.size, 1)
    band_top = 2.0 ** (1 - bR)
    nzt = t[t != 0]
    binades = np.unique(np.frexp(nzt)[1]).size if nzt.size else 0
    return dict(flushed=np.count_nonzero(t == 0) / n, band=np.count_nonzero((t != 0) & (t < band_top)) / n,
                normal=np.count_nonzero(t >= band_top) / n, binades=binades)


# ------------------------------------------------------------------------------------------ operands
def _clog2(k):
    return max(0, math.ceil(math.log2(max(1, k))))


def windows(E, M, bA, bB, bR, K, flags, spare=0):
    """Exponent-code windows (inclusive) of the operands: (a_lo, a_hi), and per column (b_lo[n], b_hi[n]).

    With qbma the product exponent P = e_a + e_b - bA - bB of two normal codes is to run from
    lo = -bR - M - 3 (three binades below the flush point) to hi = (1 - bR - M) + 19 - ceil(log2 K): a term is
    below 4 * 2^P, so K of them stay below 2^22 u.  Without qbma the unit is the product of the operands' own
    steps 2^(a_lo - M - bA) 2^(b_lo - M - bB); the terms then are below 4 * 2^(2M + wa + wb + spread of bB) u, which
    leaves wa + wb = 18 - 2M - ceil(log2 K) - spread code steps by that worst case.  The worst case is far from
    the draw (a term's mean is about a tenth of it: uniform codes, uniform mantissas), so at least one step per
    operand is kept; the CPU test decides.  Windows are cut to the codes the format has; code 0 stands for the
    subnormals (and zero).  The v5 model (one bias b) decodes r = e_a + e_b - b as an exponent code of the
    (E, M, b) grid: r runs from 1 to 18 - M - ceil(log2 K), so that K terms below 2^(r + 1 - b) stay below 2^22
    steps 2^(1 - b - M).  v5 cases are drawn from normal codes without zeros: a zero or an underflowing sum wraps
    (mod 2^M, floor division) to a term far from its neighbours, which spends the budget on one product; the
    every-code-pair tests pin those."""
    emax = (1 << E) - 1
    bB = np.asarray(bB, np.int64).reshape(-1)
    cl = _clog2(K) + spare  # (spare: bits of the budget a case keeps for an operand off the grid)
    spread = int(bB.max() - bB.min())
    if flags & pc.V5:
        b = int(bA)
        r_lo, r_hi = 1, min(emax, BUDGET_LOG2 - 4 - M - cl)
        t_lo, w = b + r_lo, r_hi - r_lo
        a_lo = max(1, min(t_lo // 2, emax))
        b_lo = max(1, min(t_lo - a_lo, emax))
        wa = min((w + 1) // 2, emax - a_lo)
        wb = min(w - wa, emax - b_lo)
        return (a_lo, a_lo + wa), (np.full(bB.shape, b_lo, np.int64), np.full(bB.shape, b_lo + wb, np.int64))
    if not flags & pc.QBMA:
        w = max(2, BUDGET_LOG2 - 4 - 2 * M - cl - spread)
        wa = min(w // 2, emax - 1)
        wb = min(w - wa, emax - 1)
        b_hi = np.full(bB.shape, emax, np.int64)
        return (emax - wa, emax), (b_hi - wb, b_hi)
    lo = -bR - M - 3
    hi = (1 - bR - M) + (BUDGET_LOG2 - 3) - cl
    if flags & pc.TB:  # no subnormal floor: Q_R rounds at the term's own binade, u = 2^(lowest binade - M); the
        lo = -bR - 3   # window straddles the expo-0 binade [2^-bR, 2^(1 - bR)) and the F7 interval above 2^-bR
        hi = lo + (BUDGET_LOG2 - 3) - cl - M - 2
    s_lo, s_hi = lo + bA + bB, hi + bA + bB           # sums of the two codes at the window's ends, per column
    span = hi - lo
    wa = min(max(span - 2, span // 2), emax)        # A takes all but two binades: P is then close to uniform
    a_lo = int(np.clip(int(s_lo.min()), 0, emax - wa))
    a_hi = a_lo + wa
    b_lo = np.clip(s_lo - a_lo, 0, emax)
    b_hi = np.clip(s_hi - a_hi, 0, emax)
    if np.any(b_lo > b_hi) or np.any(s_lo - a_lo > emax) or np.any(s_hi - a_hi < 0):
        raise ValueError(f"E{E}M{M} biases {bA, bB.min(), bB.max(), bR}: no exponent codes inside the window")
    return (a_lo, a_hi), (b_lo, b_hi)


def draw(rng, E, M, shape, bias, lo, hi, zero_frac):
    """On-grid values: exponent codes uniform (stratified) in [lo, hi] (broadcast), code 0 = subnormal with a
    mantissa whose bit length is uniform (small subnormals as likely as large ones), both signs, a share of zeros."""
    bias = np.broadcast_to(np.asarray(bias, np.int64), shape)
    lo = np.broadcast_to(np.asarray(lo, np.int64), shape)
    hi = np.broadcast_to(np.asarray(hi, np.int64), shape)
    n = int(np.prod(shape))
    strat = ((rng.permutation(n) + rng.random(n)) / n).reshape(shape)  # (stratified: small shapes cover the window)
    code = lo + (strat * (hi - lo + 1)).astype(np.int64)
    mant = rng.integers(0, 1 << M, size=shape)
    bits = rng.integers(1, M + 1, size=shape)
    sub = (rng.integers(0, 1 << 30, size=shape) % (1 << bits)) | (1 << (bits - 1))  # bit length `bits`: 1 .. 2^M - 1
    v = np.where(code == 0, np.ldexp(sub / 2.0 ** M, (1 - bias).astype(np.int32)),
                 np.ldexp(1.0 + mant / 2.0 ** M, (code - bias).astype(np.int32)))
    v = v * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(shape) < zero_frac] = 0.0
    return v.astype(np.float32)


def operands(E, M, bA, bB, bR, shape, flags, seed=0, zero_frac=0.1, spare=0):
    """(A [Mr, K], B [K, N]) on the grids of (E, M, bA) and (E, M, bB[n]), drawn inside windows()."""
    Mr, K, N = shape
    bB = np.broadcast_to(np.asarray(bB, np.int64).reshape(-1), (N,))
    (a_lo, a_hi), (b_lo, b_hi) = windows(E, M, bA, bB, bR, K, flags, spare)
    rng = np.random.default_rng([SEED + seed, E, M, Mr, K, N])  # (one draw per window: the flag sets share it)
    if flags & pc.V5:
        zero_frac = 0.0
    A = draw(rng, E, M, (Mr, K), bA, a_lo, a_hi, zero_frac)
    B = draw(rng, E, M, (K, N), bB[None, :], b_lo[None, :], b_hi[None, :], zero_frac)
    return A, B


def per_column_bias(base, N, spread, seed=0):
    """bB per column: base .. base + spread, every value present where N allows."""
    rng = np.random.default_rng([seed, N, spread])
    b = base + rng.integers(0, spread + 1, size=N)
    b[:min(N, spread + 1)] = base + np.arange(min(N, spread + 1))
    return b.astype(np.int32)


# ------------------------------------------------------------------------------------------ cases
# Bias triples (bA, first bB, spread of bB over the columns, bR) per format: the ones the kernels' own test
# files use for sums (E4M3: bA + min bB - bR >= 17, E5M2: >= 33 keep every term inside the scaled fp8 range;
# E3M4: inside gemm_tt16_kernel's f16 window), E2M5 with bR three higher so that a quarter of the terms is normal.
BIASES = {(4, 3): (10, 14, 2, 7), (5, 2): (20, 20, 2, 7), (3, 4): (7, 9, 2, 8), (2, 5): (5, 7, 1, 9)}
FL = pc.flag_word(True, True, True, False)           # the matrix-core / tile-table flag set
FL_FAST = pc.flag_word(True, False, True, True)      # one fast-kernel flag set with a band (qbma on)
MAT_SHAPES = [(1, 64, 1), (65, 17, 63), (257, 17, 5), (130, 300, 129)]
SPLITK_SHAPE = (64, 2304, 64)
V5_SWITCHES = [(False, False, False), (True, True, False), (True, True, True)]
V5_TABLE = {(4, 3): "d3", (3, 4): "d4", (2, 5): "d5", (5, 2): "zero"}


def one_table_per_mode():
    """(E, M, table name) per packing mode of pack_table: E4M3 gives the five one-word modes, E2M5 the two
    two-word ones."""
    out, seen = [], set()
    for (E, M) in ((4, 3), (2, 5)):
        for name, t in pc.tables(E, M).items():
            mode = pc.table_mode(t, M)
            if mode not in seen:
                seen.add(mode)
                out.append((E, M, name))
    return out


def _mat(fam, E, M, table, flags, shape, **kw):
    Mr, K, N = shape
    tag = kw.pop("tag", "")
    key = f"{fam}-E{E}M{M}-{table}-f{flags}-{Mr}x{K}x{N}" + ("-offgrid" if kw.get("offgrid") else "") + \
        ("-posA" if kw.get("posA") else "")
    cid = key + (f"-{tag}" if tag and tag != "offgrid" else "")
    return dict(kind="mat", id=cid, pkey=key, fam=fam, E=E, M=M, table=table, flags=flags, shape=shape, **kw)


def matmul_cases():
    """Matrix launches: per path of run_gemm the formats and tables the issue lists, at every shape."""
    out = []
    for shape in MAT_SHAPES:
        K = shape[1]
        out += [_mat("f8mx", 4, 3, "nocomp", FL, shape), _mat("f8mx", 4, 3, "zero", FL, shape),
                _mat("f8mx", 5, 2, "zero", FL, shape), _mat("tt", 2, 5, "nocomp", FL, shape),
                _mat("tt" if K < 64 else "tt16", 3, 4, "nocomp", FL, shape), _mat("tt16", 3, 4, "comp3", FL, shape)]
        for (E, M, name) in one_table_per_mode():
            for fl in pc.v9_flag_words(False):
                out.append(_mat("fast", E, M, name, fl, shape))
            out.append(_mat("fast", E, M, name, pc.flag_word(False, False, True, True), shape))
        out.append(_mat("v5mx", 5, 2, "zero", pc.v5_flag_word(True, False, False), shape))
        for (E, M) in ((4, 3), (3, 4), (2, 5)):
            for sw in V5_SWITCHES:
                out.append(_mat("v5fast", E, M, V5_TABLE[(E, M)], pc.v5_flag_word(*sw), shape))
    # one off-grid A value per family: the approx kernels mark its units and the exact kernel recomputes them; the
    # v5 kernels decode it to a code while staging, like the oracle (no fallback exists there)
    big = MAT_SHAPES[-1]
    out += [_mat("f8mx", 4, 3, "nocomp", FL, big, offgrid=True, tag="offgrid"),
            _mat("f8mx", 5, 2, "zero", FL, big, offgrid=True, tag="offgrid"),
            _mat("tt", 2, 5, "nocomp", FL, big, offgrid=True, tag="offgrid"),
            _mat("tt16", 3, 4, "nocomp", FL, big, offgrid=True, tag="offgrid"),
            _mat("fast", 4, 3, "nocomp", FL_FAST, big, offgrid=True, tag="offgrid"),
            _mat("v5mx", 5, 2, "zero", pc.v5_flag_word(True, False, False), big, offgrid=True, tag="offgrid"),
            _mat("v5fast", 4, 3, "d3", pc.v5_flag_word(True, True, True), big, offgrid=True, tag="offgrid")]
    return out


def splitk_cases():
    """(64, 2304, 64) with the split count forced; the in-launch sum (splitk_fixup) exists for gemm_f8mx only."""
    out = []
    for fam, E, M, fl in (("f8mx", 4, 3, FL), ("tt", 2, 5, FL), ("fast", 4, 3, FL_FAST)):
        for S in (2, 3, 6):
            for fix in ((0, 1) if fam == "f8mx" else (0,)):
                out.append(_mat(fam, E, M, "nocomp", fl, SPLITK_SHAPE, opts={"splitk": S, "splitk_fixup": fix},
                                tag=f"s{S}x{fix}", split=True))
    return out


# xm_wave_rows selects between the two 128 x 64 instances, which run only with xm_ncg = 4 (and xm_pipe = 1, the
# default): both are forced in one launch.  xm_sign_rows builds the positive-sign rows alone only when A holds no
# negative value: its two values run on the drawn A (both signs: the full build either way) and on |A|.
SCHEDULES = [{"xm_ncg": 1}, {"xm_ncg": 2}, {"xm_ncg": 4}, {"af32_maxct": 0}, {"af32_maxct": 64}, {"xm_pipe": 0},
             {"xm_pipe": 1}, {"xm_ncg": 4, "xm_wave_rows": 0}, {"xm_ncg": 4, "xm_wave_rows": 1},
             {"xm_sign_rows": 0}, {"xm_sign_rows": 1}]
SCHEDULES_POS = [{"xm_sign_rows": 0}, {"xm_sign_rows": 1}]
SCHED_CONV = dict(B=2, cin=16, cout=24, k=3, s=1, p=1, d=1, g=1, hw=12)
SCHED_CONV_1X1 = dict(B=2, cin=32, cout=24, k=1, s=1, p=0, d=1, g=1, hw=12)  # (A staged from fp32 needs a 1 x 1 conv)


def _opt_tag(o):
    return "_".join(f"{k}{v}" for k, v in o.items())


def schedule_cases():
    out = [_mat("f8mx", 4, 3, "nocomp", FL, MAT_SHAPES[-1], opts=o, tag=_opt_tag(o)) for o in SCHEDULES]
    out += [_mat("f8mx", 4, 3, "nocomp", FL, MAT_SHAPES[-1], opts=o, tag=_opt_tag(o), posA=True) for o in SCHEDULES_POS]
    out += [_conv("f8mx", 4, 3, "nocomp", FL, SCHED_CONV_1X1 if "af32_maxct" in o else SCHED_CONV, opts=o,
                  tag=_opt_tag(o)) for o in SCHEDULES]
    out += [_conv("f8mx", 4, 3, "nocomp", FL, SCHED_CONV, opts=o, tag=_opt_tag(o), posA=True) for o in SCHEDULES_POS]
    return out


def expected_sign_build(c):
    """fp8a_xm_sign_stats of one gemm_f8mx launch of a case: the half build only with xm_sign_rows on (the default)
    and no negative A value."""
    half = bool(c.get("posA")) and (c.get("opts") or {}).get("xm_sign_rows", 1) != 0
    return dict(half=int(half), full=int(not half))


# the geometries of tests/test_gpu_f8mx.py::test_conv_fast_path_matches_oracle with batch <= 2, <= 32 channels
CONVS = [
    dict(B=2, cin=3, cout=32, k=7, s=2, p=3, d=1, g=1, hw=30),     # conv1 class, K = 147
    dict(B=2, cin=16, cout=24, k=3, s=1, p=1, d=1, g=1, hw=13),    # ragged M (338), N (24)
    dict(B=2, cin=24, cout=32, k=3, s=2, p=2, d=2, g=1, hw=17),    # dilation
    dict(B=2, cin=32, cout=24, k=1, s=2, p=0, d=1, g=1, hw=15),    # 1x1 downsample class
    dict(B=2, cin=16, cout=32, k=3, s=1, p=1, d=1, g=2, hw=9),     # groups
    dict(B=1, cin=32, cout=32, k=3, s=1, p=1, d=1, g=1, hw=7),     # the deepest K (288)
    dict(B=2, cin=16, cout=24, k=3, s=2, p=1, d=1, g=1, hw=28),    # stride 2, H*W % 4 == 0
    dict(B=2, cin=24, cout=16, k=1, s=2, p=0, d=1, g=1, hw=16),    # 1x1 stride-2 downsample
    dict(B=2, cin=8, cout=20, k=3, s=2, p=2, d=2, g=2, hw=14),     # stride 2 + dilation + groups
    dict(B=2, cin=8, cout=20, k=3, s=2, p=2, d=2, g=2, hw=15),     # the same with H*W % 4 != 0
]


def _conv(fam, E, M, table, flags, cfg, **kw):
    tag = kw.pop("tag", "")
    geo = f"c{cfg['cin']}o{cfg['cout']}k{geo_tag(cfg['k'])}s{geo_tag(cfg['s'])}p{geo_tag(cfg['p'])}" \
          f"d{geo_tag(cfg['d'])}g{cfg['g']}hw{geo_tag(cfg['hw'])}"
    if "name" in cfg:                                   # (the geometry cases go by their names)
        geo = cfg["name"]
    key = f"conv-{fam}-E{E}M{M}-{table}-f{flags}-{geo}" + ("-posA" if kw.get("posA") else "") + \
        ("-offgrid" if kw.get("offgrid") else "")
    cid = key + (f"-{tag}" if tag else "")
    return dict(kind="conv", id=cid, pkey=key, fam=fam, E=E, M=M, table=table, flags=flags, cfg=cfg, **kw)


def conv_cases():
    out = []
    for cfg in CONVS:
        Kg = cfg["cin"] // cfg["g"] * cfg["k"] ** 2
        out += [_conv("f8mx", 4, 3, "nocomp", FL, cfg), _conv("tt" if Kg < 64 else "tt16", 3, 4, "nocomp", FL, cfg),
                _conv("tt", 2, 5, "nocomp", FL, cfg), _conv("fast", 4, 3, "nocomp", FL_FAST, cfg)]
    return out


# ------------------------------------------------------------------------------------------ non-square geometry
# Every other convolution case gives the approximate product one number per (h, w) pair.  Here no pair that can
# differ is equal by accident: H != W throughout, and per case the kernel, stride, padding or dilation differ in
# the direction the name says.  K <= 288 (the deepest case above), so the windows are those of the cases above.
def _geo(name, B, cin, H, W, cout, k, s, p, d, g):
    return dict(name=name, B=B, cin=cin, cout=cout, k=k, s=s, p=p, d=d, g=g, hw=(H, W))


GEO_CONVS = [
    _geo("h9w16", 2, 8, 9, 16, 24, (3, 3), (1, 1), (1, 1), (1, 1), 1),        # Ho != Wo, W % 4 == 0: widened left border
    _geo("h16w9", 2, 8, 16, 9, 24, (3, 3), (1, 1), (1, 1), (1, 1), 1),        # transposed: W % 4 != 0, H W % 4 == 0
    _geo("k1x7", 2, 6, 10, 12, 20, (1, 7), (1, 1), (0, 3), (1, 1), 1),        # ph = 0, pw = 3 widened
    _geo("k7x1", 2, 6, 12, 10, 20, (7, 1), (1, 1), (3, 0), (1, 1), 1),        # pw = 0, ph = 3
    _geo("dense-geo", 2, 16, 15, 17, 24, (3, 3), (2, 1), (1, 2), (1, 2), 1),  # the exact product's rectangular case
    _geo("dense-geo-t", 2, 16, 17, 15, 24, (3, 3), (1, 2), (2, 1), (2, 1), 1),
    _geo("k3x2-g2", 2, 8, 11, 13, 20, (3, 2), (1, 1), (1, 0), (1, 1), 2),     # even kw, groups, kh != kw
    _geo("pad-wide", 1, 4, 6, 12, 16, (3, 3), (1, 1), (3, 5), (1, 1), 1),     # pw > 4, W % 4 == 0; all-padding outputs
    _geo("k1-s2x1", 2, 32, 12, 15, 16, (1, 1), (2, 1), (0, 0), (1, 1), 1),    # the fp32-staged A form, sh != sw
    _geo("k1-padded", 2, 16, 7, 10, 24, (1, 1), (1, 1), (1, 0), (1, 1), 1),   # 1 x 1 that is not fp32-staged
    _geo("k2x4-s2x3", 2, 8, 13, 14, 24, (2, 4), (2, 3), (0, 1), (1, 1), 1),   # K = 64: E3M4 on gemm_tt16
]
GEO_WIDE = ("h9w16", "h16w9", "dense-geo", "dense-geo-t")  # the widest M (288, 288, 272, 272): the 128 x 64 store
GEO_WIDE_OPTS = [{"xm_ncg": 4, "xm_wave_rows": 0}, {"xm_ncg": 4, "xm_wave_rows": 1}]
# the v5 model on a padded convolution: with_UF_opt, as tbdw_cases (the padding's zeros are operands too)
FL_V5_GEO = pc.v5_flag_word(True, False, True)


def geo_conv_cases():
    """Per geometry one case per product family; gemm_f8mx's 128 x 64 instances on the widest M; the 1 x 1
    strided case a second time with the fp32 staging off (the pre-pass)."""
    out = []
    for cfg in GEO_CONVS:
        kh, kw = cfg["k"]
        Kg = cfg["cin"] // cfg["g"] * kh * kw
        out += [_conv("f8mx", 4, 3, "nocomp", FL, cfg), _conv("f8mx", 5, 2, "zero", FL, cfg),
                _conv("tt", 2, 5, "nocomp", FL, cfg), _conv("tt" if Kg < 64 else "tt16", 3, 4, "nocomp", FL, cfg),
                _conv("fast", 4, 3, "nocomp", FL_FAST, cfg), _conv("v5mx", 5, 2, "zero", FL_V5_GEO, cfg),
                _conv("v5fast", 4, 3, "d3", FL_V5_GEO, cfg)]
        if cfg["name"] in GEO_WIDE:
            out += [_conv("f8mx", 4, 3, "nocomp", FL, cfg, opts=o, tag=_opt_tag(o)) for o in GEO_WIDE_OPTS]
        if cfg["name"] == "k1-s2x1":
            out += [_conv("f8mx", 4, 3, "nocomp", FL, cfg, opts={"af32_maxct": 0}, tag="af32_maxct0"),
                    _conv("f8mx", 5, 2, "zero", FL, cfg, opts={"af32_maxct": 0}, tag="af32_maxct0")]
    return out


BAND_BIASES = (5, 7)   # E2M5: bA, bB of the constructed wave-tiles
BAND_SHAPE = (130, 12, 80)
BAND_SPOT = (70, 5, 37)  # (row, K position, column): second row half, second staged tile, not its first K-step


def band_cases():
    """gemm_tt_kernel's wave-tile forms (E2M5): every operand has exponent code 1 or 2, so every product is
    below 2^(6 - bA - bB); `band`: bR puts that at the grid's smallest normal 2^(1 - bR) and the one product of
    the two code-3 operands at BAND_SPOT sits exactly there; `zero`: bR puts it at half the quantum
    2^(-bR - M) and that product is the tie (`zero`) or one mantissa step above it (`zero1`)."""
    out = []
    for regime in ("band", "zero", "zero1"):
        for tb in (0, 1):
            for table in ("nocomp", "zero"):
                key = f"band-{regime}-{table}"
                out.append(dict(kind="band", id=f"{key}-tt_band{tb}", pkey=key, fam="tt", E=2, M=5, table=table,
                                flags=FL, regime=regime, opts={"tt_band": tb}, shape=BAND_SHAPE))
    return out


BMM_SHAPES = [(70, 64, 65), (65, 70, 64)]
BMM_FORMATS = [(4, 3, "nocomp"), (5, 2, "zero"), (3, 4, "nocomp")]   # LUT + conversion (twice), arithmetic


def bmm_cases():
    out = []
    for (E, M, name) in BMM_FORMATS:
        for shape in BMM_SHAPES:
            for off in (False, True):
                cid = f"bmm-E{E}M{M}-{name}-{'x'.join(map(str, shape))}" + ("-offgrid" if off else "")
                out.append(dict(kind="bmm", id=cid, pkey=cid, fam="bmm", E=E, M=M, table=name, flags=FL, shape=shape,
                                offgrid=off, items=3))
    return out


# ------------------------------------------------------------------------------------------ exact product, qamaa
DENSE_FORMS = {"bf16": (4, 3), "e4m3": (4, 3), "e5m2": (5, 2)}   # operand grid per dense form (tests/test_gpu_dense.py)
DENSE_SHAPES = [(7, 33, 5), (130, 300, 129)]
# test_gpu_dense.py's first geometry; one with K = 27 <= 32, N <= 64 (dn_direct_kernel)
DENSE_CONV = dict(B=2, cin=16, H=15, W=17, cout=24, k=3, stride=(2, 1), pad=(1, 2), dil=(1, 2))
DENSE_DIRECT = dict(B=2, cin=3, H=12, W=13, cout=32, k=3, stride=(1, 1), pad=(1, 1), dil=(1, 1))
DENSE_DW = dict(B=2, C=8, hw=9)


def dense_cases():
    """fp8a_dense_matmul / fp8a_dense_conv2d / fp8a_grouped_conv2d: the float64 product of on-grid operands, cast
    to float32.  The off-grid value 1 + 2^-8 (the fp32 units of dn_fix recompute its row) spends five more bits
    of the budget, not twenty; that case's windows are narrower by as much."""
    out = []
    for form, (E, M) in DENSE_FORMS.items():
        for shape in DENSE_SHAPES:
            cid = f"dense-{form}-{'x'.join(map(str, shape))}"
            out.append(dict(kind="dense", id=cid, pkey=cid, fam="dense", form=form, E=E, M=M, flags=0, shape=shape))
        cid = f"dense-{form}-130x300x129-offgrid"
        out.append(dict(kind="dense", id=cid, pkey=cid, fam="dense", form=form, E=E, M=M, flags=0,
                        shape=DENSE_SHAPES[1], offgrid=True))
        out.append(dict(kind="dconv", id=f"dense-{form}-conv", pkey=f"dense-{form}-conv", fam="dense", form=form, E=E,
                        M=M, flags=0, geo=DENSE_CONV, opts={}))
        for d in (0, 1):
            out.append(dict(kind="dconv", id=f"dense-{form}-conv-dn_direct{d}", pkey=f"dense-{form}-convk27",
                            fam="dense", form=form, E=E, M=M, flags=0, geo=DENSE_DIRECT, opts={"dn_direct": d}))
    for stride in (1, 2):
        for d in (0, 1, 2):
            out.append(dict(kind="ddw", id=f"dense-dw3x3-s{stride}-dw3_{d}", pkey=f"dense-dw3x3-s{stride}", fam="dense",
                            E=4, M=3, flags=0, stride=stride, opts={"dw3": d}))
    return out


QAMAA = dict(id="qamaa-E4M3-65x70x63", pkey="qamaa-E4M3-65x70x63", kind="qamaa", fam="qamaa", E=4, M=3, flags=0,
             shape=(65, 70, 63), maxval=2.5)


# fp8a_conv2d_qamaa on the k3x2-g2 geometry (even kw, groups, kh != kw): K = 24 per group
QAMAA_CONV = dict(id="qamaa-E4M3-conv-k3x2-g2", pkey="qamaa-E4M3-conv-k3x2-g2", kind="qconv", fam="qamaa", E=4, M=3,
                  flags=0, maxval=2.5, geo=_geo("k3x2-g2", 2, 8, 11, 13, 20, (3, 2), (1, 1), (1, 0), (1, 1), 2))


def _product_terms(A, B):
    return A.astype(np.float64)[:, :, None] * B.astype(np.float64)[None, :, :]


def _dense_operands(c, shape, seed, spare=0):
    E, M = c["E"], c["M"]
    bA, base, _, bR = BIASES[(E, M)]
    return operands(E, M, bA, np.full(shape[2], base, np.int32), bR, shape, 0, seed=seed, spare=spare) + (bA, base)


def _dense_image(c, xshape, wshape, K, seed):
    """x and w of an exact-product convolution, drawn directly inside the windows of a K-term sum."""
    E, M = c["E"], c["M"]
    bA, base, _, bR = BIASES[(E, M)]
    (a_lo, a_hi), (b_lo, b_hi) = windows(E, M, bA, [base], bR, K, 0)
    rng = np.random.default_rng([SEED + seed, E, M, K] + list(xshape))
    return (draw(rng, E, M, xshape, bA, a_lo, a_hi, 0.1), draw(rng, E, M, wshape, base, int(b_lo[0]), int(b_hi[0]), 0.1))


def _dense_problem(c):
    E, M = c["E"], c["M"]
    if c["kind"] == "dense":
        A, B, bA, _ = _dense_operands(c, c["shape"], 1, spare=5 if c.get("offgrid") else 0)
        if c.get("offgrid"):  # 1 + 2^-8: the shortest significand off bf16's grid too, five bits finer than E4M3's
            A[70, 5] = np.float32(np.ldexp(1.0 + 2.0 ** -8, (1 << E) - 1 - bA))
        return dict(A=A, B=B, parts=[(A, B, _product_terms(A, B), slice(None))])
    if c["kind"] == "dconv":
        g = c["geo"]
        K = g["cin"] * g["k"] ** 2
        x, w = _dense_image(c, (g["B"], g["cin"], g["H"], g["W"]), (g["cout"], g["cin"], g["k"], g["k"]), K, 2)
        import torch
        cols = torch.nn.functional.unfold(torch.from_numpy(x), (g["k"], g["k"]), dilation=g["dil"], padding=g["pad"],
                                          stride=g["stride"])
        cols = cols.transpose(1, 2).reshape(-1, K).numpy()
        Bm = np.ascontiguousarray(w.reshape(g["cout"], -1).T)
        return dict(x=x, w=w, parts=[(cols, Bm, _product_terms(cols, Bm), slice(None))])
    g = DENSE_DW                                         # depthwise 3 x 3, padding 1: one part per channel
    x, w = _dense_image(c, (g["B"], g["C"], g["hw"], g["hw"]), (g["C"], 1, 3, 3), 9, 3)
    cfg = dict(k=3, d=1, p=1, s=c["stride"])
    cols = unfold(x, cfg)                                # [B Ho Wo, C * 9]
    parts = []
    for ch in range(g["C"]):
        Ac = np.ascontiguousarray(cols[:, ch * 9:(ch + 1) * 9])
        Bc = np.ascontiguousarray(w[ch].reshape(1, 9).T)
        parts.append((Ac, Bc, _product_terms(Ac, Bc), slice(ch, ch + 1)))
    return dict(x=x, w=w, parts=parts)


def _qamaa_problem(c):
    """fq(sum_k fq(a b)): operands on a power-of-two-scaled 4-bit-significand grid, their products from four
    binades below the quantizer's subnormal step up to what the budget allows; the inner terms fq(a b) come from
    the oracle's quantizer (oracle.fp8_fake_quant)."""
    from oracle import oracle as orc
    E, M = c["E"], c["M"]
    Mr, K, N = c["shape"]
    _, bias = orc.fp8_fake_quant(np.ones(1, np.float32), c["maxval"], E, M)
    lu = 1 - int(bias[0]) - M                           # log2 of the quantizer's subnormal step
    lo, hi = lu - 4, lu + BUDGET_LOG2 - 3 - _clog2(K)
    rng = np.random.default_rng([SEED + 5, Mr, K, N])
    wa = (hi - lo) - 2
    A = draw(rng, 5, M, (Mr, K), 0, 8, 8 + wa, 0.1) * np.float32(2.0 ** (lo - 16))
    B = draw(rng, 5, M, (K, N), 0, 8, 10, 0.1)
    P = (A[:, :, None] * B[None, :, :]).astype(np.float32)   # exact: two 4-bit significands
    T, _ = orc.fp8_fake_quant(P.reshape(1, -1), c["maxval"], E, M)
    return dict(A=A.astype(np.float32), B=B, bR=int(bias[0]), parts=[(A, B, T.reshape(P.shape), slice(None))])


def _qamaa_operands(rng, M, lo, hi, xshape, wshape):
    """_qamaa_problem's operands: A over all but two binades of the window, B over three."""
    wa = (hi - lo) - 2
    A = draw(rng, 5, M, xshape, 0, 8, 8 + wa, 0.1) * np.float32(2.0 ** (lo - 16))
    return A.astype(np.float32), draw(rng, 5, M, wshape, 0, 8, 10, 0.1)


def _qconv_problem(c):
    """_qamaa_problem for the convolution entry point: x and w drawn as its A and B, one part per group."""
    from oracle import oracle as orc
    E, M, g = c["E"], c["M"], c["geo"]
    (H, W), (kh, kw) = g["hw"], g["k"]
    cig, cog = g["cin"] // g["g"], g["cout"] // g["g"]
    K = cig * kh * kw
    _, bias = orc.fp8_fake_quant(np.ones(1, np.float32), c["maxval"], E, M)
    lu = 1 - int(bias[0]) - M
    rng = np.random.default_rng([SEED + 19, g["cin"], g["cout"], H, W, kh, kw])
    x, w = _qamaa_operands(rng, M, lu - 4, lu + BUDGET_LOG2 - 3 - _clog2(K), (g["B"], g["cin"], H, W),
                           (g["cout"], cig, kh, kw))
    cols = unfold(x, g)
    parts = []
    for i in range(g["g"]):
        Ag = np.ascontiguousarray(cols[:, i * K:(i + 1) * K])
        Bg = np.ascontiguousarray(w[i * cog:(i + 1) * cog].reshape(cog, -1).T)
        P = (Ag[:, :, None] * Bg[None, :, :]).astype(np.float32)   # exact: two 4-bit significands
        T, _ = orc.fp8_fake_quant(P.reshape(1, -1), c["maxval"], E, M)
        parts.append((Ag, Bg, T.reshape(P.shape), slice(i * cog, (i + 1) * cog)))
    return dict(x=x, w=w, bR=int(bias[0]), parts=parts)


# ------------------------------------------------------------------------------------------ tensor-bias depthwise
FL_TB_DIRECT = pc.flag_word(True, False, True, False)   # s2n off: conv_tb_direct_kernel alone
TB_PLANES = [7, 9, 14]


def _tbdw(form, E, M, table, flags, hw, stride, opts):
    key = f"tbdw-E{E}M{M}-{table}-f{flags}-hw{hw}s{stride}"
    return dict(kind="tbdw", id=key + (f"-{_opt_tag(opts)}" if opts else ""), pkey=key, fam=form, E=E, M=M, table=table,
                flags=flags, hw=hw, stride=stride, opts=opts, C=8, B=2)


def tbdw_cases():
    """Depthwise 3 x 3 (single-output-channel groups: tensor-bias semantics), padding 1, all nine taps nonzero,
    8 channels with their own bW, planes whose width is and is not a multiple of 4.  The v5 form runs with the
    adder wrap and with_UF_opt: the padding's zeros are operands too, and without the underflow option their
    wrapped terms alone spend the budget (2^32 u)."""
    out = []
    for hw in TB_PLANES:
        for stride in (1, 2):
            for tbs in (0, 1, 2):
                for rw in (1, 2):
                    out.append(_tbdw("tbx", 4, 3, "nocomp", FL, hw, stride, {"tbs": tbs, "tbx_rw": rw}))
            out += [_tbdw("tb_fast", 3, 4, "nocomp", FL, hw, stride, {}),
                    _tbdw("tb_fast", 2, 5, "nocomp", FL, hw, stride, {}),
                    _tbdw("tb_direct", 4, 3, "nocomp", FL_TB_DIRECT, hw, stride, {})]
            for v in (0, 1):
                out.append(_tbdw("v5dw", 5, 2, "zero", pc.v5_flag_word(True, False, True), hw, stride, {"v5ds": v}))
    return out


def _tbgeo(name, B, cin, H, W, cout, g, k, s, p, d):
    return dict(name=name, B=B, cin=cin, cout=cout, g=g, hw=(H, W), k=k, s=s, p=p, d=d)


# Groups with one output channel (cout == groups) on non-square geometry: the branches of the tensor-bias kernels
# that the 3 x 3, padding-1, one-input-channel layers above never reach.
GEO_TBDW = [
    _tbgeo("dw-p0x1", 2, 12, 9, 14, 12, 12, (3, 3), 1, (0, 1), 1),        # ph != pw in all staged forms
    _tbgeo("dw-p1x0-s2", 2, 12, 14, 9, 12, 12, (3, 3), 2, (1, 0), 1),     # the same at stride 2, transposed
    _tbgeo("dw-p2x2", 2, 8, 7, 12, 8, 8, (3, 3), 1, (2, 2), 1),           # border wider than the kernel's reach
    _tbgeo("dw-p1x5", 1, 8, 6, 12, 8, 8, (3, 3), 1, (1, 5), 1),           # pw > 4: the staged forms' column guards
    _tbgeo("kh1", 2, 8, 8, 11, 8, 8, (1, 3), 1, (0, 1), 1),               # the general kh loop
    _tbgeo("kh5-s2", 2, 8, 13, 10, 8, 8, (5, 3), 2, (2, 1), 1),           # kh = 5; the two-row form's 2 + 5 rows
    _tbgeo("kh2-dh2", 2, 8, 10, 9, 8, 8, (2, 3), 1, (1, 1), (2, 1)),      # r * dh stepping; tbx_rw = 2 gives way
    _tbgeo("cig3-s1", 2, 12, 9, 10, 4, 4, (3, 3), 1, (1, 1), 1),          # the cpg loop, K = 27
    _tbgeo("cig3-s2", 2, 12, 9, 10, 4, 4, (3, 3), 2, (1, 1), 1),
    _tbgeo("kw2", 2, 8, 9, 11, 8, 8, (3, 2), 1, (1, 0), 1),               # no table form: conv_tb_fast_kernel
    _tbgeo("s2x1", 2, 8, 11, 9, 8, 8, (3, 3), (2, 1), (1, 1), 1),         # sh != sw: conv_tb_fast_kernel
]
TBX_OPTS = [{"tbs": tbs, "tbx_rw": rw} for tbs in (0, 1, 2) for rw in (1, 2)]


def _tbdw_geo(form, E, M, table, flags, geo, opts):
    key = f"tbdw-E{E}M{M}-{table}-f{flags}-{geo['name']}"
    return dict(kind="tbdw", id=key + (f"-{_opt_tag(opts)}" if opts else ""), pkey=key, fam=form, E=E, M=M, table=table,
                flags=flags, geo=geo, opts=opts, C=geo["cout"], B=geo["B"])


def geo_tbdw_cases():
    """Per geometry the option sets tbdw_cases sweeps, the table forms on E5M2 too."""
    out = []
    for geo in GEO_TBDW:
        out += [_tbdw_geo("tbx", 4, 3, "nocomp", FL, geo, o) for o in TBX_OPTS]
        out += [_tbdw_geo("tbx", 5, 2, "zero", FL, geo, o) for o in TBX_OPTS]
        out += [_tbdw_geo("tb_fast", 3, 4, "nocomp", FL, geo, {}), _tbdw_geo("tb_fast", 2, 5, "nocomp", FL, geo, {}),
                _tbdw_geo("tb_direct", 4, 3, "nocomp", FL_TB_DIRECT, geo, {})]
        out += [_tbdw_geo("v5dw", 5, 2, "zero", FL_V5_GEO, geo, {"v5ds": v}) for v in (0, 1)]
    return out


def v5dw_word_form(geo):
    """conv_v5_depthwise's rule for its word forms (else the literal kernel alone, counted as `exact`)."""
    (kh, kw), (sh, sw), (_, dw) = pair(geo["k"]), pair(geo["s"]), pair(geo["d"])
    return geo["cin"] == geo["g"] and kw == 3 and kh <= 5 and dw == 1 and sh == sw and sw in (1, 2)


def tbdw_geo(c):
    """The geometry of a tensor-bias case: its own (the geometry cases), or the depthwise 3 x 3, padding 1, on a
    square plane."""
    return c.get("geo") or dict(B=c["B"], cin=c["C"], cout=c["C"], g=c["C"], hw=c["hw"], k=3, s=c["stride"], p=1, d=1)


def _tbdw_problem(c):
    from oracle import oracle as orc
    E, M, fl, g = c["E"], c["M"], c["flags"], tbdw_geo(c)
    C, cig = g["cout"], g["cin"] // g["g"]
    (H, W), (kh, kw) = pair(g["hw"]), pair(g["k"])
    Kg = cig * kh * kw
    bA, bW, bR = case_biases(c, C)
    tfl = fl if fl & pc.V5 else fl | pc.TB
    (a_lo, a_hi), (b_lo, b_hi) = windows(E, M, bA, bW, bR, Kg, tfl)
    seed = [SEED + 13, E, M, c["hw"], c["stride"], int(fl)] if "geo" not in c else \
        [SEED + 17, E, M, g["cin"], C, H, W, kh, kw, *pair(g["s"]), *pair(g["p"]), *pair(g["d"]), int(fl)]
    rng = np.random.default_rng(seed)
    x = draw(rng, E, M, (g["B"], g["cin"], H, W), bA, a_lo, a_hi, 0.0 if fl & pc.V5 else 0.1)
    sh = (C, 1, 1, 1)
    w = draw(rng, E, M, (C, cig, kh, kw), bW.reshape(sh), b_lo.reshape(sh), b_hi.reshape(sh), 0.0)
    cols = unfold(x, g)
    tab = case_table(c)
    parts = []
    for ch in range(C):                                  # (one output channel per group: group ch)
        Ac = np.ascontiguousarray(cols[:, ch * Kg:(ch + 1) * Kg])
        Bc = np.ascontiguousarray(w[ch].reshape(1, Kg).T)
        parts.append((Ac, Bc, orc.terms(Ac, Bc, E, M, bA, bW[ch:ch + 1], bR, tab, tfl), slice(ch, ch + 1)))
    return dict(x=x, w=w, bA=bA, bB=bW, bR=bR, table=tab, parts=parts, flags=tfl)


CONV_OFFGRID_SPOT = (1, 3, 4, 7)   # (image, channel, row, column) of the off-grid input value


def conv_offgrid_cases():
    """h9w16 on gemm_f8mx with one off-grid input value: the producer whose gated exact kernel stores (and, chained,
    emits) the recomputed units (store_cases).  The oracle's terms quantize each product, so the budget holds as for
    the clean twin; tests/test_exact_sums_cpu.py proves it like every case's."""
    cfg = next(g for g in GEO_CONVS if g["name"] == "h9w16")
    return [_conv("f8mx", 4, 3, "nocomp", FL, cfg, offgrid=True), _conv("f8mx", 5, 2, "zero", FL, cfg, offgrid=True)]


def all_cases():
    return matmul_cases() + splitk_cases() + schedule_cases() + band_cases() + conv_cases() + bmm_cases() + \
        dense_cases() + [QAMAA] + tbdw_cases() + geo_conv_cases() + geo_tbdw_cases() + [QAMAA_CONV] + conv_offgrid_cases()


def geo_cases():
    return geo_conv_cases() + geo_tbdw_cases()


# ------------------------------------------------------------------------------------------ chained pairs
# fp8a_conv2d_chain on non-square geometry: the producer is one of the geometry cases above, so its output y is known
# by bits on the CPU; the consumer quantizes y itself (fused input quantizer, maxval `mx`) and its own terms are
# drawn inside the budget too (its weights' codes `wcodes`, its result bias `bR`), so that its output is compared by
# bits as well.  form: the words the producer emits (0 matrix core, 1 tensor-bias table form, 2 v5).
def _chain(name, E, M, producer, form, cout, k, p, g, mx, bW, bR, wcodes, flags=None):
    return dict(id=f"chain-{name}-E{E}M{M}", kind="chain", E=E, M=M, producer=producer, form=form, cout=cout, k=k, p=p,
                g=g, mx=mx, bW=bW, bR=bR, wcodes=wcodes, flags=FL if flags is None else flags)


def _geo_id(cases, name, E, M, fam):
    return next(c["id"] for c in cases if (c.get("cfg") or c["geo"])["name"] == name and (c["E"], c["M"]) == (E, M) and
                c["fam"] == fam and (c.get("opts") or {}) in ({}, {"tbs": 2, "tbx_rw": 2}, {"v5ds": 1}))


def chain_cases():
    conv, tb = geo_conv_cases(), geo_tbdw_cases()
    out = []
    for (E, M, bW, bR, wc) in ((4, 3, 14, 8, (4, 12)), (5, 2, 22, 10, (13, 21))):
        h9w16, dw = _geo_id(conv, "h9w16", E, M, "f8mx"), _geo_id(tb, "dw-p0x1", E, M, "tbx")
        out += [_chain("a-1x7", E, M, h9w16, 0, 20, (1, 7), (0, 3), 1, 5.5, bW, bR, wc),        # matrix-core consumer
                _chain("b-dw3x3", E, M, h9w16, 1, 24, (3, 3), (0, 1), 24, 5.5, bW, bR, (10, 12)),  # table-form consumer
                _chain("c-dw-1x1", E, M, dw, 0, 16, (1, 1), (0, 0), 1, 5.5, bW, bR, wc)]        # staged depthwise producer
    out.append(_chain("d-v5-1x1", 5, 2, _geo_id(tb, "dw-p0x1", 5, 2, "v5dw"), 2, 16, (1, 1), (0, 0), 1, 3.5, 20, 12,
                      (16, 24), flags=FL_V5_GEO))
    return out


def chain_problem(c):
    """The producer's problem and NCHW output, the consumer's geometry, weights, biases and its oracle terms on the
    oracle's quantizer of y."""
    from oracle import oracle as orc
    pc_ = CASES[c["producer"]]
    pp = problem_of.__wrapped__(pc_["pkey"])
    pg = pc_.get("cfg") or pc_["geo"]
    Ho, Wo = conv_out_hw(dict(pg, hw=pair(pg["hw"])))
    y = np.concatenate([expected(T) for (_, _, T, _) in pp["parts"]], axis=1)
    y = np.ascontiguousarray(y.reshape(pg["B"], Ho, Wo, pg["cout"]).transpose(0, 3, 1, 2))
    E, M = c["E"], c["M"]
    q, bias = orc.fp8_fake_quant(y, c["mx"], E, M)
    geo = dict(name=c["id"], B=pg["B"], cin=pg["cout"], cout=c["cout"], g=c["g"], hw=(Ho, Wo), k=c["k"], s=1, p=c["p"], d=1)
    cig, cog = geo["cin"] // geo["g"], geo["cout"] // geo["g"]
    rng = np.random.default_rng([SEED + 23, E, M, c["form"], c["cout"], *c["k"]])
    w = draw(rng, E, M, (c["cout"], cig) + tuple(c["k"]), c["bW"], c["wcodes"][0], c["wcodes"][1], 0.0)
    bW = np.full(c["cout"], c["bW"], np.int32)
    fl = c["flags"] | (pc.TB if cog == 1 and not c["flags"] & pc.V5 else 0)
    tab = case_table(pc_)
    cols = unfold(q, geo)
    Kg = cig * c["k"][0] * c["k"][1]
    parts = []
    for i in range(geo["g"]):
        sl = slice(i * cog, (i + 1) * cog)
        Ag = np.ascontiguousarray(cols[:, i * Kg:(i + 1) * Kg])
        Bg = np.ascontiguousarray(w[sl].reshape(cog, -1).T)
        parts.append((Ag, Bg, orc.terms(Ag, Bg, E, M, int(bias[0]), bW[sl], c["bR"], tab, fl), sl))
    return dict(producer=pp, pcase=pc_, pgeo=pg, y=y, q=q, geo=geo, w=w, bA=int(bias[0]), bB=bW, bR=c["bR"], table=tab,
                parts=parts, flags=fl)


def word_image_bytes(Bn, C, H, W, ph, pw):
    """The size the layout comment of csrc/fp8approx.hip gives: a 256-byte header, then [Bn][C][H + 2 ph][W'] words
    rounded up to 256 bytes; W' = W + 2 pw, or with 0 < pw <= 4 and W % 4 == 0 the left border widened to 4 and the row
    rounded up to a multiple of 4."""
    Wp = (W + 4 + pw + 3) // 4 * 4 if 0 < pw <= 4 and W % 4 == 0 else W + 2 * pw
    return 256 + (Bn * C * (H + 2 * ph) * Wp * 4 + 255) // 256 * 256


# ------------------------------------------------------------------------------------------ exchanged pairs
EXCHANGES = ("p", "s", "d", "k", "hw")   # ph <-> pw, sh <-> sw, dh <-> dw, transposed taps, transposed planes


def exchanged(geo, x, w, which):
    """(geometry, x, w) of the problem a kernel would compute if it took one (h, w) pair the wrong way round:
    the pair `which` of the geometry exchanged; for `k` the taps transposed with it, for `hw` the planes.  None if
    that is the same problem."""
    g = dict(geo)
    g[which] = pair(geo[which])[::-1]
    x2 = np.ascontiguousarray(np.swapaxes(x, 2, 3)) if which == "hw" else x
    w2 = np.ascontiguousarray(np.swapaxes(w, 2, 3)) if which == "k" else w
    same = g[which] == pair(geo[which]) and x2.shape == x.shape and w2.shape == w.shape and \
        np.array_equal(x2, x) and np.array_equal(w2, w)
    return None if same else (g, x2, w2)


def conv_output(geo, x, w, mm):
    """A convolution [B, Ho, Wo, cout] from the unfolded rows: mm(A [M, Kg], B [Kg, cog], channel slice) per group."""
    cols = unfold(x, geo)
    ng, cog = geo["g"], geo["cout"] // geo["g"]
    Kg = cols.shape[1] // ng
    out = np.empty((cols.shape[0], geo["cout"]), np.float32)
    for i in range(ng):
        sl = slice(i * cog, (i + 1) * cog)
        out[:, sl] = mm(np.ascontiguousarray(cols[:, i * Kg:(i + 1) * Kg]),
                        np.ascontiguousarray(w[sl].reshape(cog, -1).T), sl)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (pair(geo[f]) for f in ("k", "s", "p", "d"))
    H, W = x.shape[2], x.shape[3]
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return out.reshape(x.shape[0], Ho, Wo, geo["cout"])


# ------------------------------------------------------------------------------------------ problems
def case_table(c):
    return (pc.v5_tables if c["flags"] & pc.V5 else pc.tables)(c["E"], c["M"])[c["table"]]


def case_biases(c, N):
    """(bA, bB[N], bR); the v5 model has one bias."""
    E, M = c["E"], c["M"]
    if c["flags"] & pc.V5:
        b = pc.v5_biases(E)[1]
        return b, np.full(N, b, np.int32), b
    bA, base, spread, bR = BIASES[(E, M)]
    return bA, per_column_bias(base, N, spread), bR


def off_grid_value(bA, window):
    """A value with 24 significant bits, on no (E, M) grid, in the middle binade of A's exponent window."""
    return np.float32(np.ldexp(np.float32(1.2001), (window[0] + window[1]) // 2 - int(bA)))


def _mat_problem(c):
    E, M = c["E"], c["M"]
    Mr, K, N = c["shape"]
    bA, bB, bR = case_biases(c, N)
    A, B = operands(E, M, bA, bB, bR, c["shape"], c["flags"])
    spot = None
    if c.get("offgrid"):
        spot = (Mr // 2, K - 1)
        A[spot] = off_grid_value(bA, windows(E, M, bA, bB, bR, K, c["flags"])[0])
    if c.get("posA"):
        A = np.abs(A)
    return dict(A=A, B=B, bA=bA, bB=bB, bR=bR, spot=spot)


def _band_problem(c):
    E, M = c["E"], c["M"]
    Mr, K, N = c["shape"]
    bA, b = BAND_BIASES
    bB = np.full(N, b, np.int32)
    top = 6 - bA - b                                  # every product of two codes <= 2 is below 2^top
    bR = 1 - top if c["regime"] == "band" else -top - M
    rng = np.random.default_rng([7, Mr, K, N])
    A = draw(rng, E, M, (Mr, K), bA, 1, 2, 0.1)
    B = draw(rng, E, M, (K, N), b, 1, 2, 0.1)
    r, k, n = BAND_SPOT
    A[r, k] = np.ldexp(1.0 + (1 / 32 if c["regime"] == "zero1" else 0.0), 3 - bA)
    B[k, n] = np.ldexp(1.0, 3 - b)
    row = draw(rng, E, M, (N,), b, 1, 1, 0.0)         # the K-step's other columns: code 1, no zero
    row[n] = B[k, n]
    B[k] = row
    A[A[:, k] == 0, k] = np.ldexp(1.0, 1 - bA)
    return dict(A=A, B=B, bA=bA, bB=bB, bR=bR, spot=None)


def pair(v):
    """A geometry field as its (h, w) pair: an int stands for both."""
    return (int(v), int(v)) if np.ndim(v) == 0 else (int(v[0]), int(v[1]))


def geo_tag(v):
    """A geometry field in a case id: 3 for an int (or an equal pair given as an int), 1x7 for a pair."""
    return str(v) if np.ndim(v) == 0 else f"{v[0]}x{v[1]}"


def conv_out_hw(cfg):
    """(Ho, Wo) of a convolution case; one int where every field of the case is one."""
    (H, W), (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (pair(cfg[f]) for f in ("hw", "k", "s", "p", "d"))
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return Ho if all(np.ndim(cfg[f]) == 0 for f in ("hw", "k", "s", "p", "d")) else (Ho, Wo)


def unfold(x, cfg):
    """im2col of x [B, C, H, W] as rows [B * Ho * Wo, C * kh * kw] (torch.nn.functional.unfold's order); k, s, p,
    d of cfg: an int or an (h, w) pair."""
    import torch
    cols = torch.nn.functional.unfold(torch.from_numpy(np.ascontiguousarray(x)), pair(cfg["k"]),
                                      dilation=pair(cfg["d"]), padding=pair(cfg["p"]), stride=pair(cfg["s"]))
    return cols.transpose(1, 2).reshape(-1, cols.shape[1]).numpy()


def _conv_problem(c):
    E, M, cfg = c["E"], c["M"], c["cfg"]
    (H, W), (kh, kw) = pair(cfg["hw"]), pair(cfg["k"])
    cig, cout = cfg["cin"] // cfg["g"], cfg["cout"]
    K = cig * kh * kw
    bA, bW, bR = case_biases(c, cout)
    (a_lo, a_hi), (b_lo, b_hi) = windows(E, M, bA, bW, bR, K, c["flags"])
    seed = [11, E, M, cfg["cin"], cout, cfg["hw"], cfg["k"], int(c["flags"])]
    if np.ndim(cfg["hw"]) or np.ndim(cfg["k"]):  # (a pair-valued geometry: every field of it in the seed)
        seed = seed[:5] + [H, W, kh, kw, *pair(cfg["s"]), *pair(cfg["p"]), *pair(cfg["d"]), cfg["g"], int(c["flags"])]
    rng = np.random.default_rng(seed)
    zf = 0.0 if c["flags"] & pc.V5 else 0.1           # (v5: normal codes without zeros, see windows())
    x = draw(rng, E, M, (cfg["B"], cfg["cin"], H, W), bA, a_lo, a_hi, zf)
    sh = (cout, 1, 1, 1)
    w = draw(rng, E, M, (cout, cig, kh, kw), bW.reshape(sh), b_lo.reshape(sh), b_hi.reshape(sh), zf)
    if c.get("posA"):
        x = np.abs(x)
    if c.get("offgrid"):  # one value off the grid: the approx kernel marks its units, the exact kernel recomputes them
        x[CONV_OFFGRID_SPOT] = off_grid_value(bA, (a_lo, a_hi))
    return dict(x=x, w=w, bA=bA, bB=bW, bR=bR)


def _bmm_problem(c):
    E, M = c["E"], c["M"]
    Mr, K, N = c["shape"]
    bA, base, _, bR = BIASES[(E, M)]
    bB = np.full(N, base, np.int32)
    items = [operands(E, M, bA, bB, bR, c["shape"], c["flags"], seed=100 + z) for z in range(c["items"])]
    A = np.stack([a for a, _ in items])
    B = np.stack([b for _, b in items])
    spot = None
    if c["offgrid"]:
        spot = (1, 5, 3)
        A[spot] = off_grid_value(bA, windows(E, M, bA, bB, bR, K, c["flags"])[0])
    return dict(A=A, B=B, bA=bA, bB=bB, bR=bR, spot=spot)


def problem(cid):
    """problem_of(pkey) of a case: cases that differ only in options share one problem."""
    return problem_of(CASES[cid]["pkey"])


@functools.lru_cache(maxsize=6)
def problem_of(pkey):
    """The operands of a case (by id) with the oracle's terms: dict with bA, bB, bR, table and `parts`, a list of
    (A [Mr, K], B [K, N], T [Mr, K, N], output slice) -- one part per group of a convolution or batch item --
    plus the launch's own arrays (A / B, or x / w)."""
    from oracle import oracle as orc
    c = next(v for v in CASES.values() if v["pkey"] == pkey)
    if c["kind"] in ("dense", "dconv", "ddw"):
        return _dense_problem(c)
    if c["kind"] == "qamaa":
        return _qamaa_problem(c)
    if c["kind"] == "qconv":
        return _qconv_problem(c)
    if c["kind"] == "tbdw":
        return _tbdw_problem(c)
    E, M, tab, fl = c["E"], c["M"], case_table(c), c["flags"]
    if c["kind"] == "conv":
        p = _conv_problem(c)
        cfg = c["cfg"]
        cols = unfold(p["x"], cfg)
        g, cog = cfg["g"], cfg["cout"] // cfg["g"]
        Kg = cols.shape[1] // g
        p["parts"] = []
        for i in range(g):
            Ag = np.ascontiguousarray(cols[:, i * Kg:(i + 1) * Kg])
            Bg = np.ascontiguousarray(p["w"][i * cog:(i + 1) * cog].reshape(cog, -1).T)
            T = orc.terms(Ag, Bg, E, M, p["bA"], p["bB"][i * cog:(i + 1) * cog], p["bR"], tab, fl)
            p["parts"].append((Ag, Bg, T, slice(i * cog, (i + 1) * cog)))
    elif c["kind"] == "bmm":
        p = _bmm_problem(c)
        p["parts"] = [(a, b, orc.terms(a, b, E, M, p["bA"], p["bB"], p["bR"], tab, fl), z)
                      for z, (a, b) in enumerate(zip(p["A"], p["B"]))]
    else:
        p = _band_problem(c) if c["kind"] == "band" else _mat_problem(c)
        T = orc.terms(p["A"], p["B"], E, M, p["bA"], p["bB"], p["bR"], tab, fl)
        p["parts"] = [(p["A"], p["B"], T, slice(None))]
    p["table"] = tab
    return p


def case_terms(p):
    """All terms of a problem as one [outputs, K] view per part, for unit() and the budget: the unit is taken
    over the whole case."""
    return [T for (_, _, T, _) in p["parts"]]


def case_unit(p):
    us = [unit(T) for T in case_terms(p)]
    us = [u for u in us if u]
    return min(us) if us else 0.0


def case_budget_log2(p):
    u = case_unit(p)
    if not u:
        return -math.inf
    return math.log2(max(float(abs_sum(T).max()) for T in case_terms(p)) / u)


def case_old_bar(p):
    """(median, max) of the old tolerance 1e-5 sum|T| over the case's outputs, in units of u."""
    u = case_unit(p)
    bars = np.concatenate([(1e-5 * abs_sum(T) / u).ravel() for T in case_terms(p)]) if u else np.zeros(1)
    return float(np.median(bars)), float(bars.max())


def case_K(c):
    if c["kind"] == "conv":
        kh, kw = pair(c["cfg"]["k"])
        return c["cfg"]["cin"] // c["cfg"]["g"] * kh * kw
    if c["kind"] == "dconv":
        return c["geo"]["cin"] * c["geo"]["k"] ** 2
    if c["kind"] == "qconv" or (c["kind"] == "tbdw" and "geo" in c):
        kh, kw = pair(c["geo"]["k"])
        return c["geo"]["cin"] // c["geo"]["g"] * kh * kw
    if c["kind"] in ("ddw", "tbdw"):
        return 9
    return c["shape"][1]


CASES = {c["id"]: c for c in all_cases()}
assert len(CASES) == len(all_cases()), "case ids are not unique"


# ------------------------------------------------------------------------------------------ store cases
# The fused store on top of the cases above (tests/store_ref.py, tests/test_gpu_store_exact.py): the launch's
# accumulator is the proved exact sum of its base case, and the store parameters -- BN scale / shift, activation
# clamp, residual, output quantizer, the next convolution's quantizer and word image -- are drawn here, on the CPU,
# so that the values the store meets cover the classes its quantizers and clamps distinguish:
#   tie_dn / tie_up   exactly on a rounding tie of the first quantizer the value meets, the lower neighbour even / odd
#   max_p / max_n     exactly +maxval / -maxval;  over_p / over_n: one float32 step beyond
#   sub               in the quantizer's subnormal band;  tiny_p / tiny_n: below half its smallest step (rounds to zero)
#   lo / hi           the BN output exactly on the activation clamp's bounds
#   plo / phi         the value after the residual exactly on the post clamp's bounds
# Planting: a residual is free per element -- res = target - v where float32(v + res) is the target (checked; an
# element where it is not keeps its random residual); without a residual whole channels are planted: a power-of-two
# scale so small that float32(acc * scale + target) is the target for every accumulator of the channel (scale 0 for
# the target 0).  The other channels take random float32 scale and shift of both signs, normalised by the channel's
# own accumulator spread so that the activation clamps a share of the values at each bound.
# tests/test_store_ref_cpu.py proves the conditions on every case from the CPU model alone.
STORE_ACTS = {"none": (0, 0.0, 0.0), "relu6": (1, 0.0, 6.0), "hardtanh": (1, -0.5, 0.75)}
_ACT_DRAW = {"none": (1.0, 0.0), "relu6": (2.5, 3.0), "hardtanh": (0.5, 0.125)}   # spread and centre of the BN output
STORE_TAILS = ("res", "res_clamp_q", "relu_uq", "bias_res_q")     # (and res_q: residual + signed quantizer, no clamp)
CONV_TAILS = ("res", "res_clamp_q", "relu_uq", "res_q")
# activation quantizers (maxval, n_bits, mantissa bits, sign bits): the block's output quantizer, signed / unsigned
OUT_Q = {1: (3.0, 8, 3, 1), 0: (6.0, 8, 3, 0)}
# The post clamps lie strictly inside the quantizers' ranges, so that the clamp itself decides values: without it
# the quantizer's own clamp to maxval would give another result (tests/test_store_ref_cpu.py asserts that dropping
# the clamp changes the output).  +-maxval and the step beyond are then out of reach behind a clamp: res_q,
# bias_res_q and the emitting cases hold those classes.
POST_CLAMP = (-1.0, 1.25)                                 # res_clamp_q's clamp, inside OUT_Q[1]'s maxval 3
RELU_CLAMP = (0.0, 1.25)                                  # relu_uq's: a clipped ReLU, inside OUT_Q[0]'s maxval 6
RES_SD = 1.0                                              # spread of the random residual: both bounds are met
Q_LITERAL = (float(2.0 ** 70), 8, 3, 1)                   # maxval outside fq_fast_ok: the literal form under fq_fast = 1
Q_INVALID = (float(2.0 ** -70), 8, None, 1)               # next quantizer whose grid lies below the window 2^-62
NEXT_BR = {3: 8, 2: 10}                                   # the consumer's result bias per word format (chain_cases)
NEXT_MX = 5.5
CLASSES_Q = ("tie_dn", "tie_up", "max_p", "max_n", "over_p", "over_n", "sub", "tiny_p", "tiny_n")
CLASSES_CLAMP = ("plo", "phi")


def _st(base, tag, entry, bn="rand", act="none", tail=None, emit=None, opts=None, fq=None, site=None):
    """One store case.  entry: conv (approx_conv2d on the base case's x / w) or mat (approx_matmul_block on its A /
    B); bn: rand (random BN + planted channels) or None; tail: one of STORE_TAILS; emit: dict(form, S, pad) or None;
    fq: the output quantizer when it is not OUT_Q's; every tail case runs with fq_fast 0 and 1."""
    return dict(kind="store", id=f"st-{base}-{tag}", base=base, entry=entry, bn=bn, act=act, tail=tail, emit=emit,
                opts=opts or {}, fq=fq, site=site or CASES[base]["fam"])


def _geo_case(cases, name, E, M, fam, opts=None):
    return next(c["id"] for c in cases if (c.get("cfg") or c.get("geo") or {}).get("name") == name and
                (c["E"], c["M"]) == (E, M) and c["fam"] == fam and (c.get("opts") or {}) == (opts or {}))


def store_cases():
    """See the site table in tests/test_gpu_store_exact.py's docstring."""
    conv, tb = geo_conv_cases(), geo_tbdw_cases()
    out = []
    # -- the implicit-GEMM stores, NCHW: h9w16 (Ho Wo = 144: the 16-byte store; 288 rows and 24 channels: row and column
    # tails), k1-padded (90: the scalar store), k1-s2x1 (90, gemm_f8mx's fp32-staged A), k2x4-s2x3 (30, K = 64)
    fams = [("f8mx", 4, 3), ("f8mx", 5, 2), ("tt", 2, 5), ("fast", 4, 3), ("v5mx", 5, 2), ("v5fast", 4, 3)]
    for name in ("h9w16", "k1-padded"):
        for fam, E, M in fams + [("tt16" if name == "h9w16" else "tt", 3, 4)]:
            base = _geo_case(conv, name, E, M, fam)
            out += [_st(base, f"bn-{a}", "conv", act=a) for a in ("none", "relu6", "hardtanh")]
            out += [_st(base, t, "conv", act="none" if t != "res_clamp_q" else "hardtanh", tail=t) for t in CONV_TAILS]
    for name, fam, E, M in (("k1-s2x1", "f8mx", 4, 3), ("k1-s2x1", "f8mx", 5, 2), ("k2x4-s2x3", "tt16", 3, 4)):
        base = _geo_case(conv, name, E, M, fam)
        out += [_st(base, "bn-relu6", "conv", act="relu6"), _st(base, "res_clamp_q", "conv", tail="res_clamp_q")]
    # gemm_f8mx's tile shapes and wave orders (store_tile_xm per xm_ncg, xm_wave_rows)
    base = _geo_case(conv, "h9w16", 4, 3, "f8mx")
    for o in ({"xm_ncg": 1}, {"xm_ncg": 2}, {"xm_ncg": 4, "xm_wave_rows": 0}, {"xm_ncg": 4, "xm_wave_rows": 1}):
        out += [_st(base, f"bn-hardtanh-{_opt_tag(o)}", "conv", act="hardtanh", opts=o),
                _st(base, f"res_clamp_q-{_opt_tag(o)}", "conv", act="hardtanh", tail="res_clamp_q", opts=o)]
    out.append(_st(base, "res_q-literal", "conv", tail="res_q", fq=Q_LITERAL))
    # -- row-major stores (approx_matmul_block; ldc = N): 129 columns (ldc % 4 != 0, row and column tails), the
    # off-grid twins (the gated exact kernel's store of the recomputed units), split-K (N = ldc = 64: the vector
    # forms of the reduction and of the in-launch sum)
    big = MAT_SHAPES[-1]
    # (fp8a_matmul_block takes the int-bias v9 families only: the v5 stores run through the convolutions above)
    for fam, E, M in (("f8mx", 4, 3), ("f8mx", 5, 2), ("tt", 2, 5), ("tt16", 3, 4), ("fast", 4, 3)):
        for off in (False, True):
            cands = [c for c in matmul_cases() if c["fam"] == fam and (c["E"], c["M"]) == (E, M) and c["shape"] == big and
                     bool(c.get("offgrid")) == off and c["table"] != ("zero" if E == 4 else "comp3") and
                     (fam != "fast" or c["flags"] == FL_FAST)]
            base = cands[0]["id"]
            site = ("exact+" if off else "") + fam
            out.append(_st(base, "bn", "mat", site=site))
            out += [_st(base, t, "mat", bn="bias" if t == "bias_res_q" else "rand", tail=t, site=site)
                    for t in (STORE_TAILS if not off else ("res_clamp_q",))]
    sk_site = lambda fam, o: "splitk-" + fam + ("-fixup" if o["splitk_fixup"] else "")  # noqa: E731
    for c in splitk_cases():
        o = c["opts"]
        out.append(_st(c["id"], "bn", "mat", opts=o, site=sk_site(c["fam"], o)))
        out += [_st(c["id"], t, "mat", bn="bias" if t == "bias_res_q" else "rand", tail=t, opts=o,
                    site=sk_site(c["fam"], o)) for t in STORE_TAILS]
        if c["fam"] == "f8mx" and o == {"splitk": 2, "splitk_fixup": 1}:   # the in-launch sum on the narrow tile shapes
            for ncg in (1, 2):
                o2 = dict(o, xm_ncg=ncg)
                out += [_st(c["id"], f"bn-xm_ncg{ncg}", "mat", opts=o2, site=sk_site("f8mx", o)),
                        _st(c["id"], f"res_clamp_q-xm_ncg{ncg}", "mat", tail="res_clamp_q", opts=o2, site=sk_site("f8mx", o))]
    # split-K forced on cases that are not the split-K shape (an exact sum does not depend on its order): the scalar
    # forms of the reduction and of the in-launch sum on ldc = 129 and on the NCHW plane of 30 pixels (k2x4-s2x3,
    # K = 64), their NCHW vector forms on the plane of 144
    for S, fix in ((2, 0), (3, 0), (2, 1)):
        o = {"splitk": S, "splitk_fixup": fix}
        base = next(c["id"] for c in matmul_cases() if c["fam"] == "f8mx" and (c["E"], c["table"]) == (4, "nocomp") and
                    c["shape"] == big and not c.get("offgrid"))
        out += [_st(base, f"bn-{_opt_tag(o)}", "mat", opts=o, site=sk_site("f8mx", o)),
                _st(base, f"res_clamp_q-{_opt_tag(o)}", "mat", tail="res_clamp_q", opts=o, site=sk_site("f8mx", o))]
        for name in ("h9w16", "k2x4-s2x3"):   # (k1-padded has K = 16, one K chunk: it cannot split)
            for fam, E, M in (("f8mx", 4, 3), ("tt", 2, 5)) if fix == 0 else (("f8mx", 4, 3),):
                base = _geo_case(conv, name, E, M, fam)
                out += [_st(base, f"bn-relu6-{_opt_tag(o)}", "conv", act="relu6", opts=o, site=sk_site(fam, o)),
                        _st(base, f"res_clamp_q-{_opt_tag(o)}", "conv", act="hardtanh", tail="res_clamp_q", opts=o,
                            site=sk_site(fam, o))]
    # -- the depthwise stores: 3 x 3 planes of width 4 (hw 7, stride 2), 9 and 14, every option set of tbdw_cases
    for c in tbdw_cases():
        if (c["hw"], c["stride"]) in ((7, 2), (9, 1), (14, 1)):
            out += [_st(c["id"], f"bn-{a}", "conv", act=a, opts=c["opts"]) for a in ("none", "relu6")]
    # -- emission: gemm_f8mx's store and the staged depthwise producer, word forms 0 and 1, E4M3 and E5M2 words, the
    # next quantizer signed and unsigned, next padding (0, 0), (1, 1), (0, 3), Wo = 16 and Wo = 10
    for (E, M) in ((4, 3), (5, 2)):
        for name in ("h9w16", "k1-padded"):
            base = _geo_case(conv, name, E, M, "f8mx")
            for S in (1, 0):
                for pad in ((0, 0), (1, 1), (0, 3)):
                    out.append(_st(base, f"emit0-s{S}-p{pad[0]}x{pad[1]}", "conv", act="relu6" if S == 0 else "none",
                                   emit=dict(form=0, S=S, pad=pad)))
                out.append(_st(base, f"emit1-s{S}", "conv", act="relu6" if S == 0 else "none", emit=dict(form=1, S=S, pad=(0, 1))))
            out.append(_st(base, "emit0-tail", "conv", act="hardtanh", tail="res_clamp_q", emit=dict(form=0, S=1, pad=(1, 1))))
            if E == 4:   # the split-K reduction and the in-launch sum emit instead of the store
                sbase = base if name == "h9w16" else _geo_case(conv, "k2x4-s2x3", E, M, "f8mx")   # (Wo = 16 / Wo = 5)
                for fix in (0, 1):
                    o = {"splitk": 2, "splitk_fixup": fix}
                    out += [_st(sbase, f"emit0-s1-p1x1-{_opt_tag(o)}", "conv", emit=dict(form=0, S=1, pad=(1, 1)), opts=o,
                                site=sk_site("f8mx", o)),
                            _st(sbase, f"emit1-s0-{_opt_tag(o)}", "conv", act="relu6", emit=dict(form=1, S=0, pad=(0, 1)),
                                opts=o, site=sk_site("f8mx", o))]
            out.append(_st(base, "emit0-invalid", "conv", emit=dict(form=0, S=1, pad=(1, 1), q=Q_INVALID)))
        # the gated exact kernel: an off-grid input value in the producer; the recomputed units are stored and emitted
        off = next(c["id"] for c in conv_offgrid_cases() if (c["E"], c["M"]) == (E, M))
        out += [_st(off, "bn-relu6", "conv", act="relu6", site="exact+f8mx"),
                _st(off, "res_clamp_q", "conv", act="hardtanh", tail="res_clamp_q", site="exact+f8mx"),
                _st(off, "emit0-s1-p1x1", "conv", emit=dict(form=0, S=1, pad=(1, 1)), site="exact+f8mx"),
                _st(off, "emit0-s0-p0x3", "conv", act="relu6", emit=dict(form=0, S=0, pad=(0, 3)), site="exact+f8mx"),
                _st(off, "emit1-s1", "conv", emit=dict(form=1, S=1, pad=(0, 1)), site="exact+f8mx")]
        # the staged depthwise producer: Wo = 14 (dw-p0x1) and Wo = 20 (dw-p1x5)
        for name in ("dw-p0x1", "dw-p1x5"):
            dw = _geo_case(tb, name, E, M, "tbx", {"tbs": 2, "tbx_rw": 2})
            out += [_st(dw, f"emit0-s{S}-p{pad[0]}x{pad[1]}", "conv", act="relu6" if S == 0 else "none",
                        emit=dict(form=0, S=S, pad=pad), opts={"tbs": 2, "tbx_rw": 2}, site="tbx-emit")
                    for S, pad in ((1, (0, 0)), (0, (0, 0)), (1, (1, 1)), (0, (0, 3)))]
    return out


def store_acc(c):
    """The base case's exact accumulator as the launch lays it out: [Mr, N] (mat) or NCHW (conv)."""
    b = CASES[c["base"]]
    p = problem_of(b["pkey"])
    rows = None
    for (_, _, T, sl) in p["parts"]:
        e = expected(T)
        if rows is None:
            ncol = e.shape[1] if sl == slice(None) else (b.get("cfg") or tbdw_geo(b))["cout"]
            rows = np.zeros((e.shape[0], ncol), np.float32)
        rows[:, sl] = e
    if c["entry"] == "mat":
        return p, rows
    g = b.get("cfg") or tbdw_geo(b)
    Ho, Wo = conv_out_hw(dict(g, hw=pair(g["hw"]), k=pair(g["k"])))
    return p, np.ascontiguousarray(rows.reshape(g["B"], Ho, Wo, rows.shape[1]).transpose(0, 3, 1, 2))


def _q_targets(fq):
    """One value per class of CLASSES_Q for the quantizer fq (its ties in the binade [0.25, 0.5), inside every
    activation clamp used here)."""
    from tests import store_ref as sr
    mx, nb, M, S = fq
    bias = sr.fq_bias(mx, nb, M, S)
    step = 2.0 ** (1 - bias - M)
    f = np.float32
    t = dict(tie_dn=0.25 * (2 ** M + 2.5) / 2 ** M, tie_up=0.25 * (2 ** M + 1.5) / 2 ** M, max_p=mx, max_n=-mx,
             over_p=np.nextafter(f(mx), f(np.inf)), over_n=np.nextafter(f(-mx), f(-np.inf)), sub=3 * step,
             tiny_p=0.25 * step, tiny_n=-0.25 * step)     # (powers of two: a residual reaches them exactly)
    return {k: f(v) for k, v in t.items()}


def store_classes(xin, fq):
    """How many elements of xin (the values entering the quantizer fq, before its clamp) fall in each class."""
    from tests import store_ref as sr
    mx, nb, M, S = fq
    bias = sr.fq_bias(mx, nb, M, S)
    x = np.asarray(xin, np.float32)
    xc = np.minimum(np.maximum(x, np.float32(-mx if S else 0.0)), np.float32(mx)).astype(np.float64)
    _, e = np.frexp(xc)
    k = (np.where(xc == 0, 1.0, np.maximum(e - 1 + bias, 1.0)) - M - bias).astype(np.int32)
    t = np.abs(np.ldexp(xc, -k))
    tie = (t - np.floor(t)) == 0.5
    half = 2.0 ** (-bias - M)
    f = np.float32
    return dict(tie_dn=int((tie & (np.floor(t) % 2 == 0)).sum()), tie_up=int((tie & (np.floor(t) % 2 == 1)).sum()),
                max_p=int((x == f(mx)).sum()), max_n=int((x == f(-mx)).sum()),
                over_p=int((x == np.nextafter(f(mx), f(np.inf))).sum()),
                over_n=int((x == np.nextafter(f(-mx), f(-np.inf))).sum()),
                sub=int(((np.abs(xc) >= half) & (np.abs(xc) < 2.0 ** (1 - bias))).sum()),
                tiny_p=int(((x > 0) & (x < half)).sum()), tiny_n=int(((x < 0) & (x > -half)).sum()))


def clamp_classes(xin, lo, hi):
    """Values entering the post clamp exactly on its bounds, and the shares it cuts at each."""
    x = np.asarray(xin, np.float32)
    return dict(plo=int((x == np.float32(lo)).sum()), phi=int((x == np.float32(hi)).sum()),
                below=float(np.mean(x < np.float32(lo))), above=float(np.mean(x > np.float32(hi))))


@functools.lru_cache(maxsize=4)
def store_problem(cid):
    """Everything a store case's launch takes and everything the CPU model says it writes: dict with the base
    problem `p`, acc, ss (scale_shift [C, 2] or None), act (act, lo, hi), res, post (post_act, lo, hi, quantizer or
    None), nextq / bR_next / Mw / form / pad (emission), bn_out (after BN + activation), y (final), obias, neg_zero
    (where y's zero has a defined sign), xin / q_first (the values entering the first quantizer, and it), and for an
    emitting case words / ok / header / img (store_ref.image)."""
    import zlib
    from tests import store_ref as sr
    c = STORE_CASES[cid]
    b = CASES[c["base"]]
    p, acc = store_acc(c)
    rng = np.random.default_rng([SEED + 31, zlib.crc32(cid.encode())])
    C = acc.shape[1]
    act, alo, ahi = STORE_ACTS[c["act"]]
    tail, em = c["tail"], c["emit"]
    post_q = None
    if tail in ("res_clamp_q", "bias_res_q", "res_q"):
        post_q = c["fq"] or OUT_Q[1]
    elif tail == "relu_uq":
        post_q = OUT_Q[0]
    Mw = b["M"]
    nextq = None
    if em:
        nextq = em.get("q") or (NEXT_MX, 8, Mw, em["S"])
        nextq = (nextq[0], nextq[1], Mw, nextq[3])
    q_first = post_q or nextq
    has_res = tail in ("res", "res_clamp_q", "bias_res_q", "res_q")
    post = (0, 0.0, 0.0)
    if tail == "res_clamp_q":
        post = (1,) + POST_CLAMP
    elif tail == "relu_uq":
        post = (1,) + RELU_CLAMP
    # what lies between the BN output and the first quantizer: the clamps a planted value must pass
    # (a residual comes after the activation: then the post clamp alone bounds what reaches the quantizer)
    lo = max(alo if act and not has_res else -np.inf, post[1] if post[0] else -np.inf)
    hi = min(ahi if act and not has_res else np.inf, post[2] if post[0] else np.inf)
    qt = {k: v for k, v in _q_targets(q_first).items() if lo <= float(v) <= hi} if q_first and q_first[0] < 2.0 ** 64 \
        and q_first[0] > 2.0 ** -62 else {}
    if post[0]:
        qt.update(plo=np.float32(post[1]), phi=np.float32(post[2]))
    # ---- BN
    ss = None
    chan_targets = {}
    if c["bn"] == "bias":
        ss = np.stack([np.ones(C, np.float32), rng.normal(0, 0.5, C).astype(np.float32)], axis=1)
    elif c["bn"] == "rand":
        a = np.moveaxis(acc, 1, 0).reshape(C, -1).astype(np.float64)
        spread = np.sqrt((a ** 2).mean(axis=1))
        spread[spread == 0] = 1.0
        sd, mid = _ACT_DRAW[c["act"]]
        sign = rng.choice([-1.0, 1.0], C)
        sign[:2] = (1.0, -1.0)
        ss = np.stack([(sign * rng.uniform(0.7, 1.3, C) * sd / spread).astype(np.float32),
                       (mid + rng.normal(0, 0.3 * sd, C)).astype(np.float32)], axis=1)
        # planted channels: the quantizer's classes first, then the clamp's bounds; at even indices (two planted
        # channels are never neighbours: max_p and over_p end in the same value) and never the last channel; at most
        # half of the channels, a third where there are fewer than 16
        plant = ([] if has_res else list(qt.items())) + ([("lo", np.float32(alo)), ("hi", np.float32(ahi))] if act else [])
        plant = plant[:C // 2 if C >= 16 else C // 3]
        chans = rng.permutation(np.arange(0, C - 1, 2))[:len(plant)]
        plant = plant[:len(chans)]
        for ch, (name, t) in zip(chans, plant):
            amax = float(np.abs(a[ch]).max()) or 1.0
            j = max(-120, int(np.floor(np.log2(abs(float(t)) * 2.0 ** -30 / amax)))) if t != 0 else None
            ss[ch] = (np.float32(0.0) if j is None else np.float32(2.0 ** j), t)
            chan_targets[int(ch)] = name
    bn_raw = sr.bn_act(acc, ss, 0, 0.0, 0.0, 1) if ss is not None else acc
    bn_out = sr.bn_act(acc, ss, act, alo, ahi, 1) if ss is not None else acc
    # ---- residual
    res = None
    if has_res:
        # (Q_LITERAL's grid has the step 2^52: its residual alone reaches it, far above the BN output)
        res = (rng.normal(0, RES_SD, acc.shape) * (2.0 ** 58 if post_q and post_q[0] > 2.0 ** 64 else 1.0)).astype(np.float32)
        if qt:  # per class a share of the elements: res = target - v, or its float32 neighbour, where v + res is the target
            flat = rng.permutation(acc.size)[:acc.size // 3]
            rr, vv = res.reshape(-1), bn_out.reshape(-1)
            for i, (name, t) in enumerate(qt.items()):
                idx = flat[i::len(qt)][:200]
                v = vv[idx]
                r0 = (np.float64(t) - v.astype(np.float64)).astype(np.float32)
                for r in (r0, np.nextafter(r0, np.float32(np.inf)), np.nextafter(r0, np.float32(-np.inf))):
                    hit = ((v + r).astype(np.float32) == t) & (rr[idx] != r)
                    hit &= ~np.isin(idx, idx[(v + rr[idx]).astype(np.float32) == t])
                    rr[idx[hit]] = r[hit]
    y, obias = sr.tail(bn_out, res, post[0], post[1], post[2], post_q)
    xpre = (bn_out + res).astype(np.float32) if has_res else bn_out       # what enters the post clamp
    xin = y if not post_q else sr.tail(bn_out, res, post[0], post[1], post[2], None)[0]   # ... the first quantizer
    neg_zero = sr.signed_zero(xin, *post_q) if post_q else None
    out = dict(case=c, base=b, p=p, acc=acc, ss=ss, act=(act, alo, ahi), res=res, post=post + (post_q,), nextq=nextq,
               bn_raw=bn_raw, bn_out=bn_out, y=y, obias=obias, neg_zero=neg_zero, xin=xin, xpre=xpre, q_first=q_first,
               chan_targets=chan_targets,
               required=[k for k in CLASSES_Q + CLASSES_CLAMP if k in qt and (has_res or k in chan_targets.values())],
               q_clamp=(post[1], post[2]) if post[0] else None)
    if em:
        out.update(bR_next=NEXT_BR[Mw], Mw=Mw, form=em["form"], pad=em["pad"])
        w, ok, header = sr.words(y, nextq, NEXT_BR[Mw], Mw, em["form"])
        ipad = (0, 0) if em["form"] == 1 else em["pad"]
        out.update(words=w, ok=ok, header=header, img=sr.image(acc.shape[0], C, acc.shape[2], acc.shape[3], *ipad))
    return out


STORE_CASES = {c["id"]: c for c in store_cases()}
assert len(STORE_CASES) == len(store_cases()), "store case ids are not unique"
