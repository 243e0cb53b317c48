"""The two tiled reductions past one tile per workgroup: the batch statistics (csrc/bn_train.h) and the MSE candidate
search (csrc/fq_mse.h).  Pure numpy; shared by tests/test_reduce_plan_cpu.py and tests/test_gpu_reduce_partitions.py.

Both kernels split a channel (row) of `tiles` tiles over parts = min(tiles, ceil(TARGET_WGS / groups)) workgroups,
workgroup p walking tiles [p tiles / parts, (p + 1) tiles / parts).  Every shape of tests/test_gpu_bn_train.py and
tests/test_gpu_mse.py has parts == tiles: one tile per workgroup.  The cases below have parts < tiles, with the
shipped constants -- which are read from the headers here, so a changed constant moves the plan with it and the
CPU file says which claim of a case no longer holds.

What is here:
  constants     BN_TILE, BN_LIN_TILE, BN_LIN_INNER, BN_TARGET_WGS, MSE_TILE, MSE_TARGET_WGS from the headers, the
                apply kernel's grid cap from k_bn.hip.
  plans         bn_plan / mse_plan: the host's bn_parts / bn_lin / mse_parts and the [t0, t1) split, restated.
  cases         BN_CASES / MSE_CASES with what each claims to reach (`expect`), inputs from fixed seeds, the float64
                reference of the BN cases (computed in channel chunks) with the bars of tests/test_gpu_bn_train.py
                (S1 / S2: dm, dv, ds, dsh; restated in numpy, pinned to that file's case() by the CPU file).
  models        the sums as the plan partitions them, in float64 -- per (part, tile, element) index set -- and the
                mutants: what a kernel with one index error in it would return.

Mutants (MUTANTS; mutant_applies says which case can show which):
  t1_floor       t1 = t0 + tiles // parts: the remainder tiles are never walked         (tiles % parts != 0)
  tile_twice     every part also takes the tile before its t0: boundary tiles twice     (parts > 1)
  tail_short     the ragged last tile loses its last element                            (a ragged last tile)
  no_wrap        BN: the offset inside a tile ignores the image wrap (di = 0), so the values past an image's end
                 come from the neighbouring channel                                     (a boundary inside a tile)
  row_base       MSE: the row's base is r tiles MSE_TILE instead of r inner             (rows > 1, a ragged tile)
  lin_unclamped  BN lin form: j1 = t1 BN_LIN_TILE is not clamped to n                   (lin, a ragged tile)
(A model's read past the end of x wraps to its start: only the model needs a value there.)
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fp8_quantization_amd", "csrc")
U = 2.0 ** -24
EPS = float(np.float32(1e-5))   # (the C-ABI takes eps as fp32)
F64 = np.float64


# ------------------------------------------------------------------------------------------ constants
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(src, name):
    m = re.search(rf"constexpr (?:int|int64_t) {name} = (\d+);", src)
    assert m, f"{name} is no longer a literal constant of the header"
    return int(m.group(1))


def constants():
    bn, ms, kb = _read("bn_train.h"), _read("fq_mse.h"), _read("k_bn.hip")
    assert re.search(r"constexpr int BN_TILE = BN_NT \* BN_V;", bn)
    assert re.search(r"constexpr int MSE_TILE = MSE_NT \* MSE_V;", ms)
    cap = re.search(r"std::min<int64_t>\(\(work \+ 255\) / 256, (\d+)\)", kb)
    assert cap and re.search(r"bn_apply_kernel<uint32_t><<<blocks, 256, 0, s>>>", kb)
    return dict(BN_TILE=_const(bn, "BN_NT") * _const(bn, "BN_V"), BN_LIN_TILE=_const(bn, "BN_LIN_TILE"),
                BN_LIN_INNER=_const(bn, "BN_LIN_INNER"), BN_TARGET_WGS=_const(bn, "BN_TARGET_WGS"),
                MSE_TILE=_const(ms, "MSE_NT") * _const(ms, "MSE_V"), MSE_TARGET_WGS=_const(ms, "MSE_TARGET_WGS"),
                APPLY_THREADS=int(cap.group(1)) * 256)


K = constants()


# ------------------------------------------------------------------------------------------ plans
def cdiv(a, b):
    return -(-a // b)


def split(tiles, parts):
    """[t0, t1) of every part."""
    return [(p * tiles // parts, (p + 1) * tiles // parts) for p in range(parts)]


def bn_lin(inner):
    return inner < K["BN_LIN_INNER"]


def bn_plan(shape):
    """bn_parts (csrc/bn_train.h) and launch_bn_train (csrc/k_bn.hip) for x of `shape` = (N, C, ...)."""
    N, C = int(shape[0]), int(shape[1])
    inner = int(np.prod(shape[2:], dtype=np.int64)) if len(shape) > 2 else 1
    n, lin = N * inner, bn_lin(inner)
    tile = K["BN_LIN_TILE"] if lin else K["BN_TILE"]
    groups = cdiv(C, 64) if lin else C
    tiles, want = cdiv(n, tile), cdiv(K["BN_TARGET_WGS"], groups)
    parts = max(1, min(tiles, want))
    vec = inner % 4 == 0                       # (torch allocations are 16-byte aligned)
    work = N * C * inner // 4 if vec else N * C * inner
    return dict(N=N, C=C, inner=inner, n=n, lin=lin, tile=tile, groups=groups, tiles=tiles, want=want, parts=parts,
                split=split(tiles, parts), last=n - (tiles - 1) * tile, vec=vec, work=work,
                strides=work // K["APPLY_THREADS"])   # grid-stride iterations every thread runs BEYOND its first


def mse_plan(shape):
    """mse_parts (csrc/fq_mse.h) for x [rows][inner]."""
    rows, inner = int(shape[0]), int(shape[1])
    tile = K["MSE_TILE"]
    tiles, want = cdiv(inner, tile), cdiv(K["MSE_TARGET_WGS"], rows)
    parts = max(1, min(tiles, want))
    return dict(rows=rows, inner=inner, n=inner, tile=tile, tiles=tiles, want=want, parts=parts,
                split=split(tiles, parts), last=inner - (tiles - 1) * tile, lin=False)


def wrap_tiles(pl):
    """BN: the tiles with an image boundary STRICTLY inside, as (tile, first tile of its part?)."""
    firsts = {t0 for (t0, _) in pl["split"]}
    out = []
    for t in range(pl["tiles"]):
        j0, j1 = t * pl["tile"], min((t + 1) * pl["tile"], pl["n"])
        k = j0 // pl["inner"] + 1                 # the first boundary above j0
        if k * pl["inner"] < j1:
            out.append((t, t in firsts))
    return out


# ------------------------------------------------------------------------------------------ cases
# `expect`: what the case is here for, in the plan's own terms (the CPU file asserts plan == expect entry by entry,
# and the plan against the built library).  sizes = tiles per part.
BN_CASES = {
    # float4 loads; an image boundary (4100) inside tile 1; tile 2, the second of part 1, starts inside image 1
    "bn-vec-uneven": dict(shape=(2, 1024, 41, 100), expect=dict(
        inner=4100, vec=True, lin=False, n=8200, tiles=3, want=2, parts=2, sizes=(1, 2), last=8, strides=4)),
    # scalar loads
    "bn-scalar-uneven": dict(shape=(3, 1030, 61, 67), expect=dict(
        inner=4087, vec=False, lin=False, n=12261, tiles=3, want=2, parts=2, sizes=(1, 2), last=4069, strides=24)),
    # want = 1: one workgroup per channel walks both tiles
    "bn-one-part": dict(shape=(5, 2050, 31, 31), expect=dict(
        inner=961, vec=False, lin=False, n=4805, tiles=2, want=1, parts=1, sizes=(2,), last=709, strides=18)),
    # the lin form: 65 channel groups, the last with 4 live channels; 34 tiles of 256 on 32 parts
    "bn-lin-uneven": dict(shape=(8453, 4100), expect=dict(
        inner=1, vec=False, lin=True, n=8453, tiles=34, want=32, parts=32, last=5, strides=66)),
    # none of the three non-lin shapes above has an image boundary strictly inside a tile that is not the first of
    # its part (their parts' later tiles only START inside an image).  Here tile 2, the second of part 1, holds the
    # boundary 8 x 1028 = 8224.
    "bn-wrap-late": dict(shape=(9, 1024, 4, 257), expect=dict(
        inner=1028, vec=True, lin=False, n=9252, tiles=3, want=2, parts=2, sizes=(1, 2), last=1060, strides=4)),
}

MSE_CASES = {
    "mse-rows-uneven": dict(shape=(700, 12293), widths="m1to6", exempt=(), expect=dict(
        tiles=4, want=3, parts=3, sizes=(1, 1, 2), last=5)),
    "mse-one-part": dict(shape=(2050, 4099), widths="m3", exempt=(), expect=dict(
        tiles=2, want=1, parts=1, sizes=(2,), last=3)),
    # per-tensor activations: four of the 2048 parts walk two tiles.  Exempt from tail_short: one term of 8.4 M
    # is below the bar B (9.5e-7 relative), so no test of a sum can see it; the single-element edge of the ragged
    # tile is carried by the two cases above.
    "mse-tensor": dict(shape=(1, 8_400_901), widths="m3", exempt=("tail_short",), expect=dict(
        tiles=2052, want=2048, parts=2048, last=5)),
}

MUTANTS = ("t1_floor", "tile_twice", "tail_short", "no_wrap", "row_base", "lin_unclamped")


def mutant_applies(pl, mutant, bn):
    if mutant == "t1_floor":
        return pl["tiles"] % pl["parts"] != 0
    if mutant == "tile_twice":
        return pl["parts"] > 1
    if mutant == "tail_short":
        return pl["last"] < pl["tile"]
    if mutant == "no_wrap":
        return bn and not pl["lin"] and bool(wrap_tiles(pl))
    if mutant == "row_base":
        return not bn and pl["rows"] > 1 and pl["inner"] % pl["tile"] != 0
    if mutant == "lin_unclamped":
        return bn and pl["lin"] and pl["n"] % pl["tile"] != 0
    raise KeyError(mutant)


def part_ranges(tiles, parts, mutant=None):
    out = []
    for p in range(parts):
        t0, t1 = p * tiles // parts, (p + 1) * tiles // parts
        if mutant == "t1_floor":
            t1 = t0 + tiles // parts
        if mutant == "tile_twice" and t0 > 0:
            t0 -= 1
        out.append((t0, t1))
    return out


def partitioned(T, ranges):
    """T [rows][tiles] -> [rows]: a part's tiles in tile order, then the parts in part order."""
    total = np.zeros(T.shape[0], F64)
    for (t0, t1) in ranges:
        s = np.zeros(T.shape[0], F64)
        for t in range(t0, t1):
            s += T[:, t]
        total += s
    return total


def ulp32(v):
    """The fp32 spacing at |v| (float64 in and out)."""
    return np.spacing(np.abs(v).astype(np.float32)).astype(F64)


# ------------------------------------------------------------------------------------------ BN
CHUNK = 128   # channels per step of the float64 work (the lin case: 128 x 8453 doubles)


def _rows64(x, pl, c0, c1):
    """Channels [c0, c1) as float64 [c1 - c0][n], a channel's values in (image, offset) order."""
    v = x.reshape(pl["N"], pl["C"], pl["inner"])[:, c0:c1]
    return np.moveaxis(v, 1, 0).reshape(c1 - c0, pl["n"]).astype(F64)


def bn_bars(mean, var, D, n, gamma, beta):
    """S1 / S2 of tests/test_gpu_bn_train.py: (dm, dv, scale, shift, ds, dsh) in float64."""
    g, b = gamma.astype(F64), beta.astype(F64)
    dm = n * 2.0 ** -52 * D
    dv = 4 * n * 2.0 ** -52 * D * D
    scale = g / np.sqrt(var + EPS)
    shift = b - mean * scale
    ds = np.abs(g) * dv / (2 * (np.maximum(var - dv, 0) + EPS) ** 1.5)
    dsh = np.abs(mean) * ds + np.abs(scale) * dm + dm * ds + 2.0 ** -52 * (np.abs(b) + np.abs(mean * scale))
    return dm, dv, scale, shift, ds, dsh


def bn_reference(x, gamma, beta):
    """The float64 two-pass statistics of x (N, C, ...) per channel, in channel chunks, and the bars."""
    pl = bn_plan(x.shape)
    C = pl["C"]
    mean, var, D = np.empty(C, F64), np.empty(C, F64), np.empty(C, F64)
    for c0 in range(0, C, CHUNK):
        c1 = min(c0 + CHUNK, C)
        v = _rows64(x, pl, c0, c1)
        mean[c0:c1] = v.mean(axis=1)
        D[c0:c1] = np.abs(v - v[:, :1]).max(axis=1)
        v -= mean[c0:c1, None]
        v *= v
        var[c0:c1] = v.mean(axis=1)
    dm, dv, scale, shift, ds, dsh = bn_bars(mean, var, D, pl["n"], gamma, beta)
    return dict(n=pl["n"], C=C, mean=mean, var=var, D=D, dm=dm, dv=dv, scale=scale, shift=shift, ds=ds, dsh=dsh)


_BN = {}


def bn_case(cid):
    """x (normal draws; channel 0 constant, channel 1 = 4096 + 2^-8 U(-1, 1), channel 2 all zeros, as case() of
    tests/test_gpu_bn_train.py), gamma, beta, the plan and the float64 reference: computed once, never modified."""
    if cid not in _BN:
        shape = BN_CASES[cid]["shape"]
        rng = np.random.default_rng(4321 + sum(shape) * 7 + len(shape))
        x = rng.standard_normal(shape, dtype=np.float32)
        x *= np.float32(1.7)
        x += np.float32(0.3)
        x[:, 0] = -2.625
        x[:, 1] = np.float32(4096.0) + np.float32(2.0 ** -8) * (rng.random(x[:, 1].shape, dtype=np.float32) * 2 - 1)
        x[:, 2] = 0.0
        gamma = rng.random(shape[1], dtype=np.float32) + np.float32(0.5)
        beta = rng.standard_normal(shape[1], dtype=np.float32)
        c = dict(bn_reference(x, gamma, beta), x=x, gamma=gamma, beta=beta, plan=bn_plan(shape), shape=shape)
        _BN[cid] = c
    return _BN[cid]


def bn_tile_sums(cid, no_wrap=False):
    """(TS, TQ, dl, dl2): sum d and sum d^2 per (channel, tile), d = x - K_c in float64 (K_c the channel's first
    value), and the last element's d and d^2.  no_wrap: a tile's values read as the kernel would with di = 0, at
    x[(img0 C + c) inner + off0 + l] -- past the image's end they are the next channel's."""
    c = bn_case(cid)
    pl, x = c["plan"], c["x"]
    C, inner, n, tile, tiles = pl["C"], pl["inner"], pl["n"], pl["tile"], pl["tiles"]
    flat = x.reshape(-1)
    K0 = x.reshape(pl["N"], C, inner)[0, :, 0].astype(F64)
    TS, TQ = np.empty((C, tiles), F64), np.empty((C, tiles), F64)
    dl, dl2 = np.empty(C, F64), np.empty(C, F64)
    edges = np.arange(tiles) * tile
    for c0 in range(0, C, CHUNK):
        c1 = min(c0 + CHUNK, C)
        if no_wrap:
            d = np.empty((c1 - c0, n), F64)
            for t in range(tiles):
                j0 = t * tile
                img0, off0 = divmod(j0, inner)
                cnt = min(tile, n - j0)
                base = (img0 * C + np.arange(c0, c1, dtype=np.int64)) * inner + off0
                d[:, j0:j0 + cnt] = flat[(base[:, None] + np.arange(cnt, dtype=np.int64)[None, :]) % flat.size]
        else:
            d = _rows64(x, pl, c0, c1)
        d -= K0[c0:c1, None]
        TS[c0:c1] = np.add.reduceat(d, edges, axis=1)
        dl[c0:c1] = d[:, -1]
        d *= d
        TQ[c0:c1] = np.add.reduceat(d, edges, axis=1)
        dl2[c0:c1] = d[:, -1]
    return TS, TQ, dl, dl2, K0


_BN_SUMS = {}


def bn_model(cid, mutant=None):
    """What bn_stats(_lin)_kernel + bn_finalize_kernel return for the case -- (save_mean, save_var, scale, shift),
    each rounded to fp32 once, as float64 -- with the sums taken over the plan's index sets, or a mutant's."""
    c = bn_case(cid)
    pl = c["plan"]
    key = (cid, mutant == "no_wrap")
    if key not in _BN_SUMS:
        _BN_SUMS[key] = bn_tile_sums(cid, no_wrap=key[1])
    TS, TQ, dl, dl2, K0 = _BN_SUMS[key]
    if mutant == "tail_short":
        TS, TQ = TS.copy(), TQ.copy()
        TS[:, -1] -= dl
        TQ[:, -1] -= dl2
    if mutant == "lin_unclamped":
        # values j in [n, tiles tile) of channel c at x[j C + c] (inner = 1), wrapped into x
        flat = c["x"].reshape(-1)
        j = np.arange(pl["n"], pl["tiles"] * pl["tile"], dtype=np.int64)
        d = flat[(j[None, :] * pl["C"] + np.arange(pl["C"], dtype=np.int64)[:, None]) % flat.size].astype(F64)
        d -= K0[:, None]
        TS, TQ = TS.copy(), TQ.copy()
        TS[:, -1] += d.sum(axis=1)
        TQ[:, -1] += (d * d).sum(axis=1)
    ranges = part_ranges(pl["tiles"], pl["parts"], mutant)
    S, Q = partitioned(TS, ranges), partitioned(TQ, ranges)
    n = float(pl["n"])
    mean = K0 + S / n
    var = np.maximum(0.0, (Q - S * S / n) / n)
    scale = c["gamma"].astype(F64) / np.sqrt(var + EPS)
    shift = c["beta"].astype(F64) - mean * scale
    return tuple(v.astype(np.float32).astype(F64) for v in (mean, var, scale, shift))


def bn_errors_over_bars(c, sm, sv, scale, shift):
    """(error, bar) of S1 / S2 for save_mean, save_var, scale, shift (float64 arrays [C])."""
    return [(np.abs(sm - c["mean"]), U * np.abs(c["mean"]) + c["dm"]),
            (np.abs(sv - c["var"]), U * c["var"] + c["dv"]),
            (np.abs(scale - c["scale"]), 2 * ulp32(c["scale"]) + c["ds"]),
            (np.abs(shift - c["shift"]), 2 * ulp32(c["shift"]) + c["dsh"])]


# ------------------------------------------------------------------------------------------ MSE
def mse_input(shape):
    """x [rows][inner] as t1_input of tests/test_gpu_mse.py draws it (zeros every 7th value, 0.97 top and
    -0.93 top planted), and 0.89 top as every row's LAST value: the one value the ragged tile's last lane holds
    (index inner - 1 would otherwise be a planted zero wherever inner % 7 == 1, and a zero has no term)."""
    rows, inner = shape
    rng = np.random.default_rng(rows * 7919 + inner)
    x = rng.standard_normal(shape).astype(np.float32) * np.linspace(0.4, 3.0, rows, dtype=np.float32)[:, None]
    x[:, ::7] = 0.0
    top = np.abs(x).max(1)
    x[:, 3 % inner] = 0.97 * top
    x[:, 11 % inner] = -0.93 * top
    x[:, inner - 1] = 0.89 * top
    return x


_MSE = {}


def mse_case(cid):
    if cid not in _MSE:
        shape = MSE_CASES[cid]["shape"]
        x = mse_input(shape)
        _MSE[cid] = dict(x=x, plan=mse_plan(shape), shape=shape)
    return _MSE[cid]


MODEL_CANDS = (0, 55, 110)   # the first, middle and last of the 111 grid rows
MODEL_MBITS = 3


def mse_model_grid(x):
    """Candidates MODEL_CANDS of linspace(0.1 top, 1.2 top, 111) per row, fp32 [3][rows] (the model's own: the GPU
    file takes the estimator's grid, whose bits are torch's)."""
    top = np.abs(x).max(1).astype(F64)
    return np.stack([(0.1 * top + (1.1 * top) * i / 110.0) for i in MODEL_CANDS]).astype(np.float32)


def mse_terms(x, grid_row, sign_bits):
    """The fp32 terms (x - fq(x))^2 of one candidate per row, from the oracle's quantizer (an unsigned format
    clamps at 0 below: the signed quantizer on max(x, 0), with the exponent width of 8 bits without a sign)."""
    from oracle import oracle
    xin = x if sign_bits else np.maximum(x, np.float32(0.0))
    q, _ = oracle.fp8_fake_quant(xin, grid_row, 8 - sign_bits - MODEL_MBITS, MODEL_MBITS, per_row=True)
    d = x - q
    return d * d


_MSE_SUMS = {}


def mse_tile_sums(cid, sign_bits, row_base=False):
    """(T [3][rows][tiles], last [3][rows], straight [3][rows]): the float64 sums of the terms per tile, the row's
    last term, and the sum over the whole row.  row_base: row r read from x + r tiles MSE_TILE, wrapped into x."""
    key = (cid, sign_bits, row_base)
    if key not in _MSE_SUMS:
        c = mse_case(cid)
        pl, x = c["plan"], c["x"]
        rows, inner, tile, tiles = pl["rows"], pl["inner"], pl["tile"], pl["tiles"]
        grid = mse_model_grid(x)
        if row_base:
            flat = x.reshape(-1)
            idx = np.arange(rows, dtype=np.int64)[:, None] * (tiles * tile) + np.arange(inner, dtype=np.int64)[None, :]
            x = flat[idx % flat.size]
        edges = np.arange(tiles) * tile
        T = np.empty((len(MODEL_CANDS), rows, tiles), F64)
        last, straight = np.empty((len(MODEL_CANDS), rows), F64), np.empty((len(MODEL_CANDS), rows), F64)
        for i in range(len(MODEL_CANDS)):
            e = mse_terms(x, grid[i], sign_bits).astype(F64)
            T[i] = np.add.reduceat(e, edges, axis=1)
            last[i] = e[:, -1]
            straight[i] = e.sum(axis=1)
        _MSE_SUMS[key] = (T, last, straight)
    return _MSE_SUMS[key]


def mse_model(cid, sign_bits, mutant=None):
    """(model, straight) [3][rows]: the float64 sums of the terms over the plan's (or a mutant's) index sets, and
    the straight sums of the unmutated terms over the whole row."""
    pl = mse_case(cid)["plan"]
    straight = mse_tile_sums(cid, sign_bits)[2]
    T, last, _ = mse_tile_sums(cid, sign_bits, row_base=mutant == "row_base")
    if mutant == "tail_short":
        T = T.copy()
        T[:, :, -1] -= last
    ranges = part_ranges(pl["tiles"], pl["parts"], mutant)
    return np.stack([partitioned(T[i], ranges) for i in range(len(MODEL_CANDS))]), straight
