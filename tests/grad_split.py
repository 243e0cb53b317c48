"""The gradient GEMM's split along K (fp8a_grad_bmm_split, csrc/gemm_grad.h): the split plan, a
numpy model of the two passes and the cases shared by tests/test_grad_split_cpu.py and tests/test_gpu_grad_split.py.
No GPU, no reference code; not collected.

The plan.  nst = ceil(K / 32) stages, per = ceil(nst / splits) stages per part, S = ceil(nst / per) parts (1 when
nst <= 1 or splits = 1; no part is empty); part s owns the flat k in [32 per s, min(32 per (s + 1), K)), k = k0 K1 +
k1, so a part may begin inside a k0 row.

The model.  Each part is grad_exact.model on the part's K-slice (its float64 sum, cast to fp32), stored as dense
64 x 64 tiles in the workspace's layout ws[s][item][tile]; the result is the fp32 sum P_0 + P_1 + ... in index order.
On exact-sum inputs (exact_sums' rule, carried over to the pieces by grad_exact) every part and every partial sum
of parts is a multiple of u below 2^22 u, so the result is expected(T) for every split count.

Mutants, bugs of the split path alone (with S = 1 the unsplit kernel runs and the first three change nothing):
  drop_part        the last part is not summed;
  stage_overlap    part s >= 1 starts one stage early;
  tail_dropped     the ragged last stage of the last part is lost;
  per_floor        per = floor(nst / splits) with the part count unchanged: the stages past S per are lost;
  ws_item_stride   the reduce pass reads a partial with nb and tiles swapped in the index.
"""
import functools

import numpy as np

from tests import exact_sums as xs
from tests import grad_exact as gx

STAGE = 32
TILE = gx.TILE
MUTANTS = ("drop_part", "stage_overlap", "tail_dropped", "per_floor", "ws_item_stride")
SPLITS = (2, 3, 4, 5)


# ------------------------------------------------------------------------------------------ the plan
def plan(K, splits):
    """(per, S) of section 1: stages per part and the effective part count."""
    assert splits >= 1
    nst = -(-K // STAGE)
    if nst == 0:
        return 1, 1
    per = -(-nst // splits)
    return per, -(-nst // per)


def ranges(K, splits, mutant=None):
    """The flat k ranges [(kbeg, kend), ...] of the parts that are summed, under a mutant of the split path."""
    per, S = plan(K, splits)
    if S == 1:
        return [(0, K)]
    if mutant == "per_floor":
        per = max(1, -(-K // STAGE) // splits)
    out = []
    for s in range(S):
        kb, ke = STAGE * per * s, min(STAGE * per * (s + 1), K)
        if mutant == "stage_overlap" and s >= 1:
            kb -= STAGE
        if mutant == "tail_dropped" and s == S - 1:
            ke -= ke % STAGE
        out.append((kb, max(kb, ke)))
    return out[:-1] if mutant == "drop_part" else out


def workspace_bytes(nb, M, N, K, splits):
    S = plan(K, splits)[1]
    return 0 if S == 1 else S * gx.num_tiles(nb, M, N) * TILE * TILE * 4


# ------------------------------------------------------------------------------------------ the model
def k_slice(A, B, kb, ke):
    """The K-slice [kb, ke) of A [nb, M, K0, K1], B [nb, K0, K1, N] as single-level operands."""
    nb, M, K0, K1 = A.shape
    N = B.shape[-1]
    a = np.ascontiguousarray(A).reshape(nb, M, K0 * K1)[:, :, kb:ke]
    b = np.ascontiguousarray(B).reshape(nb, K0 * K1, N)[:, kb:ke]
    return a.reshape(nb, M, 1, ke - kb), b.reshape(nb, 1, ke - kb, N)


def _to_workspace(P):
    """A part's [nb, M, N] result as the product pass stores it: [nb, tiles, 64, 64], tile = row tile + num_mt *
    column tile, rows and columns beyond M and N zero."""
    nb, M, N = P.shape
    num_mt, num_nt = -(-M // TILE), -(-N // TILE)
    ws = np.zeros((nb, num_mt * num_nt, TILE, TILE), np.float32)
    for t in range(num_mt * num_nt):
        m0, n0 = (t % num_mt) * TILE, (t // num_mt) * TILE
        blk = P[:, m0:m0 + TILE, n0:n0 + TILE]
        ws[:, t, :blk.shape[1], :blk.shape[2]] = blk
    return ws


def _from_workspace(ws, M, N, swapped):
    nb, tiles = ws.shape[:2]
    num_mt = -(-M // TILE)
    flat = ws.reshape(nb * tiles, TILE, TILE)
    out = np.empty((nb, M, N), np.float32)
    for i in range(nb):
        for t in range(tiles):
            m0, n0 = (t % num_mt) * TILE, (t // num_mt) * TILE
            blk = flat[t * nb + i] if swapped else flat[i * tiles + t]
            out[i, m0:m0 + TILE, n0:n0 + TILE] = blk[:min(TILE, M - m0), :min(TILE, N - n0)]
    return out


def model_split(A, B, splits, mutant=None):
    """What grad_bmm(split_k=splits) stores into C [nb, M, N], in numpy; `mutant`: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    nb, M, K0, K1 = A.shape
    N, K = B.shape[-1], K0 * K1
    rs = ranges(K, splits, mutant)
    if plan(K, splits)[1] == 1:
        return gx.model(A, B)
    acc = None
    for (kb, ke) in rs:
        P = gx.model(*k_slice(A, B, kb, ke))                       # float64 per part, cast to fp32
        P = _from_workspace(_to_workspace(P), M, N, mutant == "ws_item_stride")
        with np.errstate(invalid="ignore", over="ignore"):
            acc = P if acc is None else (acc + P).astype(np.float32)   # fp32 adds, index order, from P_0
    return acc


def slice_sum(parts):
    """P_0 + P_1 + ... of a list of fp32 arrays, fp32 adds in index order."""
    acc = parts[0]
    for P in parts[1:]:
        acc = (acc + P).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------ cases
NB = 2
# (M, N, K0, K1): 70 x 67 is a 2 x 2 tile grid, ragged on both sides; K = 129: five stages, the last of one element
SQUARE_K = [(1, 129), (1, 160), (4, 40), (1, 96)]
GRID_K = (5, 32)
PAD_K = [(4, 40), (40, 4)]            # the padded views' K0 x K1 (family W; 4 x 40 is a case of SQUARE_K too)


def _case(fam, M, N, K0, K1):
    cid = f"{fam}-{K0}x{K1}-{M}x{N}"
    return cid, dict(id=cid, fam=fam, nb=NB, M=M, N=N, K0=K0, K1=K1)


def cases():
    out = []
    for fam in "WG":
        out += [_case(fam, 70, 67, K0, K1) for (K0, K1) in SQUARE_K]
        out += [_case(fam, M, N, *GRID_K) for (M, N) in gx.TWO_LEVEL]
    out.append(_case("W", 70, 67, 40, 4))
    return dict(out)


CASES = cases()


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dict(A, B, T, want) of a case: contiguous operands, the float64 terms [nb, M, K, N], expected(T)."""
    c = CASES[cid]
    A, B = gx.family(c["fam"], c["nb"], c["M"], c["K0"], c["K1"], c["N"])
    T = gx.terms(A, B)
    return dict(A=A, B=B, T=T, want=xs.expected(T, axis=2))


# ------------------------------------------------------------------------------------------ the slice identity
def slice_operands(K0, K1, nb=3, M=70, N=67, seed=0):
    """Operands on which the order of the adds matters: A = N(0, 1) 2^e with mixed exponents, B on the E4M3 grid
    (gx.grid_b's full 8-bit significands cut to 4).  Contiguous A [nb, M, K0, K1], B [nb, K0, K1, N]."""
    rng = np.random.default_rng([gx.SEED, 23, seed, nb, M, K0, K1, N])
    A = (rng.standard_normal((nb, M, K0, K1)) * np.exp2(rng.integers(-6, 7, size=(nb, M, K0, K1)))).astype(np.float32)
    mant = rng.integers(8, 16, size=(nb, K0, K1, N)) / 8.0
    B = mant * np.exp2(rng.integers(-4, 4, size=mant.shape)) * rng.choice([-1.0, 1.0], size=mant.shape)
    B[rng.random(mant.shape) < 0.1] = 0.0
    return A, B.astype(np.float32)
