"""The gradient GEMM (gemm_grad_kernel, csrc/gemm_grad.h) on sums that can be compared bit for
bit: data and a plain numpy model shared by tests/test_grad_exact_cpu.py and tests/test_gpu_grad_exact.py.
No GPU, no reference code; not collected.

The rule is tests/exact_sums.py's: if every term of a case is a multiple of u and sum_k |T| <= 2^22 u per output,
the fp32 sum is the same in any order and equals expected(T) = float32(sum_k float64(T)).  It carries over to the
kernel's three-piece split: every piece of a is a multiple of a's last set bit and has a's sign, so the piece
terms p0 b, p1 b, p2 b have the unit of a b and the same absolute sum.

Operands are numpy views of the kernel's logical shapes, A [nb, M, K0, K1] and B [nb, K0, K1, N].

  * family W (wide A): A integers in [-2^8, 2^8) with three entries per row (all, when K < 3) replaced by odd
    integers in [2^17, 2^18) with bit 9 set, of either sign -- all three pieces nonzero -- times 2^-30; B
    +-{1/2, 1, 2}, 10 % zeros.
  * family G (grid B): A integers in [-2^7, 2^7) times 2^-30; B +-(j / 128) {1/2, 1}, j in 128..255 -- full 8-bit
    significands, the kernel's contract for B -- 10 % zeros.
  * routing: B holds one +-2^j per column, every k chosen by a column; A arbitrary (22-bit significands,
    exponents in [-60, 60]).  Every output is one number a 2^j and every partial sum of its pieces has at most
    22 bits: exact without a global unit.
  * pairs: item i, row r: A[k = i] = 1, A[k = r] = +-2^-21 (i != r), B all ones, K = 64: every position pair
    of two stages.
  * sparse: one nonzero a per row (at k = 5 m mod K), B = +-b everywhere: every output is the one product a b.
    The window-edge and small-product tests plant their elements in it.

model() restates the kernel's arithmetic -- split3 of tests/test_grad_cpu.py, B truncated to bf16, terms summed in
float64, one 64 x 64 tile per block into a sentinel-filled C -- and takes a named mutant, a bug the GPU tests
must catch (tests/test_grad_exact_cpu.py shows which case catches which).
"""
import functools
import math

import numpy as np

from tests.test_grad_cpu import split3, trunc16

SEED = 0
A_SCALE = 2.0 ** -30          # one global power of two on A: exact_sums' global-unit helpers apply
SENTINEL = np.float32(-77.25)
TILE = 64
MUTANTS = ("drop_p2", "drop_p1", "b7", "drop_last_k", "swap_tile_counts", "no_wrap")


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


# ------------------------------------------------------------------------------------------ operands
def grid_b(rng, shape):
    """Family G's B: +-(j / 128) {1/2, 1}, j in 128..255, 10 % zeros."""
    v = rng.integers(128, 256, size=shape) / 128.0 * rng.choice([0.5, 1.0], size=shape)
    v = v * rng.choice([-1.0, 1.0], size=shape)
    v[rng.random(shape) < 0.1] = 0.0
    return v.astype(np.float32)


def small_ints(rng, shape, bits=7):
    """Family G's A: integers in [-2^bits, 2^bits) times 2^-30."""
    return (rng.integers(-(1 << bits), 1 << bits, size=shape) * A_SCALE).astype(np.float32)


def family(fam, nb, M, K0, K1, N):
    """(A [nb, M, K0, K1], B [nb, K0, K1, N]) contiguous float32."""
    K = K0 * K1
    rng = _rng(ord(fam), nb, M, K0, K1, N)
    if fam == "W":
        a = rng.integers(-256, 256, size=(nb, M, K))
        # (bit 9 set as well: what p0's eight bits leave then spans ten bits, so p1 leaves a nonzero p2)
        wide = (rng.integers(1 << 17, 1 << 18, size=(nb, M, K)) | 0x201) * rng.choice([-1, 1], size=(nb, M, K))
        pick = np.zeros((nb, M, K), bool)
        if K < 3:
            pick[:] = True
        else:
            for i in range(nb):
                for m in range(M):
                    pick[i, m, rng.choice(K, size=3, replace=False)] = True
        A = (np.where(pick, wide, a) * A_SCALE).astype(np.float32)
        B = (rng.choice([0.5, 1.0, 2.0], size=(nb, K, N)) * rng.choice([-1.0, 1.0], size=(nb, K, N)))
        B[rng.random((nb, K, N)) < 0.1] = 0.0
        B = B.astype(np.float32)
    else:
        A = small_ints(rng, (nb, M, K))
        B = grid_b(rng, (nb, K, N))
    return A.reshape(nb, M, K0, K1), B.reshape(nb, K0, K1, N)


def routing(nb=2, M=70, K0=2, K1=37, N=80):
    K = K0 * K1
    assert N >= K
    rng = _rng(7, nb, M, K, N)
    sig = rng.integers(1 << 21, 1 << 22, size=(nb, M, K)) | 1          # 22 bits, the last one set
    A = np.ldexp(sig.astype(np.float64), rng.integers(-60, 61, size=(nb, M, K)) - 21)
    A = (A * rng.choice([-1.0, 1.0], size=A.shape)).astype(np.float32)
    B = np.zeros((nb, K, N), np.float32)
    for i in range(nb):
        ks = np.concatenate([rng.permutation(K), rng.integers(0, K, size=N - K)])
        B[i, ks, np.arange(N)] = np.ldexp(rng.choice([-1.0, 1.0], size=N), rng.integers(-8, 9, size=N))
    return A.reshape(nb, M, K0, K1), B.reshape(nb, K0, K1, N)


def pairs(sign):
    """nb = M = K = 64: row r of item i holds 1 at k = i and sign 2^-21 at k = r (i != r; the row r = i holds
    the 1 alone); B all ones, 16 columns.  (A, B, expected)."""
    n = 64
    A = np.zeros((n, n, n), np.float32)
    idx = np.arange(n)
    A[:, idx, idx] = np.float32(sign * 2.0 ** -21)
    for i in range(n):
        A[i, :, i] = 1.0
    B = np.ones((n, n, 16), np.float32)
    want = np.full((n, n, 16), np.float32(1.0 + sign * 2.0 ** -21))
    want[idx, idx] = 1.0
    return A.reshape(n, n, 1, n), B.reshape(n, 1, n, 16), want


def sparse(a, b, nb, M, K0, K1, N):
    """One nonzero per A row, sign a at k = 5 m mod K; B = +-b everywhere."""
    K = K0 * K1
    rng = _rng(11, nb, M, K, N)
    A = np.zeros((nb, M, K), np.float32)
    m = np.arange(M)
    A[:, m, (5 * m) % K] = (rng.choice([-1.0, 1.0], size=(nb, M)) * a).astype(np.float32)
    B = (rng.choice([-1.0, 1.0], size=(nb, K, N)) * b).astype(np.float32)
    return A.reshape(nb, M, K0, K1), B.reshape(nb, K0, K1, N)


def product64(A, B):
    """float32(float64 product): the expected result where every output has one nonzero term (or is not finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("imkl,ikln->imn", A.astype(np.float64), B.astype(np.float64)).astype(np.float32)


def terms(A, B):
    """T[i, m, k, n] = a b in float64 (exact: 24 + 24 bits)."""
    nb, M, K0, K1 = A.shape
    a = np.ascontiguousarray(A).reshape(nb, M, K0 * K1).astype(np.float64)
    b = np.ascontiguousarray(B).reshape(nb, K0 * K1, -1).astype(np.float64)
    return a[:, :, :, None] * b[:, None, :, :]


# ------------------------------------------------------------------------------------------ padded views
def _perm(x, axes):
    return x.permute(*axes) if hasattr(x, "permute") else x.transpose(axes)


PAD_M, PAD_K1, PAD_N = 3, 5, 4


def a_view(buf, layout, M, K1):
    """A [nb, M, K0, K1] inside its padded buffer: "k1": buf [nb, M + 3, K0, K1 + 5]; "m" (unit stride on m):
    buf [nb, K0, K1 + 5, M + 3].  Works on numpy arrays and on torch tensors."""
    if layout == "k1":
        return buf[:, :M, :, :K1]
    return _perm(buf, (0, 3, 1, 2))[:, :M, :, :K1]


def b_view(buf, layout, K1, N):
    """B [nb, K0, K1, N]: "k1" (with A's: unit stride on k1): buf [nb, N + 4, K0, K1 + 5]; "m" (unit stride on
    n): buf [nb, K0, K1 + 5, N + 4]."""
    if layout == "k1":
        return _perm(buf, (0, 2, 3, 1))[:, :, :K1, :N]
    return buf[:, :, :K1, :N]


def c_view(buf, layout):
    """C [nb, M, N] as the interior of a sentinel buffer: "k1": buf [nb, M + 2, N + 2] (unit stride on n); "m":
    buf [nb, N + 2, M + 2] (unit stride on m)."""
    if layout == "k1":
        return buf[:, 1:-1, 1:-1]
    return _perm(buf, (0, 2, 1))[:, 1:-1, 1:-1]


def padded(A, B, layout):
    """(buffer of A, buffer of B): NaN everywhere but inside the views a_view / b_view, which hold A and B."""
    nb, M, K0, K1 = A.shape
    N = B.shape[-1]
    if layout == "k1":
        ba = np.full((nb, M + PAD_M, K0, K1 + PAD_K1), np.nan, np.float32)
        bb = np.full((nb, N + PAD_N, K0, K1 + PAD_K1), np.nan, np.float32)
    else:
        ba = np.full((nb, K0, K1 + PAD_K1, M + PAD_M), np.nan, np.float32)
        bb = np.full((nb, K0, K1 + PAD_K1, N + PAD_N), np.nan, np.float32)
    a_view(ba, layout, M, K1)[...] = A
    b_view(bb, layout, K1, N)[...] = B
    return ba, bb


def c_buffer(nb, M, N, layout):
    return np.full((nb, M + 2, N + 2) if layout == "k1" else (nb, N + 2, M + 2), SENTINEL, np.float32)


# ------------------------------------------------------------------------------------------ the model
def _read_no_wrap(X, k_axis):
    """X (a view with its two k axes at k_axis, k_axis + 1) read as load_tile would without the k0 step of its
    wrap: a thread's eight loads start at the right (k0, k1) and then only ever step by the k1 stride."""
    root = X
    while root.base is not None:
        root = root.base
    assert root.flags.c_contiguous
    flat = root.reshape(-1)
    st = [s // X.itemsize for s in X.strides]
    off = (X.__array_interface__["data"][0] - root.__array_interface__["data"][0]) // X.itemsize
    K0, K1 = X.shape[k_axis], X.shape[k_axis + 1]
    k = np.arange(K0 * K1)
    kb = k // 8 * 8
    ka = (kb // K1) * st[k_axis] + (kb % K1 + k - kb) * st[k_axis + 1]
    idx = np.full((), off, np.int64)
    for ax, n in enumerate(X.shape):
        if ax != k_axis + 1:
            idx = idx[..., None] + (ka if ax == k_axis else np.arange(n) * st[ax])
    assert idx.min() >= 0 and idx.max() < flat.size
    return flat[idx].reshape(X.shape)


def model(A, B, mutant=None):
    """What the kernel stores into a SENTINEL-filled C [nb, M, N], in numpy; `mutant`: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    nb, M, K0, K1 = A.shape
    N, K = B.shape[-1], K0 * K1
    if mutant == "no_wrap":
        A, B = _read_no_wrap(A, 2), _read_no_wrap(B, 1)
    a = np.ascontiguousarray(A).reshape(nb, M, K)
    b = np.ascontiguousarray(B).reshape(nb, K, N)
    p = list(split3(a))
    if mutant == "drop_p2":
        p = p[:2]
    if mutant == "drop_p1":
        p = [p[0], p[2]]
    if mutant == "b7":
        bt = (b.view(np.uint32) & np.uint32(0xFFFE0000)).view(np.float32)
    else:
        bt = trunc16(b)
    if mutant == "drop_last_k":
        p = [q[:, :, :K - 1] for q in p]
        bt = bt[:, :K - 1]
    with np.errstate(invalid="ignore"):
        full = sum(np.einsum("imk,ikn->imn", q.astype(np.float64), bt.astype(np.float64)) for q in p)
    full = full.astype(np.float32)
    out = np.full((nb, M, N), SENTINEL, np.float32)
    num_mt, num_nt = -(-M // TILE), -(-N // TILE)
    div = num_nt if mutant == "swap_tile_counts" else num_mt
    for bid in range(num_mt * num_nt):
        m0, n0 = (bid % div) * TILE, (bid // div) * TILE
        out[:, m0:m0 + TILE, n0:n0 + TILE] = full[:, m0:m0 + TILE, n0:n0 + TILE]
    return out


def num_tiles(nb, M, N):
    return nb * (-(-M // TILE)) * (-(-N // TILE))


# ------------------------------------------------------------------------------------------ cases
NB = 2
TWO_LEVEL = [(130, 40), (40, 130)]                       # 3 x 1 and 1 x 3 tile grids, K0 x K1 = 2 x 37
SINGLE = [(65, 64, 32), (64, 65, 33), (64, 64, 64), (64, 64, 1), (64, 64, 7), (70, 67, 96), (1, 1, 5)]  # (M, N, K)
PAD_SHAPE = (70, 67)                                     # (M, N) of the padded views
PAD_K = [(2, 37), (15, 5), (37, 2), (74, 1)]


def _case(cid, fam, M, N, K0, K1, nb=NB):
    return cid, dict(id=cid, fam=fam, nb=nb, M=M, N=N, K0=K0, K1=K1)


def edge_cases():
    out = []
    for fam in "WG":
        out += [_case(f"{fam}-2x37-{M}x{N}", fam, M, N, 2, 37) for (M, N) in TWO_LEVEL]
        out += [_case(f"{fam}-1x{K}-{M}x{N}", fam, M, N, 1, K) for (M, N, K) in SINGLE]
    return dict(out)


def pad_cases():
    return dict(_case(f"W-pad-{K0}x{K1}", "W", *PAD_SHAPE, K0, K1) for (K0, K1) in PAD_K)


CASES = dict(**edge_cases(), **pad_cases(), **dict([_case("routing", "routing", 70, 80, 2, 37)]))


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dict(A, B, want): contiguous operands and the expected C; for the families also T, the float64 terms
    [nb, M, K, N] (the budget runs over axis 2)."""
    from tests import exact_sums as xs
    c = CASES[cid]
    if c["fam"] == "routing":
        A, B = routing(c["nb"], c["M"], c["K0"], c["K1"], c["N"])
        return dict(A=A, B=B, want=product64(A, B), T=None)
    A, B = family(c["fam"], c["nb"], c["M"], c["K0"], c["K1"], c["N"])
    T = terms(A, B)
    return dict(A=A, B=B, T=T, want=xs.expected(T, axis=2))


# ------------------------------------------------------------------------------------------ window edges
GOOD_A = np.float32(2.0 ** -103 * (1 + 2.0 ** -21))      # exponent field 24: the smallest accepted binade
A_REJECTED = {"field23": np.float32(2.0 ** -104 * (1 + 2.0 ** -21)), "field1": np.float32(2.0 ** -126),
              "field0": np.float32(2.0 ** -130), "nan": np.float32(np.nan), "-inf": np.float32(-np.inf)}
B_REJECTED = {"bf16-subnormal": np.float32(2.0 ** -130), "+inf": np.float32(np.inf), "nan": np.float32(np.nan),
              "1+2^-12": np.float32(1 + 2.0 ** -12)}


def exponent_field(x):
    return int((np.float32(x).view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF))


def window_case(M, N, operand=None, name=None):
    """The sparse case of a window test at (M, N), K0 x K1 = 2 x 37: A's nonzeros GOOD_A against b = 2^100
    (operand "B": a = 2^100 against b = 2^-100, so that a planted 2^-130 meets a = 2^100), with one rejected
    element planted in item 1 -- A's as the only nonzero of a row of the last row tile, at k = 70 (the last,
    ragged stage); B's at k = 5 in a column of the last column tile.  Returns dict(A, B, want, spot, tiles):
    tiles = the tiles that stage the element, as (item, row tile, column tile)."""
    nb, K0, K1 = NB, 2, 37
    a, b = (GOOD_A, 2.0 ** 100) if operand != "B" else (2.0 ** 100, 2.0 ** -100)
    A, B = sparse(a, b, nb, M, K0, K1, N)
    num_mt, num_nt = -(-M // TILE), -(-N // TILE)
    tiles, spot = [], None
    if operand == "A" and name is not None:
        m = (num_mt - 1) * TILE + (M - (num_mt - 1) * TILE) // 2
        A[1, m] = 0.0
        A[1, m, 70 // K1, 70 % K1] = A_REJECTED[name]
        spot, tiles = (1, m, 70), [(1, m // TILE, nt) for nt in range(num_nt)]
    elif operand == "B" and name is not None:
        n = (num_nt - 1) * TILE + (N - (num_nt - 1) * TILE) // 2
        B[1, 0, 5, n] = B_REJECTED[name]
        spot, tiles = (1, 5, n), [(1, mt, n // TILE) for mt in range(num_mt)]
    return dict(A=A, B=B, want=product64(A, B), spot=spot, tiles=tiles)


# small products: (a, b).  The first two products are normal while a piece term is an fp32 subnormal: the pieces
# of 2^-100 (1 + 2^-21) are 2^-100, 2^-121, 0 and those of 2^-100 (1 + 2^-9 + 2^-21) are 2^-100, 2^-109, 2^-121, and
# 2^-121 2^-10 = 2^-131.  The third product is subnormal as a whole.
SMALL = {"piece-term-subnormal": (np.float32(2.0 ** -100 * (1 + 2.0 ** -21)), np.float32(2.0 ** -10)),
         "third-piece-term-subnormal": (np.float32(2.0 ** -100 * (1 + 2.0 ** -9 + 2.0 ** -21)), np.float32(2.0 ** -10)),
         "product-subnormal": (np.float32(2.0 ** -100), np.float32(2.0 ** -40))}


def small_case(name, M=70, N=67):
    a, b = SMALL[name]
    A, B = sparse(a, b, 1, M, 2, 37, N)
    return dict(A=A, B=B, want=product64(A, B))


# ------------------------------------------------------------------------------------------ STE operators
CONV_U = 2.0 ** -23     # x, w multiples of 2^-3, dy of 2^-20
GRID_U = 2.0 ** -38     # linear / batched: dy multiples of 2^-30, the grid operands of 2^-8
CONV = dict(x=(3, 4, 13, 11), cout=6, k=(3, 2), padding=(1, 0), dilation=(1, 2))
CONV_GROUPS = (1, 2, 4)
CONV_STRIDES = ((1, 1), (2, 1))


def conv_problem(groups, stride):
    """x, w multiples of 1/8 up to 15/8, dy = i 2^-20, |i| < 2^9 (torch float32 tensors on the CPU)."""
    import torch
    rng = _rng(13, groups, *stride)
    cin = CONV["x"][1]
    cout = 4 if groups == 4 else CONV["cout"]
    x = torch.from_numpy((rng.integers(-15, 16, size=CONV["x"]) / 8.0).astype(np.float32))
    w = torch.from_numpy((rng.integers(-15, 16, size=(cout, cin // groups) + CONV["k"]) / 8.0).astype(np.float32))
    y = torch.nn.functional.conv2d(x, w, None, stride, CONV["padding"], CONV["dilation"], groups)
    dy = torch.from_numpy((rng.integers(-511, 512, size=tuple(y.shape)) * 2.0 ** -20).astype(np.float32))
    return x, w, dy


def conv_backward64(x, w, dy, groups, stride, use_abs=False):
    """(dx, dw) of F.conv2d in float64 on the CPU; use_abs: on |x|, |w|, |dy| (the budget's sums)."""
    import torch
    x, w, dy = (t.double().abs() if use_abs else t.double() for t in (x, w, dy))
    x, w = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = torch.nn.functional.conv2d(x, w, None, stride, CONV["padding"], CONV["dilation"], groups)
    return torch.autograd.grad(y, (x, w), dy)


LINEAR = dict(R=70, cin=130, cout=67)


def linear_problem():
    """Family G with dy in A's role: dy [R, out] integers 2^-30, xq [R, in] and wq [out, in] on the 8-bit grid."""
    rng = _rng(17)
    R, cin, cout = LINEAR["R"], LINEAR["cin"], LINEAR["cout"]
    return grid_b(rng, (R, cin)), grid_b(rng, (cout, cin)), small_ints(rng, (R, cout))


BMM = dict(b=2, H=3, S=70, d=8)


def bmm_problem():
    """Head buffers [b, S, H d] of both operands on the 8-bit grid, dc [b, H, S, S] integers 2^-30."""
    rng = _rng(19)
    b, H, S, d = BMM["b"], BMM["H"], BMM["S"], BMM["d"]
    return grid_b(rng, (b, S, H * d)), grid_b(rng, (b, S, H * d)), small_ints(rng, (b, H, S, S))


def heads(t):
    """[b, S, H d] -> the head view [b, H, S, d] (numpy or torch)."""
    H, d = BMM["H"], BMM["d"]
    return _perm(t.reshape(t.shape[:-1] + (H, d)), (0, 2, 1, 3))


def budget_of(abs_grad, u):
    """log2(max |gradient product on absolute values| / u)."""
    return math.log2(float(np.asarray(abs_grad, np.float64).max()) / u)
