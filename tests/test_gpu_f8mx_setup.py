"""gemm_f8mx_kernel's 32-bit tile setup and store indexing against the oracle, bit for bit.

The kernel decomposes blockIdx.x -> (split, tile) -> (row tile, column tile) and its rows -> (image, ho, wo) with
host-made fastdiv magics, and its store (store_tile_xm) advances output offsets by adds.  The shapes here are the
ones where that index code can go wrong, not a workload's: sums drawn by tests/exact_sums.py's construction (every
partial sum an exact float32: the budget is asserted per case), compared with expected(oracle.terms) by bits.

  * 3 x 3 pad-1 convolution on 7 x 7 images, batch 5: M = 245 (two 128-row tiles, the second partial), a 49-pixel
    plane (not a multiple of 4: the scalar NCHW store, a thread's four rows straddling two images); K = 27, N = 70
    (a second, partial column tile); the same on 8 x 8 images, batch 3, stride 2 (16-pixel plane: the 16-byte
    store) and stride 1 (M = 192); a 1 x 1 stride-2 convolution with K = 19, word-staged and fp32-staged
    (af32_maxct 0 / 64); two groups (the store's channel offset coff = 35 inside ctot = 70);
  * each under xm_ncg 4 / 2 / 1 (the 128 x 64 two-slab store, the single-slab 128 x 32 and 256 x 16 tiles);
  * a row-major matrix product 130 x 70 (and x 72: the 16-byte row form) with K = 24; 200 x 96 with K = 800 and
    the split count forced to 2 and 3, summed by the reduction pass and inside the launch;
  * E4M3 and E5M2;
  * a chained 3 x 3 pair through the word image, ReLU and signed producer: the producer's y against the oracle,
    the whole emitted image and its header words [0] / [5] / [6] against the words of the oracle's quantizer on
    y (the function the unchained consumer's pre-pass evaluates), and the chained consumer's output against the
    unchained one's;
  * one launch captured into a graph and replayed three times.

Every launch asserts the f8mx path counter, flag word 0 and no fallback.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_sums as xs
from tests.test_gpu_exact_sums import _counted, _launch_conv, _launch_mat, _options

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = [(4, 3, "nocomp"), (5, 2, "zero")]
ZERO_WORD = 253 << 23

CONVS = {
    "k3-7x7-b5": dict(B=5, cin=3, cout=70, k=3, s=1, p=1, d=1, g=1, hw=7),
    "k3-8x8-b3-s2": dict(B=3, cin=3, cout=70, k=3, s=2, p=1, d=1, g=1, hw=8),
    "k3-8x8-b3": dict(B=3, cin=3, cout=70, k=3, s=1, p=1, d=1, g=1, hw=8),
    "k1-s2-K19": dict(B=5, cin=19, cout=70, k=1, s=2, p=0, d=1, g=1, hw=7),
    "k3-7x7-b5-g2": dict(B=5, cin=6, cout=70, k=3, s=1, p=1, d=1, g=2, hw=7),
    "k3-8x8-b3-g2": dict(B=3, cin=6, cout=70, k=3, s=1, p=1, d=1, g=2, hw=8),
}
NCG = [4, 2, 1]


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


_PROBLEMS = {}


def _problem(c):
    """Operands and oracle terms of a case, as exact_sums.problem_of builds them (these cases are not in its table);
    computed once per problem key and left unchanged."""
    key = (c["pkey"], c["cfg"]["B"] if c["kind"] == "conv" else 0)  # (the conv key leaves the batch out)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    E, M, tab, fl = c["E"], c["M"], xs.case_table(c), c["flags"]
    if c["kind"] == "conv":
        p = xs._conv_problem(c)
        cfg = c["cfg"]
        cols = xs.unfold(p["x"], cfg)
        g, cog = cfg["g"], cfg["cout"] // cfg["g"]
        Kg = cols.shape[1] // g
        p["parts"] = []
        for i in range(g):
            Ag = np.ascontiguousarray(cols[:, i * Kg:(i + 1) * Kg])
            Bg = np.ascontiguousarray(p["w"][i * cog:(i + 1) * cog].reshape(cog, -1).T)
            T = orc.terms(Ag, Bg, E, M, p["bA"], p["bB"][i * cog:(i + 1) * cog], p["bR"], tab, fl)
            p["parts"].append((Ag, Bg, T, slice(i * cog, (i + 1) * cog)))
    else:
        p = xs._mat_problem(c)
        p["parts"] = [(p["A"], p["B"], orc.terms(p["A"], p["B"], E, M, p["bA"], p["bB"], p["bR"], tab, fl), slice(None))]
    p["table"] = tab
    assert xs.case_budget_log2(p) <= xs.BUDGET_LOG2, f"{c['id']}: the drawn terms miss the exact-sum budget"
    _PROBLEMS[key] = p
    return p


def _assert_f8mx(cid, paths, flag, fb):
    others = {k: v for k, v in paths.items() if v and k != "f8mx"}
    assert paths["f8mx"] >= 1 and not others, f"{cid}: expected the f8mx path alone, counters say {paths}"
    assert flag == 0 and fb == dict(exact_launches=0, exact_units=0, f32_reruns=0, tb_launches=0), \
        f"{cid}: flag {flag}, fallback counters {fb}"


def _check(c, got, flag, paths, fb):
    p = _problem(c)
    print(f"SETUP {c['id']} paths={ {k: v for k, v in paths.items() if v} } flag={flag} "
          f"budget=2^{xs.case_budget_log2(p):.2f}")
    for (_, _, T, sl) in p["parts"]:
        xs.assert_same(got[:, sl], xs.expected(T), c["id"], T)
    _assert_f8mx(c["id"], paths, flag, fb)


# ------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("E,M,table", FORMATS, ids=["E4M3", "E5M2"])
@pytest.mark.parametrize("geo", list(CONVS))
def test_conv_index_shapes_bit_exact(geo, E, M, table):
    cfg = CONVS[geo]
    opt_sets = [{"xm_ncg": n} for n in NCG]
    if cfg["k"] == 1:  # word-staged and fp32-staged A (its own aoff[] form)
        opt_sets = [dict(o, af32_maxct=a) for o in opt_sets for a in (0, 64)]
    for o in opt_sets:
        c = xs._conv("f8mx", E, M, table, xs.FL, cfg, opts=o, tag=xs._opt_tag(o))
        (y, flag), paths, fb, nsplit = _launch_conv(c, _problem(c))
        _check(c, y.transpose(0, 2, 3, 1).reshape(-1, y.shape[1]), flag, paths, fb)
        assert paths["f8mx"] == cfg["g"] and nsplit == 0, (paths, nsplit)


# ------------------------------------------------------------------------------------------ matrix products
@pytest.mark.parametrize("E,M,table", FORMATS, ids=["E4M3", "E5M2"])
@pytest.mark.parametrize("N", [70, 72])
def test_matrix_row_major_bit_exact(N, E, M, table):
    for n in NCG:
        o = {"xm_ncg": n, "splitk": 1}
        c = xs._mat("f8mx", E, M, table, xs.FL, (130, 24, N), opts=o, tag=xs._opt_tag(o))
        (got, flag), paths, fb, nsplit = _launch_mat(c, _problem(c))
        _check(c, got, flag, paths, fb)
        assert paths["f8mx"] == 1 and nsplit == 0, (paths, nsplit)


@pytest.mark.parametrize("E,M,table", FORMATS, ids=["E4M3", "E5M2"])
@pytest.mark.parametrize("S", [2, 3])
def test_forced_split_bit_exact(S, E, M, table):
    """200 x 96 with K = 800: blockIdx.x / tiles is the split.  The reduction pass and the in-launch sum (E4M3)."""
    for fix in (0, 1):
        for n in (4, 2):
            o = {"splitk": S, "splitk_fixup": fix, "xm_ncg": n}
            c = xs._mat("f8mx", E, M, table, xs.FL, (200, 800, 96), opts=o, tag=xs._opt_tag(o))
            (got, flag), paths, fb, nsplit = _launch_mat(c, _problem(c))
            _check(c, got, flag, paths, fb)
            assert paths["f8mx"] == 1 and nsplit == 1, (paths, nsplit)


# ------------------------------------------------------------------------------------------ the emitting store
def _words(q, M, bR):
    """xm_word_a of on-grid values q (gemm_f8mx.h): scale exponent 254 + xb - bR - (exponent field) in bits 23-30,
    the row 8 s + m in bits 3-6; zeros the zero word."""
    u = np.ascontiguousarray(q, np.float32).view(np.uint32).astype(np.int64)
    ua = u & 0x7FFFFFFF
    xb = 7 if M == 3 else 15
    se = 254 + xb - bR - ((ua >> 23) & 0xFF)
    assert ((se >= 1) & (se <= 252))[ua != 0].all(), "a word outside the scale range: choose another bias"
    row = (u >> 31) * 8 + ((ua >> (23 - M)) & ((1 << M) - 1))
    return np.where(ua == 0, ZERO_WORD, (se << 23) | (row << 3)).astype(np.uint32)


@pytest.mark.parametrize("E,M,table", FORMATS, ids=["E4M3", "E5M2"])
@pytest.mark.parametrize("producer", ["relu", "signed"])
@pytest.mark.parametrize("hw", [7, 8])
def test_chained_pair_through_the_word_image(hw, producer, E, M, table):
    from fp8_quantization_amd import _lib
    from fp8_quantization_amd.approx_ops import approx_conv2d, bn_act_epilogue, new_word_image
    cfg = dict(B=5, cin=3, cout=70, k=3, s=1, p=1, d=1, g=1, hw=hw)
    Bn, cmid, cout2 = cfg["B"], cfg["cout"], 16
    c = xs._conv("f8mx", E, M, table, xs.FL, cfg, tag=f"chain-{producer}")
    p = _problem(c)
    want = np.concatenate([xs.expected(T) for (_, _, T, _) in p["parts"]], 1)  # [B hw hw, cmid]
    want = np.ascontiguousarray(want.reshape(Bn, hw, hw, cmid).transpose(0, 3, 1, 2))
    if producer == "relu":
        want = np.maximum(want, np.float32(0.0))
    dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)  # noqa: E731
    x, w1, bW1 = dev(p["x"]), dev(p["w"]), dev(p["bB"], torch.int32)
    tab = torch.from_numpy(np.ascontiguousarray(p["table"]))
    ep = bn_act_epilogue(torch.zeros(cmid), torch.ones(cmid), torch.ones(cmid), torch.zeros(cmid), 0.0,
                         torch.nn.ReLU() if producer == "relu" else None)  # scale 1, shift 0: exact
    ep = (ep[0].to(DEV),) + tuple(ep[1:])
    b = 2 ** (E - 1)
    mx2 = 5.5
    qin2 = (torch.tensor([mx2], device=DEV), 8, M, 1)
    bR2 = torch.tensor([b], dtype=torch.int32, device=DEV)
    g = torch.Generator().manual_seed(5)
    w2 = torch.ldexp(1.0 + torch.randint(0, 2 ** M, (cout2, cmid, 3, 3), generator=g).float() / 2 ** M,
                     torch.randint(-8, 0, (cout2, cmid, 3, 3), generator=g).int()).to(DEV)
    bW2 = torch.full((cout2,), b + 6, dtype=torch.int32, device=DEV)
    kw = dict(flags=xs.FL, padding=(1, 1))
    for n in NCG:
        with _options({"xm_ncg": n}):
            img = new_word_image(Bn, cmid, hw, hw, 1, 1, DEV)
            out, paths, fb, nsplit = _counted(lambda: approx_conv2d(
                x, w1, E, M, p["bA"], bW1, p["bR"], tab, epilogue=ep,
                chain=(None, (img, (1, 1), qin2, bR2, M)), **kw)[0].cpu().numpy())
            _assert_f8mx(f"{c['id']} ncg {n}", paths, 0, fb)
            assert nsplit == 0, "the producer's own store is meant, not the reduction's"
            xs.assert_same(out, want, f"{c['id']} ncg {n}: y")
            # the image: header + words of the oracle's quantizer on y, inside the zero border
            q, _ = orc.fp8_fake_quant(want, mx2, 8 - 1 - M, M)
            words = img.view(torch.int32).cpu().numpy().view(np.uint32)
            awW = hw + 2 if hw % 4 else (hw + 4 + 1 + 3) // 4 * 4
            pwl = 1 if hw % 4 else 4
            ref = np.full((Bn, cmid, hw + 2, awW), ZERO_WORD, np.uint32)
            ref[:, :, 1:1 + hw, pwl:pwl + hw] = _words(q, M, b)
            got = words[64:64 + ref.size].reshape(ref.shape)
            assert np.array_equal(got, ref), f"ncg {n}: {np.count_nonzero(got != ref)} image words differ"
            nz = ref[ref != ZERO_WORD]
            assert int(words[0]) == 0, "the emitted image was flagged invalid"
            assert int(words[5]) == int((255 - (nz >> 23)).max()), "header word [5]: the scale-exponent extreme"
            assert int(words[6]) == int(bool((nz & 0x40).any())), "header word [6]: a negative word was written"
            assert bool(words[6]) == (producer == "signed")
            # the consumer: from the image, and unchained through its own pre-pass
            y = torch.from_numpy(out).to(DEV)
            (z2, ib2), paths2, fb2, _ = _counted(lambda: approx_conv2d(y, w2, E, M, None, bW2, bR2, tab, qin=qin2,
                                                                        chain=(img, None), **kw)[:2])
            (z1, ib1), paths1, fb1, _ = _counted(lambda: approx_conv2d(y, w2, E, M, None, bW2, bR2, tab, qin=qin2,
                                                                        **kw)[:2])
            torch.cuda.synchronize()
            assert paths1 == paths2 and paths1["f8mx"] == 1 and paths1["fast"] == 0 and fb1 == fb2, (paths1, paths2, fb1, fb2)
            assert torch.equal(z1.view(torch.int32), z2.view(torch.int32)), "consumer output differs with the image"
            assert torch.equal(ib1, ib2)


# ------------------------------------------------------------------------------------------ capture and replay
def test_captured_launch_replays_bit_exact():
    from fp8_quantization_amd.approx_ops import approx_conv2d
    from tests.test_gpu_graph import _capture
    E, M, table = FORMATS[0]
    c = xs._conv("f8mx", E, M, table, xs.FL, CONVS["k3-7x7-b5"], tag="graph")
    p = _problem(c)
    want = np.concatenate([xs.expected(T) for (_, _, T, _) in p["parts"]], 1)
    x, w = torch.from_numpy(p["x"]).to(DEV), torch.from_numpy(p["w"]).to(DEV)
    bW = torch.from_numpy(np.ascontiguousarray(p["bB"], np.int32)).to(DEV)
    tab = torch.from_numpy(np.ascontiguousarray(p["table"]))
    with _options({"xm_ncg": 4}):
        g, out, _ = _capture(lambda: approx_conv2d(x, w, E, M, p["bA"], bW, p["bR"], tab, flags=xs.FL, padding=(1, 1)))
        for i in range(3):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            got = out.cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, out.shape[1])
            xs.assert_same(got, want, f"replay {i}")
