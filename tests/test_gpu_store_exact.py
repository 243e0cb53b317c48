"""The fused store against its CPU model, bit for bit (tests/store_ref.py, tests/exact_sums.py).

Every launch here sits on an exact-sum case: its fp32 accumulator is known by bits (tests/test_exact_sums_cpu.py).
From there the store is a fixed chain of fp32 operations -- BN as one fused multiply-add, the activation clamp, the
residual add, the post clamp, the output quantizer, the next convolution's word -- which tests/store_ref.py restates
on the CPU (checked against exact rationals, the oracle and the committed reference outputs by
tests/test_store_ref_cpu.py, which also proves what each case's inputs hold: separating BN draws, differing
neighbour channels, clamped shares, the planted quantizer classes).  So every stored value, every reported
quantizer bias, every emitted word and the image's header words are compared by bits, with no tolerance, through
the production entry points (approx_conv2d(epilogue=, post=, chain=), approx_matmul_block).

Zeros: by value, except that a negative value which a signed quantizer rounds to zero must be -0.0 (store_ref's
docstring gives the rule and the kernel comment it follows).

Sites.  The counters (path_stats, splitk_stats, fallback_stats, fp8a_xm_sign_stats) assert per launch: which GEMM path
moved, that a split launch ran split and an unsplit one did not, that the exact kernel recomputed units exactly in the
off-grid cases, that no depthwise form fell back to the direct kernel, and gemm_f8mx's full tile-table build.  They
cannot tell apart xm_ncg 1 / 2 / 4, xm_wave_rows 0 / 1, the fp32-staged A, tbs 0 / 1 / 2, conv_tb_fast and
conv_tb_direct, or the reduction kernel from the in-launch sum: those are selected by forcing the option and by the
geometry, as in tests/test_gpu_exact_sums.py.

  store_tile_xm (gemm_f8mx)      E4M3 and E5M2 convolutions on h9w16 (Ho Wo = 144: 16-byte NCHW stores; 288 rows, 24
                                 channels: row and column tails) and k1-padded (90: scalar stores), xm_ncg 1 / 2 / 4,
                                 xm_wave_rows 0 / 1, the fp32-staged A (k1-s2x1); (130, 300, 129) row-major, ldc = 129
  store_tile                     gemm_tt (E2M5; E3M4 at K = 16), gemm_tt16 (E3M4 at K = 72 and 64), gemm_fast (one
                                 flag set): the same two geometries and the same matrix; gemm_v5mx and
                                 gemm_fast<TM_V5>: the two geometries (fp8a_matmul_block takes the v9 families only)
  splitk_reduce_kernel           (64, 2304, 64) on gemm_f8mx, gemm_tt and gemm_fast with 2 / 3 / 6 splits (row-major
                                 vector form); with splitk forced on other exact-sum cases (the sum does not depend
                                 on its order): (130, 300, 129) (row-major scalar form), h9w16 (NCHW vector form),
                                 k2x4-s2x3 (K = 64, 30 pixels: NCHW scalar form), on gemm_f8mx and gemm_tt
  splitk_finish_tile             splitk_fixup on (gemm_f8mx E4M3): the split-K shape on the 128 x 64 tile and with
                                 xm_ncg 1 / 2 on the narrow tiles, and the forced-split cases above
  the gated exact kernel         the off-grid twins of the (130, 300, 129) launches: the recomputed units' store
  the depthwise stores           3 x 3 planes of width 4, 9 and 14 under tbs 0 / 1 / 2, tbx_rw 1 / 2, conv_tb_fast,
                                 conv_tb_direct, v5ds 0 / 1 (BN and BN + ReLU6; no block tail)

Every site takes BN alone, BN + ReLU6 and BN + Hardtanh(-0.5, 0.75) (the matrix entry point has no activation); the
block entry points take residual only, residual + clamp + signed quantizer, ReLU clipped at 1.25 + unsigned quantizer,
residual + signed quantizer without a clamp and (linear) bias + residual + quantizer, each with fq_fast 0 and 1.  The
post clamps lie strictly inside the quantizers' ranges, values are planted on both bounds, and the CPU file proves
that a store without the clamp differs.  One case runs a quantizer outside fq_fast_ok (the literal form under fq_fast
= 1).  Emission: gemm_f8mx's store, the split-K reduction, the in-launch sum, the exact kernel and the staged
depthwise producer; word
forms 0 and 1, E4M3 and E5M2 words, signed and unsigned next quantizer, next padding (0, 0), (1, 1), (0, 3), Wo % 4
== 0 and not; the interior words equal store_ref.words, every other word of the image (border, row padding, the tail
up to 256 bytes, the unused header words) is unchanged from a snapshot taken before the launch, header words [0] ..
[6] equal the model's ([2] is the next quantizer's reported bias); one case's next quantizer lies below the exactness
window and its image comes back invalid.

Emission from the gated exact kernel: h9w16 with one off-grid input value (exact_sums.conv_offgrid_cases), whose
recomputed units are stored and emitted by gemm_exact_kernel; `exact_units > 0` is asserted.

Not covered here (named in DESIGN.md §2): the GELU tail (no bit-exact CPU twin), word form 2 (no written layout).

Every case prints `ST <case> site=<counters> fma_sep=<share> ties=<n>` (run with -s: profiles/store_exact/).
"""
import collections

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import exact_sums as xs
from tests import pairs_cases as pc
from tests import store_ref as sr
from tests.test_gpu_exact_sums import _counted, _options
from tests.test_gpu_flag_matrix import _stop_on_device_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fp8_quantization_amd import _lib
    _lib.load()
    orc.lib()


def _dev(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _quant(q):
    return None if q is None else (torch.tensor([q[0]], dtype=torch.float32, device=DEV), q[1], q[2], q[3])


@_stop_on_device_error
def _launch(c, sp, fq_fast):
    """One launch of a store case: (y, reported output-quantizer bias or None, image words or None, snapshot)."""
    from fp8_quantization_amd.approx_ops import approx_conv2d, approx_matmul_block, new_word_image
    b, p = sp["base"], sp["p"]
    tab = torch.from_numpy(np.ascontiguousarray(p["table"], np.int32))
    ss = None if sp["ss"] is None else _dev(sp["ss"])
    pact, plo, phi, pq = sp["post"]
    post = None
    if c["tail"]:
        post = (None if sp["res"] is None else _dev(sp["res"]), pact, plo, phi, _quant(pq))
    opts = dict(c["opts"])
    if fq_fast is not None:
        opts["fq_fast"] = fq_fast
    img = snap = None
    with _options(opts):
        if c["entry"] == "mat":
            W = np.ascontiguousarray(p["B"].T)                  # B = W^T of a row-major [N][K] weight
            out = approx_matmul_block(_dev(p["A"]), _dev(W).t(), b["E"], b["M"], p["bA"], _dev(p["bB"], torch.int32),
                                      p["bR"], tab, b["flags"], bias_epi=ss, post=post)
            y, ob = out[0], out[2]
        else:
            g = b.get("cfg") or xs.tbdw_geo(b)
            kw = dict(flags=b["flags"], stride=xs.pair(g["s"]), padding=xs.pair(g["p"]), dilation=xs.pair(g["d"]),
                      groups=g["g"], epilogue=None if ss is None else (ss,) + tuple(sp["act"]))
            chain = None
            if c["emit"]:
                Bn, C, Ho, Wo = sp["acc"].shape
                ipad = (0, 0) if sp["form"] == 1 else sp["pad"]
                img = new_word_image(Bn, C, Ho, Wo, *ipad, DEV)
                torch.cuda.synchronize()
                snap = img.clone()
                chain = (None, (img, sp["pad"], _quant(sp["nextq"]),
                                torch.tensor([sp["bR_next"]], dtype=torch.int32, device=DEV), sp["Mw"], sp["form"]))
            out = approx_conv2d(_dev(p["x"]), _dev(p["w"]), b["E"], b["M"], p["bA"], _dev(p["bB"], torch.int32), p["bR"],
                                tab, post=post, chain=chain, **kw)
            y, ob = (out[0], out[2]) if isinstance(out, tuple) else (out, None)
        torch.cuda.synchronize()
    words = None if img is None else (img.cpu().numpy().view(np.uint32), snap.cpu().numpy().view(np.uint32))
    return y.cpu().numpy(), None if ob is None else float(ob.cpu().item()), words


def _check_site(c, b, paths, fb, nsplit):
    """What the library's counters can say about the site: the GEMM path that moved (or none, for the tensor-bias
    kernels), split or not, units recomputed by the exact kernel or not, no direct-kernel launch behind a depthwise
    form.  No counter tells xm_ncg 1 / 2 / 4, xm_wave_rows 0 / 1, the fp32-staged A, tbs 0 / 1 / 2, conv_tb_fast or
    conv_tb_direct apart (tests/test_gpu_exact_sums.py says the same of its depthwise cases): those sites are
    selected by the forced option and the geometry, and the name in the log line is the case's label, not a
    measurement."""
    site = c["site"]
    others = lambda *keep: {k: v for k, v in paths.items() if v and k not in keep + ("exact",)}  # noqa: E731
    if b["kind"] == "tbdw":
        want = ("fast",) if b["fam"] == "v5dw" else ()
        assert not others(*want) and fb["tb_launches"] == 0 and fb["exact_units"] == 0, f"{c['id']}: {paths}, {fb}"
        if want:
            assert paths["fast"] == 1, f"{c['id']}: {paths}"
        return
    K = xs.case_K(b)
    want = pc.expected_matmul_path(b["E"], b["M"], xs.case_table(b), b["flags"], K=K)
    assert paths[want] >= 1 and not others(want), f"{c['id']}: expected `{want}`, counters say {paths}"
    assert fb["f32_reruns"] == 0, f"{c['id']}: {fb}"
    if site.startswith("exact+"):
        assert fb["exact_launches"] >= 1 and fb["exact_units"] > 0, f"{c['id']}: the off-grid value recomputed nothing: {fb}"
    else:
        assert fb["exact_units"] == 0, f"{c['id']}: units were recomputed: {fb}"
    if site.startswith("splitk"):
        assert nsplit == 1, f"{c['id']}: the launch did not run split along K"
    elif b["kind"] == "mat":
        assert nsplit == 0, f"{c['id']}: an unexpected split launch"


def _first_bad(same, got, want):
    i = tuple(int(v) for v in np.argwhere(~same)[0])
    return f"{int((~same).sum())} of {same.size} differ; first at {i}: got {got[i]!r} ({got.view(np.uint32)[i]:#010x}) " \
           f"expected {want[i]!r} ({want.view(np.uint32)[i]:#010x})"


def _run_case(c):
    from fp8_quantization_amd import _lib
    sp = xs.store_problem(c["id"])
    b = sp["base"]
    fasts = (0, 1) if (c["tail"] or c["emit"]) else (None,)
    for fq_fast in fasts:
        _lib.xm_sign_stats(reset=True)
        (y, ob, words), paths, fb, nsplit = _counted(lambda: _launch(c, sp, fq_fast))
        signs = _lib.xm_sign_stats(reset=True)
        ran = "+".join(k if v == 1 else f"{k}x{v}" for k, v in paths.items() if v) or "none"
        sep = "-"
        if c["bn"] == "rand":
            nd = sp["acc"].ndim
            twice = sr.mul_add32(sp["acc"], sp["ss"][:, 0].reshape((1, -1) + (1,) * (nd - 2)),
                                 sp["ss"][:, 1].reshape((1, -1) + (1,) * (nd - 2)))
            sep = f"{float(np.mean(twice != sp['bn_raw'])):.3f}"
        ties = "-"
        if sp["q_first"] is not None and sp["required"]:
            cl = xs.store_classes(sp["xin"], sp["q_first"])
            ties = cl["tie_dn"] + cl["tie_up"]
        print(f"ST {c['id']}{'' if fq_fast is None else f' fq_fast={fq_fast}'} site={c['site']}:{ran},split={nsplit},"
              f"exact_units={fb['exact_units']},tb={fb['tb_launches']},signs={signs['half']}/{signs['full']} fma_sep={sep} ties={ties}")
        assert y.shape == sp["y"].shape, (y.shape, sp["y"].shape)
        same = sr.compare(y, sp["y"], sp["neg_zero"])
        assert same.all(), f"{c['id']} fq_fast={fq_fast}: y: " + _first_bad(same, y, sp["y"])
        if sp["post"][3] is not None:
            assert ob == float(sp["obias"]), f"{c['id']}: reported output-quantizer bias {ob}, model {sp['obias']}"
        _check_site(c, b, paths, fb, nsplit)
        if b["fam"] == "f8mx":  # A holds negative values: every gemm_f8mx launch builds both halves of its tile table
            assert signs["half"] == 0 and signs["full"] >= 1, f"{c['id']}: sign build {signs}"
        if c["emit"]:
            img, snap = words
            im, hdr = sp["img"], sp["header"]
            assert img.size == im["words"], (img.size, im["words"])
            assert int(img[0]) == hdr[0], f"{c['id']}: header[0] = {int(img[0])}, model {hdr[0]}"
            # header [1] .. [4] (emit_prep_kernel): the next quantizer's maxval, its float bias -- the bias an emitting
            # launch reports for the next quantizer -- the bits of 2^(1 - bias), and the consumer's bR
            nfb = sr.fq_bias(*sp["nextq"])
            want_hdr = [int(np.float32(sp["nextq"][0]).view(np.uint32)), int(np.float32(nfb).view(np.uint32)),
                        (128 - int(nfb)) << 23, sp["bR_next"] & 0xFFFFFFFF]
            assert [int(v) for v in img[1:5]] == want_hdr, f"{c['id']}: header [1..4] = {list(img[1:5])}, model {want_hdr}"
            if hdr[0] == 1:
                continue                                        # an invalid image: nothing is said about its words
            idx = im["index"]
            got = img[idx]
            bad = got != sp["words"]
            assert not bad.any(), f"{c['id']} fq_fast={fq_fast}: {int(bad.sum())} interior words differ; first at " \
                f"{tuple(int(v) for v in np.argwhere(bad)[0])}: {int(got[bad][0]):#010x} != {int(sp['words'][bad][0]):#010x}"
            outside = np.ones(img.size, bool)
            outside[idx.reshape(-1)] = False
            outside[:7] = False                                 # header words [0] .. [6]: written by design
            moved = np.flatnonzero(outside & (img != snap))
            assert moved.size == 0, f"{c['id']}: {moved.size} words outside the interior were written; first at word " \
                                    f"{int(moved[0])} ({int(snap[moved[0]]):#010x} -> {int(img[moved[0]]):#010x})"
            if sp["form"] == 0:
                assert (int(img[5]), int(img[6] != 0)) == (hdr[5], hdr[6]), \
                    f"{c['id']}: header [5], [6] = {int(img[5])}, {int(img[6])}; model {hdr[5]}, {hdr[6]}"


def _groups():
    out = collections.OrderedDict()
    for c in xs.store_cases():
        out.setdefault(f"{c['site']}|{c['base']}", []).append(c)
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", list(GROUPS), ids=list(GROUPS))
def test_store_bit_exact(group):
    for c in GROUPS[group]:
        _run_case(c)
