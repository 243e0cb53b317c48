"""C-ABI surface checks that need no GPU: the library loads and exports every entry point
include/fp8approx.h declares; host-side argument validation reports the reference's errors."""
import ctypes
import os
import re

import pytest

from fp8_quantization_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "fp8approx.h")).read()
    return sorted(set(re.findall(r"\b(fp8a_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_match_binding_table():
    assert declared_symbols() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol():
    L = _lib.load()
    for name in declared_symbols():
        assert hasattr(L, name), name
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value


def test_version_string():
    assert _lib.version().startswith("fp8approx gfx950")


def _a256(x):
    return (x + 255) // 256 * 256


def _units(M, N):
    """The per-64x64-unit fallback marks after the flag word: row, column and tile bytes."""
    nur, nuc = (M + 63) // 64, (N + 63) // 64
    return _a256(nur + nuc + nur * nuc)


def test_workspace_queries_are_host_only():
    L = _lib.load()
    assert L.fp8a_matmul_workspace_size() >= 4
    flag = L.fp8a_matmul_workspace_size()
    # split-K sizing is host logic (no device: 256 CUs assumed): a fraction-of-a-wave shape
    # gets room for partial sums, a many-wave shape does not; every GEMM-shaped query also
    # holds the matrix-core E4M3 path's pre-decoded operands (A words + B column pairs)
    Mr, N, K = 3211264, 64, 147
    kpad, npad = (K + 15) // 16 * 16, (N + 63) // 64 * 64
    assert L.fp8a_matmul_workspace_size_mnk(Mr, N, K) == flag + _units(Mr, N) + (
        _a256(Mr * kpad * 4) + _a256(kpad * npad * 8) + 16384 + _a256(kpad * npad // 16 * 2))
    Mr, N, K = 12544, 512, 4608
    assert L.fp8a_matmul_workspace_size_mnk(Mr, N, K) > flag + _a256(Mr * K * 4) + _a256(K * N // 2 * 8)  # split
    # depthwise (single output channel per group): the tensor-bias kernels need the flag word and
    # the table forms' input words, + the v5 word form's (channel, tap) words
    assert L.fp8a_conv2d_workspace_size(2, 8, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 8) == flag + _a256(2 * 8 * 6 * 6 * 4) + 8 * 9 * 8
    # implicit-GEMM conv: no im2col image; the A words of one group's input slice in a zero
    # border (ph rows above / below; W % 4 == 0: a 4-word left margin and rows rounded up to 4
    # words, here 8 + 4 + 1 -> 16), + the B image (sized for the v5 form's 8 B per (k, n)) + the
    # table image + the E5M2 exponent ranges (unsplit here)
    n2 = L.fp8a_conv2d_workspace_size(2, 3, 8, 8, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    assert n2 == flag + _units(2 * 8 * 8, 4) + _a256(2 * 3 * 10 * 16 * 4) + _a256(32 * 64 * 8) + 16384 + 256
    n3 = L.fp8a_conv2d_workspace_size(2, 3, 7, 7, 4, 3, 3, 1, 1, 1, 1, 1, 1, 1)  # W % 4 != 0: 9 x 9
    assert n3 == flag + _units(2 * 7 * 7, 4) + _a256(2 * 3 * 9 * 9 * 4) + _a256(32 * 64 * 8) + 16384 + 256
    assert L.fp8a_conv2d_workspace_size(256, 3, 224, 224, 4, 7, 7, 2, 2, 3, 3, 1, 1, 1) >= flag + 256 * 3 * 230 * 230 * 4


def test_bad_format_maps_to_value_error():
    L = _lib.load()
    rc = L.fp8a_quant(None, 0, 0, 3, None, 0, None, None)  # E = 0: rejected before any launch
    with pytest.raises(ValueError):
        _lib.check(rc, "fp8a_quant")


def test_bad_extent_maps_to_assertion_error():
    L = _lib.load()
    rc = L.fp8a_matmul(None, 2, None, 1, 1, None, 4, 3, 4, 5, 4, 3, None, None, 0, None, None, 0, None, 0, None)
    with pytest.raises(AssertionError):
        _lib.check(rc, "fp8a_matmul")


def test_word_image_queries_are_host_only():
    """fp8a_word_image_bytes / fp8a_conv2d_wants_image (the word-image hand-off,
    fp8a_conv2d_chain) are host logic: sizes of the zero-bordered image behind its 256-B header,
    and which convolutions would read one (matrix-core path with its A pre-pass: 1; the depthwise
    table form: 2)."""
    import torch
    L = _lib.load()
    # W % 4 == 0: left border widened to 4 words, rows rounded to a multiple of 4
    assert L.fp8a_word_image_bytes(2, 64, 56, 56, 1, 1) == 256 + _a256(2 * 64 * 58 * 64 * 4)
    assert L.fp8a_word_image_bytes(1, 3, 7, 7, 1, 1) == 256 + _a256(3 * 9 * 9 * 4)
    assert L.fp8a_word_image_bytes(0, 3, 7, 7, 1, 1) == 0
    fl = _lib.APPROX | _lib.S2N | _lib.QBMA
    z = torch.zeros((8, 8), dtype=torch.int32)
    z4 = torch.zeros((4, 4), dtype=torch.int32)
    wants = lambda cout, k, p, g, E, M, t, f=fl, s=1: L.fp8a_conv2d_wants_image(  # noqa: E731
        cout, k, k, p, p, g, E, M, _lib.host_ptr(t), f, s, s, 1, 1)
    assert wants(64, 3, 1, 1, 4, 3, z) == 1          # 3x3: the A pre-pass runs
    assert wants(64, 3, 1, 1, 5, 2, z4) == 1         # E5M2 too
    assert wants(64, 1, 0, 1, 4, 3, z) == 0          # 1x1, one column tile: staged from fp32
    assert wants(1024, 1, 0, 1, 4, 3, z) == 1        # 1x1, 16 column tiles: pre-pass
    assert wants(64, 3, 1, 2, 4, 3, z) == 0          # grouped
    assert wants(1, 3, 1, 1, 4, 3, z) == 0           # one output channel: tensor-bias path
    assert wants(64, 3, 1, 1, 3, 4, torch.zeros((16, 16), dtype=torch.int32)) == 0  # E3M4: tile-table kernel
    assert wants(64, 3, 1, 1, 4, 3, z, _lib.APPROX | _lib.QBMA) == 0  # no s2n: not the matrix-core form
    # single-output-channel groups (depthwise): the table form's words (form 2) only with
    # FP8A_CHAIN_TBX=1 (measured a net loss on MobileNetV2)
    tbx = 2 if os.environ.get("FP8A_CHAIN_TBX", "0") not in ("", "0") else 0
    assert wants(64, 3, 1, 64, 4, 3, z) == tbx
    assert wants(64, 3, 1, 64, 5, 2, z4, s=2) == tbx
    assert wants(64, 5, 2, 64, 4, 3, z) == 0         # 5-wide rows: the general tensor-bias kernel
    assert wants(64, 3, 1, 64, 3, 4, torch.zeros((16, 16), dtype=torch.int32)) == 0  # E3M4


# ------------------------------------------------------------------ code-object completeness
# Round 4 met a HIP abort "Cannot find Symbol with name: _ZN4fp8a13v5mx_decode_bENS_8GemmArgsEl":
# the host side registered a kernel the gfx950 code object did not contain (a source edited while
# hipcc ran its device pass and then its host pass; build_native.py now compiles from a snapshot).
# This checks the shipped library on the CPU: every kernel the host side can launch (one
# `__device_stub__` per kernel) has its `.kd` descriptor in a gfx950 code object of .hip_fatbin.
def _elf_sections(data):
    import struct
    assert data[:4] == b"\x7fELF" and data[4] == 2, "not an ELF64 object"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    hdrs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = hdrs[shstrndx]
    nm = lambda off: data[names[4] + off:data.index(b"\0", names[4] + off)].decode()
    return {nm(h[0]): h for h in hdrs}, hdrs


def _elf_symbols(data, symtab=".symtab"):
    import struct
    secs, hdrs = _elf_sections(data)
    if symtab not in secs:
        return []
    st = secs[symtab]
    strtab = hdrs[st[6]]  # sh_link
    out = []
    for off in range(st[4], st[4] + st[5], 24):
        name_off, info = struct.unpack_from("<IB", data, off)
        s0 = strtab[4] + name_off
        out.append((data[s0:data.index(b"\0", s0)].decode(), info & 0xF))
    return out


def _gfx950_code_objects(so):
    import struct
    secs, _ = _elf_sections(so)
    fb = secs[".hip_fatbin"]
    blob = so[fb[4]:fb[4] + fb[5]]
    assert b"CCOB" not in blob[:8], "compressed offload bundle: not handled by this check"
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    cos, pos = [], blob.find(magic)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + 24)
        q = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "gfx950" in triple:
                cos.append(blob[pos + off:pos + off + size])
        pos = blob.find(magic, pos + 24)
    return cos


def test_every_host_kernel_is_in_the_gfx950_code_object():
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    stubs = set()
    for name, _ in _elf_symbols(so, ".dynsym") + _elf_symbols(so, ".symtab"):
        m = re.search(r"(\d+)__device_stub__", name)
        if m:  # <len>__device_stub__<ident> -> <len - 15><ident>: the kernel's device name
            stubs.add(name[:m.start()] + str(int(m.group(1)) - 15) + name[m.end():])
        elif name.startswith("__device_stub__"):  # an extern "C" kernel
            stubs.add(name[len("__device_stub__"):])
    cos = _gfx950_code_objects(so)
    assert cos, "no gfx950 code object in .hip_fatbin"
    kd = set()
    for co in cos:
        kd |= {n[:-3] for n, _ in _elf_symbols(co) if n.endswith(".kd")}
    assert len(stubs) > 20, "no kernel stubs found in the host part of the library"
    missing = sorted(stubs - kd)
    assert not missing, f"kernels registered on the host but absent from the gfx950 code objects: {missing[:5]}"


def _f8mx_expected_instances(xf):
    """gemm_f8mx_kernel's instances of result-grid form xf by launch_shape's rule (k_f8mx.hip), over every value
    of the launch's runtime switches."""
    import itertools

    def xm_pipe(ncg, emit, fix):  # XmPipe<NCG, EMIT, FIX> (gemm_f8mx.h)
        if ncg == 1 and fix:
            return 0
        return 2 if (ncg == 4 and not emit and not fix) else 1

    shapes = [(1, 4), (2, 4)] + ([(4, 8)] if xf != 2 else [])
    names = set()
    for (ncg, rb), af32, emit, skcnt, pipe_opt, wave_rows in itertools.product(shapes, *[(False, True)] * 5):
        fix = xf == 0 and skcnt
        piped = xf != 2 and pipe_opt and not af32
        pipe = xm_pipe(ncg, emit, fix) if piped else 0
        wrows = piped and not fix and ncg == 4 and wave_rows
        names.add("_ZN4fp8a16gemm_f8mx_kernelILi%dELi%dELb%dELi%dELb%dELb%dELi%dELb%dEEEvNS_8GemmArgsE"
                  % (ncg, rb, af32, xf, emit, fix, pipe, wrows))
    return names


def test_f8mx_instances_are_exactly_the_launch_rule():
    """The gfx950 code objects hold exactly the gemm_f8mx_kernel instances launch_shape's rule yields, no more
    (compile time: part 0 alone is over 3 MB of code) and no fewer (a launch would abort).  Counts of the commit
    that wrote the rule down, the same as its parent's: part 0 (E4M3) 36, part 1 (E5M2) 20, part 2 (E5M2
    halved-block) 8."""
    with open(_lib.LIB_PATH, "rb") as f:
        so = f.read()
    built = set()
    for co in _gfx950_code_objects(so):
        built |= {n[:-3] for n, _ in _elf_symbols(co) if n.endswith(".kd") and "gemm_f8mx_kernel" in n}
    expected = [_f8mx_expected_instances(xf) for xf in range(3)]
    assert [len(e) for e in expected] == [36, 20, 8]
    want = set().union(*expected)
    assert sorted(built - want) == [], "instances the rule does not yield"
    assert sorted(want - built) == [], "instances the rule yields but the library lacks"
