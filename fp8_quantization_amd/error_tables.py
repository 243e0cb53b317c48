"""Error-compensation tables of the approximate FP8 mantissa multiplier.

Data transcribed from the reference's comp_table_NN_list (approx_matmul_whole_v9.py:393-549);
one string per row, '.' = 0, '-' = -1, digits as themselves.  Entry [mA][mB] is subtracted,
times 2^-M, from the exact mantissa product (mult_result_mant, v9:178-184).
get_error_table_NN reproduces the reference's selection logic (v9:555-592), including its
quirks: E4M3 ignores dnsmp_factor; withComp=True on E4M3 is the all-zero table;
unsupported (E, M) raise ValueError; an unlisted dnsmp_factor for E3M4/E2M5 with withComp
raises UnboundLocalError exactly as the reference does.
"""
import hashlib
import os

import numpy as np
import torch

_DEC = {".": 0, "-": -1, "1": 1, "2": 2, "3": 3, "4": 4, "5": 5}

_TABLES = {
    ("E4M3", "nocomp"): (
        "........",
        "....11..",
        "...1111.",
        "..11111.",
        ".11111..",
        ".11111..",
        "..11....",
        "........",
    ),
    ("E3M4", "comp3"): (
        "................",
        "........111111..",
        "....-.....--..1.",
        "...1.....1..1.1.",
        "..-.........1.1.",
        ".....1........1.",
        "..............1.",
        ".......1...-..1.",
        ".1........1.....",
        ".1.1............",
        ".1-.....1.......",
        ".1-....-.....-..",
        ".1.11...........",
        ".1.........-....",
        "..111111........",
        "................",
    ),
    ("E3M4", "nocomp"): (
        "................",
        "........111111..",
        ".....1111111111.",
        "...111111222211.",
        "...111222222211.",
        "..1112222222111.",
        "..1122222222111.",
        "..1122232221111.",
        ".1112222222111..",
        ".1122222221111..",
        ".1122222211111..",
        ".112222111111...",
        ".11221111111....",
        ".1111111111.....",
        "..111111........",
        "................",
    ),
    ("E2M5", "comp3"): (
        "................----------------",
        "..............................--",
        ".........1111111........1111...-",
        "......1111111111.111111111111..-",
        "....-...----....-----......-1..-",
        "........--.................-1..-",
        "...1..........11...11111..--1..-",
        "...1...1....1111.1111111..--1..-",
        "...1--..---.--..----...-11..1..-",
        "..11--..-...-..........-11.....-",
        "..11-...-......1...-..--1......-",
        "..11-......1..11...-..--1......-",
        "..11...1--..-...11..1..........-",
        "..11...1-.......1...1......-...-",
        "..11..11...1...............-...-",
        "..11..11..11.......-...-...-...-",
        "-...-...-...11..111.11.....-11..",
        "-..1-..1-...1...11..11....--11..",
        "-..1-..1-.......1...1.....--11..",
        "-..1-.11-.--...-.........---11..",
        "-..1-.11....11..111.....1...11..",
        "-..1..11........11..........11..",
        "-..1..11..--...........-....1...",
        "-..1..11----...-......--....1...",
        "-.11....1111........1...........",
        "-.11....11.........-............",
        "-.11..--.........---.......-....",
        "-.11----.....-------......--....",
        "-..111111.......11111111........",
        "-...............111111..........",
        "--..............................",
        "----------------................",
    ),
    ("E2M5", "comp4"): (
        "................................",
        "................11111111111111..",
        "........-.........------......1.",
        "......11.........1..........1.1.",
        "....-.....--........-.....1..-1.",
        "................1111......1..-1.",
        "...1..............-..........-1.",
        "...1...1....11...1...........-1.",
        "..-.......-............-....1.1.",
        ".........1...1..1111...-......1.",
        "....-...-.....-...1.....1.....1.",
        "....-......1......1.....1.....1.",
        ".......1....-........-........1.",
        ".......1.1.......-...-.....-..1.",
        "..........-................-..1.",
        "...................-...-...-..1.",
        ".1...1...1........1.......1.....",
        ".1.1.1.1.1...-..................",
        ".1-..1-..111....1...1...........",
        ".1-..1...1.....-.........-......",
        ".1-.-.............1.....1.......",
        ".1-.........--..................",
        ".1-...................1.....1...",
        ".1-.....--.....-............1...",
        ".1........11........1...........",
        ".1.................-............",
        ".1..11..........1.........1.....",
        ".1...........---................",
        ".1.1....1.............11........",
        ".1..----........................",
        "..11111111111111................",
        "................................",
    ),
    ("E2M5", "nocomp"): (
        "................................",
        "................11111111111111..",
        ".........1111111111111112222111.",
        "......1111111111122222222222211.",
        ".....11111112222222223333332211.",
        "....111111222222333333333332211.",
        "...1111122222233333444443322211.",
        "...1111222223333344444443322211.",
        "...1112222233344444444433322211.",
        "..11112223333444555544433322111.",
        "..11122223334445555444333222111.",
        "..11122233344455555444333222111.",
        "..11222333444555554443332222111.",
        "..11222334445555544443332221111.",
        "..11223344455555444433332221111.",
        "..11223344555555444333322221111.",
        ".11123334555554444433322222111..",
        ".11223344555544444333322221111..",
        ".11223344555444443333222221111..",
        ".11223444544444333332222211111..",
        ".11223444444443333322222211111..",
        ".11233444444333333222222111111..",
        ".1123344443333332222222111111...",
        ".1123344333333322222221111111...",
        ".122333333332222222221111111....",
        ".122333333222222222111111111....",
        ".12233222222222221111111111.....",
        ".1222222222221111111111111......",
        ".11222222111111111111111........",
        ".111111111111111111111..........",
        "..11111111111111................",
        "................................",
    ),
}


def _decode(rows):
    return torch.tensor([[_DEC[ch] for ch in r] for r in rows], dtype=torch.int32)


_CACHE = {}


def table(fmt, name):
    key = (fmt, name)
    if key not in _CACHE:
        _CACHE[key] = _decode(_TABLES[key])
    return _CACHE[key]


def get_error_table_NN(expo_width, mant_width, withComp, dnsmp_factor, zero_table_ext=False):
    """Return the int32 [2^M, 2^M] error table (a CPU tensor: it is packed into the kernel
    launch arguments on the host, so no device copy is ever needed).

    zero_table_ext (opt-in extension, not in the reference): a format the reference has no
    table for -- E5M2 above all (BASELINE configs 3 and 5), which v9:588-590 rejects with
    ValueError -- gets an all-zero table instead, i.e. the approx product becomes the Q_R-quantised
    exact product; the v9 arithmetic itself is format-generic and pinned for E5M2 by
    the reference-generated G1 / G2 fixtures."""
    n = 2 ** mant_width
    if (expo_width, mant_width) == (4, 3):
        return torch.zeros((n, n), dtype=torch.int32) if withComp else table("E4M3", "nocomp")
    if (expo_width, mant_width) == (3, 4):
        if not withComp:
            return table("E3M4", "nocomp")
        if dnsmp_factor == 3:
            return table("E3M4", "comp3")
        if dnsmp_factor >= 4:
            return torch.zeros((n, n), dtype=torch.int32)
        raise UnboundLocalError("local variable 'error_table_NN' referenced before assignment")
    if (expo_width, mant_width) == (2, 5):
        if not withComp:
            return table("E2M5", "nocomp")
        if dnsmp_factor == 3:
            return table("E2M5", "comp3")
        if dnsmp_factor == 4:
            return table("E2M5", "comp4")
        if dnsmp_factor == 5:
            return torch.zeros((n, n), dtype=torch.int32)
        raise UnboundLocalError("local variable 'error_table_NN' referenced before assignment")
    if zero_table_ext and 1 <= mant_width <= 5:
        return torch.zeros((n, n), dtype=torch.int32)
    raise ValueError("Invalid combination of expo_width and mant_width")


# Compensation tables of the superseded integer-adder model (approx_matmul_whole_v5.py:362-550,
# transcribed from the values tests/golden/g7_v5.npz recorded from the reference).  Entry
# [mA][mB] is ADDED to the integer code sum (approx_mult_new, v5:159).
_TABLES_V5 = {
    ('E4M3', 'd3'): (
        "........",
        "....11..",
        "...1111.",
        "..11111.",
        ".11111..",
        ".11111..",
        "..11....",
        "........",
    ),
    ('E3M4', 'd3'): (
        "................",
        "................",
        "....1111112211..",
        "....1111112211..",
        "..111122222211..",
        "..111122222211..",
        "..112222222211..",
        "..112222222211..",
        "..112222221111..",
        "..112222221111..",
        "..222222111111..",
        "..222222111111..",
        "..1111111111....",
        "..1111111111....",
        "................",
        "................",
    ),
    ('E3M4', 'd4'): (
        "................",
        "........111111..",
        ".....1111111111.",
        "...111111222211.",
        "...111222222211.",
        "..1112222222111.",
        "..1122222222111.",
        "..1122232221111.",
        ".1112222222111..",
        ".1122222221111..",
        ".1122222211111..",
        ".112222111111...",
        ".11221111111....",
        ".1111111111.....",
        "..111111........",
        "................",
    ),
    ('E2M5', 'd3'): (
        "................1111111111111111",
        "................1111111111111111",
        "................1111111111111111",
        "................1111111111111111",
        "....1111222222223333333333331111",
        "....1111222222223333333333331111",
        "....1111222222223333333333331111",
        "....1111222222223333333333331111",
        "....2222333344445555444422221111",
        "....2222333344445555444422221111",
        "....2222333344445555444422221111",
        "....2222333344445555444422221111",
        "....2222444455554444333322221111",
        "....2222444455554444333322221111",
        "....2222444455554444333322221111",
        "....2222444455554444333322221111",
        "1111333355554444333322222222....",
        "1111333355554444333322222222....",
        "1111333355554444333322222222....",
        "1111333355554444333322222222....",
        "1111333344443333222222221111....",
        "1111333344443333222222221111....",
        "1111333344443333222222221111....",
        "1111333344443333222222221111....",
        "1111333322222222222211111111....",
        "1111333322222222222211111111....",
        "1111333322222222222211111111....",
        "1111333322222222222211111111....",
        "1111111111111111................",
        "1111111111111111................",
        "1111111111111111................",
        "1111111111111111................",
    ),
    ('E2M5', 'd4'): (
        "................................",
        "................................",
        "........1111111111222222222211..",
        "........1111111111222222222211..",
        "....11111122222222223333332222..",
        "....11111122222222223333332222..",
        "....11112222223333444444332222..",
        "....11112222223333444444332222..",
        "..1111222233334444444444332211..",
        "..1111222233334444444444332211..",
        "..1122223333445555444433222211..",
        "..1122223333445555444433222211..",
        "..1122223344555555444433222211..",
        "..1122223344555555444433222211..",
        "..1122334455555544443333222211..",
        "..1122334455555544443333222211..",
        "..1122334455554444333322221111..",
        "..1122334455554444333322221111..",
        "..2222444444444433332222221111..",
        "..2222444444444433332222221111..",
        "..2233444444443333222222111111..",
        "..2233444444443333222222111111..",
        "..22334444333333222222111111....",
        "..22334444333333222222111111....",
        "..22333333222222222211111111....",
        "..22333333222222222211111111....",
        "..222222222222221111111111......",
        "..222222222222221111111111......",
        "..11222211111111111111..........",
        "..11222211111111111111..........",
        "................................",
        "................................",
    ),
    ('E2M5', 'd5'): (
        "................................",
        "................11111111111111..",
        ".........1111111111111112222111.",
        "......1111111111122222222222211.",
        ".....11111112222222223333332211.",
        "....111111222222333333333332211.",
        "...1111122222233333444443322211.",
        "...1111222223333344444443322211.",
        "...1112222233344444444433322211.",
        "..11112223333444555544433322111.",
        "..11122223334445555444333222111.",
        "..11122233344455555444333222111.",
        "..11222333444555554443332222111.",
        "..11222334445555544443332221111.",
        "..11223344455555444433332221111.",
        "..11223344555555444333322221111.",
        ".11123334555554444433322222111..",
        ".11223344555544444333322221111..",
        ".11223344555444443333222221111..",
        ".11223444544444333332222211111..",
        ".11223444444443333322222211111..",
        ".11233444444333333222222111111..",
        ".1123344443333332222222111111...",
        ".1123344333333322222221111111...",
        ".122333333332222222221111111....",
        ".122333333222222222111111111....",
        ".12233222222222221111111111.....",
        ".1222222222221111111111111......",
        ".11222222111111111111111........",
        ".111111111111111111111..........",
        "..11111111111111................",
        "................................",
    ),
}


def table_v5(fmt, name):
    key = ("v5",) + (fmt, name)
    if key not in _CACHE:
        _CACHE[key] = _decode(_TABLES_V5[(fmt, name)])
    return _CACHE[key]


def get_comp_table_NN_v5(expo_width, mant_width, withComp, dnsmp_factor, zero_table_ext=False):
    """v5's get_comp_table_NN (approx_matmul_whole_v5.py:516-541): compensation tables exist only
    with withComp; E3M4 takes dnsmp 3 / >= 4, E2M5 3 / 4 / >= 5; a smaller dnsmp_factor leaves
    the table unassigned (UnboundLocalError), anything else raises ValueError, as there."""
    if (expo_width, mant_width) == (4, 3) and withComp:
        return table_v5("E4M3", "d3")
    if (expo_width, mant_width) == (3, 4) and withComp:
        if dnsmp_factor == 3:
            return table_v5("E3M4", "d3")
        if dnsmp_factor >= 4:
            return table_v5("E3M4", "d4")
        raise UnboundLocalError("local variable 'comp_table_NN' referenced before assignment")
    if (expo_width, mant_width) == (2, 5) and withComp:
        if dnsmp_factor == 3:
            return table_v5("E2M5", "d3")
        if dnsmp_factor == 4:
            return table_v5("E2M5", "d4")
        if dnsmp_factor >= 5:
            return table_v5("E2M5", "d5")
        raise UnboundLocalError("local variable 'comp_table_NN' referenced before assignment")
    if zero_table_ext and withComp and 1 <= mant_width <= 5 and (expo_width, mant_width) not in ((4, 3), (3, 4), (2, 5)):
        return torch.zeros((2 ** mant_width, 2 ** mant_width), dtype=torch.int32)  # (as get_error_table_NN)
    raise ValueError("Invalid combination of expo_width and mant_width")


# ---------------------------------------------------------------------------------------------
# Custom error tables: a user's own multiplier through the same kernels.
# custom_approx_params["error_table"] takes anything load_error_table accepts.
_ROW_CHARS = {".": 0, "-": -1, **{str(d): d for d in range(10)}}
_ROW_OF = {v: k for k, v in _ROW_CHARS.items()}
_ROW_OF[0] = "."


def _parse_rows(text, what):
    """Text in this module's row notation: one row per line, '.' = 0, '-' = -1, digits as themselves;
    blank lines and '#' comments are skipped."""
    rows = []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        for col, ch in enumerate(line):
            if ch not in _ROW_CHARS:
                raise ValueError(f"{what}: line {ln}, column {col + 1}: {ch!r} is not a table entry "
                                 "('.' = 0, '-' = -1, digits 0-9)")
        rows.append([_ROW_CHARS[ch] for ch in line])
    return rows


def load_error_table(spec, mant_width):
    """Normalise a user's error table to a contiguous CPU int32 tensor [2^M, 2^M].

    spec: an integer tensor, an ndarray, a nested list, the path of a .npy file, or the path of a
    text file in this module's row notation.  Entry [m_a][m_b] is subtracted, times 2^-M, from the exact
    significand product (v9:178-184), exactly as the built-in tables are.  ValueError (naming the
    offending entry) for a wrong shape, non-integer values, or entries outside the int8 range the
    kernels' table pack holds."""
    n = 2 ** int(mant_width)
    what = "error table"
    if isinstance(spec, (str, os.PathLike)):
        path = os.fspath(spec)
        what = f"error table {path}"
        if path.endswith(".npy"):
            arr = np.load(path, allow_pickle=False)
        else:
            with open(path) as f:
                rows = _parse_rows(f.read(), what)
            if len({len(r) for r in rows}) > 1:
                bad = next(i for i, r in enumerate(rows) if len(r) != len(rows[0]))
                raise ValueError(f"{what}: row {bad} has {len(rows[bad])} entries, row 0 has {len(rows[0])}")
            arr = np.asarray(rows, dtype=np.int64).reshape(len(rows), -1)
    elif isinstance(spec, torch.Tensor):
        arr = spec.detach().cpu().numpy()
    else:
        try:
            arr = np.asarray(spec)
        except ValueError as e:  # ragged nested list
            raise ValueError(f"{what}: not a rectangular array ({e})") from None
    if arr.dtype == object or arr.dtype.kind not in "iufb":
        raise ValueError(f"{what}: entries must be integers, got dtype {arr.dtype}")
    if arr.shape != (n, n):
        raise ValueError(f"{what}: shape {tuple(arr.shape)}, expected ({n}, {n}) for mant_width {mant_width}")
    if arr.dtype.kind == "f":
        bad = np.argwhere(~(np.isfinite(arr) & (arr == np.round(arr))))
        if len(bad):
            i, j = (int(v) for v in bad[0])
            raise ValueError(f"{what}: entry [{i}][{j}] = {arr[i, j].item()!r} is not an integer")
    arr = arr.astype(np.int64)
    bad = np.argwhere((arr < -128) | (arr > 127))
    if len(bad):
        i, j = (int(v) for v in bad[0])
        raise ValueError(f"{what}: entry [{i}][{j}] = {int(arr[i, j])} is outside the int8 range [-128, 127]")
    return torch.from_numpy(np.ascontiguousarray(arr.astype(np.int32)))


def format_error_table(t):
    """The inverse of the text form load_error_table reads: one string per row ('.' = 0, '-' = -1,
    digits).  ValueError for an entry the notation has no character for (outside -1 .. 9)."""
    arr = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    if arr.ndim != 2:
        raise ValueError(f"error table: shape {tuple(arr.shape)} is not two-dimensional")
    rows = []
    for i, r in enumerate(arr.tolist()):
        for j, v in enumerate(r):
            if v != int(v) or int(v) not in _ROW_OF:
                raise ValueError(f"error table: entry [{i}][{j}] = {v!r} has no character in the row notation "
                                 "(-1 .. 9); save it as .npy instead")
        rows.append("".join(_ROW_OF[int(v)] for v in r))
    return rows


def table_from_multiplier(fn, mant_width):
    """The error table of an approximate significand multiplier.  fn(ma, mb) is the approximate product
    of the significands (2^M + ma) and (2^M + mb) as an integer in units of 2^-2M; the entry is
    ((2^M + ma)(2^M + mb) - fn(ma, mb)) / 2^M.  ValueError when that is not an integer: the model
    subtracts whole units of 2^-M only (v9:182)."""
    M = int(mant_width)
    n = 2 ** M
    rows = []
    for ma in range(n):
        row = []
        for mb in range(n):
            approx = fn(ma, mb)
            if approx != int(approx):
                raise ValueError(f"multiplier({ma}, {mb}) = {approx!r} is not an integer (units of 2^-{2 * M})")
            diff = (n + ma) * (n + mb) - int(approx)
            if diff % n:
                raise ValueError(f"multiplier({ma}, {mb}) = {int(approx)}: the error {diff} x 2^-{2 * M} is not a "
                                 f"whole number of 2^-{M} units, which is all the model subtracts")
            row.append(diff // n)
        rows.append(row)
    return load_error_table(rows, M)


def table_digest(t):
    """sha256 (hex) of the table's int8 bytes, row-major: what result files and ranks compare."""
    arr = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    if np.any(arr != np.round(arr)) or np.any((arr < -128) | (arr > 127)):
        raise ValueError("error table: entries outside the int8 range have no digest")
    return hashlib.sha256(np.ascontiguousarray(arr.astype(np.int8)).tobytes()).hexdigest()
