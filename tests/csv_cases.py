"""CSV texts that put row ends, delimiters, row starts, numbers and the chunk
end on every edge of the CSV tile path (src/gpu/csv_kernels.hip), their
expected arrays from the Python oracle (pyref.parse_csv), and a small model of
what sends a chunk to the exact kernels.

Helper of test_csv_cases_cpu.py and test_gpu_csv_edges.py.  Pure Python and
numpy, deterministic, built once per process.  Every file is ONE chunk for the
GPU parser (the tests read it with a chunk size above the file size), so a
byte offset in the file is a byte offset in the chunk; every offset the
builder means to hit is recorded as a mark and checked when the case is built.
"""
import collections
import functools
import itertools

import numpy as np

import pyref

# the geometry of the walk: kTileBytes (src/gpu/kernels.h), kStep, the 16 bytes
# a lane classifies per step, kExt and kListCap (src/gpu/csv_kernels.hip)
TILE = 8192
STEP = 1024
LANE = 16
EXT = 4096
LIST_CAP = 512
MAX_FILE = 64 * 1024

GROUPS = ("a", "b", "c", "d", "e", "f", "g", "h")
# the code shapes chosen from (label_column, weight_column): positional count
# + kCol0 fill (twice), positional count + general fill, walking count +
# general fill with the column scan
SHAPES = ((-1, -1), (0, -1), (-1, 0), (2, -1))
G_LABELS = (0, 1, 511, 512, 513, 2999)
G_WEIGHTS = (-1, 0, 1500, 2999, 4000)
# a weight column equal to the label column is refused by both parsers
# (csv_parser.h and device_parser.cc CHECK it): the tests pin the refusal
REFUSED = ((1, 1), (0, 0))
G_CONFIGS = tuple(c for c in itertools.product(G_LABELS, G_WEIGHTS) if c[0] != c[1])
TAB_GROUPS = ("a", "b", "e")
INDEX64_GROUPS = ("c", "g")

# group e: file size minus the start of its last tile's predecessor (see _group_e)
END_SIZES = (1, 15, 16, 17, STEP - 1, STEP, STEP + 1, TILE,
             TILE + STEP, TILE + 2 * STEP, TILE + 3 * STEP, TILE + 4 * STEP)
END_BYTES = {"digit": "7", "delim": ",", "cr": "\r", "blank": " "}  # each also before a final \\n

Case = collections.namedtuple("Case", "name group delim text expect marks")


def configs(group):
    if group == "g":
        return SHAPES + tuple(c for c in G_CONFIGS if c not in SHAPES)
    return SHAPES


def delims(group):
    return (",", "\t") if group in TAB_GROUPS else (",",)


def query(label_column, weight_column, delim):
    q = f"?label_column={label_column}&weight_column={weight_column}"
    return q + ("&delimiter=\t" if delim != "," else "")


class Builder:
    """appends text; `,` in what it is given stands for the case's delimiter"""

    def __init__(self, delim):
        self.delim = delim
        self.buf = []
        self.n = 0
        self.marks = []
        self.filler = 0

    def tr(self, s):
        return s.replace(",", self.delim)

    def put(self, s):
        self.buf.append(self.tr(s))
        self.n += len(s)

    def mark(self, off, ch):
        self.marks.append((off, self.tr(ch)))

    def fill_to(self, off):
        """short filler rows (`1.5,2,3` style) up to exactly `off`; the last one ends there"""
        gap = off - self.n
        assert gap == 0 or gap >= 2, (off, self.n)
        while gap >= 16:
            self.filler += 1
            self.put(f"{self.filler % 10}.5,2,3\n")
            gap -= 8
        if gap >= 8:
            self.put("4.5,2," + "3" * (gap - 7) + "\n")
        elif gap >= 2:
            self.put("7" * (gap - 1) + "\n")
        assert self.n == off

    def put_at(self, off, s, lead="1.5,2,3"):
        """`s` with its first byte at `off`, behind `lead` in the same row"""
        self.fill_to(off - len(lead))
        self.put(lead)
        assert self.n == off
        for k, ch in enumerate(s):
            if k == 0 or ch in "\r\n":
                self.mark(off + k, ch)
        self.put(s)

    def finish(self, name, group, expect, tail=300, newline=True):
        if tail:
            self.fill_to(self.n + tail)
        text = "".join(self.buf)
        if not newline:
            assert text.endswith("\n")
            text = text[:-1]
        assert len(text) < MAX_FILE, (name, len(text))
        for off, ch in self.marks:
            assert text[off] == ch, (name, off, ch, text[off])
        return Case(f"{group}_{name}", group, self.delim, text, expect, tuple(self.marks))


def long_row(nbytes, seed=0):
    """`nbytes` of `d.25,` fields without a line end; the last byte is a digit"""
    s = "".join(f"{(seed + i) % 9 + 1}.25," for i in range(nbytes // 5 + 1))[:nbytes]
    return s[:-1] + "7" if nbytes else s


# ---------------------------------------------------------------------------
# a. row ends


def _a_edge(b, T, kind):
    if kind < 4:
        b.put_at(T - 2 + kind, "\n")
    elif kind == 4:
        b.put_at(T - 1, "\r\n")
    elif kind == 5:
        b.put_at(T - 2, "\n\n\n\n")
    else:
        b.put_at(T - 2, "\r\n\r\n")
    # step and lane edges inside the tile
    b.put_at(T + STEP - 1, "\n")
    b.put_at(T + 2 * STEP, "\n")
    b.put_at(T + 3 * STEP - 1, "\r\n")
    b.put_at(T + 4 * STEP + LANE * 5 - 1, "\n")
    b.put_at(T + 4 * STEP + LANE * 9, "\n")
    b.put_at(T + 4 * STEP + LANE * 13 - 1, "\r\n")


def _group_a(delim):
    out = []
    for name, kinds in (("edges1", (0, 1, 2, 3)), ("edges2", (4, 5, 6))):
        b = Builder(delim)
        for t, kind in enumerate(kinds):
            _a_edge(b, (t + 1) * TILE, kind)
        out.append(b.finish(name, "a", "tile"))
    # tile 0 (carry_eol = 1 without a read): the file opens with line ends
    for name, head in (("tile0_nl", "\n"), ("tile0_nl4", "\n\n\n\n"), ("tile0_crlf", "\r\n"),
                       ("tile0_crlf2", "\r\n\r\n"), ("tile0_row", "")):
        b = Builder(delim)
        b.put(head)
        for k in range(len(head)):
            b.mark(k, head[k])
        b.put_at(STEP - 1, "\n")
        b.put_at(STEP + LANE, "\r\n")
        out.append(b.finish(name, "a", "tile"))
    # a tile of line ends only: as tile 0 it owns nothing; behind a tile with
    # rows, that tile finds no row start within its extension (exact kernels)
    b = Builder(delim)
    b.put("\n" * (TILE // 2) + "\r\n" * (TILE // 4))
    b.mark(0, "\n")
    b.mark(TILE - 1, "\n")
    out.append(b.finish("eol_tile0", "a", "tile", tail=900))
    b = Builder(delim)
    b.fill_to(TILE)
    b.put("\n" * TILE)
    b.mark(TILE, "\n")
    b.mark(2 * TILE - 1, "\n")
    out.append(b.finish("eol_tile1", "a", "exact", tail=6000))
    return out


# ---------------------------------------------------------------------------
# b. delimiters on an edge

_B_FOLLOW = (("digit", "7,8\n"), ("eol", "\n"), ("delim", ",9\n"), ("blank", " 4.5,6\n"))


def _b_positions(T):
    return (("tile", T - 1), ("lane", T + LANE * 5 + LANE - 1), ("step", T + 2 * STEP - 1))


def _group_b(delim):
    out = []
    b = Builder(delim)
    for t, (_, follow) in enumerate(_B_FOLLOW):
        for _, pos in _b_positions((t + 1) * TILE):
            b.put_at(pos, "," + follow, lead="1.5,2")
    out.append(b.finish("edges", "b", "tile"))
    for where, pos in _b_positions(TILE):
        b = Builder(delim)
        b.put_at(pos, ",", lead="1.5,2")
        out.append(b.finish(f"end_{where}", "b", "tile", tail=0))
    # tile 0: the file opens with a delimiter (an empty first field)
    b = Builder(delim)
    b.put(",5,6\n")
    b.mark(0, ",")
    b.put_at(LANE - 1, ",\n", lead="2")
    out.append(b.finish("tile0", "b", "tile"))
    return out


# ---------------------------------------------------------------------------
# c. ownership


def _row_until(b, start, nl_at, seed=0):
    """a row from `start` whose line end is the byte `nl_at`"""
    b.fill_to(start)
    b.mark(start, long_row(5, seed)[0])
    b.put(long_row(nl_at - start, seed))
    b.mark(nl_at, "\n")
    b.put("\n")


def _group_c(delim):
    out = []
    b = Builder(delim)
    T = TILE
    b.put_at(T - 1, "4.5,2,3\n", lead="1.5,2,3\n")  # a row that starts at the last byte of a tile
    T += TILE
    b.fill_to(T)                                   # first row start: lane 0, bit 0
    b.mark(T - 1, "\n")
    b.mark(T, str((b.filler + 1) % 10))
    T += TILE
    _row_until(b, T - 100, T + STEP - 2)            # lane 63, bit 15 of step 0
    b.put_at(T + STEP - 1, "6.5,2,3\n", lead="")
    T += TILE
    _row_until(b, T - 100, T + LANE * 7 + 4, 3)     # mid-slice
    b.put_at(T + LANE * 7 + 5, "8.5,2,3\n", lead="")
    out.append(b.finish("starts", "c", "tile"))
    # Walk::pre: the previous row's last 1, 2 and 500 fields open the tile
    b = Builder(delim)
    b.put_at(TILE - 1, ",7\n", lead="1.5,2")
    b.put_at(2 * TILE - 1, ",7,8\n", lead="1.5,2")
    b.put_at(3 * TILE - 1, "," + "".join(f"{k % 10}," for k in range(499)) + "1\n", lead="1.5,2")
    out.append(b.finish("pre", "c", "tile"))
    # a tile without a row start inside one long row: the chunk's last tile
    # (tile path), or a full tile (the row is past the extension: exact)
    for name, nl in (("norow_end", False), ("norow_end_nl", True)):
        b = Builder(delim)
        b.fill_to(2 * TILE - 6000)
        b.put(long_row(9000 - 1, 2) + "\n")
        out.append(b.finish(name, "c", "tile", tail=0, newline=nl))
    b = Builder(delim)
    _row_until(b, TILE - 500, TILE + 9500, 4)
    out.append(b.finish("norow_full", "c", "exact", tail=2000))
    return out


# ---------------------------------------------------------------------------
# d. the extension limit


def _group_d(delim):
    out = []
    T = TILE
    end = T + TILE + EXT
    for name, nl_at, expect in (("ext_m2", end - 2, "either"), ("ext_m1", end - 1, "either"),
                                ("ext_0", end, "either"), ("ext_4000", T + TILE + 4000, "tile"),
                                ("ext_5000", T + TILE + 5000, "exact")):
        b = Builder(delim)
        _row_until(b, T + TILE - 200, nl_at, 1)
        out.append(b.finish(name, "d", expect, tail=1000))
    return out


# ---------------------------------------------------------------------------
# e. the chunk end


def _group_e(delim):
    out = []
    T = TILE
    for size, (last, ch), nl in itertools.product(END_SIZES, END_BYTES.items(), (False, True)):
        n = T + size
        # the last row crosses into the last tile; from TILE on it starts in
        # tile 1 and is 5500 bytes long (size TILE + 4 * STEP: it ends with
        # the last extension step, and the bytes at T + 10240 are digits)
        start = n - (300 if size <= STEP + 1 else 5500)
        end = ch + "\n" if nl else ch
        if len(end) > size:
            continue  # (one byte past the tile start: no room for both)
        b = Builder(delim)
        b.fill_to(start)
        b.put(long_row(n - start - len(end), size) + end)
        b.mark(n - len(end), ch)
        b.mark(n - 1, end[-1])
        if size == TILE + 4 * STEP:
            assert "".join(b.buf)[T + 10 * STEP].isdigit()
        out.append(b.finish(f"end_{size}_{last}" + ("_nl" if nl else ""), "e", "tile", tail=0))
        assert len(out[-1].text) == n
    return out


# ---------------------------------------------------------------------------
# f. field and row density


def _dense(nfields):
    """1024 bytes that hold `nfields` field starts (behind a delimiter)"""
    if nfields <= LIST_CAP:
        s = "".join(f"{k % 10}," for k in range(nfields - 1))
        return s + "8" * (STEP - len(s) - 1) + ","
    if nfields == STEP:
        return "," * STEP
    extra = nfields - LIST_CAP  # `d,,,`: three starts in four bytes
    s = "".join(f"{k % 10}," for k in range(LIST_CAP - 2 * extra)) + "1,,," * extra
    assert len(s) == STEP
    return s


def step_field_starts(text, delim):
    """field starts in every aligned 1 KiB step, and the row starts, as the
    kernels see them: a row starts behind a line end (or the chunk start), a
    field at a row start or behind a delimiter, unless a line end stands there"""
    raw = np.frombuffer(text.encode("latin-1"), np.uint8)
    e = (raw == 10) | (raw == 13)
    d = raw == ord(delim)
    pe = np.concatenate([[True], e[:-1]])
    pd = np.concatenate([[False], d[:-1]])
    lm = ~e & pe
    fm = lm | (pd & ~e)
    pad = (-len(raw)) % STEP
    per_step = np.concatenate([fm, np.zeros(pad, bool)]).reshape(-1, STEP).sum(1)
    return per_step, np.flatnonzero(lm)


def exact_reasons(text, delim):
    """why the tile path gives this chunk up (empty: it does not)"""
    per_step, starts = step_field_starts(text, delim)
    why = []
    if per_step.max(initial=0) > LIST_CAP:
        why.append(f"{int(per_step.max())} field starts in step {int(per_step.argmax())}")
    n = len(text)
    for t in range((n + TILE - 1) // TILE):
        tile_end = (t + 1) * TILE
        if not ((starts >= t * TILE) & (starts < tile_end)).any() or n <= tile_end + EXT:
            continue
        if not ((starts >= tile_end) & (starts < tile_end + EXT)).any():
            why.append(f"no row start within {EXT} bytes of the end of tile {t}")
    return why


def _group_f(delim):
    out = []
    s0 = TILE + 2 * STEP
    plan = [(511, 0, "tile"), (512, 0, "tile"), (513, 0, "exact"), (1024, 0, "exact"),
            (511, 1, "tile"), (512, 1, "tile"), (513, 1, "tile"), (514, 1, "exact"),
            (1024, 1, "exact")]
    for nfields, shift, expect in plan:
        b = Builder(delim)
        b.fill_to(s0 - 100)
        content = _dense(nfields)
        b.put(long_row(100 + shift - 1, nfields) + ",")
        b.mark(s0 + shift, content[0])
        b.put(content + "5,6\n")
        out.append(b.finish(f"fields_{nfields}_shift{shift}", "f", expect))
    for shift in (0, 1):
        b = Builder(delim)
        b.fill_to(s0 - 8)
        b.put("1.5,2," + "3" * (1 + shift) + "\n")
        b.mark(s0 + shift, "0")
        b.put("".join(f"{k % 10}\n" for k in range(512)))
        out.append(b.finish(f"rows_512_shift{shift}", "f", "tile"))
    return out


# ---------------------------------------------------------------------------
# g. columns across steps


def _group_g(delim):
    b = Builder(delim)
    start = TILE + TILE // 2
    b.fill_to(start)
    b.mark(start, "0")
    b.put("".join(f"{k % 10}," for k in range(3000)) + "\n")  # 512 field starts per step
    b.mark(start + 6000, "\n")
    # short rows without the label and / or weight column
    b.put("5\n5,6\n5,6,\n,\n,,7\n")
    edge = TILE + 10 * STEP
    b.put_at(edge - 1, ",\n", lead="5,6")  # a trailing delimiter on a step edge ends a short row
    b.put("1,2,3,4\n")
    return [b.finish("row3000", "g", "tile")]


# ---------------------------------------------------------------------------
# h. numbers across the ring


def _h_numbers():
    digits = "12345678901234567890"
    nums = []
    for n in range(1, 21):
        nums.append(digits[:n])
        k = (n + 1) // 2
        nums.append(digits[:k] + "." + digits[k:n])
    return nums


H_SHAPES = ("1e3", "2.5E-2", "123456789.5", "-1.5e-3")


def _group_h(delim):
    places = [(s, k) for s in _h_numbers() for k in range(1, 16)]
    places += [(s, k) for s in H_SHAPES for k in range(1, len(s))]
    # every (number, k) once at the end of an even step (slot 0 -> slot 1) and
    # once at the end of an odd step (slot 1 -> the mirror of slot 0's head)
    edges = [(s, k, parity) for s, k in places for parity in (0, 1)]
    out = []
    per_file = 6 * (TILE // STEP)
    for f in range(0, len(edges), per_file):
        b = Builder(delim)
        for j, (s, k, parity) in enumerate(edges[f:f + per_file]):
            assert j % 2 == parity
            edge = TILE + (j + 1) * STEP  # step j of its tile ends here
            b.put_at(edge - k, s + ",3\n", lead="1.5,")
        out.append(b.finish(f"ring{f // per_file}", "h", "tile"))
    return out


_BUILD = {"a": _group_a, "b": _group_b, "c": _group_c, "d": _group_d, "e": _group_e,
          "f": _group_f, "g": _group_g, "h": _group_h}


@functools.lru_cache(maxsize=None)
def cases(group, delim=","):
    out = _BUILD[group](delim)
    assert len({c.name for c in out}) == len(out)
    return out


def write(case, path):
    with open(path, "wb") as f:
        f.write(case.text.encode("latin-1"))
    return path


@functools.lru_cache(maxsize=None)
def _oracle(text, delim, label_column, weight_column):
    rows = pyref.parse_csv(text, label_column, delim, weight_column)
    lens = [len(r[1]) for r in rows]
    weight = [r[2] for r in rows] if weight_column >= 0 else [1.0] * len(rows)
    return {
        "label": np.array([r[0] for r in rows], np.float32),
        "weight": np.array(weight, np.float32),
        "offset": np.cumsum([0] + lens).astype(np.uint64),
        "index": np.array([i for n in lens for i in range(n)], np.uint64),
        "value": np.array([v for r in rows for v in r[1]], np.float32),
    }


def oracle(case, label_column, weight_column):
    """the arrays of pyref.concat_blocks that the reference grammar gives"""
    return _oracle(case.text, case.delim, label_column, weight_column)


def first_difference(case, got, want):
    """None, or a message: the array, the first differing row, its byte offset"""
    _, starts = step_field_starts(case.text, case.delim)
    for k in ("offset", "label", "weight", "index", "value"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("label", "weight", "value"):
            g, w = g.astype(np.float32).view(np.uint32), w.astype(np.float32).view(np.uint32)
        if g.shape == w.shape and np.array_equal(g, w):
            continue
        m = min(len(g), len(w))
        bad = np.flatnonzero(g[:m] != w[:m])
        at = int(bad[0]) if len(bad) else m
        row = at
        if k == "offset":
            row = max(at - 1, 0)
        elif k in ("index", "value"):
            row = int(np.searchsorted(np.asarray(want["offset"]), at, side="right")) - 1
        where = int(starts[row]) if row < len(starts) else -1
        show = lambda a: (a[at] if at < len(a) else None)  # noqa: E731
        return (f"{case.name} (delimiter {case.delim!r}): {k}[{at}] is {show(got[k])!r}, want "
                f"{show(want[k])!r} (lengths {len(g)} / {len(w)}); row {row} starts at byte {where} "
                f"= tile {where // TILE} + {where % TILE}: {case.text[where:where + 48]!r}; "
                f"marks {case.marks[:8]}")
    return None


# ---------------------------------------------------------------------------
# the chunk-end sizes of group e for the LibSVM / LibFM tile fill


@functools.lru_cache(maxsize=None)
def svm_end_cases(fmt):
    """(name, text): files of every END_SIZES length past a tile start whose
    last line (3000 or 5500 bytes) crosses into the last tile and ends in a
    digit, a blank or `\\r`, with and without a final line end"""
    tok = (lambda i: f"{i % 9000 + 1}:0.{i % 97}") if fmt == "libsvm" else \
          (lambda i: f"{i % 7}:{i % 9000 + 1}:0.{i % 97}")
    out = []
    ends = {"digit": "", "blank": " ", "cr": "\r"}
    ends.update({k + "_nl": v + "\n" for k, v in ends.items()})
    for size, last in itertools.product(END_SIZES, ends):
        n = TILE + size
        start = n - (3000 if size <= STEP + 1 else 5500)
        parts, at, i = [], 0, 0
        while at + 64 <= start:
            parts.append(f"{i % 2} {tok(i)} {tok(i + 5)}\n")
            at += len(parts[-1])
            i += 1
        parts.append("1 " + tok(3)[:-1] + "5" * (start - at - 2 - len(tok(3))) + "\n")
        text = "".join(parts)
        assert len(text) == start
        body = n - start - len(ends[last])
        line = "1"
        while len(line) + 40 < body:
            i += 1
            line += " " + tok(i)
        line += " " + tok(4)
        line += "3" * (body - len(line))
        text += line + ends[last]
        assert len(text) == n and (last != "digit" or text[-1].isdigit())
        out.append((f"{fmt}_end_{size}_{last}", text))
    return out
