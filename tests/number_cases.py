"""Number strings at the places where a float decoder can go wrong, the files
that carry them through every text format at every byte phase, and their
expected float32 bits from the Python oracle (pyref.strtof: the reference
strtof arithmetic, src/data/strtonum.h).

Helper of test_number_decode_cpu.py and test_gpu_number_decode.py.  Pure
Python and numpy; everything is deterministic (fixed seeds) and built once per
process.  The conditions a corpus must meet on the host (phase coverage,
straddled boundaries, line lengths, file sizes, the share of zero values) are
plain asserts that run when the corpus is built.
"""
import decimal
import functools
import itertools

import numpy as np

import pyref

ONE = 0x3F800000  # bits of 1.0f: a missing weight, a feature without a value
MAX_FILE = 2_000_000
MAX_LINE = 200
MIN_LINES = 8192
CLASSES = ("A", "B", "C", "D", "E", "F")

_BITS = {}


def expected_bits(strings):
    """float32 bits of every string under the reference arithmetic"""
    out = np.empty(len(strings), np.float32)
    for i, s in enumerate(strings):
        v = _BITS.get(s)
        if v is None:
            v = _BITS[s] = np.float32(pyref.strtof(s))
        out[i] = v
    return out.view(np.uint32)


def _unique(strings):
    return list(dict.fromkeys(strings))


# ---------------------------------------------------------------------------
# the classes


def _boundary_distance(q):
    """distance of the float64 values q to the nearest float32 rounding
    boundary (the midpoint of two neighbouring floats), in ulps of float32(q)"""
    r32 = q.astype(np.float32)
    r = r32.astype(np.float64)
    up = np.nextafter(r32, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r32, np.float32(-np.inf)).astype(np.float64)
    d_up = np.abs((r + up) / 2 - q) / (up - r)
    d_dn = np.abs((r + dn) / 2 - q) / (r - dn)
    return np.minimum(d_up, d_dn)


@functools.lru_cache(maxsize=None)
def frac_exhaustive():
    """A: every fraction of 1..5 digits; every 37th also behind a signed
    integer part of 1..7 digits (placed right after its plain form, so the
    long strings are spread evenly)"""
    rng = np.random.default_rng(101)
    out = []
    n = 0
    for k in range(1, 6):
        for f in range(10 ** k):
            frac = f"{f:0{k}d}"
            out.append("0." + frac)
            if n % 37 == 0:
                nd = 1 + (n // 37) % 7
                ip = int(rng.integers(10 ** (nd - 1), 10 ** nd))
                out.append(f"-{ip}.{frac}")
            n += 1
    assert n == 111110
    return out


@functools.lru_cache(maxsize=None)
def frac_hard():
    """B: fractions of 6 and 7 digits: the 4000 nearest to a float32 rounding
    boundary, 4000 for which the uncorrected product F * RN(10^-k) is not the
    rounded quotient, 2000 random ones"""
    rng = np.random.default_rng(102)
    out = []
    for k in (6, 7):
        n = 10 ** k
        dist = np.empty(n)
        naive_off = np.empty(n, bool)
        inv = np.float32(10.0 ** -k)
        for lo in range(0, n, 1 << 20):
            f = np.arange(lo, min(n, lo + (1 << 20)), dtype=np.float64)
            q = f / float(n)
            dist[lo:lo + len(f)] = _boundary_distance(q)
            naive_off[lo:lo + len(f)] = f.astype(np.float32) * inv != q.astype(np.float32)
        near = np.sort(np.argpartition(dist, 4000)[:4000])
        off = np.flatnonzero(naive_off)
        assert len(off) > 4000  # the correction step matters for many inputs
        off = off[np.linspace(0, len(off) - 1, 4000).astype(np.int64)]
        rnd = rng.integers(0, n, 2000)
        for f in itertools.chain(near, off, rnd):
            out.append(f"0.{int(f):0{k}d}")
    return _unique(out)


def _int_parts(nd, rng, count):
    special = [2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 1, 2 ** 24 - 2, 9999999, 2 ** 22,
               2 ** 22 + 1, 2 ** 21 + 1, 2 ** 20 + 1]
    special += [10 ** j for j in range(7)] + [10 ** j - 1 for j in range(1, 8)]
    got = [v for v in special if len(str(v)) == nd]
    got += [int(v) for v in rng.integers(10 ** (nd - 1), 10 ** nd, count)]
    return np.array(sorted(set(got)), np.int64)


@functools.lru_cache(maxsize=None)
def sum_hard():
    """C: integer part + fraction whose exact sum lies next to a float32
    rounding boundary (100 per pair of digit counts), and exact ties of the
    final add: I + .5 / .25 / .0625 for I in 2^22 .. 2^24 - 1"""
    rng = np.random.default_rng(103)
    out = []
    for ni in range(1, 8):
        ints = _int_parts(ni, rng, 150)
        for nf in range(1, 8):
            fr = set(int(v) for v in rng.integers(0, 10 ** nf, 300))
            fr |= {5 * 10 ** (nf - 1), 10 ** nf - 1, 1, 0}
            if nf >= 2:
                fr.add(25 * 10 ** (nf - 2))
            if nf >= 4:
                fr.add(625 * 10 ** (nf - 4))
            fr = np.array(sorted(fr), np.int64)
            q = ints[:, None].astype(np.float64) + fr[None, :].astype(np.float64) / 10.0 ** nf
            dist = _boundary_distance(q).ravel()
            pick = np.sort(np.argsort(dist, kind="stable")[:100])  # (all, where fewer exist)
            for j in pick:
                out.append(f"{ints[j // len(fr)]}.{int(fr[j % len(fr)]):0{nf}d}")
    step = (2 ** 24 - 2 ** 22) // 1000
    for i in itertools.chain(range(2 ** 22, 2 ** 24, step), (2 ** 23 - 1, 2 ** 23, 2 ** 24 - 1)):
        for tie in (".5", ".25", ".0625"):
            out.append(f"{i}{tie}")
    return _unique(out)


@functools.lru_cache(maxsize=None)
def frac_long():
    """D: fractions of 8..25 digits around float32 rounding boundaries: the
    exact decimal midpoint of a random float in (0, 1) and its successor, cut
    to each length, and that plus one unit in the last place; fractions that
    begin with eight zeros; some behind a 7-digit integer part"""
    rng = np.random.default_rng(104)
    # (long and short in turn: lines of consecutive strings are equally long)
    lengths = [8, 25, 9, 21, 10, 20, 11, 19, 12, 16, 13, 15, 14]
    # log-uniform over 2^-32 .. 1: leading zeros of every count (1800 floats:
    # with 2000 the LibFM file of the class passes the 2 MB limit)
    bits = rng.integers(0x2F800000, 0x3F800000, 1800).astype(np.uint32)
    out = []
    for n, f in enumerate(bits.view(np.float32)):
        nxt = np.nextafter(f, np.float32(2))
        mid = (float(f) + float(nxt)) / 2  # exact in double
        digits = format(decimal.Decimal(mid), "f").split(".")[1]
        head = ("0", "1234567", "8388607", "")[n % 4] if n % 20 < 4 else "0"
        for nf in lengths:
            cut = digits[:nf].ljust(nf, "0")
            out.append(f"{head}.{cut}")
            up = str(int(cut) + 1).rjust(nf, "0")
            if len(up) == nf:
                out.append(f"{head}.{up}")
    for nd in (1, 2, 4, 7, 8, 11, 12, 13):
        for _ in range(12):
            tail = "".join(str(int(d)) for d in rng.integers(0, 10, nd))
            out.append("0.00000000" + tail)
            out.append("-7654321.00000000" + tail)
    return _unique(out)


E_MANTISSAS = ("1", "9999999", "1.5", ".5", "5.", "1234567.25", "9.999999", "1.17549435",
               "3.4028235", "1.4", "7", "0.0",
               # the clamp at 38 keeps the listed mantissas above 1e-38: these
               # reach the smallest denormals and the ties below them
               # (1e-45, 1.4e-45, 7e-46 and 2.1e-45 at e-38)
               ".0000001", ".00000014", ".00000007", ".00000021")


@functools.lru_cache(maxsize=None)
def exponent_grid():
    """E: mantissas x (e|E) x (none|+|-) x 0..45, three- and four-digit and
    empty exponents, both mantissa signs"""
    out = []
    for sign in ("", "-"):
        for m in E_MANTISSAS:
            for e in range(46):
                for n, es in enumerate(("", "+", "-")):
                    out.append(f"{sign}{m}{'eE'[(e + n) % 2]}{es}{e}")
                    out.append(f"{sign}{m}{'Ee'[(e + n) % 2]}{es}{e}")
            for ex in ("007", "038", "100", "0005", "-007", "+010", "-011", "-045", "-0038"):
                out.append(f"{sign}{m}e{ex}")
            for ex in ("e", "e+", "e-", "E"):
                out.append(f"{sign}{m}{ex}")
    out += ["1e", "2e+", "7e-", "-0.0e5", "1.4e-45", "7e-46"]
    return _unique(out)


@functools.lru_cache(maxsize=None)
def longest_forms():
    """F: the longest strings each decoder takes, and each one byte longer
    (declined: the next decoder, in the end the generic grammar, takes it)"""
    return _unique([
        "-1234567.123456789012345e-10",    # 28 bytes: the longest for parse_num
        "-1234567.123456789012345e-010",   # three exponent digits
        "-1234567.123456789012345e-0010",  # four: declined
        "-1234567.1234567890123456e-10",   # 16 fraction digits: declined
        "-12345678.123456789012345e-10",   # 8 integer digits: declined
        "-1234567.123456789012345e38",     # 27 bytes: the longest for parse_num_ext
        "-1234567.123456789012345e-38",    # 28: declined there
        "-1234567.123456789012345e-11",
        "+1234567.1234567e+10", "+1234567.1234567e+11", "+1234567.1234567e+010",
        "+1234567.12345678e+10", "+1234567.1234567e+0010",
        "1234567", "12345678", "123456789", "1234567e10", "12345678e10", "1234567e-11",
        "1234567.1234567", "1234567.12345678", "-9999999.9999999", "9999999.99999999",
        "0.123456789012345", "0.1234567890123456", ".123456789012345", "-.1234567890123456",
        "8388607.500000000000000", "8388607.5000000000000000",
        "0.999999999999999e10", "0.9999999999999999e10",
    ])


BUILDERS = {"A": frac_exhaustive, "B": frac_hard, "C": sum_hard, "D": frac_long,
            "E": exponent_grid, "F": longest_forms}
TAIL = "-1234567.123456789012345e-10"  # ends every file, without a newline


def class_strings(cls):
    return BUILDERS[cls]()


@functools.lru_cache(maxsize=None)
def ext_only_strings():
    """strings of class E that wait in the fill's deferred queue (an exponent
    beyond the one-multiply branch, |e| > 10) and are short enough for more
    than 256 `i:value` tokens in 2 KiB: 4 and 5 bytes long in turn"""
    short = {4: [], 5: []}
    for s in exponent_grid():
        e = s.lower().partition("e")[2].lstrip("+-")
        if len(s) in short and e.isdigit() and int(e) > 10:
            short[len(s)].append(s)
    n = len(short[4])
    assert n >= 100 and len(short[5]) >= n
    five = short[5][::len(short[5]) // n][:n]
    return [s for pair in zip(short[4], five) for s in pair]


@functools.lru_cache(maxsize=None)
def thinned_zero_strings(cls):
    """the class's strings with those whose value is +-0 thinned to every
    16th (class E: one in twelve would be zero): a zero cell of a hashed row
    cannot be located, and the fused kernel's test bounds their share"""
    strings = class_strings(cls)
    zero = (expected_bits(strings) & 0x7FFFFFFF) == 0
    nth = np.cumsum(zero)
    return [s for s, z, k in zip(strings, zero, nth) if not z or k % 16 == 0]


# ---------------------------------------------------------------------------
# embedding


class Corpus:
    """one file: its bytes, the expected bits of every float column in file
    order (cols), the string behind each of them (srcs, None where the file
    has none: the bits of 1.0), and where the class's strings lie in the file"""

    def __init__(self, text, cols, srcs, starts=(), lens=()):
        self.text = text
        self.cols = cols
        self.srcs = srcs
        self.starts = np.asarray(starts, np.int64)
        self.lens = np.asarray(lens, np.int64)

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self.text)
        return path


def first_mismatch(name, got, want, srcs):
    """'' when the uint32 arrays are equal, else a message that names the
    first string whose bits differ"""
    got = np.asarray(got)
    if got.shape != want.shape:
        return f"{name}: {got.shape} values, expected {want.shape}"
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return ""
    i = int(bad[0])
    return (f"{name}[{i}] {srcs[i]!r}: expected {int(want[i]):#010x}, got {int(got[i]):#010x} "
            f"({len(bad)} of {len(want)} differ)")


def _bits_or_one(strings):
    out = np.full(len(strings), ONE, np.uint32)
    have = [k for k, s in enumerate(strings) if s is not None]
    out[have] = expected_bits([strings[k] for k in have])
    return out


def _pad_tokens(room, fm):
    """valueless features that fill exactly `room` bytes, blanks included"""
    head, lo, hi = (" 1:", 4, 10) if fm else (" ", 2, 8)
    out = []
    while room:
        c = min(hi, room)
        if 0 < room - c < lo:
            c = room - lo
        assert c >= lo
        out.append(head + "8" * (c - len(head)))  # (digits no class string consists of)
        room -= c
    return out


def _check_file(blob, strings, starts, lens, width, nlines, full_sweep):
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    for s, n, want in zip(starts, lens, strings):
        assert blob[s:s + n] == want.encode(), (s, want)
    assert np.all(starts[1:] >= starts[:-1] + lens[:-1])
    if width is not None:  # (None: lines of their own lengths)
        assert width % 2 == 1 and width <= MAX_LINE
    assert nlines >= MIN_LINES
    assert max(len(ln) for ln in blob.split(b"\n")) < MAX_LINE
    assert len(blob) < MAX_FILE, len(blob)
    assert len(np.unique(starts % 16)) == 16
    if not full_sweep:
        return
    # class F: every phase of an 8 KiB tile, tokens across every boundary
    assert len(np.unique(starts % 8192)) == 8192
    last = starts + lens - 1
    for unit in (8192, 2048, 1024):
        assert np.any(starts // unit != last // unit), unit
    # the last 40 bytes of the second 1 KiB slot of a 2 KiB ring: a token at
    # every one of them, and across the ring's end wherever a 16-byte load
    # past the token start (a decoder window) would cross it
    ring = starts % 2048
    for o in range(984, 1024):
        here = ring == 1024 + o
        assert here.any(), o
        if o + 16 > 1024:
            assert np.any(here & (ring + lens > 2048)), o


def _feature(i, j, s, fm, one_feature):
    idx = (i * 7 + j) % 1000 if one_feature else j + 1
    return f"{idx % 7}:{idx}:{s}" if fm else f"{idx}:{s}"


def _svm_layout(strings, fm, per_line, one_feature, min_lines, column):
    """per line: (label, weight, features, the text up to the trailing
    padding, the valueless features in it), and the lines' width.  column: the
    first feature starts there in every line, behind valueless features."""
    src = itertools.cycle(strings)
    least = 4 if fm else 2  # the shortest padding
    lines = []
    used = 0
    while len(lines) < min_lines or used < len(strings):
        i = len(lines)
        label = next(src) if i % 3 == 0 else None
        weight = next(src) if i % 11 == 0 and not one_feature else None
        feats = [next(src) for _ in range(per_line)]
        used += len(feats) + (label is not None) + (weight is not None)
        head = label if label is not None else str(i % 2)
        if weight is not None:
            head += ":" + weight
        lines.append([label, weight, feats, head])
    if column:
        column = max(len(ln[3]) for ln in lines) + least
    for i, ln in enumerate(lines):
        lead = _pad_tokens(column - len(ln[3]), fm) if column else []
        ln[3] += "".join(lead) + "".join(" " + _feature(i, j, s, fm, one_feature)
                                         for j, s in enumerate(ln[2]))
        ln.append(len(lead))
    width = max(len(ln[3]) for ln in lines) + least + 1  # padding, the newline
    return lines, width + 1 - width % 2


@functools.lru_cache(maxsize=None)
def svm_corpus(cls, fm=False, one_feature=False):
    """LibSVM (fm: LibFM) file of a class.  The value of each feature, every
    third line's label and every eleventh line's weight are the class's
    strings in turn (cycled up to 8192 lines).  Every line is padded with
    trailing valueless features to the same odd number of bytes, so the tokens
    walk through every byte phase; the file ends with TAIL and no newline.
    Class F (one feature per line) also has valueless features before the
    feature, up to a fixed column: whatever the label and the weight, its
    value starts at line * width + a constant, which visits every residue
    modulo 8192; twice 8192 lines, for a long form at each of them.
    one_feature: one feature per row, no weights and no padding, for the fused
    tokenize -> hash kernel: the +-0 values thinned (thinned_zero_strings) and,
    where the file would pass the size limit, every stride-th string only."""
    base = thinned_zero_strings(cls) if one_feature else class_strings(cls)
    sweep = cls == "F" and not one_feature
    # as many features per line as 8192 lines need to hold the class once
    per_line = 1 if one_feature else min(14, -(-len(base) // MIN_LINES))
    stride = 1
    while True:
        strings = base[::stride]
        lines, width = _svm_layout(strings, fm, per_line, one_feature,
                                   MIN_LINES * (2 if sweep else 1), sweep)
        if width > MAX_LINE and per_line > 1:
            per_line -= 1
        elif one_feature and sum(len(ln[3]) + 1 for ln in lines) >= MAX_FILE:
            stride += 1
        else:
            break
    text, toks, starts, lens = [], [], [], []
    lab, wgt, val = [], [], []
    pos = 0
    for i, (label, weight, feats, raw, nlead) in enumerate(lines):
        lab.append(label if label is not None else str(i % 2))
        wgt.append(weight)
        # (one feature per row: no padding, the lines are as long as they are)
        pads = [] if one_feature else _pad_tokens(width - 1 - len(raw), fm)
        val.extend([None] * nlead + feats + [None] * len(pads))
        text.append(raw + "".join(pads) + "\n")
        assert one_feature or len(text[-1]) == width
        # where the class's strings lie: in text order, each after the last
        at = 0
        for n, s in enumerate([label, weight] + feats):
            if s is not None:
                # (a value ends its token: the blank tells it from an index)
                at = (raw + " ").index(":" + s + " ", at) + 1 if n else 0
                toks.append(s)
                starts.append(pos + at)
                lens.append(len(s))
                at += len(s)
        pos += len(text[-1])
    last = "1 " + _feature(0, 0, TAIL, fm, one_feature)
    text.append(last)
    toks.append(TAIL)
    starts.append(pos + len(last) - len(TAIL))
    lens.append(len(TAIL))
    lab.append("1")
    wgt.append(None)
    val.append(TAIL)
    blob = "".join(text).encode()
    _check_file(blob, toks, starts, lens, None if one_feature else width, len(lines), sweep)
    cols = {"label": expected_bits(lab), "weight": _bits_or_one(wgt), "value": _bits_or_one(val)}
    if one_feature:
        zero = (cols["value"] & 0x7FFFFFFF) == 0
        assert zero.sum() * 100 < len(zero), (int(zero.sum()), len(zero))
    return Corpus(blob, cols, {"label": lab, "weight": wgt, "value": val}, starts, lens)


@functools.lru_cache(maxsize=None)
def svm_small_corpus(name):
    """two more LibSVM files of class E.  `tokens40`: 40 tokens (single decode
    rounds, no pair round, the queue drained at the end).  `extwrap`: every
    value waits in the deferred queue, more than 256 of them in any 2 KiB of
    text (the queue's 256-entry ring wraps)."""
    lab, val, text = [], [], []
    if name == "tokens40":
        strings = exponent_grid()[5::277][:32]
        assert len(strings) == 32
        for r in range(8):
            feats = strings[4 * r:4 * r + 4]
            text.append(f"{r % 2} " + " ".join(f"{j + 1}:{s}" for j, s in enumerate(feats)))
            lab.append(str(r % 2))
            val.extend(feats)
        blob = "\n".join(text).encode()  # no final newline
    else:
        assert name == "extwrap"
        src = itertools.cycle(ext_only_strings())
        for r in range(1200):
            feats = [next(src) for _ in range(24)]
            text.append("1" + "".join(f" {j % 9 + 1}:{s}" for j, s in enumerate(feats)) + "\n")
            lab.append("1")
            val.extend(feats)
        blob = "".join(text).encode()
        assert max(len(t) for t in text) <= MAX_LINE
        colon = np.frombuffer(blob, np.uint8) == ord(":")
        before = np.concatenate([[0], np.cumsum(colon)])
        window = before[2048:] - before[:-2048]  # value tokens in every 2 KiB window
        assert window.min() > 256, int(window.min())
    cols = {"label": expected_bits(lab), "weight": np.full(len(lab), ONE, np.uint32),
            "value": expected_bits(val)}
    return Corpus(blob, cols, {"label": lab, "weight": [None] * len(lab), "value": val})


@functools.lru_cache(maxsize=None)
def csv_corpus(cls, delim=","):
    """CSV file of a class: rows of three of its strings in turn and a field
    of digits that pads every row to the same odd length; the last row ends
    the file with TAIL and no newline.  cols["field"]: the expected bits,
    (rows, 4)."""
    strings = class_strings(cls)
    src = itertools.cycle(strings)
    rows = []
    while len(rows) < MIN_LINES or 3 * len(rows) < len(strings):
        rows.append([next(src), next(src), next(src)])
    width = max(sum(len(s) for s in r) for r in rows) + 3 + 1 + 1  # delimiters, a digit, newline
    width += 1 - width % 2
    text, toks, starts, lens, fields = [], [], [], [], []
    pos = 0
    for r in rows:
        pad = "7" * (width - 1 - 3 - sum(len(s) for s in r))
        p = pos
        for s in r:
            toks.append(s)
            starts.append(p)
            lens.append(len(s))
            p += len(s) + 1
        text.append(delim.join(r + [pad]) + "\n")
        assert len(text[-1]) == width
        fields.extend(r + [pad])
        pos += width
    last = [strings[0], strings[-1], "5", TAIL]
    text.append(delim.join(last))
    fields.extend(last)
    toks.append(TAIL)
    starts.append(pos + len(text[-1]) - len(TAIL))
    lens.append(len(TAIL))
    blob = "".join(text).encode()
    _check_file(blob, toks, starts, lens, width, len(rows), cls == "F")
    return Corpus(blob, {"field": expected_bits(fields).reshape(-1, 4)}, {"field": fields},
                  starts, lens)
