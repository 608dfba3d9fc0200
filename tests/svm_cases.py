"""LibSVM / LibFM texts that put line ends, token starts, whole tokens, decode
rounds, `qid:` tokens, owned lines and the chunk end on every edge of the token
tile path (src/gpu/tile_count_kernels.hip: k_tile_count; tile_fill_kernels.hip:
k_tile_fill, k_tile_hash), and a small model of the walk's step accounting.

Helper of test_svm_cases_cpu.py and test_gpu_svm_edges.py.  Pure Python and
numpy, deterministic, built once per process.  Every file is ONE chunk for the
GPU parser (the tests read it with a chunk size above the file size), so a
byte offset in the file is a byte offset in the chunk.  Every case states the
quantities it means to hit as claims ("step 1 of tile 1 ends with carry 63");
they are checked against the model when the case is built.  The model is a
reading of the kernels: it proves placement and is never used for expected
output -- that comes from the C++ parser, which test_svm_cases_cpu.py holds to
the Python oracle (pyref.parse_libsvm / parse_libfm) on the same files.
"""
import collections
import functools
import itertools
import re

import numpy as np

import csv_cases
import number_cases
import pyref

# the geometry of the walk, each next to its source
TILE = 8192            # kTileBytes (src/gpu/kernels.h): one wave per tile
COUNT_STRIDE = 1024    # k_tile_count: load j of a lane is at j * 1024 (kCountLoads)
STEP = 2048            # kStepBytes (tile_common.h): a tile is staged in 4 steps
HALF = 1024            # the `a` and `b` slices of a lane: bload16(trs, loff [+ 1024])
LANE = 16              # bytes of a lane's slice (one 16 B load)
TAIL = 64              # kSlotBytes = kStepBytes + 64: the bytes staged behind a step
WINDOW = 32            # token_decode.h: two 16 B reads cover a number (win_byte: 0..31)
ROUND = 64             # a decode round: lane i decodes token i (dev::kWave)
PAIR = 128             # a pair round: `r0 + 2 * dev::kWave <= ndec`, tok::decode2
DECODE_CARRY = 64      # kDecodeCarry: fewer than 64 tokens wait for the next step
QUEUE_CAP = 256        # kQueueCap: the ring of deferred tokens
HASH_LIST_CAP = 428    # kHashListCap: k_tile_hash's list; more tokens split the step
HASH_CARRY = 1024      # kHashCarry: the text of carried tokens ahead of the staged step
STEPS = TILE // STEP
LIST_CAP = DECODE_CARRY + STEP // 2  # kListCap
MAX_FILE = 64 * 1024

GROUPS = ("a", "b", "c", "d", "e", "f", "g")
FORMATS = ("libsvm", "libfm")
INDEX64_GROUPS = ("c", "e")
DYADIC_GROUPS = ("a", "b", "d", "e", "f")
# "Edge": these offsets inside a chunk of two or more tiles (lane, half-step,
# step starts, the tile start and a step start of the second tile)
EDGES = (16, 1024, 2048, 4096, 6144, 8192, 8192 + 2048)
# the named cases whose path the code leaves open: these inputs leave none
EITHER = ()

Case = collections.namedtuple("Case", "name group fmt text expect marks claims hexpect dyadic fp8")


# ---------------------------------------------------------------------------
# the model


def _starts(text, fmt):
    """(bytes, token starts, line starts, letter-started token starts): a token
    starts at a byte > 0x20 behind a byte <= 0x20, a line at a non-EOL byte
    behind an EOL byte; the byte before the chunk is `\\n`.  Letter-started
    tokens (LibSVM `qid:`) are no list entries of a qid chunk: taken out."""
    raw = np.frombuffer(text.encode("latin-1"), np.uint8)
    sep = raw <= 0x20
    eol = (raw == 10) | (raw == 13)
    tm = ~sep & np.concatenate([[True], sep[:-1]])
    lm = ~eol & np.concatenate([[True], eol[:-1]])
    q = tm & ((raw & 0x40) != 0)
    if fmt == "libsvm":
        tm = tm & ~q
    return raw, tm, lm, q


starts = functools.lru_cache(maxsize=16)(_starts)


FillStep = collections.namedtuple("FillStep", "ntok nline carry_in total rest ndec carry")


def _fill_steps(tm, lm, n):
    out = {}
    for t in range(-(-n // TILE)):
        carry = 0
        for s in range(STEPS):
            lo = t * TILE + s * STEP
            ntok = int(tm[lo:lo + STEP].sum())
            nline = int(lm[lo:lo + STEP].sum())
            total = carry + ntok
            rest = min(total % ROUND, ntok)
            ndec = total if s + 1 == STEPS else total - rest
            out[t, s] = FillStep(ntok, nline, carry, total, rest, ndec, total - ndec)
            carry = total - ndec
    return out


@functools.lru_cache(maxsize=64)
def fill_model(text, fmt):
    """k_tile_fill's accounting per (tile, step): `total = carry + ntok`,
    `rest = min(total % 64, ntok)`, `ndec = last ? total : total - rest`"""
    _, tm, lm, _ = starts(text, fmt)
    return _fill_steps(tm, lm, len(text))


_NUM = re.compile(r"[+-]?(\d*)(?:\.(\d*))?(?:[eE][+-]?(\d*))?$")


def defers(token):
    """the register-window decoder (token_decode.h decode / parse_num) declines
    the token: 8 or more integer digits, 16 or more fraction digits, an
    exponent of more than 3 digits or above 10, or a token past the window"""
    if len(token) >= WINDOW:
        return True
    for f in token.split(":"):
        m = _NUM.match(f)
        if not m:
            return True
        ip, fp, ex = m.groups()
        if len(ip) > 7 or (fp is not None and len(fp) > 15):
            return True
        if ex is not None and (len(ex) > 3 or ex == "" or int(ex) > 10):
            return True
    return False


def tokens_of(text, fmt, lo, hi):
    """(offset, token) of the list entries that start in [lo, hi)"""
    _, tm, _, _ = starts(text, fmt)
    out = []
    for p in np.flatnonzero(tm[lo:hi]) + lo:
        m = re.compile(r"[^ \t\r\n]+").match(text, int(p))
        out.append((int(p), m.group()))
    return out


HashStep = collections.namedtuple(
    "HashStep", "ntok_a ntok_b carry_in total split last rest carry first_left")
HashTile = collections.namedtuple("HashTile", "own steps exact")


@functools.lru_cache(maxsize=64)
def hash_model(text, fmt):
    """k_tile_hash per tile: `own` (the line starts of the tile), and per step
    of its walk (which goes on past the tile end until the last owned line
    ends) the owned token starts of the two halves, the split rule
    (`carry + ntok > kHashListCap`; a half above the cap: the exact kernels),
    which step is `last`, and the carry: `total % 64` tokens, unless the first
    of them starts before step byte 1024 (its text would not fit the carry
    area: everything is decoded)"""
    raw, tm, lm, _ = starts(text, fmt)
    n = len(raw)
    tiles = {}
    for t in range(-(-n // TILE)):
        tile0 = t * TILE
        own = int(lm[tile0:tile0 + TILE].sum())
        steps, exact = [], False
        lcnt, carried, s = 0, [], 0
        while own:
            cur = tile0 + s * STEP
            nxt = cur + STEP
            l, tk = lm[cur:nxt], tm[cur:nxt]
            ordn = lcnt + np.cumsum(l)
            offs = [int(o) for o in np.flatnonzero(tk & (ordn >= 1) & (ordn <= own))]
            a = [HASH_CARRY + o for o in offs if o < HALF]
            b = [HASH_CARRY + o for o in offs if o >= HALF]
            carry = len(carried)
            split = carry + len(offs) > HASH_LIST_CAP
            if split and (carry + len(a) > HASH_LIST_CAP or len(b) > HASH_LIST_CAP):
                exact = True
                steps.append(HashStep(len(a), len(b), carry, carry + len(offs), True, True, 0, 0, None))
                break
            lcnt += int(l.sum())
            eol_end = nxt <= n and raw[nxt - 1] in (10, 13)
            last = nxt >= n or lcnt > own or (s + 1 >= STEPS and lcnt == own and eol_end)
            parts = [carried + a, b] if split else [carried + a + b]
            # the a half of a split step is decoded whole (rest 0), so what a
            # step leaves is what its last part leaves
            for part, pl in enumerate(parts):
                total = len(pl)
                rest = 0 if last or (split and part == 0) else total % ROUND
                if rest and pl[total - rest] < STEP:  # kHashText - kHashCarry - 64
                    rest = 0
                assert rest == 0 or part + 1 == len(parts)
            left = pl[total - rest:] if rest else []
            steps.append(HashStep(len(a), len(b), carry, carry + len(offs), split, last, rest,
                                  len(left), left[0] - HASH_CARRY if left else None))
            if last:
                break
            carried = [o - STEP for o in left]
            s += 1
        tiles[t] = HashTile(own, tuple(steps), exact)
    return tiles


_QID_OK = re.compile(r"qid:[+-]?\d*$")


def exact_reasons(text, fmt, hashed=False):
    """why the tile path gives this chunk up (empty: it does not): a letter
    token that is no `qid:` second token of its line (any letter token in
    LibFM), a line that starts with a blank; for the hash kernel also a half
    step above its list"""
    why = []
    for ln in re.split(r"[\r\n]+", text):
        if ln[:1] in (" ", "\t"):
            why.append("a line starts with a blank")
        toks = ln.split()
        for k, tok in enumerate(toks):
            if ord(tok[0]) & 0x40:
                if fmt != "libsvm" or k != 1 or not _QID_OK.match(tok) or ord(toks[0][0]) & 0x40:
                    why.append(f"letter token {tok!r} as token {k} of its line")
    if hashed:
        for t, ht in hash_model(text, fmt).items():
            if ht.exact:
                s = ht.steps[-1]
                why.append(f"tile {t} step {len(ht.steps) - 1}: carry {s.carry_in} + "
                           f"{s.ntok_a} / {s.ntok_b} tokens")
    return why


def check_claims(text, fmt, claims):
    """every claim of a case against the model; returns the statements"""
    raw, tm, lm, q = starts(text, fmt)
    said = []
    for c in claims:
        kind = c[0]
        if kind == "fill":
            _, t, s, field, want = c
            got = getattr(fill_model(text, fmt)[t, s], field)
            said.append(f"fill step {s} of tile {t}: {field} == {want}")
        elif kind == "hash":
            _, t, s, field, want = c
            got = getattr(hash_model(text, fmt)[t].steps[s], field)
            said.append(f"hash step {s} of tile {t}: {field} == {want}")
        elif kind == "hash_tile":
            _, t, field, want = c
            ht = hash_model(text, fmt)[t]
            got = len(ht.steps) if field == "nsteps" else getattr(ht, field)
            said.append(f"hash tile {t}: {field} == {want}")
        elif kind == "slice":
            _, off, want = c
            assert off % LANE == 0
            got = int(tm[off:off + LANE].sum())
            said.append(f"the 16-byte slice at {off} holds {want} token starts")
        elif kind == "tok":
            _, off, want = c
            got = bool(tm[off])
            said.append(f"byte {off} {'starts' if want else 'does not start'} a token")
        elif kind == "line":
            _, off, want = c
            got = bool(lm[off])
            said.append(f"byte {off} {'starts' if want else 'does not start'} a line")
        elif kind == "q":
            _, off, want = c
            got = bool(q[off])
            said.append(f"byte {off} starts a letter token")
        elif kind == "last_tok":
            _, t, s, off = c
            lo = t * TILE + s * STEP
            got, want = int(np.flatnonzero(tm[lo:lo + STEP])[-1]) + lo, off
            said.append(f"the token at {off} is the last one listed in step {s} of tile {t}")
        elif kind == "defer":
            _, t, s, want = c
            lo = t * TILE + s * STEP
            got = sum(defers(tok) for _, tok in tokens_of(text, fmt, lo, lo + STEP))
            said.append(f"{want} tokens of step {s} of tile {t} are deferred")
        elif kind == "defer_tail":
            _, t, s, want = c
            lo = t * TILE + s * STEP
            toks = tokens_of(text, fmt, lo, lo + STEP)
            got = sum(defers(tok) for _, tok in toks[len(toks) - fill_model(text, fmt)[t, s].rest:])
            said.append(f"{want} of the tokens step {s} of tile {t} carries are deferred")
        elif kind == "nolines":
            _, t, want = c
            got, want = int(lm[t * TILE:(t + 1) * TILE].sum()), 0
            said.append(f"tile {t} holds no line start")
        elif kind == "notokens":
            _, t, want = c
            got, want = int(tm[t * TILE:(t + 1) * TILE].sum()), 0
            said.append(f"tile {t} holds no token start")
        else:
            raise AssertionError(c)
        assert got == want, (said[-1], "model says", got)
    return said


# ---------------------------------------------------------------------------
# the builder

DY = ("0.5", "1.25", "0.75", "2.5", "-1.5", "3", "0.25", "-0.5")


def step_of(off):
    """(tile, step) of a byte"""
    return off // TILE, off % TILE // STEP


class Builder:
    """appends whole lines; between placements it pads with regular rows whose
    token count it chooses, so that the fill's carry is what a case wants"""

    def __init__(self, fmt):
        self.fmt = fmt
        self.buf = []
        self.n = 0
        self.marks = []
        self.claims = []
        self.k = 0

    def text(self):
        return "".join(self.buf)

    def put(self, s):
        self.buf.append(s)
        self.n += len(s)

    def mark(self, off, ch):
        self.marks.append((off, ch))

    def claim(self, *c):
        self.claims.append(tuple(c))

    def feat(self, size=9):
        """a regular feature of at most `size` bytes, its value a small dyadic"""
        self.k += 1
        i, v = self.k % 89 + 1, DY[self.k % len(DY)]
        if self.fmt == "libsvm":
            forms = (f"{i}:{v}", f"{i}", f"{i % 9 + 1}")
        else:
            forms = (f"{self.k % 5}:{i}:{v}", f"{self.k % 5}:{i % 9 + 1}")
        for t in forms:
            if len(t) <= size:
                return t
        raise AssertionError((self.fmt, size))

    def defer_feat(self):
        """a feature the register decoder declines: a 4-digit exponent (dyadic value)"""
        self.k += 1
        tok = f"{self.k % 89 + 1}:{self.k % 6}.5e0001"
        return tok if self.fmt == "libsvm" else f"{self.k % 5}:" + tok

    def block(self, k, nbytes, defer=frozenset()):
        """exactly `k` token starts in exactly `nbytes`, whole lines of up to
        four tokens; the tokens in `defer` (ordinals) take the deferred shape"""
        assert k >= 1 and nbytes >= 2 * k, (k, nbytes)
        per = nbytes // k - 1
        only_labels = per < (1 if self.fmt == "libsvm" else 3)
        out = []
        for i in range(k):
            label = only_labels or i % 4 == 0
            if i in defer:
                tok = "2e0000" if label else self.defer_feat()
            else:
                tok = str(i // 4 % 2) if label else self.feat(per)
            out.append(("\n" if label else " ") + tok)
        s = "".join(out)[1:]
        assert len(s) + 1 <= nbytes, (k, nbytes, len(s))
        return s + " " * (nbytes - len(s) - 1) + "\n"

    def step_state(self):
        """(carry into the step being written, token starts already in it)"""
        text = self.text()
        raw, tm, lm, _ = _starts(text, self.fmt)
        st = self.n // STEP * STEP
        carry = 0
        if st % TILE:
            carry = _fill_steps(tm[:st], lm[:st], st)[step_of(st - 1)].carry
        return carry, int(tm[st:].sum())

    def pad_to(self, off, mod=None, extra=0):
        """regular rows up to exactly `off`.  Every step that is completed on
        the way ends with carry 0 where its room allows; with `mod`, the step
        that holds `off` gets `total % 64 == mod` once the caller has added
        `extra` more token starts to it."""
        assert off >= self.n and (self.n == 0 or self.buf[-1].endswith("\n")), (off, self.n)
        while self.n < off:
            end = min(off, (self.n // STEP + 1) * STEP)
            seg = end - self.n
            if seg == 1:  # an empty line
                self.put("\n")
                continue
            carry, have = self.step_state()
            final = end == off
            base = max(1, seg // 11)
            cnt = base
            if not final or mod is not None:
                want = mod if final and mod is not None else 0
                add = extra if final else 0
                cnt = base + (want - (carry + have + base + add)) % ROUND
                while 2 * cnt > seg:
                    cnt -= ROUND
                if cnt < 1:
                    assert not (final and mod is not None), (off, seg, mod)
                    cnt = base
            self.put(self.block(cnt, seg))
        assert self.n == off

    def put_at(self, off, s, lead="1 ", mod=None, extra=0):
        """`s` with its first byte at `off`, behind `lead` in the same line"""
        self.pad_to(off - len(lead), mod, extra)
        self.put(lead)
        for k, ch in enumerate(s):
            if k == 0 or ch in "\r\n":
                self.mark(off + k, ch)
        self.put(s)

    def finish(self, name, group, expect, hexpect=None, tail=300, dyadic=None, end=""):
        if tail:
            self.pad_to(self.n + tail)
        text = self.text() + end
        assert len(text) < MAX_FILE, (name, len(text))
        for off, ch in self.marks:
            assert text[off] == ch, (name, off, ch, text[off])
        check_claims(text, self.fmt, self.claims)
        dyadic = group in DYADIC_GROUPS if dyadic is None else dyadic
        fp8 = False
        if dyadic:
            # any f32 summation order of a hashed row is exact: multiples of
            # 1/4 below 64 whose absolute row sum stays below 2^20
            top = 0.0
            for row in oracle_rows(text, self.fmt):
                vals = [1.0 if f[-1] is None else f[-1] for f in row[-1]]
                assert all(abs(v) < 64 and v * 4 == int(v * 4) for v in vals), name
                top = max(top, sum(abs(v) for v in vals))
            assert top < 2 ** 20, (name, top)
            fp8 = top <= pyref.E4M3_MAX
        hexpect = expect if hexpect is None else hexpect
        assert (expect == "exact") == bool(exact_reasons(text, self.fmt)), name
        assert (hexpect == "exact") == bool(exact_reasons(text, self.fmt, True)), name
        return Case(f"{group}_{name}", group, self.fmt, text, expect, tuple(self.marks),
                    tuple(self.claims), hexpect, dyadic, fp8)


def long_line(b, nbytes, first="1"):
    """one regular line of exactly `nbytes` (its line end included)"""
    parts, size = [first], len(first)
    while size + 12 < nbytes:
        parts.append(" " + b.feat())
        size += len(parts[-1])
    return "".join(parts) + " " * (nbytes - size - 1) + "\n"


# ---------------------------------------------------------------------------
# a. line ends on edges


def _group_a(fmt):
    out = []
    for name, s, d in (("nl_m2", "\n", -2), ("nl_m1", "\n", -1), ("nl_0", "\n", 0),
                       ("nl_p1", "\n", 1), ("crlf", "\r\n", -1), ("nl4", "\n\n\n\n", -2),
                       ("crlf2", "\r\n\r\n", -2)):
        b = Builder(fmt)
        for edge in EDGES:
            lead = "1 " + b.feat(5)
            b.put_at(edge + d, s, lead=lead)
        out.append(b.finish(name, "a", "tile"))
    # a label whose first byte is the first byte of a tile, a step and a lane;
    # the line end before it is the last byte of the tile / step / lane
    b = Builder(fmt)
    for off in (TILE, TILE + STEP, TILE + 2 * STEP + 5 * LANE, 2 * TILE):
        b.pad_to(off)
        b.mark(off - 1, "\n")
        b.claim("line", off, True)
        b.put("1 " + b.feat() + "\n")
    out.append(b.finish("label_first", "a", "tile"))
    # a tile without a line start: every token of it has line ordinal 0
    b = Builder(fmt)
    b.pad_to(4000)
    b.put(long_line(b, 17 * 1024 + 600))
    b.claim("nolines", 1, 0)
    out.append(b.finish("noline_tile", "a", "tile"))
    # a tile without a token: blanks between two features of a regular line
    b = Builder(fmt)
    b.pad_to(8000)
    b.put("1 " + b.feat() + " " * 9000 + b.feat() + "\n")
    b.claim("notokens", 1, 0)
    out.append(b.finish("notoken_tile", "a", "tile"))
    # a tile of nothing but line ends
    b = Builder(fmt)
    b.pad_to(TILE)
    b.put("\n" * TILE)
    b.mark(TILE, "\n")
    b.mark(2 * TILE - 1, "\n")
    b.claim("nolines", 1, 0)
    b.claim("notokens", 1, 0)
    out.append(b.finish("eol_tile", "a", "tile"))
    # a line that counts while its first token does not start it, at a tile
    # start behind label-only lines (no entry before it: the feature's entry
    # ordinal in the tile is -1).  The count pass turns the chunk away; one
    # pass finds it in the fill itself, whose stores must stay in bounds.
    for name, head in (("blank_only_tile_start", " \n1 "), ("blank_started_tile_start", " 1 ")):
        b = Builder(fmt)
        b.put("1\n" * (TILE // 2))
        b.mark(TILE, " ")
        b.claim("line", TILE, True)
        b.claim("tok", TILE, False)
        b.put(head + b.feat() + " " + b.feat() + "\n")
        out.append(b.finish(name, "a", "exact"))
    # 4096 lines in one tile: the widest line ordinal.  (The hash kernel's
    # list holds 428 tokens of a half step: 512 send it to the exact kernels.)
    b = Builder(fmt)
    b.pad_to(TILE)
    b.put("1\n" * (TILE // 2))
    for s in range(STEPS):
        b.claim("fill", 1, s, "nline", STEP // 2)
    out.append(b.finish("lines4096", "a", "tile", hexpect="exact"))
    return out


# ---------------------------------------------------------------------------
# b. token starts on edges

_SLICES = {
    "libsvm": ((3, "1:2 3:4 12:0.25 "), (4, "1:1 2:1 3:1 4:1 "), (8, "1 2 3 4 5 6 7 8 ")),
    "libfm": ((3, "1:2 3:4 1:2:0.5 "), (4, "1:2 3:4 5:6 7:8 ")),
}


def _group_b(fmt):
    out = []
    for d in (-1, 0, 1):
        # the separator before the token is in another lane, half, step, tile
        b = Builder(fmt)
        for edge in EDGES:
            b.put_at(edge + d, b.feat() + " " + b.feat() + "\n", lead="1 " + b.feat(5) + " ")
            b.claim("tok", edge + d, True)
        out.append(b.finish(f"feature_{d + 1}", "b", "tile"))
        b = Builder(fmt)
        for edge in EDGES:
            b.pad_to(edge + d)
            b.mark(edge + d, "1")
            b.claim("line", edge + d, True)
            b.put("1 " + b.feat() + "\n")
        out.append(b.finish(f"label_{d + 1}", "b", "tile"))
    # 3, 4 and 8 starts in one slice: lane 0 and lane 63 of the a and b half
    b = Builder(fmt)
    for j, (count, s16) in enumerate(_SLICES[fmt]):
        assert len(s16) == LANE
        S = (1 + j) * TILE + STEP
        for off, body in ((S, s16), (S + HALF - LANE, s16 + s16), (S + STEP - LANE, s16)):
            b.put_at(off, body + b.feat() + "\n")
            for o in range(off, off + len(body), LANE):
                b.claim("slice", o, count)
    out.append(b.finish("dense_slices", "b", "tile"))
    # the list at its capacity: 1024 one-byte tokens behind a carry of 63
    b = Builder(fmt)
    b.pad_to(TILE + STEP, mod=ROUND - 1)
    b.put("1\n" * (STEP // 2))
    b.claim("fill", 1, 1, "carry_in", ROUND - 1)
    b.claim("fill", 1, 1, "total", LIST_CAP - 1)
    out.append(b.finish("full_list", "b", "tile", hexpect="exact"))
    if fmt == "libsvm":
        b = Builder(fmt)  # a tile of 4096 tokens in one line
        b.pad_to(TILE)
        b.put("1" + " 1" * (TILE // 2 - 1) + "\n")
        for s in range(STEPS):
            b.claim("fill", 1, s, "ntok", STEP // 2)
        b.claim("fill", 1, 0, "nline", 1)
        out.append(b.finish("tile4096", "b", "tile", hexpect="exact"))
    return out


# ---------------------------------------------------------------------------
# c. tokens across edges

C_BACK = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)
C_LENGTHS = (31, 32, 33, 63, 64, 65, 70, 200, 2100)
C_SHAPES = ("plain", "exponent", "long")
_DIGITS = "3141592653589793238462643383279502884197169399375105820974944592"


def _digits(n, seed):
    s = (_DIGITS[seed % 50:] + _DIGITS) * (n // 60 + 1)
    return s[:n]


@functools.lru_cache(maxsize=None)
def _hard_numbers(exponent):
    """number_cases' hard values by length: sums and long fractions at float
    rounding boundaries, or the exponent grid and the longest forms"""
    by = collections.defaultdict(list)
    for cls in ("E", "F") if exponent else ("C", "D"):
        for v in number_cases.class_strings(cls):
            by[len(v)].append(v)
    return by


def c_token(fmt, shape, length, seed):
    """a feature of exactly `length` bytes: plain `idx:0.ddd`, an exponent
    value (the extended decoder), or 9 integer digits and a long fraction
    (the generic parser)"""
    head = f"{seed % 9 + 1}:" if fmt == "libsvm" else f"{seed % 5}:{seed % 9 + 1}:"
    short = {"libsvm": {1: "7", 2: "12", 3: "1:2", 4: "1:25"},
             "libfm": {3: "1:2", 4: "1:23", 5: "1:2:3", 6: "1:2:.5"}}[fmt]
    if length in short:
        return short[length]
    room = length - len(head)
    # at most 19 fraction digits (more wrap the reference's 64-bit fraction, 64
    # divide by zero): a longer token grows by leading zeros of its integer
    # part, which the generic parser takes as well (8 or more integer digits)
    nfrac = (7, 15, 16, 19)[seed % 4]

    def number(room, lead):
        frac = min(nfrac, room - len(lead) - 1)
        return "0" * (room - len(lead) - 1 - frac) + lead + "." + _digits(frac, seed)
    hard = _hard_numbers(shape == "exponent")[room] if shape != "long" else ()
    if hard:  # a hard value of exactly this length
        tok = head + hard[seed * 7919 % len(hard)]
    elif shape == "exponent" and room >= 8:
        tok = head + number(room - 4, "1") + ("e-05" if seed % 2 else "E+12")
    elif shape == "long" and room >= 12:
        tok = head + number(room, _digits(9, seed + 3).replace("0", "1"))
    else:
        assert room >= 3, (fmt, length)
        tok = head + number(room, "0")
    assert len(tok) == length, (tok, length)
    return tok


def c_placements(fmt):
    """(step, k, length, shape, carried): every (step end, k, length) with the
    token decoded in its own step, every (step end but the tile's, k, length)
    with the token carried; the shape rotates, so that each (k, length) meets
    all three shapes"""
    out = []
    floor = 1 if fmt == "libsvm" else 3
    for carried in (False, True):
        for step in range(STEPS - 1 if carried else STEPS):
            j = 0
            for k in C_BACK:
                for length in sorted({k + 1, *C_LENGTHS}):
                    if length <= k or length < floor:
                        continue
                    out.append((step, k, length, C_SHAPES[(j + step + carried) % 3], carried))
                    j += 1
    return out


def _group_c(fmt):
    queues = {s: [p for p in c_placements(fmt) if p[0] == s] for s in range(STEPS)}
    out, b, seed = [], Builder(fmt), 0
    carries = (1, 2, ROUND - 1, 17)
    while any(queues.values()):
        end = (b.n + 400) // STEP * STEP + STEP  # the next step end with room before it
        t, s = step_of(end - 1)
        if not queues[s]:
            b.pad_to(end)
            continue
        _, k, length, shape, carried = queues[s].pop(0)
        seed += 1
        tok = c_token(fmt, shape, length, seed)
        want = carries[seed % 4] if carried else 0
        b.put_at(end - k, tok + " " + b.feat() + "\n", mod=want if s + 1 < STEPS else None, extra=2)
        b.claim("last_tok", t, s, end - k)
        b.claim("fill", t, s, "carry", want)
        if b.n > MAX_FILE - 3 * TILE:
            out.append(b.finish(f"across{len(out)}", "c", "tile"))
            b = Builder(fmt)
    if b.n:
        out.append(b.finish(f"across{len(out)}", "c", "tile"))
    return out


# ---------------------------------------------------------------------------
# d. round arithmetic

D_TOTALS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def _blank_step(b, at, carry, ntok=0, long_token=False):
    """the step at `at` holds `ntok` token starts of its own (inside a line:
    a run of blanks, or one token longer than the step) and is entered with
    `carry`"""
    lead = "1 " + b.feat(5) + " "
    b.pad_to(at - len(lead) - (8 if long_token else 0), mod=carry, extra=2 + long_token)
    b.put(lead)
    if long_token:
        head = "7:" if b.fmt == "libsvm" else "1:7:"  # leading zeros: the value stays small
        b.put(head + "0" * (STEP + 8 - len(head) - 12) + "1." + _digits(10, 5))
    else:
        inner = "".join(b.feat() + " " for _ in range(ntok))
        b.put(" " * (STEP - len(inner)) + inner)
    b.put(" " + b.feat() + "\n")
    t, s = step_of(at)
    b.claim("fill", t, s, "carry_in", carry)
    b.claim("fill", t, s, "ntok", ntok)


def _group_d(fmt):
    out = []
    # every total, entered with carry 0 and with carry 37 (or the total itself)
    for name, carry_of in (("totals", lambda total: 0), ("totals_carried", lambda total: min(37, total))):
        b = Builder(fmt)
        at = TILE + STEP
        for total in D_TOTALS:
            carry = carry_of(total)
            if total == carry:
                _blank_step(b, at, carry)
            else:
                b.pad_to(at, mod=carry)
                b.put(b.block(total - carry, STEP))
            t, s = step_of(at)
            b.claim("fill", t, s, "total", total)
            b.claim("fill", t, s, "carry_in", carry)
            at += 2 * STEP  # steps 1 and 3 of each tile: the step between sets the carry
        out.append(b.finish(name, "d", "tile"))
    # fewer tokens than the carried remainder: carry 60, then 0 and 3 tokens
    for name, ntok, long_token in (("short_step0", 0, False), ("short_step3", 3, False),
                                   ("short_step_token", 0, True)):
        b = Builder(fmt)
        _blank_step(b, TILE + STEP, 60, ntok, long_token)
        b.claim("fill", 1, 1, "rest", ntok)
        b.claim("fill", 1, 1, "ndec", 60)
        _blank_step(b, 2 * TILE + 2 * STEP, 60, ntok, long_token)
        out.append(b.finish(name, "d", "tile", dyadic=not long_token))
    # the last step of a tile with carry 63 and no token of its own
    b = Builder(fmt)
    _blank_step(b, TILE + 3 * STEP, ROUND - 1)
    b.claim("fill", 1, 3, "ndec", ROUND - 1)
    out.append(b.finish("last_step_carry63", "d", "tile"))
    # the deferred ring
    plans = (("defer_all", 160, range(160), 160), ("defer_one_per_round", 192, (5, 69, 133), 3),
             ("defer_64", 160, range(40, 104), 64), ("defer_65", 160, range(40, 105), 65))
    for name, k, which, count in plans:
        b = Builder(fmt)
        for at in (TILE + STEP, 2 * TILE + 3 * STEP):
            b.pad_to(at, mod=0)
            b.put(b.block(k, STEP, frozenset(which)))
            t, s = step_of(at)
            b.claim("defer", t, s, count)
            b.claim("fill", t, s, "carry_in", 0)
        out.append(b.finish(name, "d", "tile"))
    b = Builder(fmt)  # a deferred token among the carried ones
    b.pad_to(TILE + STEP, mod=0)
    b.put(b.block(131, STEP, frozenset((7, 128, 129, 130))))
    b.claim("fill", 1, 1, "carry", 3)
    b.claim("defer_tail", 1, 1, 3)
    out.append(b.finish("defer_carried", "d", "tile"))
    return out


# ---------------------------------------------------------------------------
# e. weights and qid (the non-lean fill)

E_QID_DIGITS = (1, 7, 8, 9, 15, 16, 17, 20)
E_NEAR = ("third", "letter", "junk", "qline")


def _group_e(fmt):
    out = []
    for d in (-1, 0, 1):
        b = Builder(fmt)
        for edge in EDGES:
            b.pad_to(edge + d)
            b.mark(edge + d, "1")
            b.claim("line", edge + d, True)
            b.put("1:0.5 " + b.feat() + "\n")
        out.append(b.finish(f"weight_label_{d + 1}", "e", "tile"))
    # the first weight of the chunk in its last tile: the column is allocated
    # then and the chunk is written again
    b = Builder(fmt)
    b.pad_to(2 * TILE + 300)
    b.put("0:0.25 " + b.feat() + "\n")
    out.append(b.finish("weight_last_tile", "e", "tile"))
    if fmt != "libsvm":
        return out
    for d in (-1, 0, 1):
        # d = 0: the label is in the previous lane, half, step, tile (prev == 0:
        # the global check, the row before R)
        b = Builder(fmt)
        for i, edge in enumerate(EDGES):
            b.put_at(edge + d, f"qid:{i + 3} " + b.feat() + "\n")
            b.claim("q", edge + d, True)
        out.append(b.finish(f"qid_{d + 1}", "e", "tile"))
    b = Builder(fmt)  # crossing a step end inside the staged tail
    for i, end in enumerate((TILE + STEP, TILE + 2 * STEP, TILE + 3 * STEP, 2 * TILE)):
        b.put_at(end - 3, f"qid:12345678{i} " + b.feat() + "\n")
        b.claim("q", end - 3, True)
    out.append(b.finish("qid_tail", "e", "tile"))
    b = Builder(fmt)  # digit counts and signs, among lines without a qid
    b.pad_to(TILE - 40)
    for n, sign in itertools.product(E_QID_DIGITS, ("", "+", "-")):
        b.put(f"1 qid:{sign}{'12345678901234567890'[:n]} " + b.feat() + "\n")
        b.put("0 " + b.feat() + "\n")
    out.append(b.finish("qid_digits", "e", "tile"))
    # near-misses at a tile start: the exact kernels own them
    near = {"third": ("0 2:1 ", "qid:9 5:1\n"), "letter": ("1 qid:7 ", "qid:8 5:1\n"),
            "junk": ("1 ", "qid:3x 6:1\n"), "qline": ("", "qid:4 1 2:2\n")}
    for name in E_NEAR:
        lead, s = near[name]
        b = Builder(fmt)
        b.put_at(TILE, s, lead=lead)
        b.claim("q", TILE, True)
        out.append(b.finish(f"near_{name}", "e", "exact"))
    return out


# ---------------------------------------------------------------------------
# f. hash-kernel ownership


def _search(build, test, lo, hi):
    """the first parameter in [lo, hi) whose text passes `test` on the model"""
    for x in range(lo, hi):
        b = build(x)
        if b is not None and test(b.text(), b.fmt):
            return b
    raise AssertionError("no placement found")


def _group_f(fmt):
    out = []
    T = TILE
    # the last owned line of tile 0 goes on past the tile end
    for name, past in (("past_1", 1), ("past_1step", STEP + 100), ("past_2steps", 2 * STEP + 100),
                       ("past_5steps", 5 * STEP + 100), ("past_2tiles", 2 * TILE + 300)):
        b = Builder(fmt)
        b.pad_to(T - 100)
        b.put(long_line(b, 100 + past + 1))
        b.mark(T + past, "\n")
        nsteps = STEPS + (past + STEP - 1) // STEP if past > 1 else STEPS + 1
        b.claim("hash_tile", 0, "nsteps", nsteps)
        if past > 2 * TILE:
            b.claim("hash_tile", 1, "own", 0)
            b.claim("hash_tile", 2, "own", 0)
        out.append(b.finish(name, "f", "tile"))
    # the first line start of a tile: lane 0 byte 1, the b half, the last byte
    for name, off in (("first_line_byte1", 1), ("first_line_b_half", HALF + 5 * LANE + 3),
                      ("first_line_last_byte", TILE - 1)):
        b = Builder(fmt)
        b.pad_to(T - 60)
        b.put(long_line(b, 60 + off))
        b.mark(T + off - 1, "\n")
        b.claim("line", T + off, True)
        b.put("1 " + b.feat() + "\n")
        text = b.text()
        assert not starts(text, fmt)[2][T:T + off].any()
        out.append(b.finish(name, "f", "tile"))
    # owned lines that end with the tile: `\n`, or `\r` with `\n` in the next tile
    b = Builder(fmt)
    b.pad_to(T)
    b.mark(T - 1, "\n")
    b.put_at(2 * T - 1, "\r\n", lead="1 " + b.feat(5))
    b.claim("hash_tile", 0, "nsteps", STEPS)
    b.claim("hash_tile", 1, "nsteps", STEPS)
    out.append(b.finish("ends_with_tile", "f", "tile"))
    # carry + ntok = 428 and 429: the second is listed in two halves
    for total in (HASH_LIST_CAP, HASH_LIST_CAP + 1):
        def build(x, total=total):
            b = Builder(fmt)
            b.pad_to(T + STEP, mod=x)    # step 0 leaves x tokens
            carry = hash_model(b.text() + "1\n", fmt)[1].steps[0].carry
            b.put(b.block(total - carry, STEP))
            return b
        b = _search(build, lambda text, f, total=total: (
            lambda st: st.total == total and st.carry_in > 0)(hash_model(text + "1\n", f)[1].steps[1]),
            5, ROUND)
        b.claim("hash", 1, 1, "total", total)
        b.claim("hash", 1, 1, "split", total > HASH_LIST_CAP)
        out.append(b.finish(f"list_{total}", "f", "tile"))
    # a half above the list: the exact kernels
    b = Builder(fmt)
    b.pad_to(T + STEP)
    b.put("1\n" * HASH_LIST_CAP + b.block(1, HALF - 2 * HASH_LIST_CAP) + b.block(20, HALF))
    b.claim("hash", 1, 1, "ntok_a", HASH_LIST_CAP + 1)
    b.claim("hash_tile", 1, "exact", True)
    out.append(b.finish("half_a_429", "f", "tile", hexpect="exact"))
    def build(x):  # the same through carried tokens: carry + ntok_a = 429
        b = Builder(fmt)
        b.pad_to(T + STEP, mod=x)
        carry = hash_model(b.text() + "1\n", fmt)[1].steps[0].carry
        if carry == 0:
            return None
        lines = HASH_LIST_CAP - carry
        b.put("1\n" * lines + b.block(1, HALF - 2 * lines) + b.block(20, HALF))
        b.claim("hash", 1, 1, "carry_in", carry)
        b.claim("hash", 1, 1, "ntok_a", lines + 1)
        return b
    b = _search(build, lambda text, f: hash_model(text + "1\n", f)[1].exact, 5, ROUND)
    b.claim("hash_tile", 1, "exact", True)
    out.append(b.finish("half_a_carry_429", "f", "tile", hexpect="exact"))
    b = Builder(fmt)
    b.pad_to(T + STEP)
    b.put(b.block(20, STEP - 2 * (HASH_LIST_CAP + 1)) + "1\n" * (HASH_LIST_CAP + 1))
    b.claim("hash", 1, 1, "ntok_b", HASH_LIST_CAP + 1)
    b.claim("hash_tile", 1, "exact", True)
    out.append(b.finish("half_b_429", "f", "tile", hexpect="exact"))
    # the carry-area rule: the left-over token starts just before / at step byte 1024
    for name, off, carry in (("left_1023", HALF - 1, 0), ("left_1024", HALF, 1)):
        tok = Builder(fmt).feat()
        def build(x, off=off, tok=tok):
            b = Builder(fmt)
            b.pad_to(T + STEP)
            lead = "1 "
            b.put(b.block(x, off - len(lead)))
            b.put(lead + tok + " " * (STEP - off - len(tok) - 1) + "\n")
            return b
        b = _search(build, lambda text, f: (
            lambda st: st.total % ROUND == 1)(hash_model(text + "1\n", f)[1].steps[1]), 60, 130)
        b.claim("hash", 1, 1, "carry", carry)
        b.claim("tok", T + STEP + off, True)
        out.append(b.finish(name, "f", "tile"))
    # a carried token that needs the generic parser (16 fraction digits): its
    # global offset lies before the step that decodes it
    tok = ("7:" if fmt == "libsvm" else "1:7:") + "0.2500000000000000"
    def build(x):
        b = Builder(fmt)
        b.pad_to(T + STEP)
        b.put(b.block(x, STEP - 40))
        b.put("1 " + tok + " " * (40 - 3 - len(tok)) + "\n")
        return b
    b = _search(build, lambda text, f: hash_model(text + "1\n", f)[1].steps[1].carry == 1, 60, 130)
    b.claim("hash", 1, 1, "carry", 1)
    b.claim("hash", 1, 1, "first_left", STEP - 38)
    b.claim("hash", 1, 2, "carry_in", 1)
    out.append(b.finish("carried_generic", "f", "tile"))
    return out


# ---------------------------------------------------------------------------
# g. chunk ends

G_SIZES = (1, 2, 15, 16, 17, 63, 64, 65, TILE, 2 * TILE)
G_ENDS = {"digit": "", "blank": " ", "cr": "\r"}


def _group_g(fmt):
    out = []
    ends = dict(G_ENDS)
    ends.update({k + "_nl": v + "\n" for k, v in G_ENDS.items()})
    for size, (last, end) in itertools.product(G_SIZES, ends.items()):
        row = "1 " + ("3:0.5" if fmt == "libsvm" else "1:3:0.5")  # the last row, at the least "1"
        room = size - len(end)
        if room < 1:
            continue
        b = Builder(fmt)
        if room >= len(row) + 2:
            b.pad_to(room - len(row))
            b.put(row)
        elif room >= len(row):
            b.put(row + "5" * (room - len(row)))
        else:
            b.put("1" * room)
        case = b.finish(f"size_{size}_{last}", "g", "tile", tail=0, end=end, dyadic=False)
        assert len(case.text) == size
        out.append(case)
    for name, text in csv_cases.svm_end_cases(fmt):
        out.append(Case("g_" + name, "g", fmt, text, "tile", (), (), "tile", False, False))
    return out


_BUILD = {"a": _group_a, "b": _group_b, "c": _group_c, "d": _group_d, "e": _group_e,
          "f": _group_f, "g": _group_g}


@functools.lru_cache(maxsize=None)
def cases(group, fmt):
    out = _BUILD[group](fmt)
    assert len({c.name for c in out}) == len(out)
    return out


def write(case, path):
    with open(path, "wb") as f:
        f.write(case.text.encode("latin-1"))
    return path


@functools.lru_cache(maxsize=None)
def oracle_rows(text, fmt):
    return pyref.parse_libsvm(text) if fmt == "libsvm" else pyref.parse_libfm(text)


@functools.lru_cache(maxsize=None)
def _oracle(text, fmt, index64):
    rows = oracle_rows(text, fmt)
    feats = [f for r in rows for f in r[-1]]
    lens = [len(r[-1]) for r in rows]
    wrap = (1 << 64) if index64 else (1 << 32)
    out = {
        "label": np.array([r[0] for r in rows], np.float32),
        "weight": np.array([1.0 if r[1] is None else r[1] for r in rows], np.float32),
        "qid": np.array([(r[2] or 0) if fmt == "libsvm" else 0 for r in rows], np.uint64),
        "offset": np.cumsum([0] + lens).astype(np.uint64),
        "index": np.array([f[-2] % wrap for f in feats], np.uint64),
        "value": np.array([1.0 if f[-1] is None else f[-1] for f in feats], np.float32),
        "field": np.array([f[0] % wrap for f in feats], np.uint64) if fmt == "libfm" else None,
    }
    return out


def oracle(case, index64=False):
    """the arrays of pyref.concat_blocks that the reference grammar gives"""
    return _oracle(case.text, case.fmt, index64)


def first_difference(case, got, want):
    """None, or a message: the array, the first differing row or entry, the
    byte offset of its token and the nearest mark"""
    _, tm, lm, _ = starts(case.text, case.fmt)
    line_at = np.flatnonzero(lm)
    feat_at = np.flatnonzero(tm & ~lm)
    keys = ("offset", "label", "weight", "qid", "index", "value") + \
        (("field",) if case.fmt == "libfm" else ())
    for k in keys:
        # (a block without features has no field array)
        g, w = (np.zeros(0, np.uint64) if x[k] is None else np.asarray(x[k]) for x in (got, want))
        if k in ("label", "weight", "value"):
            g, w = g.astype(np.float32).view(np.uint32), w.astype(np.float32).view(np.uint32)
        if g.shape == w.shape and np.array_equal(g, w):
            continue
        m = min(len(g), len(w))
        bad = np.flatnonzero(g[:m] != w[:m])
        at = int(bad[0]) if len(bad) else m
        if k in ("index", "value", "field"):
            where = int(feat_at[at]) if at < len(feat_at) else -1
        else:
            row = max(at - 1, 0) if k == "offset" else at
            where = int(line_at[row]) if row < len(line_at) else -1
        near = min(case.marks, key=lambda mk: abs(mk[0] - where)) if case.marks else None
        show = lambda a: (a[at] if at < len(a) else None)  # noqa: E731
        return (f"{case.name} ({case.fmt}): {k}[{at}] is {show(g)!r}, want {show(w)!r} "
                f"(lengths {len(g)} / {len(w)}); its token starts at byte {where} = tile "
                f"{where // TILE} + {where % TILE} (step {where % TILE // STEP}, byte "
                f"{where % STEP}): {case.text[where:where + 48]!r}; nearest mark {near}")
    return None
