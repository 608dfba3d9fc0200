"""Pure-Python reference of the framework's text grammars (documented in
src/data/libsvm_parser.h, libfm_parser.h, csv_parser.h) and of the reference
dmlc strtof arithmetic, used as an independent oracle for the C++ and HIP
parsers."""
import struct

import numpy as np

DIGITCHARS = set("0123456789+-.eE")


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def strtof(s: str) -> float:
    """Reference dmlc::data::strtof arithmetic (src/data/strtonum.h:37-97)."""
    p, n = 0, len(s)
    sign = True
    if p < n and s[p] == "-":
        sign, p = False, p + 1
    elif p < n and s[p] == "+":
        p += 1
    value = f32(0.0)
    while p < n and s[p].isdigit():
        value = f32(f32(value * f32(10.0)) + f32(float(ord(s[p]) - 48)))
        p += 1
    if p < n and s[p] == ".":
        p += 1
        pow10, val2 = 1, 0
        while p < n and s[p].isdigit():
            val2 = (val2 * 10 + ord(s[p]) - 48) % (1 << 64)
            pow10 = (pow10 * 10) % (1 << 64)
            p += 1
        value = f32(value + f32(float(val2) / float(pow10)))
    if p < n and s[p] in "eE":
        p += 1
        frac = False
        if p < n and s[p] == "-":
            frac, p = True, p + 1
        elif p < n and s[p] == "+":
            p += 1
        expon = 0
        while p < n and s[p].isdigit():
            expon = (expon * 10 + ord(s[p]) - 48) % (1 << 32)
            p += 1
        expon = min(expon, 38)
        scale = f32(1.0)
        while expon >= 8:
            scale = f32(scale * 1e8)
            expon -= 8
        while expon > 0:
            scale = f32(scale * 10.0)
            expon -= 1
        value = f32(value / scale) if frac else f32(value * scale)
    return value if sign else -value


def strtouint(s: str, bits: int = 32) -> int:
    p = 0
    if p < len(s) and s[p] in "+-":
        p += 1
    v = 0
    while p < len(s) and s[p].isdigit():
        v = (v * 10 + ord(s[p]) - 48) % (1 << bits)
        p += 1
    return v


def parse_pair(tok: str, t1, t2):
    """ParsePair inside one token -> (r, v1, v2)."""
    i, n = 0, len(tok)
    while i < n and tok[i] not in DIGITCHARS:
        i += 1
    if i == n:
        return 0, None, None
    j = i
    while j < n and tok[j] in DIGITCHARS:
        j += 1
    v1 = t1(tok[i:j])
    p = j
    while p < n and tok[p] in " \t":
        p += 1
    if p == n or tok[p] != ":":
        return 1, v1, None
    p += 1
    while p < n and tok[p] not in DIGITCHARS:
        p += 1
    q = p
    while q < n and tok[q] in DIGITCHARS:
        q += 1
    return 2, v1, t2(tok[p:q])


def parse_triple(tok: str):
    r, a, rest = 0, None, None
    i, n = 0, len(tok)
    while i < n and tok[i] not in DIGITCHARS:
        i += 1
    if i == n:
        return 0, None, None, None
    j = i
    while j < n and tok[j] in DIGITCHARS:
        j += 1
    a = strtouint(tok[i:j])
    if j == n or tok[j] != ":":
        return 1, a, None, None
    r2, b, c = parse_pair(tok[j + 1:], strtouint, strtof)
    if r2 == 0:
        return 2, a, 0, None
    if r2 == 1:
        return 2, a, b, None
    return 3, a, b, c


def _lines(text: str):
    import re
    for line in re.split(r"[\r\n]+", text):
        if line:
            yield line


def parse_libsvm(text: str):
    rows = []  # (label, weight|None, qid|None, [(idx, val|None)])
    for line in _lines(text):
        toks = [t for t in line.replace("\t", " ").split(" ") if t]
        if not toks:
            continue
        r, lab, w = parse_pair(toks[0], strtof, strtof)
        if r < 1:
            continue
        qid = None
        feats = []
        for k, tok in enumerate(toks[1:]):
            if k == 0 and tok.startswith("qid:"):
                s = tok[4:]
                neg = s.startswith("-")
                v = strtouint(s.lstrip("+-"), 64)
                qid = (-v) % (1 << 64) if neg else v
                continue
            rr, idx, val = parse_pair(tok, strtouint, strtof)
            if rr < 1:
                continue
            feats.append((idx, val if rr == 2 else None))
        rows.append((lab, w if r == 2 else None, qid, feats))
    return rows


def parse_libfm(text: str):
    rows = []
    for line in _lines(text):
        toks = [t for t in line.replace("\t", " ").split(" ") if t]
        if not toks:
            continue
        r, lab, w = parse_pair(toks[0], strtof, strtof)
        if r < 1:
            continue
        feats = []
        for tok in toks[1:]:
            rr, fid, idx, val = parse_triple(tok)
            if rr <= 1:
                continue
            feats.append((fid, idx, val if rr == 3 else None))
        rows.append((lab, w if r == 2 else None, feats))
    return rows


_FIELD_VALUES = {}


def _field_value(f: str) -> float:
    v = _FIELD_VALUES.get(f)
    if v is None:
        v = _FIELD_VALUES[f] = strtof(f.lstrip(" \t\r\n\f"))
    return v


def parse_csv(text: str, label_column=-1, delim=",", weight_column=-1):
    """rows (label, features); with a weight column (src/data/csv_parser.h:
    the label column is tested first, a row without the column weighs 1.0)
    rows (label, features, weight)"""
    rows = []
    for line in _lines(text):
        fields = line.split(delim)
        # reference csv_parser.h:83-96: after skipping a delimiter the loop stops
        # when p reaches the line end, so a trailing delimiter adds no field
        if len(fields) > 1 and fields[-1] == "":
            fields.pop()
        lab, wgt = 0.0, 1.0
        feats = []
        for c, f in enumerate(fields):
            v = _field_value(f)
            if c == label_column:
                lab = v
            elif c == weight_column:
                wgt = v
            else:
                feats.append(v)
        rows.append((lab, feats, wgt) if weight_column >= 0 else (lab, feats))
    return rows


def concat_blocks(blocks):
    """Concatenate host blocks into semantic per-row arrays (NULL -> default)."""
    label, weight, qid, offset, index, value, field = [], [], [], [0], [], [], []
    for b in blocks:
        n = len(b["label"])
        label.append(b["label"])
        weight.append(b["weight"] if b["weight"] is not None else np.ones(n, np.float32))
        qid.append(b["qid"] if b["qid"] is not None else np.zeros(n, np.uint64))
        nnz = len(b["index"])
        index.append(b["index"])
        value.append(b["value"] if b["value"] is not None else np.ones(nnz, np.float32))
        if b.get("field") is not None:
            field.append(b["field"])
        offset.extend((b["offset"][1:] + offset[-1]).tolist())
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return {
        "label": cat(label, np.float32), "weight": cat(weight, np.float32),
        "qid": cat(qid, np.uint64), "offset": np.array(offset, np.uint64),
        "index": cat(index, np.uint64), "value": cat(value, np.float32),
        "field": cat(field, np.uint64) if field else None,
    }


# ---------------------------------------------------------------------------
# References of the numeric kernels (K9 hash, OCP fp8 e4m3, bf16, HashedFM).
# Plain numpy in fp64 / integer arithmetic; tests/test_pyref_numeric.py checks
# them on the CPU.

M64 = (1 << 64) - 1


def ref_hash(keys: np.ndarray, seed: int) -> np.ndarray:
    """K9's hash: murmur3 fmix64 of key ^ seed * golden ratio, low 32 bits."""
    x = [int(k) for k in keys]
    out = np.empty(len(x), dtype=np.uint64)
    s = (seed * 0x9E3779B97F4A7C15) & M64
    for i, v in enumerate(x):
        v ^= s
        v = ((v ^ (v >> 33)) * 0xFF51AFD7ED558CCD) & M64
        v = ((v ^ (v >> 33)) * 0xC4CEB9FE1A85EC53) & M64
        v ^= v >> 33
        out[i] = v & 0xFFFFFFFF
    return out


def ref_dense(host, dim, seed, libfm):
    """fp64 hashed dense rows of a host CSR and the number of terms per bucket."""
    rows = len(host["label"])
    off = host["offset"].astype(np.int64)
    idx = host["index"].astype(np.uint64)
    val = (host["value"].astype(np.float64) if host.get("value") is not None
           else np.ones(len(idx)))
    keys = idx ^ (host["field"].astype(np.uint64) << np.uint64(40)) if libfm else idx
    h = ref_hash(keys, seed)
    bucket = (h % np.uint64(dim)).astype(np.int64)
    sign = np.where(h & np.uint64(0x80000000), -1.0, 1.0)
    rowid = np.repeat(np.arange(rows), np.diff(off))
    out = np.zeros((rows, dim), dtype=np.float64)
    np.add.at(out, (rowid, bucket), sign * val)
    share = np.zeros((rows, dim), dtype=np.int64)
    np.add.at(share, (rowid, bucket), 1)
    return out, share


def ref_dense_abs(host, dim, seed, libfm):
    """sum of |value| per bucket (the scale of the f32 accumulation bound)"""
    pos = dict(host)
    pos["value"] = (np.abs(host["value"]) if host.get("value") is not None
                    else np.ones(len(host["index"]), np.float32))
    rows = len(host["label"])
    off = host["offset"].astype(np.int64)
    idx = host["index"].astype(np.uint64)
    keys = idx ^ (host["field"].astype(np.uint64) << np.uint64(40)) if libfm else idx
    bucket = (ref_hash(keys, seed) % np.uint64(dim)).astype(np.int64)
    rowid = np.repeat(np.arange(rows), np.diff(off))
    out = np.zeros((rows, dim), dtype=np.float64)
    np.add.at(out, (rowid, bucket), pos["value"].astype(np.float64))
    return out


def e4m3_decode_table() -> np.ndarray:
    """float64 value of every OCP e4m3fn byte (bias 7, no inf, 0x7F / 0xFF NaN)"""
    out = np.empty(256, dtype=np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        out[b] = -v if b & 0x80 else v
    return out


E4M3 = e4m3_decode_table()
E4M3_FINITE = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=np.uint8)
E4M3_MAX = 448.0
# the largest magnitude that rounds to a finite code: the midpoint of 448 and
# the 480 that 0x7F would be, a tie that goes to the even mantissa of 448
E4M3_ROUND_MAX = 464.0


def e4m3_nearest_even(x) -> np.ndarray:
    """round-to-nearest-even of finite |x| <= 464 to an e4m3fn byte, by search
    over the decoded codes (ties: the code with the even mantissa bit); -0 and
    negative values that round to zero give 0x80"""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.abs(x) <= E4M3_ROUND_MAX)
    mag = E4M3[:0x7F]  # 0x00 .. 0x7E ascending
    a = np.abs(x)
    hi = np.searchsorted(mag, a, side="left").clip(1, 0x7E)
    lo = hi - 1
    dlo, dhi = a - mag[lo], mag[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    exact = mag[hi.clip(0, 0x7E)] == a
    code = np.where(exact, hi, code)
    code = np.where(a == 0, 0, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def fp8_edge_values() -> np.ndarray:
    """f32 inputs where an f32 -> e4m3 conversion can go wrong: every finite
    code, every midpoint of neighbouring codes with the f32 neighbours on both
    sides, +-0, 2^-10 (the tie between 0 and the smallest subnormal) and its
    neighbours, +-448 and the values up to 464 that still round to 448"""
    mag = E4M3[:0x7F].astype(np.float32)
    mids = ((mag[:-1].astype(np.float64) + mag[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.all(mids.astype(np.float64) * 2 == mag[:-1].astype(np.float64) + mag[1:])
    inf = np.float32(np.inf)
    pos = np.concatenate([
        mag, mids, np.nextafter(mids, inf), np.nextafter(mids, -inf),
        np.nextafter(mag[1:], inf), np.nextafter(mag[1:], -inf),
        np.array([2.0 ** -10, 2.0 ** -11, 2.0 ** -20, 1e-30, 448, 449, 456, 460, 463, 464],
                 dtype=np.float32),
        np.nextafter(np.array([2.0 ** -10, 448, 464], dtype=np.float32), -inf),
        np.nextafter(np.array([2.0 ** -10, 448], dtype=np.float32), inf)])
    vals = np.concatenate([pos, -pos]).astype(np.float32)
    assert np.all(np.abs(vals) <= E4M3_ROUND_MAX)
    return vals


def fp8_out_of_range_values() -> np.ndarray:
    """f32 inputs past the finite range of the conversion: just above 464, the
    would-be next codes, large finite values, +-inf and NaN"""
    inf = np.float32(np.inf)
    pos = np.array([np.nextafter(np.float32(464), inf), 465, 480, 512, 1000, 65504, 1e10,
                    3.0e38, np.inf], dtype=np.float32)
    return np.concatenate([pos, -pos, np.array([np.nan], dtype=np.float32)])


def bf16_round(x) -> np.ndarray:
    """float32 -> bfloat16 (round to nearest even) -> float32, finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def f32_mul(a, b) -> np.ndarray:
    """the f32 product of f32 operands (one rounding), as the kernels form it"""
    return (np.asarray(a, np.float32) * np.asarray(b, np.float32)).astype(np.float32)


U23 = 2.0 ** -23
U24 = 2.0 ** -24


def fm_forward_ref(xb, wt, q, bias, sx):
    """F1 / F5 forward in fp64 on the kernel's own operands.

    xb: uint8 e4m3 codes [rows, dim]; wt: [17, dim] values exactly
    representable in bf16 (row 0 w, rows 1..16 V^T); q: f32 [dim]; sx as passed
    (an f32).  Returns (y, xv, y_tol, xv_tol).

    Bounds: a K-term product sum is allowed K * 2^-23 * sum |a_k b_k| (twice
    the any-order f32 bound: the MFMA's internal accumulation rounding is not
    specified; the bf16 x bf16 products and x^2 are exact in f32).  They go to
    first order through y = b + sx lin + 1/2 sx^2 (sum_f a_f^2 - x^2.q), plus
    8 * 2^-24 of the sum of the absolute terms for the epilogue's roundings;
    xv = sx a_f adds one more rounding."""
    x = E4M3[xb]
    rows, dim = x.shape
    wt = np.asarray(wt, np.float64)
    q = np.asarray(q, np.float64)
    sx = float(np.float32(sx))
    acc = x @ wt.T                      # [rows, 17]
    e_acc = dim * U23 * (np.abs(x) @ np.abs(wt).T)
    x2q = (x * x) @ q
    e_q = dim * U23 * ((x * x) @ np.abs(q))
    lin, a = acc[:, 0], acc[:, 1:]
    sq = (a * a).sum(1)
    y = bias + sx * lin + 0.5 * sx * sx * (sq - x2q)
    mag = abs(bias) + np.abs(sx * lin) + 0.5 * sx * sx * (sq + np.abs(x2q))
    y_tol = (abs(sx) * e_acc[:, 0]
             + 0.5 * sx * sx * ((2 * np.abs(a) * e_acc[:, 1:]).sum(1) + e_q) + 8 * U24 * mag)
    xv = sx * a
    xv_tol = abs(sx) * e_acc[:, 1:] + 2 * U24 * np.abs(xv)
    return y, xv, y_tol, xv_tol


def fm_g_operand(g, xv):
    """F2's G = [g, g xv] as put_g rounds it: bf16(g), bf16(f32(g * xv_f));
    g f32 [rows], xv f32 [rows, 16] -> fp64 [rows, 17]"""
    g = np.asarray(g, np.float32)
    xv = np.asarray(xv, np.float32)
    return np.concatenate([bf16_round(g)[:, None], bf16_round(f32_mul(g[:, None], xv))],
                          axis=1).astype(np.float64)


def fm_backward_ref(xb, g, xv):
    """sum over blocks of F2's partials in fp64: rows 0..16 Z = G^T x, row 17
    t = (x^2)^T g (g in f32, x^2 exact).  Returns (z [18, dim], tol): a product
    sum over the batch's rows gets rows * 2^-23 * sum |terms| (fm_forward_ref)."""
    x = E4M3[xb]
    rows = x.shape[0]
    gm = fm_g_operand(g, xv)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    z = np.concatenate([gm.T @ x, (g64[None, :] @ (x * x))], axis=0)
    mag = np.concatenate([np.abs(gm).T @ np.abs(x), np.abs(g64)[None, :] @ (x * x)], axis=0)
    return z, max(rows, 1) * U23 * mag


def fm_grads_ref(part, v, sx):
    """F3 / F4 in fp64: Z = sum_b part[b]; dw = s Z_0, dV_nf = s Z_{1+f,n} -
    V_nf s^2 Z_17,n.  part [nblk, 18, dim], v [dim, 16].  Returns (dw, dv,
    dw_tol, dv_tol): the nblk-term f32 sums get (nblk + 4) * 2^-24 * sum |part|
    (any order), the two or three products and the subtraction 4 * 2^-24 of
    the absolute terms."""
    p = np.asarray(part, np.float64)
    v = np.asarray(v, np.float64)
    sx = float(np.float32(sx))
    nblk = p.shape[0]
    z = p.sum(0)
    ez = (nblk + 4) * U24 * np.abs(p).sum(0)
    dw = sx * z[0]
    dw_tol = abs(sx) * ez[0] + 4 * U24 * np.abs(dw)
    t = sx * sx * z[17]
    dv = sx * z[1:17].T - v * t[:, None]
    dv_tol = (abs(sx) * ez[1:17].T + np.abs(v) * (sx * sx * ez[17])[:, None]
              + 4 * U24 * (np.abs(sx * z[1:17].T) + np.abs(v * t[:, None])))
    return dw, dv, dw_tol, dv_tol


def csr_dot_ref(off, idx, val, w, bias=0.0):
    """K11 in fp64: y, and its f32 any-order bound (terms + 4) * 2^-24 * (sum
    |v_j w_j| + |bias|) per row.  off may start above 0 (a row slice)."""
    off = np.asarray(off, np.int64)
    idx = np.asarray(idx).astype(np.int64)
    lo, hi = int(off[0]), int(off[-1])
    lens = np.diff(off)
    rows = np.repeat(np.arange(len(lens)), lens)
    v = (np.ones(len(idx)) if val is None else np.asarray(val, np.float64))[lo:hi]
    prod = v * np.asarray(w, np.float64)[idx[lo:hi]]
    y = np.bincount(rows, weights=prod, minlength=len(lens)) + bias
    mag = np.bincount(rows, weights=np.abs(prod), minlength=len(lens)) + abs(bias)
    return y, (lens + 4) * U24 * mag


def csr_dot_t_ref(off, idx, val, d, nfeat):
    """K11^T in fp64: g[index[j]] += value[j] * d[row(j)], and the same bound
    with the feature's entry count as the number of terms"""
    off = np.asarray(off, np.int64)
    idx = np.asarray(idx).astype(np.int64)
    lo, hi = int(off[0]), int(off[-1])
    lens = np.diff(off)
    rows = np.repeat(np.arange(len(lens)), lens)
    v = (np.ones(len(idx)) if val is None else np.asarray(val, np.float64))[lo:hi]
    prod = v * np.asarray(d, np.float64)[rows]
    g = np.zeros(nfeat)
    mag = np.zeros(nfeat)
    np.add.at(g, idx[lo:hi], prod)
    np.add.at(mag, idx[lo:hi], np.abs(prod))
    cnt = np.bincount(idx[lo:hi], minlength=nfeat)
    return g, (cnt + 4) * U24 * mag
