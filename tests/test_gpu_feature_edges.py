"""K9 (ops.hashed_dense), the fused text -> hash kernels and K11 (ops.spmv /
ops.spmv_t) at the shapes and values the synthetic-data tests never reach:
a second row per wave, every dim path up to the documented limits (LDS rows
of 64 KiB and more), 64-bit keys, every e4m3 rounding edge, row lengths
around the 16-lane group and the grid-stride loops.

References: pyref's independent hash with fp64 sums, torch's CPU e4m3 cast
(checked against a nearest-even search in test_pyref_numeric.py), fp64
bincounts.  f32 sums are allowed the any-order accumulation bound
terms * 2^-24 * sum |terms|; nothing in range is exempt from a comparison.
Inputs are built by hand as tensors, so every case runs in a few seconds.
"""
from decimal import Decimal

import numpy as np
import pytest
import torch

import pyref
from dmlc_core_amd import data, ops

pytestmark = pytest.mark.gpu
U24 = pyref.U24


def _csr(lens, rng, index64=False, value=True, field=False, idx_bits=31, field_max=30):
    """host dict (pyref.ref_dense's layout) and device dict of a random CSR
    with the given row lengths"""
    lens = np.asarray(lens, np.int64)
    nnz = int(lens.sum())
    host = {"label": np.zeros(len(lens), np.float32),
            "offset": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            "index": rng.integers(0, 1 << idx_bits, size=nnz, dtype=np.uint64),
            "value": None, "field": None}
    if value:
        mag = rng.uniform(0.5, 2.0, size=nnz)
        host["value"] = (mag * rng.choice([-1.0, 1.0], size=nnz)).astype(np.float32)
    if field:
        host["field"] = rng.integers(0, field_max, size=nnz, dtype=np.uint64)
    return host, _to_device(host, index64)


def _to_device(host, index64=False):
    it = np.int64 if index64 else np.int32
    t = {"offset": torch.from_numpy(host["offset"]).cuda(),
         "index": torch.from_numpy(host["index"].astype(it)).cuda()}
    if host.get("value") is not None:
        t["value"] = torch.from_numpy(host["value"]).cuda()
    if host.get("field") is not None:
        t["field"] = torch.from_numpy(host["field"].astype(it)).cuda()
    return t


def _e4m3(x32):
    """torch's CPU float32 -> e4m3fn cast, as bytes"""
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(
        torch.float8_e4m3fn).view(torch.uint8).numpy()


def _bytes(t):
    return t.cpu().view(torch.uint8).numpy()


def _check_f32(got, ref, mag, share):
    """same buckets, and every sum within share * 2^-24 * sum |v| of fp64
    (one term: exact; the sum of two f32 is correctly rounded: half an ulp)"""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got != 0, ref != 0)
    tol = np.where(share <= 1, 0.0, share * U24 * mag)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5])


def _check_fp8(got, ref, mag, share, scale):
    """bytes equal torch's cast of the f32 sum times scale (product in f32)
    where the f32 sum is order-independent (at most 2 terms); elsewhere the
    conversion is monotonic, so the byte lies between the casts of the two
    ends of the accumulation bound"""
    got = _bytes(got)
    assert got.shape == ref.shape
    want = _e4m3(pyref.f32_mul(ref.astype(np.float32), scale))
    few = share <= 2
    bad = few & (got != want)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    if (~few).any():
        tol = share * U24 * mag
        lo = pyref.E4M3[_e4m3(pyref.f32_mul((ref - tol).astype(np.float32), scale))]
        hi = pyref.E4M3[_e4m3(pyref.f32_mul((ref + tol).astype(np.float32), scale))]
        val = pyref.E4M3[got]
        bad = ~few & ~((val >= np.minimum(lo, hi)) & (val <= np.maximum(lo, hi)))
        assert not bad.any(), (np.argwhere(bad)[:5], val[bad][:5], lo[bad][:5], hi[bad][:5])


# ------------------------------------------------------------------ K9 rows
@pytest.fixture(scope="module")
def two_pass_rows():
    """70 000 rows of 0..3 entries: K9 runs at most 16 384 workgroups of 4
    waves, so row r + 65 536 is the second row of the wave that took row r.
    Rows 0, 4, 8, ... have 3 entries and rows 65 536, 65 540, ... none: what
    the first pass leaves in the LDS row would show in the second."""
    rng = np.random.default_rng(70000)
    lens = rng.integers(0, 4, size=70000)
    lens[0:70000 - 65536:4] = 3
    lens[65536::4] = 0
    host, dev = _csr(lens, rng)
    return host, dev


@pytest.mark.parametrize("dim", [16, 12])
def test_k9_second_row_of_a_wave(two_pass_rows, dim):
    """the readout that consumes an LDS row re-zeroes it for the wave's next
    row: wide (dim 16), 4-column fp8 and scalar f32 (dim 12) readouts"""
    host, dev = two_pass_rows
    ref, share = pyref.ref_dense(host, dim, 5, False)
    mag = pyref.ref_dense_abs(host, dim, 5, False)
    assert (ref[:4464:4] != 0).any(1).all() and not ref[65536::4].any()
    got = ops.hashed_dense(dev, dim, seed=5, fp8=False)
    _check_f32(got, ref, mag, share)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)
    for scale in (1.0, 0.5):
        _check_fp8(ops.hashed_dense(dev, dim, seed=5, fp8=True, scale=scale), ref, mag, share, scale)


# ------------------------------------------------------------------ K9 dims
@pytest.fixture(scope="module")
def shaped_rows():
    """empty rows (leading, trailing, in runs), rows of 1, 63, 64, 65 and
    1 000 entries (one wave iteration is 64 entries) and a 500-entry row"""
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 30, size=260)
    lens[[0, 1, 7, 8, 9, 258, 259]] = 0
    lens[[2, 100]] = 1
    lens[3], lens[4], lens[5], lens[6], lens[50] = 63, 64, 65, 1000, 500
    host, dev = _csr(lens, rng, field=True)
    return host, dev


@pytest.mark.parametrize("dim", [4, 12, 20, 200, 4092, 16, 48, 4096, 4112, 8192, 8188])
def test_k9_every_dim_path(shaped_rows, dim):
    """4-column path (4 .. 4092, 8188) and 16-column path (16 .. 8192), from
    one LDS-atomic address per 125 entries to LDS rows of 128 KiB per
    workgroup, against the independent hash and fp64 sums"""
    host, dev = shaped_rows
    ref, share = pyref.ref_dense(host, dim, 11, True)
    mag = pyref.ref_dense_abs(host, dim, 11, True)
    got = ops.hashed_dense(dev, dim, seed=11, fp8=False)
    _check_f32(got, ref, mag, share)
    if dim == 4:
        # heavy collisions: the 500-entry row lands in 4 buckets
        assert share[50].sum() == 500 and share[50].min() > 64
        err = np.abs(got.cpu().numpy()[50].astype(np.float64) - ref[50])
        assert (err <= 500 * U24 * mag[50]).all(), (err, mag[50])
    for scale in (1.0, 0.3):
        _check_fp8(ops.hashed_dense(dev, dim, seed=11, fp8=True, scale=scale), ref, mag, share, scale)


def test_k9_dim_must_be_a_multiple_of_4(shaped_rows):
    _, dev = shaped_rows
    for dim in (0, 6, 18, 8190, 8196):
        with pytest.raises(Exception, match="multiple of 4"):
            ops.hashed_dense(dev, dim, seed=1, fp8=False)


# ------------------------------------------------------------------ K9 keys
def test_k9_64_bit_keys_fields_and_valueless():
    """index64 with indices at and above 2^40 and fields whose `field << 40`
    meets those bits; indices that differ only above bit 32 hash apart;
    value=None is 1.0; LibFM field 0 is the same key as no field"""
    rng = np.random.default_rng(40)
    lens = rng.integers(0, 12, size=300)
    lens[0] = 4
    host, _ = _csr(lens, rng, field=True, idx_bits=46, field_max=1 << 12)
    host["index"][0::3] |= np.uint64(1 << 40)
    # row 0: the same low 32 bits, apart only above bit 32; the same index in two fields
    host["index"][0:4] = np.array([77, 77 + (1 << 33), 77 + (1 << 45), 77], np.uint64)
    host["field"][0:4] = np.array([3, 3, 3, 3 + (1 << 6)], np.uint64)
    dev = _to_device(host, index64=True)
    for dim in (16, 12):
        ref, share = pyref.ref_dense(host, dim, 2, True)
        mag = pyref.ref_dense_abs(host, dim, 2, True)
        _check_f32(ops.hashed_dense(dev, dim, seed=2, fp8=False), ref, mag, share)
        _check_fp8(ops.hashed_dense(dev, dim, seed=2, fp8=True), ref, mag, share, 1.0)
    # the four keys of row 0 are four different hashes (dim 4096: no chance collision)
    keys = host["index"][0:4] ^ (host["field"][0:4] << np.uint64(40))
    assert len(set(pyref.ref_hash(keys, 2).tolist())) == 4
    ref, share = pyref.ref_dense(host, 4096, 2, True)
    assert (share[0] == 1).sum() == 4
    _check_f32(ops.hashed_dense(dev, 4096, seed=2, fp8=False), ref,
               pyref.ref_dense_abs(host, 4096, 2, True), share)
    # without fields, and without values (every entry 1.0)
    nofield = {k: v for k, v in dev.items() if k != "field"}
    ref, share = pyref.ref_dense(host, 48, 2, False)
    mag = pyref.ref_dense_abs(host, 48, 2, False)
    _check_f32(ops.hashed_dense(nofield, 48, seed=2, fp8=False), ref, mag, share)
    bare = dict(host, value=None)
    ref1, share1 = pyref.ref_dense(bare, 48, 2, True)
    got = ops.hashed_dense({k: v for k, v in dev.items() if k != "value"}, 48, seed=2, fp8=False)
    np.testing.assert_array_equal(got.cpu().numpy(), ref1)  # small integers: exact
    # field 0 everywhere == no field, 32- and 64-bit
    for i64 in (False, True):
        h32 = dict(host, index=host["index"] & np.uint64(0x7FFFFFFF),
                   field=np.zeros_like(host["field"]))
        d0 = _to_device(h32, index64=i64)
        a = ops.hashed_dense(d0, 20, seed=9, fp8=False)
        b = ops.hashed_dense({k: v for k, v in d0.items() if k != "field"}, 20, seed=9, fp8=False)
        assert torch.equal(a, b)
        ref, share = pyref.ref_dense(h32, 20, 9, False)
        _check_f32(a, ref, pyref.ref_dense_abs(h32, 20, 9, False), share)


# ------------------------------------------------------------------ fp8 rounding
def _one_entry_rows(vals):
    n = len(vals)
    return {"label": np.zeros(n, np.float32), "offset": np.arange(n + 1, dtype=np.int64),
            "index": np.arange(1000, 1000 + n, dtype=np.uint64),
            "value": np.asarray(vals, np.float32), "field": None}


@pytest.mark.parametrize("dim", [16, 12])
@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_k9_fp8_rounding_every_edge(dim, scale):
    """one entry per row, so the f32 input of v_cvt_pk_fp8_f32 is known
    exactly (+-value * scale, the product in f32): all 254 finite codes, every
    midpoint of neighbouring codes and its f32 neighbours, the subnormals,
    2^-10, +-448 and the values up to 464.  Every byte equals torch's CPU
    cast -- round to nearest even, no element exempt."""
    vals = pyref.fp8_edge_values()
    if scale != 1.0:
        # values whose f32 product with the scale is an edge value, where one exists
        pre = (vals.astype(np.float64) / np.float32(scale)).astype(np.float32)
        hit = pyref.f32_mul(pre, scale) == vals
        vals = np.concatenate([vals, pre[hit]])
    host = _one_entry_rows(vals)
    dev = _to_device(host)
    ref, share = pyref.ref_dense(host, dim, 4, False)
    assert share.max() == 1 and np.array_equal(np.abs(ref).max(1), np.abs(vals))
    x = pyref.f32_mul(ref.astype(np.float32), scale)
    assert np.abs(x).max() <= 464
    got = _bytes(ops.hashed_dense(dev, dim, seed=4, fp8=True, scale=scale))
    want = _e4m3(x)
    np.testing.assert_array_equal(want, pyref.e4m3_nearest_even(x))
    bad = got != want
    assert not bad.any(), (x[bad][:8], got[bad][:8], want[bad][:8])
    if scale == 1.0:
        assert set(np.unique(got)) >= set(pyref.E4M3_FINITE.tolist()) - {0x80}


# Bytes of f32 values past the finite e4m3 range, as produced by gfx950's
# conversion (v_cvt_pk_fp8_f32): recorded from the hardware, not derived.
# Finite values beyond +-464 and +-inf become the NaN code with the value's
# sign, which is also what torch's CPU cast gives; a NaN becomes 0xFF whether
# the hash's sign is + or - (K9 multiplies the value by the hash's +-1.0
# before it accumulates and converts), where torch gives 0x7F for a +NaN.
FP8_OVERFLOW = {False: 0x7F, True: 0xFF}   # by the sign of the converted f32
FP8_NAN = {1: 0xFF, -1: 0xFF}              # +NaN entry, by the hash's sign


@pytest.mark.parametrize("dim", [16, 12])
def test_k9_fp8_out_of_range_is_pinned(dim):
    """|x| > 464, +-inf and NaN: the bytes as produced by gfx950's conversion,
    the same on the 16-column and the 4-column path"""
    vals = pyref.fp8_out_of_range_values()
    vals = np.concatenate([vals[~np.isnan(vals)], [np.nan, np.nan]]).astype(np.float32)
    host = _one_entry_rows(vals)
    # the two NaN entries get indices whose hash signs differ
    h = pyref.ref_hash(np.arange(5000, 5064, dtype=np.uint64), 4)
    neg = (h & np.uint64(0x80000000)) != 0
    host["index"][-2] = 5000 + int(np.argmin(neg))
    host["index"][-1] = 5000 + int(np.argmax(neg))
    h = pyref.ref_hash(host["index"], 4)
    hsign = np.where(h & np.uint64(0x80000000), -1, 1)
    col = (h % np.uint64(dim)).astype(np.int64)
    assert hsign[-2] == 1 and hsign[-1] == -1
    got = _bytes(ops.hashed_dense(_to_device(host), dim, seed=4, fp8=True))
    seen = {}
    for i, v in enumerate(vals):
        b = int(got[i, col[i]])
        assert not np.delete(got[i], col[i]).any()
        key = ("nan", int(hsign[i])) if np.isnan(v) else float(v) * int(hsign[i])
        seen[key] = hex(b)
    print("fp8 out-of-range bytes:", seen)
    for i, v in enumerate(vals):
        b = int(got[i, col[i]])
        if np.isnan(v):
            assert b == FP8_NAN[int(hsign[i])], (i, hex(b))
        else:
            assert b == FP8_OVERFLOW[bool(np.signbit(v * hsign[i]))], (float(v), hex(b))
            # here the hardware agrees with torch's cast
            assert b == int(_e4m3(np.array([v * hsign[i]], np.float32))[0])


# ------------------------------------------------------------------ fused hash
def _cpu_rows(path, fmt):
    return pyref.concat_blocks(list(data.iter_blocks(path, type=fmt)))


@pytest.mark.parametrize("fmt", ["libsvm", "libfm"])
@pytest.mark.parametrize("dim", [4096, 4080, 4092])
def test_fused_hash_at_the_largest_dims(tmp_path, fmt, dim):
    """the fused kernels at their documented limit: dims 4096 and 4080 on the
    tile kernel (64 KiB of dynamic LDS next to its static staging), 4092 on
    the exact per-line kernel; f32 and fp8 against the independent hash of
    the CPU parser's rows"""
    p = str(tmp_path / f"d.{fmt}")
    data.write_synthetic(p, 0, 200, format=fmt, seed=21)
    host = _cpu_rows(p, fmt)
    libfm = fmt == "libfm"
    ref, share = pyref.ref_dense(host, dim, 6, libfm)
    mag = pyref.ref_dense_abs(host, dim, 6, libfm)
    for fast in (1, 0):
        g = data.GPUParser(p, format=fmt, fast_path=fast)
        f32 = g.parse_all_hashed(dim, seed=6, fp8=False, strategy="fused")
        assert g.stats()["exact_chunks"] == 0 or fast == 0 or dim % 16 != 0
        np.testing.assert_array_equal(f32["label"].cpu().numpy(), host["label"])
        _check_f32(f32["x"], ref, mag, share)
        np.testing.assert_allclose(f32["x"].cpu().numpy(), ref, rtol=1e-6, atol=1e-6)
        f8 = data.GPUParser(p, format=fmt, fast_path=fast).parse_all_hashed(
            dim, seed=6, fp8=True, scale=0.5, strategy="fused")["x"]
        assert f8.dtype == torch.float8_e4m3fn
        _check_fp8(f8, ref, mag, share, 0.5)


def _decimal(v):
    """exact decimal of an f32, cut to 19 fraction digits (the parsers'
    fraction accumulator is 64 bits wide)"""
    d = Decimal(float(v))
    s = format(d.quantize(Decimal(1).scaleb(-19)) if -d.as_tuple().exponent > 19 else d, "f")
    return s


@pytest.mark.parametrize("dim", [16, 12])
@pytest.mark.parametrize("scale", [0.5, 0.3])
def test_fused_fp8_edges_equal_k9_and_torch(tmp_path, dim, scale):
    """the fp8 edge values as text, one feature per line: the fused kernels
    (tile kernel at dim 16, per-line kernel at dim 12) convert the CPU
    parser's f32 value times scale exactly as K9 and torch's cast do.  A power
    of two is applied per token and any other scale at the flush; with 0.5
    the file holds twice the edge values, so the conversion still sees them.
    The out-of-range values go through the same bytes as K9's."""
    edge = pyref.fp8_edge_values()
    vals = (edge * np.float32(2)) if scale == 0.5 else edge
    oor = pyref.fp8_out_of_range_values()
    with np.errstate(over="ignore"):
        oor = oor[np.isfinite(oor)] * np.float32(2 if scale == 0.5 else 4)
    oor = oor[np.isfinite(oor)]
    every = np.concatenate([vals, oor])
    p = str(tmp_path / "edge.libsvm")
    with open(p, "w") as f:
        for i, v in enumerate(every):
            f.write(f"{i % 2} {1000 + i}:{_decimal(v)}\n")
    host = _cpu_rows(p, "libsvm")
    assert len(host["label"]) == len(every)
    parsed = host["value"]
    # the parser reproduces every exactly written code and midpoint
    assert np.isin(pyref.E4M3[:0x7F].astype(np.float32) * np.float32(2 if scale == 0.5 else 1),
                   parsed).all()
    ref, share = pyref.ref_dense(host, dim, 4, False)
    assert share.max() == 1
    x = pyref.f32_mul(ref.astype(np.float32), scale)
    inr = np.abs(x).max(1) <= 464
    assert inr.sum() >= len(vals) - 8 and (~inr).sum() >= len(oor) - 8
    k9 = _bytes(ops.hashed_dense(_to_device(host), dim, seed=4, fp8=True, scale=scale))
    want = _e4m3(x)
    for fast in (1, 0):
        g = data.GPUParser(p, format="libsvm", fast_path=fast)
        f8 = _bytes(g.parse_all_hashed(dim, seed=4, fp8=True, scale=scale, strategy="fused")["x"])
        if fast == 1 and dim % 16 == 0:
            assert g.stats()["exact_chunks"] == 0
        np.testing.assert_array_equal(f8, k9)  # out-of-range rows included
        bad = (f8 != want) & inr[:, None]
        assert not bad.any(), (x[bad][:8], f8[bad][:8], want[bad][:8])


# ------------------------------------------------------------------ K11
GROUP_LENS = [0, 0, 1, 15, 16, 17, 31, 32, 33, 1000, 0, 2, 0, 0]


def _spmv_case(index64, value, rng, lens=GROUP_LENS, nfeat=5000):
    lens = np.asarray(lens, np.int64)
    nnz = int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, nfeat, size=nnz)
    val = rng.standard_normal(nnz).astype(np.float32) if value else None
    t = {"offset": torch.from_numpy(off).cuda(),
         "index": torch.from_numpy(idx.astype(np.int64 if index64 else np.int32)).cuda()}
    if value:
        t["value"] = torch.from_numpy(val).cuda()
    return off, idx, val, t


def _close(got, ref, tol):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    bad = ~(np.abs(got - ref) <= tol)
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5], tol[bad][:5])


@pytest.mark.parametrize("index64", [False, True])
@pytest.mark.parametrize("value", [True, False])
def test_k11_row_lengths_around_the_group(index64, value):
    """rows of 0, 1, 15, 16, 17, 31, 32, 33 and 1 000 entries (16 lanes per
    row) with leading and trailing empty rows, 32- and 64-bit indices, with
    and without values, forward and transposed, against fp64"""
    rng = np.random.default_rng(16)
    nfeat = 5000
    off, idx, val, t = _spmv_case(index64, value, rng, nfeat=nfeat)
    w = rng.standard_normal(nfeat).astype(np.float32)
    for bias in (0.0, -1.25):
        y, tol = pyref.csr_dot_ref(off, idx, val, w, bias)
        _close(ops.spmv(t, torch.from_numpy(w).cuda(), bias), y, tol)
    d = rng.standard_normal(len(off) - 1).astype(np.float32)
    g, gtol = pyref.csr_dot_t_ref(off, idx, val, d, nfeat)
    _close(ops.spmv_t(t, torch.from_numpy(d).cuda(), nfeat), g, gtol)


def test_k11_row_slice_and_no_rows():
    """a batch that is rows [b, e) of a larger CSR (offset[0] != 0, the whole
    index / value arrays), and a CSR of no rows"""
    rng = np.random.default_rng(3)
    nfeat = 300
    off, idx, val, t = _spmv_case(False, True, rng, lens=GROUP_LENS * 3, nfeat=nfeat)
    w = rng.standard_normal(nfeat).astype(np.float32)
    b, e = 9, 30
    assert off[b] != 0
    part = {"offset": t["offset"][b:e + 1], "index": t["index"], "value": t["value"]}
    y, tol = pyref.csr_dot_ref(off[b:e + 1], idx, val, w, 0.5)
    _close(ops.spmv(part, torch.from_numpy(w).cuda(), 0.5), y, tol)
    d = rng.standard_normal(e - b).astype(np.float32)
    g, gtol = pyref.csr_dot_t_ref(off[b:e + 1], idx, val, d, nfeat)
    _close(ops.spmv_t(part, torch.from_numpy(d).cuda(), nfeat), g, gtol)
    none = {"offset": t["offset"][:1], "index": t["index"], "value": t["value"]}
    assert ops.spmv(none, torch.from_numpy(w).cuda(), 1.0).numel() == 0
    g0 = ops.spmv_t(none, torch.zeros(0, device="cuda"), nfeat)
    assert g0.shape == (nfeat,) and not g0.any()


@pytest.fixture(scope="module")
def many_rows():
    """300 000 rows of 0..2 entries: the K11 kernels run at most 16 384
    workgroups of 16 rows, so every 16-lane group takes a second row"""
    rng = np.random.default_rng(300000)
    nfeat = 1000
    lens = rng.integers(0, 3, size=300000)
    off, idx, val, t = _spmv_case(False, True, rng, lens=lens, nfeat=nfeat)
    idx[::7] = 5  # many rows hit one feature
    t["index"] = torch.from_numpy(idx.astype(np.int32)).cuda()
    return nfeat, off, idx, val, t, rng


def test_k11_grid_stride_rows(many_rows):
    nfeat, off, idx, val, t, rng = many_rows
    w = rng.standard_normal(nfeat).astype(np.float32)
    y, tol = pyref.csr_dot_ref(off, idx, val, w, 0.25)
    _close(ops.spmv(t, torch.from_numpy(w).cuda(), 0.25), y, tol)
    d = rng.standard_normal(len(off) - 1).astype(np.float32)
    d[rng.random(len(d)) < 0.3] = 0.0  # rows the transposed kernel skips
    d[5::11] = -0.0
    g, gtol = pyref.csr_dot_t_ref(off, idx, val, d, nfeat)
    assert np.bincount(idx, minlength=nfeat)[5] > 40000
    _close(ops.spmv_t(t, torch.from_numpy(d).cuda(), nfeat), g, gtol)
    # all-zero d: nothing is added anywhere
    assert not ops.spmv_t(t, torch.zeros(len(d), device="cuda"), nfeat).any()


def test_k11_pairs_over_a_transpose(many_rows):
    """k_spmv_pairs (interleaved index / value pairs of ops.transpose) over
    the transpose of the same data, with empty columns: more than 262 144
    columns, so its grid-stride loop runs too"""
    _, off, idx, val, t, rng = many_rows
    nfeat = 270000  # ids < 1000: the other columns are empty
    tt = ops.transpose(t, nfeat)
    assert ops._paired(tt)
    d = rng.standard_normal(len(off) - 1).astype(np.float32)
    g, gtol = pyref.csr_dot_t_ref(off, idx, val, d, nfeat)
    got = ops.spmv(tt, torch.from_numpy(d).cuda(), 0.0)
    _close(got, g, gtol)
    assert not got[1000:].any()
    # and a transpose with few columns, every one of them long
    small = ops.transpose(t, 1000)
    _close(ops.spmv(small, torch.from_numpy(d).cuda(), 0.0), g[:1000], gtol[:1000])


def test_pairs_and_unpaired_agree():
    """a transpose read as interleaved pairs (k_spmv_pairs, M1p) and as its
    contiguous copies (k_spmv, M1): K11 sums in no fixed order, so the two
    agree within its any-order bound; M1 and M1p promise one summation order,
    so the SpMM bytes are equal"""
    rng = np.random.default_rng(133)
    nrows, nfeat = 133, 257
    lens = np.resize([0, 1, 15, 16, 17, 70], nrows)
    off, idx, val, t = _spmv_case(False, True, rng, lens=lens, nfeat=nfeat)
    tt = ops.transpose(t, nfeat)
    flat = ops._unpair(tt)
    assert ops._paired(tt) and not ops._paired(flat)
    assert flat["index"].is_contiguous() and flat["value"].is_contiguous()
    d = rng.standard_normal(nrows).astype(np.float32)
    g, gtol = pyref.csr_dot_t_ref(off, idx, val, d, nfeat)
    dd = torch.from_numpy(d).cuda()
    paired, unpaired = ops.spmv(tt, dd), ops.spmv(flat, dd)
    _close(paired, g, gtol)
    _close(unpaired, g, gtol)
    _close(paired, unpaired.cpu().numpy().astype(np.float64), gtol)
    for k in (1, 4, 7):
        D = torch.from_numpy(rng.standard_normal((nrows, k)).astype(np.float32)).cuda()
        a, b = ops.spmm(tt, D), ops.spmm(flat, D)
        assert a.shape == (nfeat, k)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


# ------------------------------------------------------------------ parser
def test_exact_path_scans_more_than_one_partial(tmp_path):
    """20 000 short lines in one chunk on the exact per-line path: its offsets
    scan (k_scan_*) runs over more than 2 048 lines, more than one partial"""
    rng = np.random.default_rng(20000)
    lines = []
    for r in range(20000):
        n = int(rng.integers(0, 4))
        feats = " ".join(f"{int(rng.integers(0, 1 << 20))}:{rng.random():.4f}" for _ in range(n))
        lines.append(f"{r % 2} {feats}".rstrip())
    p = str(tmp_path / "short.libsvm")
    with open(p, "w") as f:
        f.write("\n".join(lines) + "\n")
    g = data.GPUParser(p, format="libsvm", fast_path=0, chunk_bytes=1 << 20)
    got = g.parse_all().to_host()
    assert g.stats()["chunks"] == 1
    want = _cpu_rows(p, "libsvm")
    np.testing.assert_array_equal(got["label"], want["label"])
    np.testing.assert_array_equal(got["offset"].astype(np.int64), want["offset"].astype(np.int64))
    np.testing.assert_array_equal(got["index"].astype(np.uint64), want["index"])
    np.testing.assert_array_equal(got["value"], want["value"])
