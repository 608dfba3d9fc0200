"""K3, the device-wide exclusive scan of u64 (LaunchScanU64,
src/gpu/scan_kernels.hip), on its own and through its consumers, across the
sizes at which it takes another path.

Every comparison is exact: the reference is numpy's cumsum over uint64 (which
wraps mod 2^64), shifted to an exclusive scan.  No tolerance appears in this
file.

The scan is reached through ``_dmlc.csr_gather_count``: G1 writes the length
of every selected row of a hand-made source row pointer -- the words to scan,
chosen one by one through the selection -- and K3 scans them in place.  The
passes and what switches them, with T = 2048 words per tile:
  reduce / down-sweep   one workgroup per tile; a ragged last tile takes the
                        word-by-word branch (n % 8 != 0 within the last lane)
  partials              one workgroup walks the ceil(n / T) tile sums in tiles
                        of T and carries the running total from tile to tile:
                        a second pass of that loop needs n > T^2 words, a
                        third n > 2 T^2; up to 7 partials (n <= 7 T) never
                        fill a lane's 8 words
  alignment             the data is read by 16-byte loads; the partials and
                        the total by single words, so they may sit at any
                        8-byte address (kernels.h) -- ops.qid_groups puts them
                        behind `rows` flags, misaligned for every odd `rows`

The consumers run across the same edges: ops.qid_groups, ops.gather_rows, the
exact text path (packed (rows << 32) | entries words) and the bucket table of
ops.transpose, whose words = buckets * blocks + 1 with 30 720 entries a block
and 1024 columns a bucket below 2^20 features."""
import numpy as np
import pytest
import torch

from dmlc_core_amd import _dmlc, ops
from test_gpu_gather_rows import bits, make_csr
from test_gpu_ops import _ref_transpose
from test_gpu_parser import assert_same, cpu_rows, gpu_rows

pytestmark = pytest.mark.gpu

T = 2048  # words per tile of the scan (pinned by test_tile_size)
SIZES = [1, 7, 8, 9, T - 1, T, T + 1, 8 * T - 1, 8 * T, 8 * T + 1,
         T * T - 1, T * T, T * T + 1, 2 * T * T + T + 3]
ONE_AT = [0, T - 1, T, T * T - 1, T * T]  # and n - 1
LENGTHS = [0, 1, 2047, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, (5 << 32) | 3, 2 ** 40]
PACKED = [(a << 32) | b for a in (0, 1) for b in (0, 1, 2, 3, 40)]  # (row valid, entries) of a line
GUARD, SENTINEL = 16, -0x0123456789ABCDEF


def test_tile_size():
    assert _dmlc.qid_scan_words(T) == 2
    assert _dmlc.qid_scan_words(T + 1) == 3


def excl_cumsum(words):
    """the reference: (exclusive scan, total) of uint64 words, mod 2^64"""
    words = np.asarray(words, dtype=np.uint64)
    incl = np.cumsum(words, dtype=np.uint64)
    excl = np.zeros_like(incl)
    excl[1:] = incl[:-1]
    return excl, int(incl[-1])


def device_scan(table, picks, partials_shift=0):
    """table[picks] scanned by G1 + K3: (scanned uint64 [n], total, error
    word).  The source has one row per table entry, of that length; its
    selection `picks` (int32) is the sequence of scanned words.  The scanned
    array and the scratch are followed by sentinel words, which must survive;
    partials_shift (bytes) moves the scratch off its 16-byte boundary."""
    table = np.asarray(table, dtype=np.uint64)
    src = np.zeros(len(table) + 1, dtype=np.uint64)
    src[1:] = np.cumsum(table, dtype=np.uint64)
    assert int(src[-1]) == sum(int(v) for v in table) < 2 ** 63  # no wrap in the row pointer
    n = len(picks)
    offset = torch.from_numpy(src.view(np.int64)).cuda()
    rows = torch.from_numpy(np.ascontiguousarray(picks, dtype=np.int32)).cuda()
    out = torch.full((n + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    words = int(_dmlc.csr_gather_scratch_words(n))
    assert partials_shift % 8 == 0 and partials_shift < 16
    lead = partials_shift // 8
    scratch = torch.full((lead + words + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    status = torch.zeros(2, dtype=torch.int64, device="cuda")  # [total, error word]
    assert out.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0
    _dmlc.csr_gather_count(offset.data_ptr(), len(table), int(src[-1]), rows.data_ptr(), False, n,
                           0, 0, 0, out.data_ptr(), 0, 0, 0, scratch.data_ptr() + partials_shift,
                           status.data_ptr(), status.data_ptr() + 8,
                           torch.cuda.current_stream().cuda_stream)
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all(), "words past the scanned array were written"
    sc = scratch.cpu().numpy()
    assert (sc[:lead] == SENTINEL).all() and (sc[lead + words:] == SENTINEL).all(), \
        "words outside the scan scratch were written"
    total, err = status.tolist()
    return got[:n].view(np.uint64), total & (2 ** 64 - 1), err


def assert_scan(table, picks, partials_shift=0):
    """the device scan of table[picks] equals numpy's; returns the total"""
    want, want_total = excl_cumsum(np.asarray(table, dtype=np.uint64)[picks])
    got, total, err = device_scan(table, picks, partials_shift)
    assert err == 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {len(picks)} words differ, the first at {bad[0]} "
                           f"(tile {bad[0] // T}, partial tile {bad[0] // (T * T)}): "
                           f"got {got[bad[0]]}, want {want[bad[0]]}")
    assert total == want_total
    return total


@pytest.mark.parametrize("n", SIZES)
def test_all_ones(n):
    """the result is arange(n): the position of a lost carry is the first
    word that differs"""
    assert assert_scan([1], np.zeros(n, dtype=np.int32)) == n


@pytest.mark.parametrize("n,pos", [(n, p) for n in SIZES
                                   for p in sorted({q for q in ONE_AT + [n - 1] if q < n})])
def test_single_one(n, pos):
    """a 1 on the first or last word of a tile, of a tile of partials, of the
    array: everything after it is 1, nothing before it"""
    picks = np.zeros(n, dtype=np.int32)
    picks[pos] = 1
    assert assert_scan([0, 1], picks) == 1


@pytest.mark.parametrize("n", SIZES)
def test_lengths_past_32_bits(n):
    """words on both sides of 2^31 and 2^32 and with both halves set: a wave
    or block scan that drops the high half, or carries wrongly into it, shows"""
    picks = np.random.default_rng(n).integers(0, len(LENGTHS), n).astype(np.int32)
    assert n * max(LENGTHS) < 2 ** 64
    assert_scan(LENGTHS, picks)


@pytest.mark.parametrize("n", SIZES)
def test_packed_pairs(n):
    """the exact text path's words, (row valid << 32) | entries: each half of
    the total is that half's own sum"""
    picks = np.random.default_rng(n + 1).integers(0, len(PACKED), n).astype(np.int32)
    words = np.asarray(PACKED, dtype=np.int64)[picks]
    total = assert_scan(PACKED, picks)
    assert total >> 32 == int((words >> 32).sum())
    assert total & 0xFFFFFFFF == int((words & 0xFFFFFFFF).sum()) < 2 ** 32


@pytest.mark.parametrize("n", [7 * T, 7 * T + 1, 8 * T - 1, 8 * T, 8 * T + 1, T * T + 1])
def test_partials_at_an_odd_word(n):
    """the scratch 8 bytes off its 16-byte boundary, on both sides of the size
    (7 T + 1) from which a lane of the partials pass has all its 8 words: the
    same scan"""
    picks = np.random.default_rng(n + 2).integers(0, len(LENGTHS), n).astype(np.int32)
    assert_scan(LENGTHS, picks, partials_shift=8)


# ---------------------------------------------------------------- consumers

def _qid(layout, rows):
    rng = np.random.default_rng(rows)
    if layout == "distinct":  # every row starts a group: the scan of all ones
        return rng.permutation(rows).astype(np.uint64)
    m = rows // 2 + 8  # runs of 1-4 rows, 2.5 on average
    q = np.repeat(rng.integers(0, 2 ** 62, m).astype(np.uint64), rng.integers(1, 5, m))[:rows]
    assert q.size == rows
    return q


@pytest.mark.parametrize("layout", ["runs", "distinct"])
@pytest.mark.parametrize("rows", [7 * T, 7 * T + 1, 7 * T + 3, T * T, T * T + 1])
def test_qid_groups(rows, layout):
    """odd and even row counts on both sides of 8 partials and of the carry
    loop; the partials follow the flags, at an odd word for odd `rows`"""
    q = _qid(layout, rows)
    want = np.concatenate([np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1]])), [q.size]])
    ptr = ops.qid_groups(torch.from_numpy(q.view(np.int64)).cuda())
    assert ptr.dtype == torch.int64 and ptr.is_cuda
    assert np.array_equal(ptr.cpu().numpy(), want)
    if layout == "distinct":
        assert len(want) == rows + 1


@pytest.fixture(scope="module")
def gather_case():
    """a 1000-row source with rows of 0-3 entries, value and label; T^2 + 5
    random row ids; numpy's gather of them"""
    rng = np.random.default_rng(17)
    host, dev = make_csr(rng.integers(0, 4, 1000), seed=18, columns=("label",))
    rows = rng.integers(0, 1000, T * T + 5)
    off = host["offset"]
    lens = off[rows + 1] - off[rows]
    want_off = np.zeros(len(rows) + 1, dtype=np.int64)
    want_off[1:] = np.cumsum(lens)
    # output entry p of selected row i is source entry off[rows[i]] + p - want_off[i]
    src = np.repeat(off[rows] - want_off[:-1], lens) + np.arange(want_off[-1])
    want = {"offset": want_off, "index": host["index"][src], "value": host["value"][src],
            "label": host["label"][rows]}
    return dev, torch.from_numpy(rows).cuda(), want


@pytest.mark.parametrize("how", ["fresh", "out"])
def test_gather_rows(gather_case, how):
    """a selection of more than T^2 rows with duplicates: the row pointer
    passes through the carry loop, G2 searches it"""
    dev, rows, want = gather_case
    out = None
    if how == "out":
        out = ops.gather_buffers(dev, rows.numel(), int(want["offset"][-1]))
    res = ops.gather_rows(dev, rows, out=out)
    assert res["offset"].dtype == torch.int64
    assert np.array_equal(res["offset"].cpu().numpy(), want["offset"])
    for k in ("index", "value", "label"):
        assert res[k].numel() == len(want[k])
        assert np.array_equal(bits(res[k]), bits(want[k])), k
    if how == "out":
        assert res["index"].data_ptr() == out["_buffers"]["index"].data_ptr()


def test_exact_text_path_past_2048_partials(tmp_path):
    """one chunk of T^2 + 1000 lines through the exact kernels: the packed
    (rows, entries) words of every line are carried through more than 2048
    partials, and the line index through its own scan"""
    rng = np.random.default_rng(23)
    n = T * T + 1000
    kinds = np.array([b"1\n", b"0\n", b"1 3:1\n", b"0 2:0.5 7:2\n"], dtype=object)
    p = str(tmp_path / "short.libsvm")
    with open(p, "wb") as f:
        f.write(b"".join(kinds[rng.choice(4, n, p=[0.45, 0.45, 0.06, 0.04])].tolist()))
    g = gpu_rows(p, "libsvm", fast_path=0, chunk_bytes=32 << 20)
    assert len(g["label"]) == n
    assert_same(g, cpu_rows(p, "libsvm"))


@pytest.mark.parametrize("nfeat,nnz,words", [(89 * 1024, 23 * 30720 - 17, T),
                                             (1 << 20, 30720 + 4099, T + 1)],
                         ids=["table-T", "table-T+1"])
def test_transpose_bucket_table(nfeat, nnz, words):
    """the bucket table of exactly one tile, and of one tile and one word"""
    buckets, blocks = -(-nfeat // 1024), -(-nnz // 30720)
    assert buckets * blocks + 1 == words
    rng = np.random.default_rng(words)
    lens = rng.multinomial(nnz, np.full(3000, 1 / 3000))
    off = np.zeros(3001, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    t = {"offset": torch.from_numpy(off).cuda(),
         "index": torch.from_numpy(rng.integers(0, nfeat, nnz).astype(np.int32)).cuda(),
         "value": torch.from_numpy(rng.standard_normal(nnz).astype(np.float32)).cuda()}
    tt = ops.transpose(t, nfeat)
    ptr, r, v = _ref_transpose(t, nfeat)
    np.testing.assert_array_equal(tt["offset"].cpu().numpy(), ptr)
    np.testing.assert_array_equal(tt["index"].cpu().numpy(), r)
    np.testing.assert_array_equal(tt["value"].cpu().numpy(), v)
