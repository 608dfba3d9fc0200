"""Two copy streams and head jobs of the chunk transport (src/gpu/chunk_feed.cc).

Consecutive chunks of a pass alternate over two H2D copy streams, so nothing is
ordered by a copy stream's own order any more: a slot's copy, unpack and parse
hang on the slot's events, and the memsets of slot and arena memory on an event
both streams wait for.  And once a pass's last piece is handed in, the first
pieces of the next pass are queued to the pack pool ("head jobs"); a rewind to
0 adopts them, anything else drops them.

Whatever the timing, every pass delivers exactly what a raw transfer over one
copy stream delivers (`packed_h2d=0, copy_streams=1`), every chunk crosses the
link either packed or raw, and nothing stalls.  Run the module under a
`timeout`: a submit loop that never comes back would show as a hang.
"""
import gc

import numpy as np
import pytest

from dmlc_core_amd import data

pytestmark = pytest.mark.gpu

ARRAYS = ("offset", "label", "index", "value")


def passes(g, n):
    outs = []
    for i in range(n):
        if i:
            g.before_first()
        outs.append(g.parse_all().to_host())
    return outs


def assert_same(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=k)
        else:
            assert x == y, k


def raw_parse(path, **cfg):
    """one pass of the raw transfer over a single copy stream, and its counters"""
    g = data.GPUParser(path, packed_h2d=0, copy_streams=1, read_threads=4, **cfg)
    out = g.parse_all().to_host()
    s = g.stats()
    assert s["packed_chunks"] == 0 and s["head_packed"] == 0
    return out, s


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """5,000 rows: hundreds of 4 KiB chunks, tens of 64 KiB ones"""
    path = str(tmp_path_factory.mktemp("copy_streams") / "small.libsvm")
    data.write_synthetic(path, 0, 5000, format="libsvm", seed=23)
    return path


@pytest.fixture(scope="module")
def small_raw(small):
    return {cb: raw_parse(small, chunk_bytes=cb) for cb in (4096, 65536)}


@pytest.fixture(scope="module")
def large(tmp_path_factory):
    """40,000 rows: some hundreds of 64 KiB chunks per pass"""
    path = str(tmp_path_factory.mktemp("copy_streams") / "large.libsvm")
    data.write_synthetic(path, 0, 40000, format="libsvm", seed=29)
    return path


@pytest.fixture(scope="module")
def large_raw(large):
    return raw_parse(large, chunk_bytes=65536)


# ------------------------------------------------------------ two copy streams
@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
@pytest.mark.parametrize("packed_h2d", [0, 1])
@pytest.mark.parametrize("device_slots", [1, 2, 3])
def test_three_passes_equal_raw(small, small_raw, device_slots, packed_h2d, chunk_bytes):
    """With one device slot the two streams alternate on the same buffers: a
    copy not ordered behind the slot's parse would overwrite text being read."""
    want, s0 = small_raw[chunk_bytes]
    assert s0["chunks"] >= (300 if chunk_bytes == 4096 else 20)
    g = data.GPUParser(small, packed_h2d=packed_h2d, device_slots=device_slots,
                       chunk_bytes=chunk_bytes, read_threads=4)
    for out in passes(g, 3):
        assert_same(want, out)
    s = g.stats()
    for k in ("bytes", "chunks", "rows", "nnz"):
        assert s[k] == 3 * s0[k], k
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]
    if not packed_h2d:
        assert s["packed_chunks"] == 0 and s["head_packed"] == 0


@pytest.mark.parametrize("packed_h2d", [0, 1])
@pytest.mark.parametrize("device_slots", [1, 2])
def test_line_longer_than_chunk(small, tmp_path, device_slots, packed_h2d):
    """The device slot is regrown mid-pass: the memset of the new buffer is
    ordered before the copy into it, whichever stream that copy is on."""
    with open(small, "rb") as f:
        lines = f.read().splitlines(keepends=True)
    long_line = b"1 " + b" ".join(b"%d:0.5" % i for i in range(1, 1500)) + b"\n"
    assert len(long_line) > 2 * 4096
    path = str(tmp_path / "long.libsvm")
    with open(path, "wb") as f:
        # two long lines: two slots are regrown (one, twice, with a single slot)
        f.write(b"".join(lines[:40]) + long_line + b"".join(lines[40:85]) + long_line +
                b"".join(lines[85:120]))
    want, s0 = raw_parse(path, chunk_bytes=4096)
    assert s0["rows"] == 122
    g = data.GPUParser(path, packed_h2d=packed_h2d, device_slots=device_slots, chunk_bytes=4096,
                       read_threads=4)
    for out in passes(g, 2):
        assert_same(want, out)
        for k in ARRAYS:
            np.testing.assert_array_equal(out[k], want[k], err_msg=k)


@pytest.mark.parametrize("packed_h2d", [0, 1])
def test_caching_first_pass_then_replay(small, small_raw, packed_h2d):
    """The arena's memset is ordered before the copies into it (with hbm_cache
    the feed keeps one copy stream); no head is queued for a pass that replays
    the cache."""
    want, s0 = small_raw[65536]
    g = data.GPUParser(small, packed_h2d=packed_h2d, hbm_cache=1, chunk_bytes=65536,
                       read_threads=4)
    for out in passes(g, 4):
        assert_same(want, out)
    s = g.stats()
    assert s["rows"] == 4 * s0["rows"]
    # only the first pass crossed the link
    assert s["packed_chunks"] + s["raw_chunks"] == s0["chunks"]
    assert s["head_packed"] == 0


@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
def test_pinned_ring_source(small, small_raw, chunk_bytes):
    want, s0 = small_raw[chunk_bytes]
    g = data.GPUParser(small, zero_copy=0, chunk_bytes=chunk_bytes, read_threads=4)
    for out in passes(g, 2):
        assert_same(want, out)
    assert g.stats()["chunks"] == 2 * s0["chunks"]


def test_one_copy_stream_still_works(small, small_raw):
    want, _ = small_raw[4096]
    g = data.GPUParser(small, packed_h2d=1, copy_streams=1, chunk_bytes=4096, read_threads=4)
    for out in passes(g, 2):
        assert_same(want, out)


# ------------------------------------------------------------------ head jobs
HEAD_CFG = dict(packed_h2d=1, read_threads=4, chunk_bytes=65536)


def test_head_adopted(large, large_raw):
    want, s0 = large_raw
    npass = 4
    g = data.GPUParser(large, **HEAD_CFG)
    for out in passes(g, npass):
        assert_same(want, out)
    s = g.stats()
    assert s["chunks"] == npass * s0["chunks"]
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]
    # the first rewind only arms the speculation; how many of the later passes
    # find their first piece packed is timing
    assert 1 <= s["head_packed"] <= npass - 2
    # every pass still moved its bytes over the link
    assert s["link_bytes"] > 0.45 * s["bytes"]


def test_pack_head_off(large, large_raw):
    want, _ = large_raw
    g = data.GPUParser(large, pack_head=0, **HEAD_CFG)
    for out in passes(g, 3):
        assert_same(want, out)
    assert g.stats()["head_packed"] == 0


def test_head_dropped_by_rewind_after_two_blocks(large, large_raw):
    want, _ = large_raw
    g = data.GPUParser(large, **HEAD_CFG)
    passes(g, 2)
    g.before_first()  # adopts the head queued at the end of the second pass
    for _ in range(2):
        assert g.next()
    g.before_first()
    assert_same(want, g.parse_all().to_host())
    g.before_first()
    assert_same(want, g.parse_all().to_host())


def test_head_dropped_by_seek_to_a_cursor(large, large_raw):
    want, _ = large_raw
    g = data.GPUParser(large, **HEAD_CFG)
    passes(g, 2)
    g.before_first()
    rows = 0
    for _ in range(3):
        assert g.next()
        rows += len(g.value_to_host()["label"])
    cursor = g.tell()
    assert 0 < cursor < g.partition_bytes
    g.parse_all()  # the rest of the pass: head jobs are open again
    g.seek(cursor)
    tail = g.parse_all().to_host()
    nz = int(want["offset"][rows])
    np.testing.assert_array_equal(tail["label"], want["label"][rows:])
    np.testing.assert_array_equal(tail["offset"], want["offset"][rows:] - want["offset"][rows])
    np.testing.assert_array_equal(tail["index"], want["index"][nz:])
    np.testing.assert_array_equal(tail["value"], want["value"][nz:])
    # and a plain rewind after that
    g.before_first()
    assert_same(want, g.parse_all().to_host())


def test_destroyed_with_head_jobs_open(large, large_raw):
    want, _ = large_raw
    g = data.GPUParser(large, **HEAD_CFG)
    passes(g, 2)
    del g
    gc.collect()
    # the device and the page cache are as they were
    g = data.GPUParser(large, **HEAD_CFG)
    assert_same(want, g.parse_all().to_host())


def test_shuffled_passes_do_not_speculate(large):
    cfg = dict(shuffle_parts=2, chunk_bytes=65536, read_threads=4)
    r = data.GPUParser(large, packed_h2d=0, copy_streams=1, **cfg)
    g = data.GPUParser(large, packed_h2d=1, **cfg)
    for want, out in zip(passes(r, 3), passes(g, 3)):
        assert_same(want, out)
    s = g.stats()
    assert s["head_packed"] == 0
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"] == r.stats()["chunks"]


def test_windowed_source_does_not_speculate(tmp_path):
    d = tmp_path / "w"
    d.mkdir()
    for i in range(3):
        data.write_synthetic(str(d / f"p{i}.libsvm"), i * 2500, (i + 1) * 2500, seed=19)
    cfg = dict(chunk_bytes=64 * 1024, zero_copy=1, zc_pin_budget_mb=1, zc_window_mb=0.25)
    want, s0 = raw_parse(str(d), **cfg)
    g = data.GPUParser(str(d), packed_h2d=1, read_threads=4, **cfg)
    for out in passes(g, 3):
        assert_same(want, out)
    s = g.stats()
    assert s["head_packed"] == 0
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"] == 3 * s0["chunks"]


def test_pack_wait_does_not_speculate(large, large_raw):
    want, s0 = large_raw
    g = data.GPUParser(large, pack_wait=1, **HEAD_CFG)
    for out in passes(g, 3):
        assert_same(want, out)
    s = g.stats()
    assert s["head_packed"] == 0
    # the deterministic counters: only the 3/4 rule sends a chunk raw
    assert s["packed_chunks"] >= 3 * (s0["chunks"] - 1)
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]


def test_pool_fault_on_a_head_job(large, large_raw):
    """The project's fault-injection hook on host code (dmlc/fault.h): the pool
    thread that opens the K-th job after `fault_configure` throws."""
    from dmlc_core_amd import _dmlc

    want, _ = large_raw
    g = data.GPUParser(large, **HEAD_CFG)
    assert_same(want, g.parse_all().to_host())
    n = g.stats()["chunks"]  # pieces of one pass
    g.before_first()  # arms the speculation
    # the second pass opens n jobs, or n - 1 when its first piece goes raw; the
    # two head jobs queued at its end follow: job n + 1 is one of them
    _dmlc.fault_configure("pack:%d" % (n + 1))
    try:
        assert_same(want, g.parse_all().to_host())
        g.before_first()
        with pytest.raises(_dmlc.DMLCError, match='injected fault at "pack"'):
            g.parse_all()
        _dmlc.fault_configure("")
        # the same parser recovers: rewound, it delivers the whole shard
        g.before_first()
        assert_same(want, g.parse_all().to_host())
        s = g.stats()
        assert s["packed_chunks"] + s["raw_chunks"] >= s["chunks"]
    finally:
        _dmlc.fault_configure("")
