"""Packed H2D (`packed_h2d`): text chunks cross the PCIe link as 4-bit codes
packed on the host (src/gpu/text_pack.h) and are expanded on the GPU
(src/gpu/unpack_kernels.hip) to the same bytes, so every parse result is
bit-identical to the raw transfer.

  * the device unpack equals the CPU reference unpack for every size class of
    the kernel (empty, below / at / above one 256-byte block, several
    workgroups), at every destination alignment 0..15, with exception blocks,
    and leaves the bytes before and after the chunk untouched;
  * `packed_h2d=1` and `packed_h2d=0` give identical CSR arrays and counts
    for each format, row shape and chunk size, for a file without a trailing
    EOL, a line longer than the chunk, a run of lines outside the alphabet
    (packed and raw chunks in one pass), the HBM cache and shuffled sub-shards.

`pack_wait=1` makes what is packed independent of timing (only the 3/4 size
rule sends a chunk raw), so the counts below are exact; the default hybrid
mode (a chunk the pool has not started goes raw) is checked for equal results.
"""
import numpy as np
import pytest

from dmlc_core_amd import data

pytestmark = pytest.mark.gpu

SYMBOLS = b"0123456789:. \n-e"
FILL = 0xA5
PAD = 64


def clean_text(n, seed=1):
    rng = np.random.RandomState(seed)
    return bytes(np.frombuffer(SYMBOLS, dtype=np.uint8)[rng.randint(0, 16, size=n)])


def with_exceptions(text, every):
    """a byte outside the alphabet in every `every`-th 256-byte block, and in the last"""
    t = bytearray(text)
    nblocks = (len(t) + 255) // 256
    for b in list(range(0, nblocks, every)) + ([nblocks - 1] if nblocks else []):
        pos = min(len(t) - 1, b * 256 + (b * 37) % 256)
        t[pos] = (0x80, 0x0D, 0x00, ord("q"))[b % 4]
    return bytes(t)


# 0, 1, 2: edge groups only; 255 / 256 / 257, 511 / 513: around one and two
# blocks; 5003: odd, two workgroups; 300001: ~74 workgroups, 1172 blocks
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 511, 513, 5003, 300001])
@pytest.mark.parametrize("every", [0, 1, 3])
def test_device_unpack_matches_reference(n, every):
    text = clean_text(n, n + 1)
    if every:
        text = with_exceptions(text, every)
    packed = data.pack_text(text, "libsvm", ",", ratio=-1)
    assert packed is not None
    assert data.unpack_text_reference(packed) == text
    for off in range(16):
        buf = data.unpack_text_device(packed, off, PAD, FILL)
        assert len(buf) == off + n + PAD
        assert buf[:off] == bytes([FILL]) * off, off
        assert buf[off:off + n] == text, off
        assert buf[off + n:] == bytes([FILL]) * PAD, off  # the pad is left intact


# ------------------------------------------------------------- the pipeline
def parse(path, fmt, passes=1, **cfg):
    if fmt == "csv":
        cfg.setdefault("label_column", 0)
    p = data.GPUParser(path, format=fmt, read_threads=4, **cfg)
    outs = []
    for i in range(passes):
        if i:
            p.before_first()
        outs.append(p.parse_all().to_host())
    return outs if passes > 1 else outs[0], p.stats()


def assert_same(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=k)
        else:
            assert x == y, k


def compare(path, fmt, chunk_bytes, **cfg):
    """raw, hybrid and deterministic packed passes agree; returns the last's stats"""
    raw, s0 = parse(path, fmt, chunk_bytes=chunk_bytes, packed_h2d=0, **cfg)
    assert s0["packed_chunks"] == 0 and s0["link_bytes"] == s0["bytes"]
    hyb, s1 = parse(path, fmt, chunk_bytes=chunk_bytes, packed_h2d=1, **cfg)
    det, s2 = parse(path, fmt, chunk_bytes=chunk_bytes, packed_h2d=1, pack_wait=1, **cfg)
    for out, s in ((hyb, s1), (det, s2)):
        assert_same(raw, out)
        for k in ("bytes", "chunks", "rows", "nnz", "exact_chunks"):
            assert s[k] == s0[k], k
        assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]
        assert s["link_bytes"] <= s["bytes"]
    return s2


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed")
    out = {}
    for fmt in ("libsvm", "libfm", "csv"):
        for shape in ("uniform", "mixed"):
            p = str(d / f"{shape}.{fmt}")
            data.write_synthetic(p, 0, 1200, format=fmt, seed=4, shape=shape)
            out[fmt, shape] = p
    return out


@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
@pytest.mark.parametrize("shape", ["uniform", "mixed"])
@pytest.mark.parametrize("fmt", ["libsvm", "libfm", "csv"])
def test_packed_equals_raw(shards, fmt, shape, chunk_bytes):
    s = compare(shards[fmt, shape], fmt, chunk_bytes)
    if shape == "uniform":
        # every chunk but a short last one is inside the alphabet: about half the bytes
        assert s["packed_chunks"] >= s["chunks"] - 1
        assert s["exception_blocks"] == 0
        assert s["link_bytes"] < 0.55 * s["bytes"]
        assert s["unpack_staging_bytes"] > 0


def uniform_lines(path):
    with open(path, "rb") as f:
        return f.read().splitlines(keepends=True)


def test_no_trailing_eol(shards, tmp_path):
    lines = uniform_lines(shards["libsvm", "uniform"])[:300]
    p = str(tmp_path / "noeol.libsvm")
    with open(p, "wb") as f:
        f.write(b"".join(lines).rstrip(b"\n"))
    s = compare(p, "libsvm", 4096)
    assert s["packed_chunks"] > 0 and s["rows"] == 300


def test_line_longer_than_chunk(shards, tmp_path):
    lines = uniform_lines(shards["libsvm", "uniform"])
    long_line = b"1 " + b" ".join(b"%d:0.5" % i for i in range(1, 1500)) + b"\n"
    assert len(long_line) > 2 * 4096
    p = str(tmp_path / "long.libsvm")
    with open(p, "wb") as f:
        f.write(b"".join(lines[:40]) + long_line + b"".join(lines[40:80]))
    s = compare(p, "libsvm", 4096)
    assert s["packed_chunks"] > 0 and s["rows"] == 81


def test_run_of_exotic_lines_goes_raw(shards, tmp_path):
    lines = uniform_lines(shards["libsvm", "uniform"])
    # `qid:` tokens are outside the alphabet: every block of the run is an exception
    exotic = [ln.replace(b" ", b" qid:7 ", 1) for ln in lines[200:400]]
    p = str(tmp_path / "exotic.libsvm")
    with open(p, "wb") as f:
        f.write(b"".join(lines[:200] + exotic + lines[400:600]))
    s = compare(p, "libsvm", 4096)
    assert s["packed_chunks"] > 0 and s["raw_chunks"] > 0
    assert s["rows"] == 600


def test_hbm_cache_first_pass_packed_replay_identical(shards):
    path = shards["libsvm", "uniform"]
    (r0, r1), s0 = parse(path, "libsvm", passes=2, chunk_bytes=65536, packed_h2d=0, hbm_cache=1)
    (p0, p1), s1 = parse(path, "libsvm", passes=2, chunk_bytes=65536, packed_h2d=1, pack_wait=1,
                         hbm_cache=1)
    for out in (r1, p0, p1):
        assert_same(r0, out)
    # the first pass went into the arena packed; the replay crossed no link
    assert s1["packed_chunks"] > 0
    assert s1["packed_chunks"] + s1["raw_chunks"] == s0["raw_chunks"]
    assert s1["link_bytes"] < 0.55 * s0["link_bytes"]
    assert s1["rows"] == s0["rows"] == 2 * 1200


def test_hbm_cache_partial_pass_then_rewind(shards):
    """The last chunks of a caching pass are submitted (the cache counts as
    complete) long before they are parsed: a rewind after one block must still
    find their text, not their codes, in the arena."""
    path = shards["libsvm", "uniform"]
    want, s0 = parse(path, "libsvm", chunk_bytes=65536, packed_h2d=0)
    assert s0["chunks"] >= 4
    for wait in (1, 0):
        g = data.GPUParser(path, chunk_bytes=65536, packed_h2d=1, pack_wait=wait, hbm_cache=1,
                           device_slots=max(3, s0["chunks"]), read_threads=4)
        assert g.next()  # one block; every other chunk is in flight, unparsed
        g.before_first()
        assert_same(want, g.parse_all().to_host())
        g.before_first()
        assert_same(want, g.parse_all().to_host())
        if wait:
            assert g.stats()["packed_chunks"] >= s0["chunks"] - 1
    # the same with the default three device slots (the pass's tail in flight)
    g = data.GPUParser(path, chunk_bytes=65536, packed_h2d=1, pack_wait=1, hbm_cache=1,
                       read_threads=4)
    for _ in range(s0["chunks"] - 2):
        assert g.next()
    g.before_first()
    assert_same(want, g.parse_all().to_host())


@pytest.mark.parametrize("pack_wait", [0, 1])
@pytest.mark.parametrize("hbm_cache", [0, 1])
def test_windowed_source(tmp_path, pack_wait, hbm_cache):
    """A partition above the pin budget: windows are released while pieces are
    queued ahead of the submit cursor and while the pool reads them."""
    d = tmp_path / "w"
    d.mkdir()
    for i in range(3):
        data.write_synthetic(str(d / f"p{i}.libsvm"), i * 2500, (i + 1) * 2500, seed=19)
    cfg = dict(chunk_bytes=64 * 1024, zero_copy=1, zc_pin_budget_mb=1, zc_window_mb=0.25,
               hbm_cache=hbm_cache)
    (w0, w1), s0 = parse(str(d), "libsvm", passes=2, packed_h2d=0, **cfg)
    (p0, p1), s1 = parse(str(d), "libsvm", passes=2, packed_h2d=1, pack_wait=pack_wait, **cfg)
    for out in (w1, p0, p1):
        assert_same(w0, out)
    for k in ("bytes", "chunks", "rows", "nnz"):
        assert s1[k] == s0[k], k
    assert s1["packed_chunks"] + s1["raw_chunks"] == s0["raw_chunks"]
    if pack_wait:
        assert s1["packed_chunks"] > 0
    # streaming blocks, rewound mid-way through a window
    g = data.GPUParser(str(d), format="libsvm", read_threads=4, packed_h2d=1, pack_wait=pack_wait,
                       **cfg)
    for _ in range(5):
        assert g.next()
    g.before_first()
    assert_same(w0, g.parse_all().to_host())


def test_pool_thread_error_surfaces_in_the_consumer(shards):
    from dmlc_core_amd import _dmlc

    path = shards["libsvm", "uniform"]
    want, _ = parse(path, "libsvm", chunk_bytes=65536, packed_h2d=0)
    _dmlc.fault_configure("pack:2")
    try:
        g = data.GPUParser(path, chunk_bytes=65536, packed_h2d=1, pack_wait=1, read_threads=4)
        with pytest.raises(_dmlc.DMLCError, match='injected fault at "pack"'):
            g.parse_all()
        _dmlc.fault_configure("")
        # the same parser recovers: rewound, it delivers the whole shard
        g.before_first()
        assert_same(want, g.parse_all().to_host())
    finally:
        _dmlc.fault_configure("")


def test_shuffle_parts(shards):
    path = shards["libfm", "uniform"]
    s = compare(path, "libfm", 65536, shuffle_parts=2)
    assert s["packed_chunks"] > 0
