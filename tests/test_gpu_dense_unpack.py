"""The dense code of the packed H2D transfer on the GPU
(src/gpu/text_pack_dense.h, k_unpack_dense in src/gpu/unpack_kernels.hip).

  * the device unpack of a dense chunk gives the text, byte for byte, for every
    size class of the kernel (empty, below / at / above one and two 256-byte
    blocks, more than one group of 16 blocks, more than one range), at every
    destination alignment 0..15, with escaped bytes, raw blocks and entries
    that sit on the edges of vectors and blocks, and leaves the bytes before
    and after the chunk untouched;
  * `pack_code=dense` and the raw transfer give identical arrays for each
    format, row shape and chunk size, with the HBM cache too, and on uniform
    text fewer than 0.47 of the bytes cross the link.

`pack_wait=1` makes what is packed independent of timing.  Run the module
under a `timeout`, like the other transport tests.
"""
import numpy as np
import pytest

from dmlc_core_amd import data

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64


def token_text(n, seed=1):
    """rows of ` iiiiii:0.dddddd` tokens, cut at n bytes"""
    rng = np.random.RandomState(seed)
    rows = []
    size = 0
    while size < n:
        toks = [b"%d:0.%06d" % (i, v) for i, v in zip(rng.randint(100000, 999999, size=30),
                                                       rng.randint(0, 999999, size=30))]
        rows.append(b"1 " + b" ".join(toks) + b"\n")
        size += len(rows[-1])
    return b"".join(rows)[:n]


def check_device(text, packed):
    n = len(text)
    assert packed is not None
    assert data.unpack_text_reference(packed) == text
    for off in range(16):
        buf = data.unpack_text_device(packed, off, PAD, FILL)
        assert len(buf) == off + n + PAD
        assert buf[:off] == bytes([FILL]) * off, off
        assert buf[off:off + n] == text, off
        assert buf[off + n:] == bytes([FILL]) * PAD, off  # the pad is left intact


def dense(text, range_blocks=1024):
    return data.pack_text(text, "libsvm", ",", ratio=-1, code="dense", range_blocks=range_blocks)


# 0, 1, 2: edge groups only; 255 .. 513: around one and two blocks; 5003: two
# groups of 16 blocks, odd; 300001: 1172 blocks, two ranges of 1024
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 511, 512, 513, 5003, 300001])
def test_device_unpack_matches_text(n):
    text = token_text(n, n + 1)
    check_device(text, dense(text))


@pytest.mark.parametrize("n", [257, 513, 5003])
def test_escapes_and_raw_blocks(n):
    t = bytearray(token_text(n, n))
    # a literal as the last byte of a block and of the text, one in a block's
    # middle, a byte >= 0x80
    for pos, c in ((255, 0x0D), (n - 1, ord("q")), (n // 2, 0x80), (3, 0x00)):
        t[pos] = c
    check_device(bytes(t), dense(bytes(t)))
    # a block outside the table is stored raw; so is a long enough last one
    t[256:512] = b"x" * len(t[256:512])
    check_device(bytes(t), dense(bytes(t), range_blocks=3))


@pytest.mark.parametrize("at", [60, 61, 62, 63, 64, 65, 66, 253, 254, 255, 256])
def test_entry_on_vector_and_block_edges(at):
    # tokens everywhere (so that `:0.` is in the table), one `:0.` at `at`
    t = bytearray(token_text(700, 5))
    t[at - 7:at + 10] = b" 123456:0.654321 "[:17]
    assert t[at:at + 3] == b":0."
    check_device(bytes(t), dense(bytes(t)))


def test_three_ranges_of_one_block():
    text = token_text(700, 9)
    packed = dense(text, range_blocks=1)
    check_device(text, packed)
    # ranges in the order the pool's threads finished them
    for threads in (1, 4):
        check_device(text, data.pack_text_pool(text, "libsvm", ",", range_blocks=1,
                                               threads=threads))


# ------------------------------------------------------------- the pipeline
ARRAYS = ("offset", "label", "index", "value")


def parse(path, fmt, passes=1, **cfg):
    if fmt == "csv":
        cfg.setdefault("label_column", 0)
    p = data.GPUParser(path, format=fmt, read_threads=4, **cfg)
    outs = []
    for i in range(passes):
        if i:
            p.before_first()
        outs.append(p.parse_all().to_host())
    return outs, p.stats()


def assert_same(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=k)
        else:
            assert x == y, k


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense")
    out = {}
    for fmt in ("libsvm", "libfm", "csv"):
        for shape in ("uniform", "mixed"):
            p = str(d / f"{shape}.{fmt}")
            data.write_synthetic(p, 0, 1200, format=fmt, seed=4, shape=shape)
            out[fmt, shape] = p
    return out


@pytest.fixture(scope="module")
def raw(shards):
    """the raw transfer of every shard at both chunk sizes, parsed once"""
    out = {}
    for (fmt, shape), path in shards.items():
        for cb in (4096, 65536):
            (r,), s = parse(path, fmt, chunk_bytes=cb, packed_h2d=0)
            assert s["packed_chunks"] == 0 and s["link_bytes"] == s["bytes"]
            out[fmt, shape, cb] = (r, s)
    return out


@pytest.mark.parametrize("chunk_bytes", [4096, 65536])
@pytest.mark.parametrize("shape", ["uniform", "mixed"])
@pytest.mark.parametrize("fmt", ["libsvm", "libfm", "csv"])
def test_dense_equals_raw(shards, raw, fmt, shape, chunk_bytes):
    want, s0 = raw[fmt, shape, chunk_bytes]
    (got,), s = parse(shards[fmt, shape], fmt, chunk_bytes=chunk_bytes, packed_h2d=1, pack_wait=1,
                      pack_code="dense")
    assert_same(want, got)
    for k in ("bytes", "chunks", "rows", "nnz", "exact_chunks"):
        assert s[k] == s0[k], k
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]
    assert s["dense_chunks"] == s["packed_chunks"] > 0
    assert s["exception_blocks"] == 0
    print(fmt, shape, chunk_bytes, s["link_bytes"] / s["bytes"], s["raw_chunks"], s["chunks"],
          s["escape_bytes"], s["raw_blocks"])
    if shape == "uniform":
        assert s["link_bytes"] < 0.47 * s["bytes"]


@pytest.mark.parametrize("fmt", ["libsvm", "csv"])
def test_hbm_cache_two_passes(shards, raw, fmt):
    want, s0 = raw[fmt, "uniform", 65536]
    (p0, p1), s = parse(shards[fmt, "uniform"], fmt, passes=2, chunk_bytes=65536, packed_h2d=1,
                        pack_wait=1, pack_code="dense", hbm_cache=1)
    assert_same(want, p0)
    assert_same(want, p1)
    # the first pass went into the arena dense; the replay crossed no link
    assert s["dense_chunks"] > 0
    assert s["link_bytes"] < 0.47 * s0["link_bytes"]
    assert s["rows"] == 2 * s0["rows"]


def test_pack_code_nibble_and_auto(shards, raw):
    """below 1 MiB chunks `auto` is the nibble code, and `nibble` always is"""
    want, _ = raw["libsvm", "uniform", 65536]
    for cfg in (dict(pack_code="nibble"), dict(pack_code="auto"), dict()):
        (got,), s = parse(shards["libsvm", "uniform"], "libsvm", chunk_bytes=65536, packed_h2d=1,
                          pack_wait=1, **cfg)
        assert_same(want, got)
        assert s["packed_chunks"] > 0 and s["dense_chunks"] == 0
        assert s["link_bytes"] > 0.45 * s["bytes"]
