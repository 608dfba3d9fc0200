"""Link-aware packed H2D (src/gpu/chunk_feed.cc, pack_pool.h DecideSubmit): in
hybrid mode a piece whose pack is not finished goes raw only while no copy is
outstanding, otherwise the submit loop leaves a device slot unfilled and comes
back.  Whatever the timing makes of that, with one, two or three device slots
the parse delivers exactly what the raw transfer delivers, every chunk crosses
the link either packed or raw, and nothing stalls (run the module under a
`timeout`: a submit loop that never comes back would show as a hang).

No count of raw chunks is asserted: at this size (25 chunks of 1 MiB per pass)
it depends on timing.
"""
import numpy as np
import pytest

from dmlc_core_amd import data

pytestmark = pytest.mark.gpu

PASSES = 3
CFG = dict(chunk_bytes=1 << 20, read_threads=4)


def passes(g, n=PASSES):
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


@pytest.fixture(scope="module")
def shard(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("link_aware") / "uniform.libsvm")
    data.write_synthetic(path, 0, 40000, format="libsvm", seed=11)
    return path


@pytest.fixture(scope="module")
def raw(shard):
    """the raw transfer's three passes (all equal) and its counters"""
    g = data.GPUParser(shard, packed_h2d=0, **CFG)
    outs = passes(g)
    s = g.stats()
    assert s["packed_chunks"] == 0 and s["chunks"] >= PASSES * 20
    for out in outs[1:]:
        assert_same(outs[0], out)
    return outs[0], s


@pytest.mark.parametrize("device_slots", [1, 2, 3])
def test_hybrid_equals_raw(shard, raw, device_slots):
    want, s0 = raw
    g = data.GPUParser(shard, packed_h2d=1, device_slots=device_slots, **CFG)
    for out in passes(g):
        assert_same(want, out)
    s = g.stats()
    for k in ("bytes", "chunks", "rows", "nnz"):
        assert s[k] == s0[k], k
    assert s["packed_chunks"] + s["raw_chunks"] == s["chunks"]
    assert s["link_bytes"] <= s["bytes"]
    assert 0 <= s["wait_pack_idle_sec"] <= s["wait_pack_sec"]


@pytest.mark.parametrize("device_slots", [1, 2, 3])
def test_hybrid_hbm_cache_first_pass_then_replay(shard, raw, device_slots):
    want, s0 = raw
    g = data.GPUParser(shard, packed_h2d=1, hbm_cache=1, device_slots=device_slots, **CFG)
    for out in passes(g):
        assert_same(want, out)
    s = g.stats()
    for k in ("bytes", "rows", "nnz"):
        assert s[k] == s0[k], k
    # only the first pass crossed the link, each of its chunks packed or raw
    assert s["packed_chunks"] + s["raw_chunks"] == s0["chunks"] // PASSES
    assert s["link_bytes"] <= s0["bytes"] // PASSES


@pytest.mark.parametrize("device_slots", [1, 2, 3])
def test_hybrid_rewind_after_two_blocks(shard, raw, device_slots):
    want, s0 = raw
    g = data.GPUParser(shard, packed_h2d=1, device_slots=device_slots, **CFG)
    for _ in range(2):
        assert g.next()  # the chunks behind these two are queued, deferred or being packed
    for _ in range(2):
        g.before_first()
        assert_same(want, g.parse_all().to_host())
    s = g.stats()
    # the chunks submitted behind the two blocks were dropped by the rewind
    assert s["packed_chunks"] + s["raw_chunks"] >= s["chunks"]
