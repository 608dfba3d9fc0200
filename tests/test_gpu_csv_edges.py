"""The CSV tile path (src/gpu/csv_kernels.hip: k_csv_tile_count,
k_csv_tile_count_pos, k_csv_tile_fill) on the placed cases of csv_cases.py:
row ends, delimiters, row starts, numbers and the chunk end on every lane,
step, tile, ring and extension edge of the walk, under each of the code shapes
that (label_column, weight_column) choose.

Every file is one chunk.  The result is compared with the C++ CSV parser --
which test_csv_cases_cpu.py holds to the Python oracle on the same files --
float arrays as uint32 bits, offsets and indices exactly: no tolerance.  A
case that must stay on the tile path asserts exact_chunks == 0, one that must
leave it exact_chunks == 1; only the three rows that end right at the
extension limit (group d) may do either, and which they did is printed.
fast_path=0 runs the same bytes through the exact kernels alone."""
import functools

import numpy as np
import pytest

from dmlc_core_amd import data
import csv_cases as cc
import pyref

pytestmark = pytest.mark.gpu

CHUNK = 1 << 20
GROUP_DELIM_CONFIGS = [(g, d, lc, wc) for g in cc.GROUPS for d in cc.delims(g)
                       for lc, wc in cc.configs(g)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """path of a case's file (each written once)"""
    root = tmp_path_factory.mktemp("csv_edges")
    done = {}

    def path(name, text):
        if name not in done:
            done[name] = str(root / name)
            with open(done[name], "wb") as f:
                f.write(text.encode("latin-1"))
        return done[name]
    return path


@functools.lru_cache(maxsize=None)
def cpu_reference(uri, fmt="csv", index64=False):
    return pyref.concat_blocks(list(data.iter_blocks(uri, type=fmt, index64=index64)))


def gpu_parse(path, delim, lc, wc, index64=False, **extra):
    cfg = dict(label_column=lc, weight_column=wc, delimiter=delim, chunk_bytes=CHUNK)
    cfg.update(extra)
    gp = data.GPUParser(path + cc.query(lc, wc, delim), format="csv", index64=index64, **cfg)
    rows = pyref.concat_blocks([gp.parse_all().to_host()])
    return rows, gp.stats()


def case_path(files, case):
    return files(case.name + ("_tab" if case.delim != "," else "") + ".csv", case.text)


def check(files, case, lc, wc, index64=False, **extra):
    """parse on the GPU, compare with the CPU parser; returns exact_chunks"""
    p = case_path(files, case)
    want = cpu_reference(p + cc.query(lc, wc, case.delim), "csv", index64)
    got, st = gpu_parse(p, case.delim, lc, wc, index64, **extra)
    how = f"label_column={lc} weight_column={wc} index64={index64} {extra}"
    msg = cc.first_difference(case, got, want)
    assert not msg, f"{how}: {msg}"
    assert st["chunks"] == 1, (case.name, st["chunks"])
    return st["exact_chunks"]


@pytest.mark.parametrize("group,delim,lc,wc", GROUP_DELIM_CONFIGS)
def test_placed_cases_equal_the_cpu_parser(files, group, delim, lc, wc):
    left = []
    for case in cc.cases(group, delim):
        runs = [dict(zero_copy=z) for z in (0, 1)] if group == "e" else [{}]
        for extra in runs:
            for index64 in ((False, True) if group in cc.INDEX64_GROUPS else (False,)):
                exact = check(files, case, lc, wc, index64, **extra)
                how = f"{case.name} ({lc}, {wc}) index64={index64} {extra}"
                if case.expect == "tile":
                    assert exact == 0, f"{how}: left the tile path"
                elif case.expect == "exact":
                    assert exact == 1, f"{how}: stayed on the tile path"
                else:
                    print(f"{how}: {'exact kernels' if exact else 'tile path'}")
                if exact:
                    left.append(case)
    # a case that ran the exact kernels proves nothing about the tile path:
    # only the "exact" cases and the group-d boundary rows may
    assert all(c.expect == "exact" or (c.expect == "either" and c.group == "d") for c in left)


@pytest.mark.parametrize("group,delim", [(g, d) for g in cc.GROUPS for d in cc.delims(g)])
def test_exact_kernels_equal_the_cpu_parser(files, group, delim):
    """fast_path=0: the two device paths and the CPU parser agree on the same bytes"""
    cfgs = cc.configs(group)
    for k, case in enumerate(cc.cases(group, delim)):
        lc, wc = cfgs[k % len(cfgs)] if group != "g" else (513, 1500)
        check(files, case, lc, wc, fast_path=0)


@pytest.mark.parametrize("lc,wc", cc.REFUSED)
def test_a_weight_column_equal_to_the_label_column_is_refused(files, lc, wc):
    """as the CPU parser does (test_csv_cases_cpu.py): nothing is parsed"""
    p = case_path(files, cc.cases("g")[0])
    with pytest.raises(Exception, match="label_column and weight_column must differ"):
        data.GPUParser(p, format="csv", label_column=lc, weight_column=wc, chunk_bytes=CHUNK)


def assert_same(got, want, name, field=False):
    for k in ("label", "weight", "value"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    for k in ("qid", "offset", "index") + (("field",) if field else ()):
        assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("fmt", ["libsvm", "libfm"])
def test_token_formats_at_every_chunk_end(files, fmt):
    """k_tile_fill stages its text through LDS windows of its own: the chunk
    ends at every size of group e behind a last line that crosses the tile
    edge, the last byte a digit, a blank, a carriage return or a line end;
    pinned ring and mapped file (the bytes behind the end differ)"""
    for name, text in cc.svm_end_cases(fmt):
        p = files(name, text)
        want = cpu_reference(p, fmt)
        for zero_copy in (0, 1):
            gp = data.GPUParser(p, format=fmt, chunk_bytes=CHUNK, zero_copy=zero_copy)
            got = pyref.concat_blocks([gp.parse_all().to_host()])
            assert gp.stats()["chunks"] == 1
            assert_same(got, want, f"{name} zero_copy={zero_copy}", field=fmt == "libfm")


@pytest.mark.parametrize("lc,wc", cc.SHAPES)
def test_replay_of_a_merged_csv_chunk(files, lc, wc):
    """two chunks, the first not a multiple of the tile: replayed from HBM as
    one merged chunk, every tile boundary of the second chunk's text falls at
    another file offset than in epoch 1.  Every epoch equals the CPU parser."""
    text = cc.cases("a")[0].text + cc.cases("c")[1].text
    p = files("replay.csv", text)
    want = cpu_reference(p + cc.query(lc, wc, ","))
    gp = data.GPUParser(p + cc.query(lc, wc, ","), format="csv", label_column=lc,
                        weight_column=wc, chunk_bytes=44 * 1024, hbm_cache=1)
    csr = data.DeviceCSR()
    for epoch in (1, 2):
        before = gp.stats()["chunks"]
        gp.before_first()
        csr.clear()
        gp.parse_all(csr)
        assert_same(pyref.concat_blocks([csr.to_host()]), want, f"epoch {epoch}")
        # two chunks streamed, then one merged chunk at the most
        counted = gp.stats()["chunks"] - before
        assert counted == 2 if epoch == 1 else counted <= 1, (epoch, counted)
    # the chunks one by one: where the first one ended
    gp.before_first()
    blocks, first = [], None
    while gp.next():
        blocks.append(gp.value_to_host())
        first = gp.tell() if first is None else first
    assert 0 < first < len(text) and first % cc.TILE != 0
    assert_same(pyref.concat_blocks(blocks), want, "epoch 3")
    assert gp.stats()["exact_chunks"] == 0
