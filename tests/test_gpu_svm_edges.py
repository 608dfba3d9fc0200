"""The token tile path (src/gpu/tile_count_kernels.hip: k_tile_count;
tile_fill_kernels.hip: k_tile_fill, k_tile_hash) on the placed cases of svm_cases.py: line ends, token starts,
whole tokens, decode-round totals, deferred tokens, weights, `qid:` tokens,
owned lines and the chunk end on every lane, half-step, step and tile edge of
the walk, LibSVM and LibFM.

Every file is one chunk.  Five paths read the same bytes: the counted fill
(lean, and with weight / qid columns), the one-pass fill over HBM-resident
text, the exact kernels (fast_path=0), the fused hash kernel (counted and one
pass) and the replay of a merged chunk.  The CSR is compared with the C++
parser -- which test_svm_cases_cpu.py holds to the Python oracle on the same
files -- float arrays as uint32 bits, everything else exactly: no tolerance.
The hashed rows of the dyadic cases (values that any f32 summation order adds
exactly) equal pyref.ref_dense of the C++ parser's rows exactly; the others
are held to ops.hashed_dense of the tile CSR within the 1e-6 of
test_gpu_hashed.py.  A case that must stay on the tile path asserts
exact_chunks == 0, one that must leave it (a `qid:` near-miss, a blank-started
line at a tile start, a half step above the hash kernel's list)
exact_chunks == 1."""
import functools

import numpy as np
import pytest
import torch

from dmlc_core_amd import data, ops
import svm_cases as sc
import pyref

pytestmark = pytest.mark.gpu

CHUNK = 1 << 20
SEED = 5
DIMS = (192, 256)  # one that is no power of two, one that is
GROUP_FORMATS = [(g, f) for g in sc.GROUPS for f in sc.FORMATS]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """path of a case's file (each written once)"""
    root = tmp_path_factory.mktemp("svm_edges")
    done = {}

    def path(name, text):
        if name not in done:
            done[name] = str(root / name)
            with open(done[name], "wb") as f:
                f.write(text.encode("latin-1"))
        return done[name]
    return path


@functools.lru_cache(maxsize=None)
def cpu_reference(path, fmt, index64=False):
    return pyref.concat_blocks(list(data.iter_blocks(path, type=fmt, index64=index64)))


def case_path(files, case):
    return files(f"{case.name}.{case.fmt}", case.text)


def same(case, got, want, how):
    msg = sc.first_difference(case, got, want)
    assert not msg, f"{how}: {msg}"


def assert_path(case, expect, exact, how, left):
    if expect == "tile":
        assert exact == 0, f"{how}: left the tile path"
    elif expect == "exact":
        assert exact == 1, f"{how}: stayed on the tile path"
    else:
        print(f"{how}: {'exact kernels' if exact else 'tile path'}")
    if exact:
        left.append((case, expect))


def only_expected_left(left):
    # a case that ran the exact kernels proves nothing about the tile path
    assert all(e == "exact" or (e == "either" and c.name in sc.EITHER) for c, e in left)


def has_qid(case):
    return case.fmt == "libsvm" and "qid:" in case.text


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_counted_fill_equals_the_cpu_parser(files, group, fmt):
    """k_tile_count + k_tile_fill: the lean instantiation, and in group e the
    one with weight and qid columns"""
    left = []
    for case in sc.cases(group, fmt):
        p = case_path(files, case)
        for index64 in ((False, True) if group in sc.INDEX64_GROUPS else (False,)):
            gp = data.GPUParser(p, format=fmt, index64=index64, chunk_bytes=CHUNK)
            got = pyref.concat_blocks([gp.parse_all().to_host()])
            how = f"{case.name} {fmt} index64={index64}"
            same(case, got, cpu_reference(p, fmt, index64), how)
            st = gp.stats()
            assert st["chunks"] == 1, (how, st["chunks"])
            assert_path(case, case.expect, st["exact_chunks"], how, left)
    only_expected_left(left)


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_one_pass_fill_equals_the_cpu_parser(files, group, fmt):
    """epoch 1 streams; then k_tile_fill<kOnePass> twice into the reused
    DeviceCSR and once into a fresh one (overflow, grow, run again)"""
    left = []
    for case in sc.cases(group, fmt):
        p = case_path(files, case)
        want = cpu_reference(p, fmt)
        gp = data.GPUParser(p, format=fmt, chunk_bytes=CHUNK, hbm_cache=1, one_pass=1)
        csr = data.DeviceCSR()
        for epoch, target in enumerate((csr, csr, csr, None), 1):
            before = gp.stats()
            gp.before_first()
            out = data.DeviceCSR() if target is None else target
            out.clear()
            gp.parse_all(out)
            how = f"{case.name} {fmt} one-pass epoch {epoch}"
            same(case, pyref.concat_blocks([out.to_host()]), want, how)
            st = gp.stats()
            assert st["chunks"] - before["chunks"] == 1, how
            assert_path(case, case.expect, st["exact_chunks"] - before["exact_chunks"], how, left)
        st = gp.stats()
        if has_qid(case):
            assert st["one_pass_chunks"] == 0, case.name  # qid data: the counted path
        elif case.expect == "tile":
            assert st["one_pass_chunks"] > 0, case.name
            if group == "e":  # a weight column the target did not have: run again
                assert st["one_pass_reruns"] >= 1, case.name
    only_expected_left(left)


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_exact_kernels_equal_the_cpu_parser(files, group, fmt):
    """fast_path=0: the two device paths and the CPU parser agree on the same bytes"""
    for case in sc.cases(group, fmt):
        p = case_path(files, case)
        gp = data.GPUParser(p, format=fmt, chunk_bytes=CHUNK, fast_path=0)
        got = pyref.concat_blocks([gp.parse_all().to_host()])
        same(case, got, cpu_reference(p, fmt), f"{case.name} {fmt} fast_path=0")
        assert gp.stats()["chunks"] == 1


def hashed(gp, dim, fp8=False, out=None):
    kw = dict(scale=1.0) if fp8 else {}
    b = gp.parse_all_hashed(dim, seed=SEED, fp8=fp8, strategy="fused", out=out, **kw)
    x = b["x"].cpu()
    x = x.view(torch.uint8).numpy() if fp8 else x.numpy()
    return b, x, b["label"].cpu().numpy()


@pytest.mark.parametrize("group,fmt", GROUP_FORMATS)
def test_fused_hash_equals_the_cpu_parser(files, group, fmt):
    """k_tile_hash, counted and (hash_one_pass=1, a replay into the reused
    batch) one pass"""
    left = []
    for case in sc.cases(group, fmt):
        p = case_path(files, case)
        rows = cpu_reference(p, fmt)
        for dim in DIMS:
            how = f"{case.name} {fmt} hashed dim={dim}"
            if case.dyadic:
                ref = pyref.ref_dense(rows, dim, SEED, fmt == "libfm")[0]
                want = ref.astype(np.float32)
                assert np.array_equal(want.astype(np.float64), ref), how  # exact in f32
            else:
                csr = data.csr_to_torch(data.GPUParser(p, format=fmt, chunk_bytes=CHUNK).parse_all())
                want = ops.hashed_dense(csr, dim, seed=SEED, fp8=False).cpu().numpy()
            gp = data.GPUParser(p, format=fmt, chunk_bytes=CHUNK, hbm_cache=1, hash_one_pass=1)
            batch = None
            for mode in ("counted", "one pass"):
                before = gp.stats()
                if batch is not None:
                    gp.before_first()
                batch, x, label = hashed(gp, dim, out=batch)
                assert np.array_equal(label.view(np.uint32), rows["label"].view(np.uint32)), how
                if case.dyadic:
                    np.testing.assert_array_equal(x, want, err_msg=f"{how} {mode}")
                else:
                    np.testing.assert_allclose(x, want, rtol=1e-6, atol=1e-6, err_msg=f"{how} {mode}")
                st = gp.stats()
                assert st["chunks"] - before["chunks"] == 1, how
                assert_path(case, case.hexpect, st["exact_chunks"] - before["exact_chunks"],
                            f"{how} {mode}", left)
            if case.hexpect == "tile":
                assert gp.stats()["one_pass_chunks"] >= 1, how
            if case.fp8:
                g8 = data.GPUParser(p, format=fmt, chunk_bytes=CHUNK)
                _, x8, _ = hashed(g8, dim, fp8=True)
                assert np.abs(ref).max() <= pyref.E4M3_MAX
                np.testing.assert_array_equal(x8, pyref.e4m3_nearest_even(ref), err_msg=how)
                assert g8.stats()["exact_chunks"] == (case.hexpect == "exact")
    only_expected_left(left)


def replay_pairs(fmt):
    """(name, first case, second case): the first is no multiple of the tile"""
    a, b, c, d, e = (sc.cases(g, fmt) for g in "abcde")
    return (("a+c", a[0], c[0]), ("b+d", b[0], d[0]), ("e+c", e[0], c[1]))


@pytest.mark.parametrize("fmt", sc.FORMATS)
@pytest.mark.parametrize("pair", range(3))
def test_replay_of_a_merged_chunk(files, fmt, pair):
    """two chunks, the first not a multiple of the tile: replayed from HBM as
    one merged chunk, every edge of the second chunk's text falls at another
    file offset than in epoch 1.  Every epoch equals the CPU parser."""
    name, first, second = replay_pairs(fmt)[pair]
    text = first.text + second.text
    p = files(f"replay_{pair}.{fmt}", text)
    want = cpu_reference(p, fmt)
    case = second._replace(name=f"replay {name}", text=text, marks=())
    gp = data.GPUParser(p, format=fmt, chunk_bytes=44 * 1024, hbm_cache=1)
    csr = data.DeviceCSR()
    for epoch in (1, 2, 3):
        before = gp.stats()["chunks"]
        gp.before_first()
        csr.clear()
        gp.parse_all(csr)
        same(case, pyref.concat_blocks([csr.to_host()]), want, f"epoch {epoch}")
        counted = gp.stats()["chunks"] - before
        assert counted == 2 if epoch == 1 else counted <= 1, (epoch, counted)
    gp.before_first()
    blocks, first_end = [], None
    while gp.next():
        blocks.append(gp.value_to_host())
        first_end = gp.tell() if first_end is None else first_end
    assert 0 < first_end < len(text) and first_end % sc.TILE != 0
    same(case, pyref.concat_blocks(blocks), want, "chunk by chunk")
    assert gp.stats()["exact_chunks"] == 0
