"""GB6 (ops.pack_forest / predict_forest, SparseGBDT.predict(method="rows") / .leaves) against
tests/forest_ref.py: leaf ids and f32 margins exactly, margins to T ulps of the f64 sum."""
import functools

import numpy as np
import pytest
import torch

import forest_ref as ref
from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT

pytestmark = pytest.mark.gpu
R = int(_dmlc.forest_staged_row_entries())
F = 2 * R + 16
POOL = np.float32([-3e38, -1.5, 0.0, 0.25, 7.0, np.inf])


@functools.lru_cache(maxsize=None)
def _matrix(wide=False):
    """features < 32 are hot (most rows, most splits); ``wide``: id 1 + 2^32 where 1 is absent"""
    rng = np.random.default_rng(3)
    ncuts = np.arange(F) % 6
    cuts = [np.sort(rng.choice(POOL, n, replace=False)) for n in ncuts]
    cut_ptr = np.concatenate([[0], np.cumsum(ncuts)]).astype(np.int64)
    p = np.where(np.arange(F) < 32, 40.0, 1.0)
    lens = [0, 1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3] + list(rng.integers(0, 40, 30))
    idx, val = [], []
    for n in lens:
        ids = rng.choice(F, n, replace=False, p=p / p.sum()).astype(np.int64)
        if n == 2 * R + 3:  # features with cuts in the second and the third chunk
            ids = np.concatenate([ids[ncuts[ids] == 0], ids[ncuts[ids] > 0]])
        for f in ids:
            c = cuts[f]
            x = np.concatenate([c, np.nextafter(c, POOL[5]), np.nextafter(c, -POOL[5]),
                                np.float32([np.inf, -np.inf, -0.0, 0.5])])
            val.append(rng.choice(x))
        if wide and 0 < n <= 65 and 1 not in ids:
            ids[0] = 1 + 2 ** 32
        idx.append(ids)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, np.concatenate(idx), np.float32(val), cut_ptr, np.concatenate(cuts)


def _forest(ntrees, depth):
    """random heap trees with early leaves; tree 0 splits on the long row's last entry, then
    on one of its second chunk; the last tree is a bare root leaf"""
    off, idx, _, cut_ptr, _ = _matrix()
    rng = np.random.default_rng(ntrees * 16 + depth)
    size, ncuts, long_row = 2 ** (depth + 1) - 1, np.diff(cut_ptr), idx[off[9]:off[10]]
    with_cuts = np.nonzero(ncuts)[0]
    trees = []
    for t in range(ntrees):
        f = rng.choice(with_cuts if t % 3 == 1 else with_cuts[:26], size)  # mostly hot ones
        if t == 0:
            f[:3] = [long_row[-1], long_row[R + 5], long_row[R + 5]]
        else:
            f[(rng.random(size) < 0.2) | (t == ntrees - 1 and ntrees > 2)] = -1
        f[size // 2:] = -1
        trees.append({"feature": f.astype(np.int64),
                      "bin": rng.integers(0, ncuts[np.maximum(f, 0)].clip(1)).astype(np.int32),
                      "default_left": rng.random(size) < 0.5,
                      "leaf": rng.standard_normal(size).astype(np.float32)})
    return trees


def _dev_csr(off, idx, val, kind="i32"):
    t = torch.from_numpy(idx) if kind in ("i64", "u64") else torch.from_numpy(idx.astype(np.int32))
    t = t.view({"u32": torch.uint32, "u64": torch.uint64}.get(kind, t.dtype))
    return {"offset": torch.from_numpy(off).cuda(), "index": t.cuda(),
            "value": None if val is None else torch.from_numpy(val).cuda()}


def _pack(trees, cut_ptr, cut):
    dev = [{k: torch.from_numpy(v).cuda() for k, v in t.items()}
           for t in list(trees) + [{"cut_ptr": cut_ptr, "cut": cut}]]
    return ops.pack_forest(dev[:-1], dev[-1])


def _check(csr, off, idx, val, trees, cut_ptr, cut, seen=None):
    want = ref.walk(off, idx, val, trees, cut_ptr, cut, seen)
    leaves = np.stack([tree["leaf"][want[:, t]] for t, tree in enumerate(trees)])  # [T, rows] f32
    m32 = functools.reduce(np.add, leaves, np.zeros(want.shape[0], np.float32))  # in tree order
    partial = np.cumsum(leaves.astype(np.float64), 0)
    m64, top = partial[-1], np.abs(partial).max(0)  # T f32 additions: T ulps of the largest sum
    forest = _pack(trees, cut_ptr, cut)
    leaf, margin = ops.predict_forest(csr, forest, "leaf"), ops.predict_forest(csr, forest)
    assert leaf.dtype == torch.int32 and torch.equal(leaf.cpu(), torch.from_numpy(want))
    assert margin.dtype == torch.float32 and torch.equal(margin.cpu(), torch.from_numpy(m32))
    assert (np.abs(margin.cpu().numpy() - m64) <= len(trees) * np.spacing(np.float32(top))).all()
    return want


@pytest.mark.parametrize("ntrees,depth,kind", [(t, d, "i32") for t in (1, 63, 64, 65, 130)
                                               for d in (1, 6)] + [(65, 6, k) for k in ("u32", "i64", "u64")])
def test_leaves_and_margins_equal_the_reference(ntrees, depth, kind):
    off, idx, val, cut_ptr, cut = _matrix(wide=kind in ("i64", "u64"))
    assert (idx >= 2 ** 32).any() == (kind in ("i64", "u64"))
    trees, seen = _forest(ntrees, depth), set()
    want = _check(_dev_csr(off, idx, val, kind), off, idx, val, trees, cut_ptr, cut, seen)
    long_row, f0 = list(idx[off[9]:off[10]]), trees[0]["feature"]  # tree 0 matches in the long
    assert long_row.index(f0[0]) >= 2 * R  # row's third chunk and, a level down, in its second
    assert depth == 1 or R <= long_row.index(f0[1]) < 2 * R
    if ntrees > 1:  # both default sides, a last-bin split; with depth: leaves of several depths
        assert seen == {"left", "right", "last", "value"}
        assert depth == 1 or len({int(i + 1).bit_length() for i in want.ravel()}) > 2


def test_operand_shapes():
    off, idx, val, cut_ptr, cut = _matrix()
    trees, whole = _forest(3, 6), _dev_csr(off, idx, val)
    _check(dict(whole, value=None), off, idx, None, trees, cut_ptr, cut)
    part = dict(whole, offset=whole["offset"][5:12])  # offset[0] != 0, rows of R +- 1 and 2 R + 3
    _check(part, off[5:12], idx, val, trees, cut_ptr, cut)
    pairs = torch.stack([whole["index"], whole["value"].view(torch.int32)], 1).contiguous()
    paired = dict(whole, index=pairs[:, 0], value=pairs.view(torch.float32)[:, 1])
    _check(paired, off, idx, val, trees, cut_ptr, cut)
    forest = _pack(trees, cut_ptr, cut)
    for rows, csr in ((0, dict(whole, offset=whole["offset"][:1])), (off.size - 1, whole)):
        none = _pack([], cut_ptr, cut) if rows else forest
        assert tuple(ops.predict_forest(csr, none, "leaf").shape) == (rows, 0 if rows else 3)
        assert ops.predict_forest(csr, none).tolist() == [0.0] * rows
    bad = np.where(np.arange(val.size) == off[10] - 1, np.float32(np.nan), val)  # tree 0's root
    bad, small = _dev_csr(off, idx, bad), _forest(3, 1)  # feature, the long row's last entry
    for some in (small, small[2:]):  # small[2]: a bare root leaf -- nothing walks, rows are checked
        with pytest.raises(ValueError, match="NaN"):
            ops.predict_forest(bad, _pack(some, cut_ptr, cut))
    went = ops.predict_forest(bad, _pack(small, cut_ptr, cut), "leaf", validate=False)
    assert int(went[9, 0]) == 2  # x <= thr is false for a NaN: right, whatever the bin


@pytest.mark.parametrize("what", ["bin is outside", "without cuts", "unequal size", "nodes, not"])
def test_pack_forest_refuses(what):  # ``what``: the message
    _, _, _, cut_ptr, cut = _matrix()
    tree = _forest(3, 1)[0]
    tree["bin"][0] += 5 * (what == "bin is outside")  # past the last bin of every feature
    if what == "without cuts":
        tree["feature"][0] = 6  # 6 % 6 == 0 cuts
    trees = [tree] + [_forest(3, 6)[0]] * (what == "unequal size")
    if what == "nodes, not":
        trees = [{k: v[:4].copy() for k, v in _forest(3, 6)[0].items()}]
    with pytest.raises(ValueError, match=what):
        _pack(trees, cut_ptr, cut)


def test_model_rows_path_equals_the_levels_path():
    rng = np.random.default_rng(21)  # the 300 x 20 table of test_gpu_gbdt.py
    x = rng.integers(0, 200, (300, 20)).astype(np.float32) / 200
    keep = rng.random(x.shape) < 0.9
    off = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    r, c = np.nonzero(keep)
    csr = _dev_csr(off, c.astype(np.int64), x[r, c])
    csr["label"] = torch.from_numpy(x[:, 3] * 2 - x[:, 7]).cuda()
    model = SparseGBDT(20, max_depth=4, learning_rate=0.5, objective="squared").fit(csr, 5)
    rows = model.predict(csr, method="rows")
    assert torch.equal(rows, model.predict(csr)) and rows.abs().max() > 0
    assert torch.equal(rows.view(torch.int32), model.predict(csr, method="rows").view(torch.int32))
    binned, leaves = ops.bin_features(csr, model.cuts, 20), model.leaves(csr)
    for t, tree in enumerate(model.trees):  # the level-by-level walk of predict()
        assert torch.equal(leaves[:, t], model._walk_levels(binned, tree))
    model.boost(binned, csr["label"])
    assert tuple(model.leaves(csr).shape) == (300, 6)  # the cached forest was dropped
