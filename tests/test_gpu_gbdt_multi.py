"""GB3m / GB4m (ops.grad_histogram_multi, ops.best_splits_multi) and vector-leaf
SparseGBDT against tests/gbdt_ref.py applied per output: histograms must equal
it exactly; split gains to 1e-12 of the summed terms (see test_gpu_gbdt.py's
_check_splits), validity taken on the integer hessian sums.

The matrix has 3 S rows (S = _dmlc.gbdt_segment_entries()) and 40 columns: 0, 1,
S - 1, S + 1 and 2 S + 3 entries among short ones, one column of 256 distinct
values (the outputs are tiled from K = 16) and one of 2."""
import functools
import math

import numpy as np
import pytest
import torch

import gbdt_ref as ref
from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT

pytestmark = pytest.mark.gpu
S = int(_dmlc.gbdt_segment_entries())
ROWS, NFEAT = 3 * S, 40
KMAX = int(_dmlc.gbdt_max_outputs())
OUTPUTS = [1, 3, 8, 16, KMAX]
FIRST = 7  # the node window starts here; rows on FIRST - 2 .. FIRST + N + 1, some outside it


@functools.lru_cache(maxsize=None)
def _binned():
    rng = np.random.default_rng(5)
    lengths = rng.integers(2, 40, NFEAT)
    lengths[[3, 9, 15, 22, 28, 34]] = [0, 1, S - 1, S + 1, 2 * S + 3, 300]
    rows, cols, vals = [], [], []
    for f, n in enumerate(lengths):
        rows.append(np.sort(rng.choice(ROWS, n, replace=False)))
        cols.append(np.full(n, f))
        if f == 22:
            vals.append(rng.permutation(np.arange(n) % 256).astype(np.float64))  # 256 cuts
        elif f == 34:
            vals.append(rng.choice([-3.0, 7.0], n))                              # 2 cuts
        else:
            vals.append(rng.standard_normal(n))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=ROWS))]).astype(np.int64)
    idx, val = cols[order].astype(np.int64), vals[order].astype(np.float32)
    cut_ptr, cut = ref.feature_cuts(off, idx, val, NFEAT, 256)
    assert set(np.diff(cut_ptr)) >= {0, 1, 2, 256}
    host = ref.bin_features(off, idx, val, NFEAT, cut_ptr, cut)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items() if k != "rows"}
    return host, dict(dev, rows=ROWS)


@functools.lru_cache(maxsize=None)
def _case(K, num_nodes):
    """gradients [ROWS, K], positions, and the reference histogram / node sums per output"""
    host, _ = _binned()
    rng = np.random.default_rng(100 * K + num_nodes)
    g = rng.standard_normal((ROWS, K)).astype(np.float32)
    h = rng.random((ROWS, K)).astype(np.float32)
    pos = rng.integers(FIRST - 2, FIRST + num_nodes + 2, ROWS).astype(np.int32)
    scale = ref.gradient_scale(g, h)
    hist = np.stack([ref.grad_histogram(host, g[:, k], h[:, k], pos, num_nodes, scale, FIRST)
                     for k in range(K)], 2)
    sums = np.stack([ref.node_sums(g[:, k], h[:, k], pos, num_nodes, scale, FIRST)
                     for k in range(K)], 1)
    return g, h, pos, scale, hist, sums


@pytest.mark.parametrize("num_nodes", [1, 33])
@pytest.mark.parametrize("K", OUTPUTS)
def test_histogram_equals_the_scalar_reference_per_output(K, num_nodes):
    g, h, pos, scale, want, _ = _case(K, num_nodes)
    args = (_binned()[1], torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda(),
            torch.from_numpy(pos).cuda(), num_nodes, scale, FIRST)
    got = ops.grad_histogram_multi(*args)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.grad_histogram_multi(*args), got)


def _gain_table(hist, sums, cut_ptr, scale, lam, gamma, mcw):
    """float64 [N, bins, 2] (-inf where invalid) and the tolerance: gbdt_ref's per-output gains
    and largest terms summed over k; valid with sum_k HL_k, sum_k HR_k >= K mcw scale on the
    integer sums (left sums are linear: those of the histogram summed over k)"""
    K = hist.shape[2]
    per_k = [(hist[:, :, k], sums[:, k], cut_ptr, scale, lam, 0.0, -np.inf) for k in range(K)]
    gain = sum(ref.gain_table(*a) for a in per_k) - gamma
    tol = 1e-12 * sum(ref.gain_table(*a, terms=True) for a in per_k)
    feat = np.repeat(np.arange(len(cut_ptr) - 1), np.diff(cut_ptr))
    hsum, nsum = hist[..., 1].sum(2), sums[..., 1].sum(1)
    csum = np.concatenate([np.zeros((len(hsum), 1), np.int64), np.cumsum(hsum, 1)], 1)
    before = csum[:, cut_ptr[:-1]]
    left = csum[:, 1:] - before[:, feat]
    miss = (nsum[:, None] - (csum[:, cut_ptr[1:]] - before))[:, feat]
    hl = np.stack([left, left + miss], 2)
    hr, least = nsum[:, None, None] - hl, K * mcw * scale
    valid = (hl.astype(np.float64) >= least) & (hr.astype(np.float64) >= least)
    return np.where(valid, gain, -np.inf), tol


def _check_splits(got, table, tol, cut_ptr):
    feature, tbin = got["feature"].cpu().numpy(), got["bin"].cpu().numpy()
    left, gain = got["default_left"].cpu().numpy(), got["gain"].cpu().numpy()
    assert got["feature"].dtype == torch.int64 and got["bin"].dtype == torch.int32
    assert got["default_left"].dtype == torch.bool and got["gain"].dtype == torch.float64
    valid = np.isfinite(table)
    for n in range(table.shape[0]):
        returned = 0.0
        if feature[n] >= 0:
            assert 0 <= tbin[n] < cut_ptr[feature[n] + 1] - cut_ptr[feature[n]]
            at = (n, cut_ptr[feature[n]] + tbin[n], int(left[n]))
            assert valid[at] and gain[n] > 0
            assert abs(gain[n] - table[at]) <= tol[at]
            returned = gain[n]
        over = valid[n] & (table[n] - returned > np.where(valid[n], tol[n], 0.0))
        assert not over.any(), (n, returned, table[n][over].max())


@pytest.mark.parametrize("mcw", [1.0, 20.0])  # 20: the short columns' light children fall away
@pytest.mark.parametrize("num_nodes", [1, 33])
@pytest.mark.parametrize("K", OUTPUTS)
def test_best_splits_against_the_float64_table(K, num_nodes, mcw):
    _, _, _, scale, hist, sums = _case(K, num_nodes)
    cut_ptr = _binned()[0]["cut_ptr"]
    dev = [torch.from_numpy(a).cuda() for a in (hist, sums, cut_ptr)]
    table, tol = _gain_table(hist, sums, cut_ptr, scale, 1.0, 0.0, mcw)
    got = ops.best_splits_multi(*dev, scale, 1.0, 0.0, mcw)
    assert (got["feature"] >= 0).all()
    _check_splits(got, table, tol, cut_ptr)
    again = ops.best_splits_multi(*dev, scale, 1.0, 0.0, mcw)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    none = ops.best_splits_multi(*dev, scale, 1.0, float(got["gain"].max()) + 1.0, mcw)
    assert (none["feature"] == -1).all() and not none["gain"].any()
    if K == 1:
        scalar = ops.best_splits(dev[0][:, :, 0].contiguous(), dev[1][:, 0].contiguous(), dev[2],
                                 scale, 1.0, 0.0, mcw)
        for k in ("feature", "bin", "default_left"):
            assert torch.equal(got[k], scalar[k]), k


@pytest.mark.parametrize("mcw", [1.0, 20.0])
@pytest.mark.parametrize("num_nodes", [1, 33])
def test_one_output_equals_the_scalar_ops_bit_for_bit(num_nodes, mcw):
    """K = 1 given as [rows, 1] runs GB3m / GB4m<1>, [rows] runs GB3 / GB4: the same histogram
    bytes, the same candidates in the same order and the same float64 gain expression."""
    g, h, pos, scale, hist, sums = _case(1, num_nodes)
    cut_ptr = _binned()[0]["cut_ptr"]
    # on the CPU first: scale is a power of two, so GB4's validity rule (float64 sums / scale
    # against mcw) and GB4m's (integer sums against K mcw scale) are one rule on this input
    assert math.frexp(scale)[0] == 0.5
    scalar_table = ref.gain_table(hist[:, :, 0], sums[:, 0], cut_ptr, scale, 1.0, 0.0, mcw)
    assert np.array_equal(scalar_table, _gain_table(hist, sums, cut_ptr, scale, 1.0, 0.0, mcw)[0])
    binned = _binned()[1]
    g, h, pos = (torch.from_numpy(a).cuda() for a in (g, h, pos))
    multi = ops.grad_histogram_multi(binned, g, h, pos, num_nodes, scale, FIRST)
    scalar = ops.grad_histogram(binned, g[:, 0].contiguous(), h[:, 0].contiguous(), pos,
                                num_nodes, scale, FIRST)
    assert tuple(multi.shape) == (num_nodes, int(cut_ptr[-1]), 1, 2)
    assert torch.equal(multi.squeeze(2), scalar)
    assert torch.equal(scalar.cpu(), torch.from_numpy(hist[:, :, 0]))
    node_sum, cuts = torch.from_numpy(sums).cuda(), binned["cut_ptr"]
    got = ops.best_splits_multi(multi, node_sum, cuts, scale, 1.0, 0.0, mcw)
    want = ops.best_splits(scalar, node_sum[:, 0].contiguous(), cuts, scale, 1.0, 0.0, mcw)
    assert (want["feature"] >= 0).all()
    for k in ("feature", "bin", "default_left"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["gain"].view(torch.int64), want["gain"].view(torch.int64))


def _wrong_call(name, what):
    """a call of ops.<name> whose hist / grad has the wrong dtype or the other layout's rank"""
    vector = name.endswith("_multi")
    if what == "rank":
        vector = not vector
    if name.startswith("grad_histogram"):
        g = torch.zeros((ROWS, 1) if vector else (ROWS,), device="cuda",
                        dtype=torch.float64 if what == "dtype" else torch.float32)
        pos = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
        return lambda: getattr(ops, name)(_binned()[1], g, g, pos, 1, 1.0)
    cut_ptr = _binned()[1]["cut_ptr"]
    middle = (1,) if vector else ()
    hist = torch.zeros((2, int(cut_ptr[-1])) + middle + (2,), device="cuda",
                       dtype=torch.int32 if what == "dtype" else torch.int64)
    node_sum = torch.ones((2,) + middle + (2,), dtype=torch.int64, device="cuda")
    return lambda: getattr(ops, name)(hist, node_sum, cut_ptr, 1.0)


@pytest.mark.parametrize("name", ["grad_histogram", "grad_histogram_multi", "best_splits",
                                  "best_splits_multi"])
def test_a_wrong_dtype_is_refused_under_the_functions_own_name(name):
    with pytest.raises(ValueError) as err:
        _wrong_call(name, "dtype")()
    assert str(err.value).startswith(name + ": "), str(err.value)


@pytest.mark.parametrize("name", ["best_splits", "best_splits_multi", "grad_histogram"])
def test_the_other_layouts_rank_is_refused(name):
    """best_splits takes no 4-D hist, best_splits_multi no 3-D one, grad_histogram no [rows, 1]"""
    with pytest.raises(ValueError) as err:
        _wrong_call(name, "rank")()
    assert str(err.value).startswith(name + ": "), str(err.value)


@functools.lru_cache(maxsize=None)
def _three_classes(rows=600):
    """class c has feature c; features 3 .. 9 are noise"""
    rng = np.random.default_rng(11)
    label = rng.integers(0, 3, rows)
    noise = rng.random((rows, 7)) < 0.3
    idx = [np.concatenate([[label[r]], 3 + np.flatnonzero(noise[r])]) for r in range(rows)]
    off = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    idx = np.concatenate(idx).astype(np.int32)
    val = np.where(idx < 3, 1.0, rng.standard_normal(idx.size)).astype(np.float32)
    return {"offset": torch.from_numpy(off).cuda(), "index": torch.from_numpy(idx).cuda(),
            "value": torch.from_numpy(val).cuda(), "label": torch.from_numpy(label).float().cuda()}


def test_softmax_model_separates_three_classes():
    csr = _three_classes()
    model = SparseGBDT(10, objective="softmax", num_outputs=3, max_depth=3)
    binned = ops.bin_features(csr, ops.feature_cuts(csr, 10), 10)
    last = math.log(3.0)
    for _ in range(4):
        loss = float(model.loss(model.boost(binned, csr["label"]), csr["label"]))
        assert loss < last
        last = loss
    assert model.trees[0]["leaf"].shape == (15, 3) and model.margin.shape == (600, 3)
    assert torch.equal(model.margin.argmax(1), csr["label"].long())
    levels, rows = model.predict(csr, method="levels"), model.predict(csr, method="rows")
    assert torch.equal(levels, model.margin) and torch.equal(rows, model.margin)
    assert tuple(model.leaves(csr).shape) == (600, 4)


@pytest.mark.parametrize("what", ["softmax_one_output", "rank_two_outputs", "label_is_K",
                                  "grad_1d", "too_many_outputs"])
def test_bad_arguments_raise(what):
    csr = _three_classes()
    with pytest.raises(ValueError):
        if what == "softmax_one_output":
            SparseGBDT(10, objective="softmax", num_outputs=1)
        elif what == "rank_two_outputs":
            SparseGBDT(10, objective="rank:ndcg", num_outputs=2)
        elif what == "label_is_K":
            label = csr["label"].clone()
            label[5] = 3.0
            SparseGBDT(10, objective="softmax", num_outputs=3).fit(dict(csr, label=label), 1)
        else:
            shape = (ROWS,) if what == "grad_1d" else (ROWS, KMAX + 1)
            g = torch.zeros(shape, device="cuda")
            ops.grad_histogram_multi(_binned()[1], g, g, torch.zeros(ROWS, dtype=torch.int32,
                                                                     device="cuda"), 1, 1.0)
