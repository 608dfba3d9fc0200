"""The host side of ranking on qid groups: SparseRanker.reference and the host
paths of SparseRanker.loss / ndcg against brute-force Python loops over the
pairs (the definitions of ops.rank_loss_parts), ops.group_rows against a loop,
the argument checks of ops.rank_loss / ndcg / qid_groups on CPU tensors, and
the extension's ranking constants and zero-group launches.  No GPU."""
import math

import pytest
import torch

from dmlc_core_amd import _dmlc, data, models, ops
from dmlc_core_amd.models import SparseRanker

# scores with ties, labels with ties; an empty group, a one-row group and a
# group whose labels are all equal (no pairs)
SCORE = [0.5, -1.0, 0.5, 2.0, 0.5, 0.25, 3.0, 1.0, 1.0, 1.0, -0.5, 0.0, 0.75, 0.75, -2.0]
LABEL = [1, 0, 2, 0, 1, 4, 2, 2, 2, 2, 0, 3, 3, 1, 0]
PTR = [0, 5, 5, 6, 10, 15]


def _rank(keys, i):
    return sum(1 for j in range(len(keys)) if keys[j] > keys[i] or (keys[j] == keys[i] and j < i))


def _disc(r):
    return 1.0 / math.log2(2 + r)


def _loop_loss(score, label, ptr, weighting, sigma):
    """(loss, grad) by loops over the pairs, in Python floats"""
    grad = [0.0] * len(score)
    total, counted = 0.0, 0
    for b, e in zip(ptr[:-1], ptr[1:]):
        s, lab = score[b:e], label[b:e]
        n = e - b
        pairs = [(i, j) for i in range(n) for j in range(n) if lab[i] > lab[j]]
        if not pairs:
            continue
        gain = [2.0 ** x - 1 for x in lab]
        d = [_disc(_rank(s, i)) for i in range(n)]
        idcg = sum(gain[i] * _disc(_rank(lab, i)) for i in range(n))
        loss = 0.0
        for i, j in pairs:
            w = 1.0 if weighting == "none" else abs(gain[i] - gain[j]) * abs(d[i] - d[j]) / idcg
            x = sigma * (s[i] - s[j])
            loss += w * (max(-x, 0.0) + math.log1p(math.exp(-abs(x))))
            rho = 1.0 / (1.0 + math.exp(x))
            grad[b + i] -= sigma / len(pairs) * w * rho
            grad[b + j] += sigma / len(pairs) * w * rho
        total += loss / len(pairs)
        counted += 1
    scale = 1.0 / max(1, counted)
    return total * scale, [g * scale for g in grad]


def _loop_ndcg(score, label, ptr, k):
    out = []
    for b, e in zip(ptr[:-1], ptr[1:]):
        s, lab = score[b:e], label[b:e]
        n = e - b
        kk = n if k is None else k
        dcg = sum((2.0 ** lab[i] - 1) * _disc(_rank(s, i)) for i in range(n) if _rank(s, i) < kk)
        ideal = sum((2.0 ** lab[i] - 1) * _disc(_rank(lab, i)) for i in range(n) if _rank(lab, i) < kk)
        out.append(dcg / ideal if ideal > 0 else 1.0)
    return out


def test_names_are_exported():
    for name in ("qid_groups", "group_rows", "rank_loss", "rank_loss_parts", "ndcg",
                 "RankLossFunction"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    assert "SparseRanker" in models.__all__ and callable(models.SparseRanker)


@pytest.mark.parametrize("sigma", [1.0, 2.5])
@pytest.mark.parametrize("weighting", ["ndcg", "none"])
def test_reference_matches_the_loops(weighting, sigma):
    score = torch.tensor(SCORE, dtype=torch.float64, requires_grad=True)
    label = torch.tensor(LABEL, dtype=torch.float32)
    loss = SparseRanker.reference(score, label, torch.tensor(PTR), weighting, sigma)
    loss.backward()
    want, grad = _loop_loss(SCORE, LABEL, PTR, weighting, sigma)
    assert want > 0
    assert abs(float(loss.detach()) - want) <= 1e-12 * want
    for got, ref in zip(score.grad.tolist(), grad):
        assert abs(got - ref) <= 1e-12 * max(abs(g) for g in grad)
    # rows of the group without pairs and of the one-row group get no gradient
    assert score.grad[5] == 0 and not score.grad[6:10].any()


def test_reference_without_any_pair_is_zero():
    score = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, requires_grad=True)
    loss = SparseRanker.reference(score, torch.tensor([2.0, 2.0, 2.0]), torch.tensor([0, 0, 3]))
    assert float(loss) == 0.0
    with pytest.raises(ValueError, match="weighting"):
        SparseRanker.reference(score, torch.zeros(3), torch.tensor([0, 3]), "pairwise")


@pytest.mark.parametrize("k", [1, 3, 10, None])
def test_reference_ndcg_matches_the_loops(k):
    got = SparseRanker.reference_ndcg(torch.tensor(SCORE, dtype=torch.float64),
                                      torch.tensor(LABEL, dtype=torch.float32), torch.tensor(PTR), k)
    want = _loop_ndcg(SCORE, LABEL, PTR, k)
    assert got.shape == (len(PTR) - 1,)
    assert want[1] == 1.0  # the empty group
    for a, b in zip(got.tolist(), want):
        assert abs(a - b) <= 1e-12
    zero = SparseRanker.reference_ndcg(torch.tensor([3.0, 1.0]), torch.zeros(2), torch.tensor([0, 2]))
    assert zero.tolist() == [1.0]


def _host_csr():
    """15 rows over 6 features with the qid runs of PTR (the empty group has no
    run: 4 groups), on host tensors"""
    g = torch.Generator().manual_seed(5)
    offset = torch.arange(0, 31, 2, dtype=torch.int64)
    index = torch.stack([torch.randperm(6, generator=g)[:2].sort().values
                         for _ in range(15)]).reshape(-1).to(torch.int32)
    value = torch.randn(30, generator=g)
    qid = torch.tensor([7] * 5 + [3] + [9] * 4 + [7] * 5, dtype=torch.int64)
    return {"offset": offset, "index": index, "value": value, "qid": qid,
            "label": torch.tensor(LABEL, dtype=torch.float32)}


def test_host_loss_and_ndcg_use_the_reference():
    csr = _host_csr()
    model = SparseRanker(6)
    with torch.no_grad():
        model.weight.copy_(torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4, 0.25]))
    ptr = [0, 5, 6, 10, 15]  # a qid that comes back (7) starts a new group
    for weighting in ("ndcg", "none"):
        model.zero_grad()
        loss = model.loss(csr, weighting=weighting, sigma=2.0)
        assert csr["_group_ptr"][1].tolist() == ptr
        loss.backward()
        score = model(csr).detach()
        want, grad = _loop_loss(score.double().tolist(), LABEL, ptr, weighting, 2.0)
        assert abs(float(loss.detach()) - want) <= 1e-5 * want
        dw = data.to_sparse_csr(csr, 6).to_dense().double().t() @ torch.tensor(grad, dtype=torch.float64)
        assert (model.weight.grad.double() - dw).abs().max() <= 1e-5 * dw.abs().max()
    want = _loop_ndcg(model(csr).detach().double().tolist(), LABEL, ptr, 10)
    assert abs(float(model.ndcg(csr, k=10)) - sum(want) / len(want)) <= 1e-6
    # an explicit group_ptr wins over qid
    explicit = dict(csr, group_ptr=torch.tensor([0, 15]))
    want, _ = _loop_loss(model(csr).detach().double().tolist(), LABEL, [0, 15], "none", 1.0)
    assert abs(float(model.loss(explicit, weighting="none").detach()) - want) <= 1e-5 * want
    with pytest.raises(ValueError, match="qid"):
        model.loss({k: v for k, v in csr.items() if k not in ("qid", "_group_ptr")})


def test_group_rows_matches_a_loop():
    ptr = torch.tensor([2, 7, 7, 8, 12, 17])
    for sel in ([3, 0, 0, 1, 4], [], [1], [2, 2]):
        rows, batch_ptr = ops.group_rows(ptr, torch.tensor(sel, dtype=torch.int64))
        want, want_ptr = [], [0]
        for g in sel:
            want += list(range(int(ptr[g]), int(ptr[g + 1])))
            want_ptr.append(len(want))
        assert rows.dtype == torch.int64 and batch_ptr.dtype == torch.int64
        assert rows.tolist() == want and batch_ptr.tolist() == want_ptr
    assert ops.group_rows(ptr, torch.tensor([4, 1], dtype=torch.int32))[0].tolist() == \
        list(range(12, 17)) + list(range(7, 7))
    with pytest.raises(ValueError, match="group_ptr"):
        ops.group_rows(ptr.float(), torch.tensor([0]))
    with pytest.raises(ValueError, match="groups"):
        ops.group_rows(ptr, torch.tensor([0.0]))


def test_argument_checks_raise_before_any_launch():
    s, lab, ptr = torch.zeros(4), torch.zeros(4), torch.tensor([0, 4])
    bad = [
        (dict(score=s.double()), "float32"),
        (dict(label=lab.long()), "float32"),
        (dict(score=torch.zeros(4, 1)), "1-D"),
        (dict(score=torch.zeros(8)[::2]), "contiguous"),
        (dict(label=torch.zeros(8)[::2]), "contiguous"),
        (dict(label=torch.zeros(5)), "entries"),
        (dict(group_ptr=ptr.int()), "int64"),
        (dict(group_ptr=torch.zeros(0, dtype=torch.int64)), "group_ptr"),
        (dict(group_ptr=torch.tensor([[0, 4]])), "group_ptr"),
        (dict(group_ptr=torch.tensor([0, 1, 2, 4])[::2]), "contiguous"),
        (dict(score=[0.0] * 4), "tensor"),
        (dict(), "device"),  # everything right but on the host
    ]
    for fn in (ops.rank_loss, ops.rank_loss_parts, ops.ndcg):
        for change, match in bad:
            args = dict(score=s, label=lab, group_ptr=ptr)
            args.update(change)
            with pytest.raises(ValueError, match=match):
                fn(**args)
    for fn in (ops.rank_loss, ops.rank_loss_parts):
        with pytest.raises(ValueError, match="weighting"):
            fn(s, lab, ptr, weighting="lambda")
        for sigma in (0.0, -1.0, float("nan"), "1"):
            with pytest.raises(ValueError, match="sigma"):
                fn(s, lab, ptr, sigma=sigma)
    for k in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ops.ndcg(s, lab, ptr, k=k)
    for qid, match in ((torch.zeros(4, dtype=torch.int32), "64-bit"), (torch.zeros(4), "64-bit"),
                       (torch.zeros((2, 2), dtype=torch.int64), "1-D"), ([1, 2], "1-D"),
                       (torch.zeros(4, dtype=torch.int64), "device")):
        with pytest.raises(ValueError, match=match):
            ops.qid_groups(qid)


def test_extension_constants_and_zero_group_launches():
    cap = _dmlc.rank_wave_group_rows()
    assert isinstance(cap, int) and cap >= 64
    assert _dmlc.rank_tile_rows() >= 64 and _dmlc.rank_max_label() == 31
    assert (_dmlc.rank_err_group, _dmlc.rank_err_label) == (1, 2)
    assert (ops._RANK_ERR_GROUP, ops._RANK_ERR_LABEL) == (1, 2)
    # no groups / no rows: accepted with null pointers, nothing is launched
    _dmlc.rank_loss(0, 0, 0, 0, 0, True, 1.0, 0, 0, 0, 0, 0, 0)
    _dmlc.rank_loss(0, 0, 0, 0, 0, False, 2.5, 0, 0, 0, 0, 0, 0)
    _dmlc.rank_ndcg(0, 0, 0, 0, 0, 10, 0, 0, 0)
    _dmlc.qid_group_ptr(0, 0, 0, 0, 0, 0, 0)
    assert _dmlc.qid_scan_words(0) >= 1 and _dmlc.qid_scan_words(5000) >= 3
