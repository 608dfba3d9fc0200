"""Q1 / Q2 and RK1 / RK2 (src/gpu/rank_kernels.hip) through ops.qid_groups,
ops.rank_loss_parts / rank_loss / ndcg and SparseRanker, against the
definitions (ops.rank_loss_parts' docstring) evaluated in float64 with numpy in
this file -- not against SparseRanker.reference.

Bound, of the form test_gpu_ffm.py derives: an output is a sum of T terms,

    |got - ref| <= (T + C) * 2^-23 * M

with M the float64 sum of |term|.  T: |P| for loss_g; for grad[i] the rows j of
the group with l_j != l_i.  For weighting="ndcg" M is formed with D(r_i) +
D(r_j) in place of |D(r_i) - D(r_j)|: the difference of two rounded discounts
cancels, its absolute error stays a few ulps of D.

C counts the kernel's f32 arithmetic per term in units of 2^-23 (u; a
correctly rounded operation is 0.5 u).  ASSUMPTION: the ROCm install carries no
table of the device library's errors, so the counts below take expf, log1pf
and log2f at 1 ulp (the figures the HIP math documentation publishes) and f32
division as correctly rounded (hipcc's default).
  x = sigma * (s_i - s_j)            1 u on x, which reaches the term through
      exp(-x): relative |x| u where exp(-|x|) is a nonzero f32, |x| < 104    104
  expf 1, log1pf 1, max(-x, 0) + log1p 0.5 (loss) / 1 + e 0.5, e / (1 + e)
      0.5 (gradient)                                                         2.5
  w: G_i, G_j one rounding each and their difference (l_i > l_j: G_i - G_j
      >= G_i / 2) 2; D = 1 / log2f(2 + r) 1.5 each, |D_i - D_j| against D_i +
      D_j 2; IDCG (f64 sum of G D, one cast) 2.5; 1 / IDCG 0.5; two products 1   8
  w * term 0.5; |P| -> f32 0.5; sum / |P| 0.5 (loss) / sigma / |P| 0.5 and the
      product with the sum 0.5 (gradient)                                      2
C_LOSS = 116.5 and C_GRAD = 117; both use C = 117.  A pair whose exp(-|x|)
underflows f32 (|x| > 104: the +-100 group) contributes its own value, below
2^-149 w, as an absolute error; the bound holds it because every row of that
group also has a pair that does not underflow (asserted where the data is made).
NDCG: both sums are f64 on the device, so the terms carry G 0.5 + D 1.5 = 2 u
in the numerator and in the denominator and the quotient's cast 0.5: C_NDCG = 5
with T = the terms of both sums and M the value itself.
Through autograd the gradient is multiplied by upstream / groups-with-pairs
(1 / count 0.5, two products 1, the upstream's own rounding 0.5): C + 2.
No other tolerance appears in this file, except the 1e-4 the end-to-end test is
given.

Groups: lengths 0, 1, 2, 3, 63, 64, 65, CAP - 1, CAP, CAP + 1 (CAP =
_dmlc.rank_wave_group_rows(), where RK1 hands over to RK2), one of 2 * (RK2's
tile) + 77 rows, the special groups below and 120 random lengths in 0 .. 40;
their number is not a multiple of 4, RK1's groups per workgroup.  group_ptr
starts at row 5 and ends 7 rows before the end."""
import functools

import numpy as np
import pytest
import torch

from dmlc_core_amd import _dmlc, data, ops
from dmlc_core_amd.models import SparseRanker

pytestmark = pytest.mark.gpu
U23 = 2.0 ** -23
C = 117.0
C_NDCG = 5.0
CAP = int(_dmlc.rank_wave_group_rows())
TILE = int(_dmlc.rank_tile_rows())
LENS = [0, 1, 2, 3, 63, 64, 65, CAP - 1, CAP, CAP + 1, 2 * TILE + 77]
G_EQUAL_SCORES, G_BIG_SCORES, G_EQUAL_LABELS, G_WIDE_LABELS = (len(LENS) + i for i in range(4))
SPECIAL = [30, 40, 20, 12]
HEAD, TAIL = 5, 7
WEIGHTINGS = ["ndcg", "none"]
SIGMAS = [1.0, 2.5]


@functools.lru_cache(maxsize=None)
def _host():
    """score, label, group_ptr (numpy)"""
    rng = np.random.default_rng(29)
    lens = np.array(LENS + SPECIAL + rng.integers(0, 41, 120).tolist(), np.int64)
    assert len(lens) % 4 != 0
    ptr = HEAD + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(ptr[-1]) + TAIL
    score = rng.standard_normal(rows).astype(np.float32)
    label = rng.integers(0, 5, rows).astype(np.float32)
    eight = rng.standard_normal(8).astype(np.float32)
    for g in range(0, len(lens), 3):  # ties are common in every third group
        b, e = ptr[g], ptr[g + 1]
        score[b:e] = eight[rng.integers(0, 8, e - b)]
    b, e = ptr[G_EQUAL_SCORES], ptr[G_EQUAL_SCORES + 1]
    score[b:e] = 0.75
    b, e = ptr[G_BIG_SCORES], ptr[G_BIG_SCORES + 1]
    score[b:e] = np.where(rng.integers(0, 2, e - b) == 1, 100.0, -100.0)
    # every row of the +-100 group has a pair that does not underflow: a tie
    # with another label, or a row above it in label and below it in score
    s, lab = score[b:e], label[b:e]
    other = lab[:, None] != lab[None, :]
    alive = (other & (s[:, None] == s[None, :])) | \
        ((lab[None, :] > lab[:, None]) & (s[None, :] < s[:, None])) | \
        ((lab[None, :] < lab[:, None]) & (s[None, :] > s[:, None]))
    assert alive.any(1).all()
    b, e = ptr[G_EQUAL_LABELS], ptr[G_EQUAL_LABELS + 1]
    label[b:e] = 3.0
    b, e = ptr[G_WIDE_LABELS], ptr[G_WIDE_LABELS + 1]
    label[b:e] = np.where(rng.integers(0, 2, e - b) == 1, 31.0, 0.0)
    label[b], label[b + 1] = 31.0, 0.0
    return score, label, ptr


def _ranks(key):
    """r_i = #{j : key_j > key_i, or key_j == key_i and j < i}"""
    n = len(key)
    before = np.arange(n)[None, :] < np.arange(n)[:, None]
    return ((key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & before)).sum(1)


def _valid(label, b, e, rows):
    if not 0 <= b <= e <= rows:
        return False
    lab = label[b:e]
    return bool(((lab >= 0) & (lab <= 31) & (lab == np.floor(lab))).all())


def _loss_ref(score, label, ptr, weighting, sigma):
    """loss_g, pairs_g, grad and the bounds of loss_g and grad; a group that
    the kernels refuse contributes zeros"""
    rows, groups = len(score), len(ptr) - 1
    loss, pairs = np.zeros(groups), np.zeros(groups, np.int64)
    loss_tol, grad, grad_tol = np.zeros(groups), np.zeros(rows), np.zeros(rows)
    for g in range(groups):
        b, e = int(ptr[g]), int(ptr[g + 1])
        if not _valid(label, b, e, rows):
            continue
        s, lab = score[b:e].astype(np.float64), label[b:e].astype(np.float64)
        pair = lab[:, None] > lab[None, :]
        npairs = int(pair.sum())
        pairs[g] = npairs
        if npairs == 0:
            continue
        x = sigma * (s[:, None] - s[None, :])
        ex = np.exp(-np.abs(x))
        sp = np.maximum(-x, 0) + np.log1p(ex)
        rho = np.where(x > 0, ex, 1.0) / (1 + ex)
        w = wm = np.ones_like(x)
        if weighting == "ndcg":
            gain = 2.0 ** lab - 1
            d = 1 / np.log2(2.0 + _ranks(s))
            idcg = (gain / np.log2(2.0 + _ranks(lab))).sum()
            dg = np.abs(gain[:, None] - gain[None, :]) / idcg
            w, wm = dg * np.abs(d[:, None] - d[None, :]), dg * (d[:, None] + d[None, :])
        loss[g] = (w * sp * pair).sum() / npairs
        loss_tol[g] = (npairs + C) * U23 * (wm * sp * pair).sum() / npairs
        grad[b:e] = sigma / npairs * (-(w * rho * pair).sum(1) + (w * rho * pair).sum(0))
        mag = sigma / npairs * ((wm * rho * pair).sum(1) + (wm * rho * pair).sum(0))
        grad_tol[b:e] = (pair.sum(1) + pair.sum(0) + C) * U23 * mag
    return loss, pairs, grad, loss_tol, grad_tol


@functools.lru_cache(maxsize=None)
def _shared_ref(weighting, sigma):
    return _loss_ref(*_host(), weighting, sigma)


def _ndcg_ref(score, label, ptr, k):
    rows, groups = len(score), len(ptr) - 1
    out, tol = np.zeros(groups), np.zeros(groups)
    for g in range(groups):
        b, e = int(ptr[g]), int(ptr[g + 1])
        if not _valid(label, b, e, rows):
            continue
        s, lab = score[b:e].astype(np.float64), label[b:e].astype(np.float64)
        kk = e - b if k is None else k
        gain = 2.0 ** lab - 1
        r, q = _ranks(s), _ranks(lab)
        dcg = (gain / np.log2(2.0 + r))[r < kk].sum()
        ideal = (gain / np.log2(2.0 + q))[q < kk].sum()
        out[g] = dcg / ideal if ideal > 0 else 1.0
        tol[g] = ((r < kk).sum() + (q < kk).sum() + C_NDCG) * U23 * out[g]
    return out, tol


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _within(got, ref, tol, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    worst = float(np.max(err / np.where(tol > 0, tol, 1.0), initial=0.0))
    print(what, "largest error / bound = %.3g" % worst)
    bad = ~(err <= tol)  # a NaN (unwritten output) is bad
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5], tol[bad][:5])


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_rank_loss_parts_match_the_definition(weighting, sigma):
    score, label, ptr = _host()
    loss, pairs, grad, loss_tol, grad_tol = _shared_ref(weighting, sigma)
    s, lab, p = _dev(score, label, ptr)
    got = ops.rank_loss_parts(s, lab, p, weighting, sigma)
    assert [t.dtype for t in got] == [torch.float32, torch.int64, torch.float32]
    what = (weighting, sigma)
    assert np.array_equal(got[1].cpu().numpy(), pairs), what
    _within(got[0], loss, loss_tol, what + ("loss",))
    _within(got[2], grad, grad_tol, what + ("grad",))
    # rows outside every group, the group without pairs, groups of 0 and 1 rows
    g = got[2].cpu().numpy()
    assert not g[:HEAD].any() and not g[-TAIL:].any()
    assert not g[ptr[G_EQUAL_LABELS]:ptr[G_EQUAL_LABELS + 1]].any()
    assert pairs[G_EQUAL_LABELS] == 0 and float(got[0][G_EQUAL_LABELS]) == 0.0
    assert not got[0][:2].any() and pairs[G_BIG_SCORES] > 0 and pairs[G_WIDE_LABELS] > 0
    # the same bytes from a second run, and without the read
    for again in (ops.rank_loss_parts(s, lab, p, weighting, sigma),
                  ops.rank_loss_parts(s, lab, p, weighting, sigma, validate=False)):
        assert all(torch.equal(a, b) for a, b in zip(got, again)), what


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_rank_loss_autograd(weighting):
    """the scalar and, for an upstream factor of 0.375, the gradient"""
    sigma, up = 2.5, 0.375
    score, label, ptr = _host()
    loss, pairs, grad, loss_tol, grad_tol = _shared_ref(weighting, sigma)
    s, lab, p = _dev(score, label, ptr)
    s.requires_grad_()
    out = ops.rank_loss(s, lab, p, weighting, sigma)
    assert out.shape == () and out.dtype == torch.float32
    count = max(1, int((pairs > 0).sum()))
    ref = loss.sum() / count
    # the per-group bounds, and the sum over the groups and the division
    tol = loss_tol.sum() / count + (len(loss) + 2) * U23 * ref
    _within(out.reshape(1), np.array([ref]), np.array([tol]), (weighting, "loss"))
    (out * up).backward()
    scale = up / count
    extra = 2 * U23 * np.abs(grad) * scale  # C + 2 in place of C: M >= |grad|
    _within(s.grad, grad * scale, grad_tol * scale + extra, (weighting, "autograd"))


@pytest.mark.parametrize("k", [1, 5, 10, None])
def test_ndcg_matches_the_definition(k):
    score, label, ptr = _host()
    ref, tol = _ndcg_ref(score, label, ptr, k)
    s, lab, p = _dev(score, label, ptr)
    got = ops.ndcg(s, lab, p, k)
    assert got.dtype == torch.float32
    _within(got, ref, tol, ("ndcg", k))
    assert torch.equal(got, ops.ndcg(s, lab, p, k, validate=False))
    assert float(got[0]) == 1.0  # no rows
    zeros = torch.zeros_like(lab)
    assert torch.equal(ops.ndcg(s, zeros, p, k), torch.ones_like(got))  # only label 0: exactly 1


def test_qid_groups_matches_numpy():
    rng = np.random.default_rng(3)
    cases = [np.arange(700, dtype=np.uint64),                       # runs of length 1
             np.full(300, 5, np.uint64),                            # one run
             np.array([7, 7, 3, 7, 7, 7, 9], np.uint64),            # 7 comes back
             np.array([4], np.uint64),
             np.repeat(rng.integers(0, 50, 900), rng.integers(1, 12, 900)).astype(np.uint64),
             np.repeat(np.array([2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 63 - 1, 2 ** 63], np.uint64),
                       [3, 1, 2, 4, 1])]
    assert cases[4].size > 2048  # more than one tile of the scan
    for q in cases:
        want = np.concatenate([np.flatnonzero(np.concatenate([[True], q[1:] != q[:-1]])), [q.size]])
        for view in (q.view(np.int64), q):
            ptr = ops.qid_groups(torch.from_numpy(view.copy()).cuda())
            assert ptr.dtype == torch.int64 and ptr.is_cuda
            assert np.array_equal(ptr.cpu().numpy(), want), q[:8]
    empty = ops.qid_groups(torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert empty.dtype == torch.int64 and empty.tolist() == [0]


@pytest.mark.parametrize("kind", ["descending", "past_rows", "negative", "fractional", "label_32"])
def test_refused_groups_are_reported_and_skipped(kind):
    """one bad group among ordinary in-bounds tensors: the call raises naming
    the check; with validate=False it returns, the group's rows have gradient
    0 and every other group matches the definition on the same operands"""
    score, label, ptr = (a.copy() for a in _host())
    g = 40  # one of the random groups
    if kind == "descending":
        g = len(ptr) - 2
        ptr[-1] = ptr[-2] - 1  # the last group ends before it starts: it has no rows
        match = "group_ptr descends"
    elif kind == "past_rows":
        g = len(ptr) - 2
        ptr[-1] = len(score) + 3
        match = "group_ptr descends or points past"
    else:
        while ptr[g + 1] - ptr[g] < 2:
            g += 1
        label[ptr[g] + 1] = {"negative": -1.0, "fractional": 1.5, "label_32": 32.0}[kind]
        match = "label is not an integer"
    s, lab, p = _dev(score, label, ptr)
    for weighting in WEIGHTINGS:
        with pytest.raises(ValueError, match=match) as info:
            ops.rank_loss_parts(s, lab, p, weighting)
        assert ("label" in str(info.value)) == (kind in ("negative", "fractional", "label_32"))
        with pytest.raises(ValueError, match=match):
            ops.rank_loss(s.clone().requires_grad_(), lab, p, weighting)
        got = ops.rank_loss_parts(s, lab, p, weighting, validate=False)
        loss, pairs, grad, loss_tol, grad_tol = _loss_ref(score, label, ptr, weighting, 1.0)
        assert pairs[g] == 0 and loss[g] == 0
        assert np.array_equal(got[1].cpu().numpy(), pairs)
        _within(got[0], loss, loss_tol, (kind, weighting, "loss"))
        _within(got[2], grad, grad_tol, (kind, weighting, "grad"))
        if kind != "descending":
            assert ptr[g + 1] - ptr[g] >= 2
            assert not got[2][int(ptr[g]):min(int(ptr[g + 1]), len(score))].any()
    with pytest.raises(ValueError, match=match):
        ops.ndcg(s, lab, p, 10)
    ref, tol = _ndcg_ref(score, label, ptr, 10)
    _within(ops.ndcg(s, lab, p, 10, validate=False), ref, tol, (kind, "ndcg"))


def _rel(got, ref):
    return abs(float(got) - float(ref)) / abs(float(ref))


def test_libsvm_file_with_qid_to_sparse_ranker(tmp_path):
    """50 queries of 5 .. 30 rows with `qid:` on every line -> GPUParser ->
    csr_to_torch -> five SGD steps of SparseRanker: at every step the device
    loss agrees with SparseRanker.reference on host copies of the same tensors
    to 1e-4 relative, and NDCG@10 does not decrease from the first step to the
    last"""
    rng = np.random.default_rng(61)
    feats = 24
    truth = rng.standard_normal(feats)
    lines = []
    for q in range(50):
        for _ in range(int(rng.integers(5, 31))):
            ids = np.sort(rng.choice(feats, 6, replace=False))
            vals = rng.standard_normal(6).round(3)
            rel = int(np.clip(np.round(1.5 + vals @ truth[ids] + 0.3 * rng.standard_normal()), 0, 4))
            lines.append("%d qid:%d %s" % (rel, 1000 + q,
                                           " ".join("%d:%.3f" % iv for iv in zip(ids, vals))))
    path = tmp_path / "rank.libsvm"
    path.write_text("\n".join(lines) + "\n")
    csr = data.GPUParser(str(path)).parse_all()
    assert csr.rows == len(lines)
    t = data.csr_to_torch(csr)
    assert t["qid"] is not None and t["qid"].numel() == len(lines)
    cpu = {k: (a.cpu() if isinstance(a, torch.Tensor) else a) for k, a in t.items()}
    dev = SparseRanker(feats).cuda()
    host = SparseRanker(feats)
    with torch.no_grad():
        dev.weight.copy_(torch.from_numpy(0.05 * rng.standard_normal(feats)).float())
    opt = torch.optim.SGD(dev.parameters(), lr=0.5)
    first = float(dev.ndcg(t, k=10))
    for step in range(5):
        host.load_state_dict({k: v.cpu() for k, v in dev.state_dict().items()})
        opt.zero_grad()
        loss = dev.loss(t)
        want = host.loss(cpu)
        assert _rel(loss.detach(), want.detach()) <= 1e-4, (step, float(loss), float(want))
        loss.backward()
        opt.step()
    assert t["_group_ptr"][1].numel() == 51 and cpu["_group_ptr"][1].tolist() == \
        t["_group_ptr"][1].tolist()
    host.load_state_dict({k: v.cpu() for k, v in dev.state_dict().items()})
    last = float(dev.ndcg(t, k=10))
    assert abs(last - float(host.ndcg(cpu, k=10))) <= 1e-4 * last
    assert last >= first, (first, last)
    # whole queries through group_rows + gather_rows: the same per-group loss, bitwise
    ptr = t["_group_ptr"][1]
    sel = torch.tensor([7, 3, 44], device="cuda")
    rows, batch_ptr = ops.group_rows(ptr, sel)
    batch = ops.gather_rows(t, rows)
    score = dev(t).detach()
    every = ops.rank_loss_parts(score, t["label"], ptr)
    part = ops.rank_loss_parts(score[rows].contiguous(), batch["label"], batch_ptr)
    assert torch.equal(part[0], every[0][sel]) and torch.equal(part[1], every[1][sel])
    assert torch.equal(part[2], every[2][rows])
