"""Models consuming the ingestion runtime.

The reference (dmlc-core) ships no model; its consumers (XGBoost, linear
learners in ps-lite/rabit) train on RowBlocks.  These demonstrators close the
loop on MI355X: device CSR from the GPU parser -> HIP SpMV / SpMM -> loss ->
gradient all-reduced over RCCL.  The tree side is
:class:`SparseGBDT`: histogram gradient boosting on the column-major binned
matrix of the same CSR.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops
from ..ops import (_stream, csr_ffm, csr_spmm, csr_spmv, hashed_dense, ndcg, qid_groups,
                   rank_loss)

__all__ = ["SparseLogReg", "HashedFM", "SparseSoftmaxReg", "SparseFM", "SparseFFM",
           "SparseRanker", "SparseGBDT"]


class SparseLogReg(torch.nn.Module):
    """Sparse logistic regression: p(y=1|x) = sigmoid(x . w + b)."""

    def __init__(self, num_features: int, grad: str = "auto"):
        super().__init__()
        self.num_features = int(num_features)
        self.grad = grad  # X^T g: "auto" / "transpose" (cached inverted index) / "atomic"
        self.weight = torch.nn.Parameter(torch.zeros(self.num_features, dtype=torch.float32))
        self.bias = torch.nn.Parameter(torch.zeros(1, dtype=torch.float32))

    def forward(self, csr) -> torch.Tensor:
        return csr_spmv(csr, self.weight, self.bias, grad=self.grad)

    def loss(self, csr) -> torch.Tensor:
        logits = self.forward(csr)
        label = csr["label"].float()
        w = csr.get("weight")
        return torch.nn.functional.binary_cross_entropy_with_logits(
            logits, label, weight=w, reduction="mean")


def _dense(csr, num_features: int) -> torch.Tensor:
    """the batch as a dense [rows, num_features] matrix (host tensors: the
    formula the HIP kernels compute, for unit tests without a GPU)"""
    from ..data import to_sparse_csr
    return to_sparse_csr(csr, num_features).to_dense()


class SparseSoftmaxReg(torch.nn.Module):
    """Multiclass (softmax) regression on raw sparse features: logits =
    X W + b with ``weight`` [F, C] and ``bias`` [C], both zero at the start;
    labels are the class ids 0 .. C-1 of a multiclass LibSVM file.  On the
    device the product is :func:`~dmlc_core_amd.ops.csr_spmm` (C up to 256,
    feature ids < F unchecked); on host tensors the same formula runs on the
    densified batch."""

    def __init__(self, num_features: int, num_classes: int, grad: str = "auto"):
        super().__init__()
        self.num_features, self.num_classes = int(num_features), int(num_classes)
        self.grad = grad  # X^T G: "auto" / "transpose" (cached inverted index) / "atomic"
        self.weight = torch.nn.Parameter(
            torch.zeros(self.num_features, self.num_classes, dtype=torch.float32))
        self.bias = torch.nn.Parameter(torch.zeros(self.num_classes, dtype=torch.float32))

    def forward(self, csr) -> torch.Tensor:
        if not csr["index"].is_cuda:
            return _dense(csr, self.num_features) @ self.weight + self.bias
        return csr_spmm(csr, self.weight, self.bias, grad=self.grad)

    def check_labels(self, label: torch.Tensor) -> None:
        """``ValueError`` unless every label is an integer in [0, C): one
        read of (min, max, all-integer) from the device"""
        if label.numel() == 0:
            return
        lab = label.double()
        lo, hi, whole = torch.stack([lab.min(), lab.max(),
                                     (lab == lab.round()).all().double()]).tolist()
        if not whole or not (0 <= lo and hi < self.num_classes):  # a NaN fails `whole`
            raise ValueError(f"labels must be integers in [0, {self.num_classes}); "
                             f"got min {lo}, max {hi}" + ("" if whole else ", not all integers"))

    def loss(self, csr, validate: bool = True) -> torch.Tensor:
        """Mean cross entropy against ``csr["label"]``; with a ``weight``
        tensor in the dict ``mean(weight * ce)`` (SparseLogReg's convention).
        ``validate`` checks the labels before any loss kernel runs: a label
        outside [0, C) or a fractional one raises ``ValueError`` instead of
        reaching torch's cross entropy (a device-side assert)."""
        label = csr["label"]
        if validate:
            self.check_labels(label)
        ce = torch.nn.functional.cross_entropy(self.forward(csr), label.long(), reduction="none")
        w = csr.get("weight")
        return (ce * w).mean() if w is not None else ce.mean()


def _squared_values(csr):
    """the dict sharing ``offset`` / ``index`` with ``csr`` and holding
    ``value ** 2``, made once per CSR dict and cached in it (it carries its own
    cached transpose); binary rows (no ``value``) are their own square"""
    value = csr.get("value")
    if value is None:
        return csr
    key = (int(value.data_ptr()), value.numel(), value._version)
    cached = csr.get("_squared")
    if cached is None or cached[0] != key:
        cached = (key, {"offset": csr["offset"], "index": csr["index"], "value": value * value})
        csr["_squared"] = cached
    return cached[1]


class SparseFM(torch.nn.Module):
    """Factorisation machine on raw feature ids (no hashing):
    ``y = b + x.w + 1/2 sum_f ((x V)_f^2 - (x^2 V^2)_f)`` with ``w`` [F, 1] and
    ``v`` [F, rank].  On the device ``x V`` is
    :func:`~dmlc_core_amd.ops.csr_spmm`, ``x.w`` and ``x^2 . rowsum(V^2)`` are
    :func:`~dmlc_core_amd.ops.csr_spmv` (the latter over the CSR with squared
    values), and autograd does the rest; rank up to 256, feature ids < F
    unchecked.  On host tensors the same formula runs on the densified batch.
    A row's feature ids are taken to be distinct, as in a LibSVM file: the
    square of a densified row is then the row's squared values."""

    def __init__(self, num_features: int, rank: int = 16, seed: int = 0):
        super().__init__()
        self.num_features, self.rank, self.seed = int(num_features), int(rank), int(seed)
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        self.w = torch.nn.Parameter(torch.zeros(self.num_features, 1))
        self.v = torch.nn.Parameter(torch.randn(self.num_features, self.rank, generator=g) * 0.01)

    def forward(self, csr) -> torch.Tensor:
        if not csr["index"].is_cuda:
            return self.reference(_dense(csr, self.num_features), self.w, self.v, self.bias)
        zero = torch.zeros(1, dtype=torch.float32, device=self.w.device)
        xv = csr_spmm(csr, self.v)
        linear = csr_spmv(csr, self.w.reshape(-1), self.bias)
        x2q = csr_spmv(_squared_values(csr), (self.v * self.v).sum(1), zero)
        return linear + 0.5 * ((xv * xv).sum(1) - x2q)

    def loss(self, csr, loss: str = "logistic") -> torch.Tensor:
        """Mean ``"logistic"`` (labels in [0, 1]) or ``"squared"`` loss against
        ``csr["label"]``, row-weighted by ``csr["weight"]`` if present
        (``mean(weight * loss)``), as :meth:`HashedFM.loss`."""
        _check_loss(loss)
        y = self.forward(csr)
        return _fm_loss(y, csr["label"], csr.get("weight"), loss)

    @staticmethod
    def reference(x: torch.Tensor, w, v, bias) -> torch.Tensor:
        """fp32 reference of the same model on a dense batch
        (:meth:`HashedFM.reference`)."""
        return HashedFM.reference(x, w, v, bias)


class SparseFFM(torch.nn.Module):
    """Field-aware factorisation machine on a LibFM batch (``field:index:value``
    entries): over a row's entries a with id ``i_a``, field ``f_a``, value ``x_a``

        y = b + sum_a x_a w[i_a] + sum_{a < b} x_a x_b <v[i_a, f_b, :], v[i_b, f_a, :]>

    with ``w`` [F, 1] and ``v`` [F, num_fields, rank] (``randn * 0.01`` from
    ``seed``, as :class:`SparseFM`).  Pairs run over entries: repeated ids in a
    row are separate entries.  On the device the pairwise term is
    :func:`~dmlc_core_amd.ops.csr_ffm` (rank a multiple of 4 up to 32; an id
    >= F or a field >= num_fields raises ``ValueError``) and the linear term
    :func:`~dmlc_core_amd.ops.csr_spmv` with its cached-transpose gradient; on
    host tensors :meth:`reference` evaluates the definition with torch ops."""

    def __init__(self, num_features: int, num_fields: int, rank: int = 4, seed: int = 0):
        super().__init__()
        self.num_features, self.num_fields = int(num_features), int(num_fields)
        self.rank, self.seed = int(rank), int(seed)
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        self.w = torch.nn.Parameter(torch.zeros(self.num_features, 1))
        self.v = torch.nn.Parameter(
            torch.randn(self.num_features, self.num_fields, self.rank, generator=g) * 0.01)

    def forward(self, csr) -> torch.Tensor:
        if not csr["index"].is_cuda:
            return self.reference(csr, self.w, self.v, self.bias)
        return csr_spmv(csr, self.w.reshape(-1), self.bias) + csr_ffm(csr, self.v)

    def loss(self, csr, loss: str = "logistic") -> torch.Tensor:
        """Mean ``"logistic"`` (labels in [0, 1]) or ``"squared"`` loss against
        ``csr["label"]``, row-weighted by ``csr["weight"]`` if present
        (``mean(weight * loss)``), as :meth:`SparseFM.loss`."""
        _check_loss(loss)
        y = self.forward(csr)
        return _fm_loss(y, csr["label"], csr.get("weight"), loss)

    @staticmethod
    def reference(csr, w, v, bias) -> torch.Tensor:
        """The model's definition on host tensors, in the dtype of ``w`` / ``v``
        (differentiable): every pair a < b of every row is listed and summed
        with ``index_add``.  A densified batch cannot stand in here, because
        the field belongs to the entry, not to the feature."""
        def signed(t):  # the parser's unsigned arrays, as torch computes with them
            if t.dtype in (torch.uint32, torch.uint64):
                t = t.view(torch.int32 if t.dtype == torch.uint32 else torch.int64)
            return t.to(torch.int64)

        off = signed(csr["offset"])
        rows = off.numel() - 1
        lo = int(off[0])
        lens = off[1:] - off[:-1]
        nnz = int(lens.sum())
        idx = signed(csr["index"])[lo:lo + nnz]
        fld = signed(csr["field"])[lo:lo + nnz]
        x = torch.ones(nnz, dtype=w.dtype) if csr.get("value") is None \
            else csr["value"][lo:lo + nnz].to(w.dtype)
        row = torch.repeat_interleave(torch.arange(rows), lens)
        y = bias + torch.zeros(rows, dtype=w.dtype).index_add(0, row, x * w[idx, 0])
        first, second, owner = [], [], []
        for r, (b, n) in enumerate(zip((off[:-1] - lo).tolist(), lens.tolist())):
            if n >= 2:
                a, c = torch.triu_indices(n, n, 1)
                first.append(a + b)
                second.append(c + b)
                owner.append(torch.full((a.numel(),), r, dtype=torch.int64))
        if first:
            a, c, owner = torch.cat(first), torch.cat(second), torch.cat(owner)
            term = x[a] * x[c] * (v[idx[a], fld[c]] * v[idx[c], fld[a]]).sum(-1)
            y = y + torch.zeros(rows, dtype=w.dtype).index_add(0, owner, term)
        return y


def _group_ptr(csr) -> torch.Tensor:
    """``csr["group_ptr"]`` if the dict has one; else the pointer of
    ``csr["qid"]``'s runs, made once per qid tensor and cached in the dict
    (keyed as :func:`_squared_values` keys its cache)"""
    ptr = csr.get("group_ptr")
    if ptr is not None:
        return ptr
    qid = csr.get("qid")
    if not isinstance(qid, torch.Tensor):
        raise ValueError("SparseRanker: csr has neither 'group_ptr' nor a 'qid' tensor "
                         "(parse a LibSVM file with qid: tokens)")
    key = (int(qid.data_ptr()), qid.numel(), qid._version)
    cached = csr.get("_group_ptr")
    if cached is None or cached[0] != key:
        if qid.is_cuda:
            ptr = qid_groups(qid)
        else:
            q = qid.view(torch.int64) if qid.dtype == torch.uint64 else qid
            start = torch.ones(q.numel(), dtype=torch.bool)
            start[1:] = q[1:] != q[:-1]
            ptr = torch.cat([torch.nonzero(start).reshape(-1),
                             torch.tensor([q.numel()])]).to(torch.int64)
        cached = (key, ptr)
        csr["_group_ptr"] = cached
    return cached[1]


class SparseRanker(torch.nn.Module):
    """Linear learning to rank on the query groups of a LibSVM file with
    ``qid:`` tokens: score = x . w, trained with the pairwise loss of
    :func:`~dmlc_core_amd.ops.rank_loss` -- RankNet (``weighting="none"``) or
    LambdaRank (``"ndcg"``) -- over the pairs of every group.  There is no
    trainable bias: a bias cancels in every pair.  Labels are integer
    relevance grades in [0, 31]; row weights (``csr["weight"]``) are not used.
    On the device the score is :func:`~dmlc_core_amd.ops.csr_spmv` (``grad``
    as there) and the loss the HIP kernels RK1 / RK2; on host tensors
    :meth:`reference` evaluates the definitions with torch ops."""

    def __init__(self, num_features: int, grad: str = "auto"):
        super().__init__()
        self.num_features = int(num_features)
        self.grad = grad  # X^T g: "auto" / "transpose" (cached inverted index) / "atomic"
        self.weight = torch.nn.Parameter(torch.zeros(self.num_features, dtype=torch.float32))

    def forward(self, csr) -> torch.Tensor:
        if not csr["index"].is_cuda:
            return _dense(csr, self.num_features) @ self.weight
        zero = torch.zeros(1, dtype=torch.float32, device=self.weight.device)
        return csr_spmv(csr, self.weight, zero, grad=self.grad)

    def loss(self, csr, weighting: str = "ndcg", sigma: float = 1.0,
             validate: bool = True) -> torch.Tensor:
        """Mean over the groups that have a pair of the pairwise loss against
        ``csr["label"]``.  The groups are ``csr["group_ptr"]`` if present, else
        the runs of ``csr["qid"]`` (:func:`~dmlc_core_amd.ops.qid_groups`,
        cached in the dict)."""
        ptr = _group_ptr(csr)
        score = self.forward(csr)
        if not score.is_cuda:
            return self.reference(score, csr["label"], ptr, weighting, sigma)
        return rank_loss(score, csr["label"], ptr, weighting, sigma, validate)

    @torch.no_grad()
    def ndcg(self, csr, k: Optional[int] = 10) -> torch.Tensor:
        """Mean NDCG@k over the groups (a group without a relevant row counts 1.0)"""
        ptr = _group_ptr(csr)
        score = self.forward(csr)
        if not score.is_cuda:
            return self.reference_ndcg(score, csr["label"], ptr, k).mean()
        return ndcg(score, csr["label"], ptr, k).mean()

    @staticmethod
    def _ranks(key: torch.Tensor) -> torch.Tensor:
        """0-based positions in a stable descending sort of ``key``"""
        order = torch.sort(key, descending=True, stable=True).indices
        pos = torch.empty_like(order)
        pos[order] = torch.arange(order.numel())
        return pos

    @staticmethod
    def reference(score, label, group_ptr, weighting: str = "ndcg", sigma: float = 1.0):
        """The loss's definition (:func:`~dmlc_core_amd.ops.rank_loss_parts`)
        on host tensors, with torch ops in the dtype of ``score``,
        differentiable in ``score``: every group's pairs as an [n, n] mask."""
        if weighting not in ("ndcg", "none"):
            raise ValueError(f"weighting must be 'ndcg' or 'none', got {weighting!r}")
        dt = score.dtype
        total, counted = torch.zeros((), dtype=dt), 0
        for b, e in zip(group_ptr[:-1].tolist(), group_ptr[1:].tolist()):
            s, lab = score[b:e], label[b:e].to(dt)
            pair = lab[:, None] > lab[None, :]
            npairs = int(pair.sum())
            if npairs == 0:
                continue
            x = sigma * (s[:, None] - s[None, :])
            term = torch.nn.functional.softplus(-x)
            if weighting == "ndcg":
                gain = torch.exp2(lab) - 1
                disc = 1 / torch.log2(2 + SparseRanker._ranks(s.detach()).to(dt))
                ideal = (gain / torch.log2(2 + SparseRanker._ranks(lab).to(dt))).sum()
                term = term * ((gain[:, None] - gain[None, :]).abs()
                               * (disc[:, None] - disc[None, :]).abs() / ideal)
            total = total + (term * pair).sum() / npairs
            counted += 1
        return total / max(1, counted)

    @staticmethod
    def reference_ndcg(score, label, group_ptr, k: Optional[int] = None) -> torch.Tensor:
        """NDCG@k of every group on host tensors (:func:`~dmlc_core_amd.ops.ndcg`),
        in the dtype of ``score``"""
        dt = score.dtype
        out = []
        for b, e in zip(group_ptr[:-1].tolist(), group_ptr[1:].tolist()):
            s, lab = score[b:e].detach(), label[b:e].to(dt)
            kk = e - b if k is None else k
            gain = torch.exp2(lab) - 1
            r, q = SparseRanker._ranks(s), SparseRanker._ranks(lab)
            dcg = (gain / torch.log2(2 + r.to(dt)))[r < kk].sum()
            ideal = (gain / torch.log2(2 + q.to(dt)))[q < kk].sum()
            out.append(dcg / ideal if float(ideal) > 0 else torch.ones((), dtype=dt))
        return torch.stack(out) if out else torch.zeros(0, dtype=dt)


class _HashedFMFunction(torch.autograd.Function):
    """HashedFM forward / backward as two HIP kernels over the fp8 batch
    (src/gpu/fm_kernels.hip): F1 reads the batch once and writes y and xV,
    F2 reads it once more and writes per-block partials of G^T X and
    (X^2)^T g, F3/F4 sum them and form dw, dV; no fp32 / bf16 copy of the
    batch exists."""

    @staticmethod
    def forward(ctx, x8, sx: float, w, v, bias):
        rows, dim = x8.shape
        dev = x8.device
        # F0: [w | V]^T in bf16 and q = rowsum(V^2), one kernel
        wf = w.detach().float().contiguous()
        vf = v.detach().float().contiguous()
        wt = torch.empty((v.shape[1] + 1, dim), dtype=torch.bfloat16, device=dev)
        q = torch.empty(dim, dtype=torch.float32, device=dev)
        _dmlc().fm_prep(wf.data_ptr(), vf.data_ptr(), dim, wt.data_ptr(), q.data_ptr(), _stream())
        b = bias.detach().float().contiguous()
        y = torch.empty(rows, dtype=torch.float32, device=dev)
        xv = torch.empty((rows, v.shape[1]), dtype=torch.float32, device=dev)
        _dmlc().fm_forward(x8.data_ptr(), rows, dim, wt.data_ptr(), q.data_ptr(), b.data_ptr(),
                           float(sx), y.data_ptr(), xv.data_ptr(), _num_cus(dev), _stream())
        ctx.save_for_backward(x8, xv, v.detach())
        ctx.sx = float(sx)
        return y

    @staticmethod
    def backward(ctx, gy):
        x8, xv, v = ctx.saved_tensors
        rows, dim = x8.shape
        g = gy.detach().float().contiguous()
        nblk = max(1, min(2 * _num_cus(x8.device), (rows + 31) // 32))
        part = torch.empty((nblk, v.shape[1] + 2, dim), dtype=torch.float32, device=x8.device)
        _dmlc().fm_backward(x8.data_ptr(), rows, dim, g.data_ptr(), xv.data_ptr(), nblk,
                            part.data_ptr(), _stream())
        # F3 + F4: partials summed and turned into dw, dV on the device
        vf = v.float().contiguous()
        z = torch.empty((v.shape[1] + 2, dim), dtype=torch.float32, device=x8.device)
        gw = torch.empty((dim, 1), dtype=torch.float32, device=x8.device)
        gv = torch.empty((dim, v.shape[1]), dtype=torch.float32, device=x8.device)
        _dmlc().fm_reduce_grads(part.data_ptr(), nblk, dim, vf.data_ptr(), ctx.sx, z.data_ptr(),
                                gw.data_ptr(), gv.data_ptr(), _stream())
        return None, None, gw.to(v.dtype), gv.to(v.dtype), g.sum().reshape(1)


class SparseGBDT:
    """Histogram gradient-boosted trees on a device CSR (the XGBoost ``hist``
    method on sparse rows): quantile cuts and 8-bit bins once
    (:func:`~dmlc_core_amd.ops.feature_cuts`,
    :func:`~dmlc_core_amd.ops.bin_features`), then per tree level
    :func:`~dmlc_core_amd.ops.grad_histogram` ->
    :func:`~dmlc_core_amd.ops.best_splits` ->
    :func:`~dmlc_core_amd.ops.advance_rows`.  An absent entry is a missing
    value and follows each split's learnt default side.  Device only: a host
    CSR raises ``ValueError``.

    Growth is depth-wise.  A tree is four tensors in heap layout (the children
    of node i are 2i + 1 and 2i + 2) of ``2**(max_depth + 1) - 1`` nodes:
    ``feature`` int64 (-1: a leaf), ``bin`` int32 (go left when the entry's bin
    is ``<= bin``; the float threshold is ``cut[cut_ptr[feature] + bin]``),
    ``default_left`` bool and ``leaf`` float32, ``-lr G / (H + lambda)`` of the
    node's rows.  Level d is the node window ``first_node = 2**d - 1``,
    ``num_nodes = 2**d``; rows of a node that did not split stay on its id,
    outside every deeper window.  Objectives: ``"logistic"`` (labels in
    [0, 1], margins are logits) and ``"squared"``; margins start at 0.
    Gradients are summed as 64-bit fixed point, so a run is reproducible bit
    for bit."""

    def __init__(self, num_features: int, max_bins: int = 256, max_depth: int = 6,
                 learning_rate: float = 0.3, reg_lambda: float = 1.0, gamma: float = 0.0,
                 min_child_weight: float = 1.0, objective: str = "logistic"):
        if objective not in ("logistic", "squared"):
            raise ValueError(f"objective must be 'logistic' or 'squared', got {objective!r}")
        if not 1 <= int(max_depth) <= 14:
            raise ValueError(f"max_depth must be in [1, 14], got {max_depth!r}")
        if not float(reg_lambda) > 0:
            raise ValueError(f"reg_lambda must be > 0, got {reg_lambda!r}")
        self.num_features, self.max_bins = int(num_features), int(max_bins)
        self.max_depth, self.learning_rate = int(max_depth), float(learning_rate)
        self.reg_lambda, self.gamma = float(reg_lambda), float(gamma)
        self.min_child_weight, self.objective = float(min_child_weight), objective
        self.cuts = None    # feature_cuts of the training data
        self.trees = []     # dicts of feature / bin / default_left / leaf
        self.margin = None  # the training rows' margins, updated by boost()

    @staticmethod
    def _device_csr(csr) -> None:
        if not csr["index"].is_cuda:
            raise ValueError("SparseGBDT runs on a device CSR (csr_to_torch of a GPU parse)")

    def _gradients(self, margin, label, weight):
        if self.objective == "logistic":
            p = torch.sigmoid(margin)
            g, h = p - label, p * (1.0 - p)
        else:
            g, h = margin - label, torch.ones_like(margin)
        if weight is not None:
            g, h = g * weight, h * weight
        return g.contiguous(), h.contiguous()

    def loss(self, margin: torch.Tensor, label: torch.Tensor, weight=None) -> torch.Tensor:
        """the objective's mean loss of ``margin`` (``mean(weight * loss)``)"""
        return _fm_loss(margin, label, weight, self.objective)

    def fit(self, csr, rounds: int) -> "SparseGBDT":
        """Cuts and bins of ``csr`` once, then ``rounds`` trees against
        ``csr["label"]`` (row-weighted by ``csr["weight"]`` if present)."""
        self._device_csr(csr)
        self.cuts = ops.feature_cuts(csr, self.num_features, self.max_bins)
        binned = ops.bin_features(csr, self.cuts, self.num_features)
        self.trees, self.margin = [], None
        label, weight = csr["label"].float(), csr.get("weight")
        for _ in range(int(rounds)):
            self.boost(binned, label, weight)
        return self

    def boost(self, binned, label: torch.Tensor, weight=None) -> torch.Tensor:
        """Grow one tree on ``binned`` and return the updated training margins
        (kept in ``self.margin``; they start at 0)."""
        rows, dev = int(binned["rows"]), binned["row"].device
        if self.cuts is None:
            self.cuts = {"cut_ptr": binned["cut_ptr"], "cut": binned["cut"]}
        if self.margin is None:
            self.margin = torch.zeros(rows, dtype=torch.float32, device=dev)
        elif self.margin.numel() != rows:
            raise ValueError(f"SparseGBDT.boost: the model tracks the margins of "
                             f"{self.margin.numel()} training rows, binned has {rows}: the trees "
                             "were grown on another matrix (fit() starts a new model)")
        label = label.to(device=dev, dtype=torch.float32)
        g, h = self._gradients(self.margin, label, weight)
        scale = ops.gradient_scale(g, h)
        qgh = torch.stack([torch.round(g.double() * scale), torch.round(h.double() * scale)],
                          1).long()
        size = 2 ** (self.max_depth + 1) - 1
        tree = {"feature": torch.full((size,), -1, dtype=torch.int64, device=dev),
                "bin": torch.zeros(size, dtype=torch.int32, device=dev),
                "default_left": torch.zeros(size, dtype=torch.bool, device=dev),
                "leaf": torch.zeros(size, dtype=torch.float32, device=dev)}
        pos = torch.zeros(rows, dtype=torch.int32, device=dev)
        for depth in range(self.max_depth + 1):
            first, n = 2 ** depth - 1, 2 ** depth
            ids = torch.arange(first, first + n, dtype=torch.int32, device=dev)
            node = pos.long() - first
            live = (node >= 0) & (node < n)
            node_sum = torch.zeros((n, 2), dtype=torch.int64, device=dev)
            node_sum.index_add_(0, node[live], qgh[live])
            sums = node_sum.double() / scale
            tree["leaf"][first:first + n] = \
                (-self.learning_rate * sums[:, 0] / (sums[:, 1] + self.reg_lambda)).float()
            if depth == self.max_depth:
                break
            hist = ops.grad_histogram(binned, g, h, pos, n, scale, first_node=first)
            split = ops.best_splits(hist, node_sum, binned["cut_ptr"], scale, self.reg_lambda,
                                    self.gamma, self.min_child_weight)
            for k in ("feature", "bin", "default_left"):
                tree[k][first:first + n] = split[k]
            pos = ops.advance_rows(binned, pos, split, *self._children(split, ids), first_node=first)
        self.trees.append(tree)
        self.margin = self.margin + tree["leaf"][pos.long()]
        return self.margin

    @staticmethod
    def _children(split, ids):
        """the ids a level's rows move to: 2i + 1 / 2i + 2, a leaf's rows stay on i"""
        is_leaf = split["feature"] < 0
        return (torch.where(is_leaf, ids, 2 * ids + 1).contiguous(),
                torch.where(is_leaf, ids, 2 * ids + 2).contiguous())

    def predict(self, csr) -> torch.Tensor:
        """The margins of the rows of ``csr`` (logits under ``"logistic"``):
        binned with the stored cuts, walked down every tree level by level."""
        self._device_csr(csr)
        if self.cuts is None:
            raise ValueError("SparseGBDT.predict: the model has no cuts (fit or boost first)")
        binned = ops.bin_features(csr, self.cuts, self.num_features)
        rows, dev = int(binned["rows"]), binned["row"].device
        margin = torch.zeros(rows, dtype=torch.float32, device=dev)
        for tree in self.trees:
            pos = torch.zeros(rows, dtype=torch.int32, device=dev)
            for depth in range(self.max_depth):
                first, n = 2 ** depth - 1, 2 ** depth
                ids = torch.arange(first, first + n, dtype=torch.int32, device=dev)
                split = {k: tree[k][first:first + n].contiguous()
                         for k in ("feature", "bin", "default_left")}
                pos = ops.advance_rows(binned, pos, split, *self._children(split, ids),
                                       first_node=first)
            margin = margin + tree["leaf"][pos.long()]
        return margin


_FM_LOSSES = {"logistic": 0, "squared": 1}


def _check_loss(loss: str) -> None:
    if loss not in _FM_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_FM_LOSSES)}, got {loss!r}")


def _fm_loss(y: torch.Tensor, label: torch.Tensor, weight: Optional[torch.Tensor],
             loss: str) -> torch.Tensor:
    """mean ``loss`` (one of ``_FM_LOSSES``) of the logits ``y`` against
    ``label``, row-weighted by ``weight`` if given (``mean(weight * loss)``)"""
    lab = label.to(y.dtype)
    if loss == "logistic":
        return torch.nn.functional.binary_cross_entropy_with_logits(y, lab, weight=weight)
    err = (y - lab) ** 2
    return (err * weight).mean() if weight is not None else err.mean()


class _HashedFMLossFunction(torch.autograd.Function):
    """Forward + loss + backward of one HashedFM step as one HIP kernel over
    the fp8 batch (F5 k_fm_fused, src/gpu/fm_kernels.hip), then F3/F4 for dw,
    dV.  The gradients exist after forward; backward scales them by the
    incoming gradient of the (scalar) loss."""

    @staticmethod
    def forward(ctx, x8, label, weight, sx: float, kind: int, y, w, v, bias):
        rows, dim = x8.shape
        dev = x8.device
        rank = v.shape[1]
        wf = w.detach().float().contiguous()
        vf = v.detach().float().contiguous()
        wt = torch.empty((rank + 1, dim), dtype=torch.bfloat16, device=dev)
        q = torch.empty(dim, dtype=torch.float32, device=dev)
        ext = _dmlc()
        ext.fm_prep(wf.data_ptr(), vf.data_ptr(), dim, wt.data_ptr(), q.data_ptr(), _stream())
        b = bias.detach().float().contiguous()
        lab = label.detach().to(device=dev, dtype=torch.float32).contiguous()
        wgt = None if weight is None else weight.detach().to(device=dev,
                                                             dtype=torch.float32).contiguous()
        if lab.numel() != rows or (wgt is not None and wgt.numel() != rows):
            raise ValueError("label / weight must have one value per row")
        # one workgroup per CU: eight waves of 248 VGPRs fill a CU
        nblk = max(1, min(_num_cus(dev), (rows + 31) // 32))
        part = torch.empty((nblk, rank + 2, dim), dtype=torch.float32, device=dev)
        lpart = torch.empty((nblk, 2), dtype=torch.float32, device=dev)
        ext.fm_fused(x8.data_ptr(), rows, dim, wt.data_ptr(), q.data_ptr(), b.data_ptr(), float(sx),
                     lab.data_ptr(), 0 if wgt is None else wgt.data_ptr(), int(kind), 1.0 / rows,
                     nblk, y.data_ptr(), part.data_ptr(), lpart.data_ptr(), _stream())
        z = torch.empty((rank + 2, dim), dtype=torch.float32, device=dev)
        gw = torch.empty((dim, 1), dtype=torch.float32, device=dev)
        gv = torch.empty((dim, rank), dtype=torch.float32, device=dev)
        ext.fm_reduce_grads(part.data_ptr(), nblk, dim, vf.data_ptr(), float(sx), z.data_ptr(),
                            gw.data_ptr(), gv.data_ptr(), _stream())
        sums = lpart.sum(0)
        ctx.save_for_backward(gw, gv, sums[1:2].clone())
        ctx.dtypes = (w.dtype, v.dtype, bias.dtype)
        return sums[0] / rows

    @staticmethod
    def backward(ctx, gl):
        gw, gv, gb = ctx.saved_tensors
        tw, tv, tb = ctx.dtypes
        return (None, None, None, None, None, None, (gw * gl).to(tw), (gv * gl).to(tv),
                (gb * gl).to(tb))


def _dmlc():
    from .. import _dmlc as ext
    return ext


_CUS = {}


def _num_cus(dev) -> int:
    i = dev.index if dev.index is not None else torch.cuda.current_device()
    if i not in _CUS:
        _CUS[i] = torch.cuda.get_device_properties(i).multi_processor_count
    return _CUS[i]


class HashedFM(torch.nn.Module):
    """Factorisation machine on hashed fp8 features (BASELINE config 5).

    Input: the ``[rows, dim]`` float8_e4m3fn batch of
    ``GPUParser.parse_all_hashed`` (fused tokenize -> hash -> fp8 kernel) or of
    :func:`~dmlc_core_amd.ops.hashed_dense`, with its quantisation ``scale``.
    ``y = b + x.w + 1/2 sum_f ((x V)_f^2 - (x^2 V^2)_f)``; the last term is
    ``x^2 . q`` with ``q = rowsum(V^2)``.  On a GPU (rank 16, dim a multiple of
    128 from 128 to 2048) forward and backward are the bf16-MFMA kernels of
    ``src/gpu/fm_kernels.hip``, each reading the fp8 batch once; elsewhere the
    fp32 formula runs on the dequantised batch (``self.gemm`` tells which).
    """

    def __init__(self, dim: int = 1024, rank: int = 16, seed: int = 0):
        super().__init__()
        if dim % 16 != 0:
            raise ValueError("dim must be a multiple of 16")
        self.dim, self.rank, self.seed = int(dim), int(rank), int(seed)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        self.w = torch.nn.Parameter(torch.zeros(dim, 1))
        self.v = torch.nn.Parameter(torch.randn(dim, rank) * 0.01)
        self.gemm = None
        self.last_logits = None

    def _native(self, x8: torch.Tensor) -> bool:
        return (x8.is_cuda and x8.dtype == torch.float8_e4m3fn and self.rank == 16
                and self.dim % 128 == 0 and self.dim <= 2048)

    def loss(self, x8: torch.Tensor, label: torch.Tensor, scale: float = 1.0,
             loss: str = "logistic", weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Mean training loss of the batch: ``"logistic"`` (binary cross
        entropy on the logits, labels in [0, 1]) or ``"squared"``, optionally
        row-weighted (``mean(weight * loss)``, as torch's
        ``binary_cross_entropy_with_logits(weight=...)``).

        On a GPU with dim 128 / 256 / 512 / 1024 this is one fused pass over
        the fp8 batch (``k_fm_fused``: forward, loss, dloss/dy and the
        backward products per 32-row tile, the batch read once per step
        instead of twice); its backward only scales the gradients it already
        holds.  Elsewhere: ``forward`` then the torch loss.  The logits of the
        last call are kept in ``self.last_logits``."""
        _check_loss(loss)
        if self._native(x8) and self.dim in (128, 256, 512, 1024) and x8.shape[0] > 0:
            self.gemm = "hip_mfma_bf16_fused"
            y = torch.empty(x8.shape[0], dtype=torch.float32, device=x8.device)
            out = _HashedFMLossFunction.apply(x8.contiguous(), label, weight, 1.0 / scale,
                                              _FM_LOSSES[loss], y, self.w, self.v, self.bias)
            self.last_logits = y
            return out
        y = self.forward(x8, scale)
        self.last_logits = y.detach()
        return _fm_loss(y, label, weight, loss)

    def forward(self, x8: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
        if self._native(x8):
            self.gemm = "hip_mfma_bf16"
            return _HashedFMFunction.apply(x8.contiguous(), 1.0 / scale, self.w, self.v, self.bias)
        self.gemm = "torch_fp32"
        return self.reference(x8.float() / scale, self.w, self.v, self.bias)
    @staticmethod
    def reference(x: torch.Tensor, w, v, bias) -> torch.Tensor:
        """fp32 reference of the same model on dequantised features."""
        xv = x @ v
        return bias + (x @ w).squeeze(-1) + 0.5 * (xv ** 2 - (x ** 2) @ (v ** 2)).sum(-1)
