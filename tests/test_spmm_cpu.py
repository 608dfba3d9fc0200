"""ops.spmm's public surface and argument checks, and SparseSoftmaxReg /
SparseFM on host tensors (the dense formula the HIP path computes), without a
GPU; the kernels themselves run in test_gpu_spmm.py."""
import pytest
import torch

from dmlc_core_amd import models, ops
from dmlc_core_amd.models import SparseFM, SparseSoftmaxReg

ROWS, FEATS, CLASSES, RANK = 64, 50, 3, 4


def test_new_names_are_exported():
    for name in ("spmm", "spmm_t", "csr_spmm"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    for name in ("SparseSoftmaxReg", "SparseFM"):
        assert name in models.__all__ and hasattr(models, name)


def _cpu_csr(seed=0, value=True, classes=None):
    """64 x 50, 0 .. 12 distinct ids per row, labels binary or 0 .. classes-1"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 13, (ROWS,), generator=g)
    lens[3] = 0
    offset = torch.zeros(ROWS + 1, dtype=torch.int64)
    offset[1:] = torch.cumsum(lens, 0)
    index = torch.cat([torch.randperm(FEATS, generator=g)[:n] for n in lens.tolist()]).to(torch.int32)
    csr = {"offset": offset, "index": index,
           "value": torch.randn(index.numel(), generator=g) if value else None,
           "label": torch.randint(0, classes or 2, (ROWS,), generator=g).float()}
    return csr, g


def _dense64(csr):
    x = torch.zeros(ROWS, FEATS, dtype=torch.float64)
    off = csr["offset"].tolist()
    for r in range(ROWS):
        for j in range(off[r], off[r + 1]):
            x[r, int(csr["index"][j])] += 1.0 if csr["value"] is None else float(csr["value"][j])
    return x


def test_spmm_rejects_a_cpu_csr():
    csr, _ = _cpu_csr()
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.spmm(csr, torch.zeros(FEATS, 4))
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.spmm_t(csr, torch.zeros(ROWS, 4), FEATS)


@pytest.mark.parametrize("w,bias,match", [
    (torch.zeros(FEATS), None, "2-D"),
    (torch.zeros(FEATS, 4, dtype=torch.float64), None, "float32"),
    (torch.zeros(FEATS, 0), None, "columns"),
    (torch.zeros(FEATS, 257), None, "columns"),
    (torch.zeros(FEATS, 8)[:, ::2], None, "contiguous"),
    (torch.zeros(4, FEATS).t(), None, "contiguous"),
    (torch.zeros(FEATS, 4), torch.zeros(5), "bias"),
    (torch.zeros(FEATS, 4), torch.zeros(1, 4), "bias"),
], ids=["1d", "f64", "k0", "k257", "strided", "transposed", "bias_len", "bias_2d"])
def test_spmm_rejects_bad_dense_operands(w, bias, match):
    """a ValueError about the operand itself, raised before the CSR is looked
    at and before anything is launched"""
    csr, _ = _cpu_csr()
    with pytest.raises(ValueError, match=match):
        ops.spmm(csr, w, bias)
    if bias is None:
        with pytest.raises(ValueError, match=match):
            ops.spmm_t(csr, w, FEATS)


def test_csr_spmm_rejects_unknown_grad_mode():
    csr, _ = _cpu_csr()
    with pytest.raises(ValueError, match="grad must be"):
        ops.csr_spmm(csr, torch.zeros(FEATS, 4), None, grad="scatter")


def _close(got, ref):
    # f32 against f64: chains of at most 64-term f32 sums, each within 64 * 2^-24 (4e-6)
    # of its magnitude sum, on values of order 1 and below
    torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("value", [True, False])
def test_softmax_reg_cpu_matches_dense_float64(value, weighted):
    csr, g = _cpu_csr(1, value, CLASSES)
    if weighted:
        csr["weight"] = torch.rand(ROWS, generator=g) + 0.5
    m = SparseSoftmaxReg(FEATS, CLASSES)
    assert m.weight.shape == (FEATS, CLASSES) and m.bias.shape == (CLASSES,)
    assert not m.weight.any() and not m.bias.any()
    with torch.no_grad():
        m.weight.copy_(torch.randn(FEATS, CLASSES, generator=g) * 0.3)
        m.bias.copy_(torch.randn(CLASSES, generator=g))
    loss = m.loss(csr)
    loss.backward()
    w = m.weight.detach().double().requires_grad_()
    b = m.bias.detach().double().requires_grad_()
    logits = _dense64(csr) @ w + b
    _close(m(csr).detach(), logits.detach())
    ce = torch.nn.functional.cross_entropy(logits, csr["label"].long(), reduction="none")
    ref = (ce * csr["weight"].double()).mean() if weighted else ce.mean()
    ref.backward()
    _close(loss.detach(), ref.detach())
    _close(m.weight.grad, w.grad)
    _close(m.bias.grad, b.grad)


@pytest.mark.parametrize("kind", ["logistic", "squared"])
@pytest.mark.parametrize("value", [True, False])
def test_sparse_fm_cpu_matches_dense_float64(value, kind):
    csr, g = _cpu_csr(2, value)
    m = SparseFM(FEATS, rank=RANK, seed=3)
    assert m.w.shape == (FEATS, 1) and m.v.shape == (FEATS, RANK) and m.bias.shape == (1,)
    assert torch.equal(m.v, SparseFM(FEATS, rank=RANK, seed=3).v)  # seeded
    with torch.no_grad():
        m.w.copy_(torch.randn(FEATS, 1, generator=g) * 0.3)
        m.v.copy_(torch.randn(FEATS, RANK, generator=g) * 0.3)
        m.bias.fill_(0.2)
    loss = m.loss(csr, loss=kind)
    loss.backward()
    p = [t.detach().double().requires_grad_() for t in (m.w, m.v, m.bias)]
    y = SparseFM.reference(_dense64(csr), *p)
    _close(m(csr).detach(), y.detach())
    lab = csr["label"].double()
    if kind == "logistic":
        ref = torch.nn.functional.binary_cross_entropy_with_logits(y, lab)
    else:
        ref = ((y - lab) ** 2).mean()
    ref.backward()
    _close(loss.detach(), ref.detach())
    for got, want in zip((m.w.grad, m.v.grad, m.bias.grad), p):
        _close(got, want.grad)
    with pytest.raises(ValueError, match="loss must be one of"):
        m.loss(csr, loss="hinge")


@pytest.mark.parametrize("bad", [float(CLASSES), 0.5, -1.0, float("nan")])
def test_softmax_loss_rejects_bad_labels(bad):
    csr, _ = _cpu_csr(4, True, CLASSES)
    m = SparseSoftmaxReg(FEATS, CLASSES)
    m.loss(csr)  # the labels as made are fine
    csr["label"][17] = bad
    with pytest.raises(ValueError, match="labels must be integers in"):
        m.loss(csr)
