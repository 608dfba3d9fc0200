"""ops.ffm's public surface and argument checks, and SparseFFM on host tensors
(the definition the HIP path computes), without a GPU; the kernels themselves
run in test_gpu_ffm.py."""
import pytest
import torch

from dmlc_core_amd import _dmlc, models, ops
from dmlc_core_amd.models import SparseFFM, SparseFM

ROWS, FEATS, FIELDS, RANK = 64, 50, 3, 4


def test_new_names_are_exported():
    for name in ("ffm", "ffm_t", "csr_ffm"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    assert "SparseFFM" in models.__all__ and callable(models.SparseFFM)
    for name in ("ffm_forward", "ffm_backward", "ffm_max_rank", "ffm_staged_row_entries"):
        assert callable(getattr(_dmlc, name))
    assert _dmlc.ffm_max_rank() == 32
    assert _dmlc.ffm_staged_row_entries() >= 64


def _cpu_csr(seed=0, value=True, fields=FIELDS):
    """64 x 50, 0 .. 12 distinct ids per row (as _cpu_csr of test_spmm_cpu.py)
    plus a random field per entry"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 13, (ROWS,), generator=g)
    lens[3] = 0
    offset = torch.zeros(ROWS + 1, dtype=torch.int64)
    offset[1:] = torch.cumsum(lens, 0)
    index = torch.cat([torch.randperm(FEATS, generator=g)[:n] for n in lens.tolist()]).to(torch.int32)
    csr = {"offset": offset, "index": index,
           "value": torch.randn(index.numel(), generator=g) if value else None,
           "field": torch.randint(0, fields, (index.numel(),), generator=g).to(torch.int32),
           "label": torch.randint(0, 2, (ROWS,), generator=g).float()}
    return csr, g


@pytest.mark.parametrize("v,match", [
    (torch.zeros(FEATS, 4), "3-D"),
    (torch.zeros(FEATS, FIELDS, 4, dtype=torch.float64), "float32"),
    (torch.zeros(FEATS, FIELDS, 0), "rank"),
    (torch.zeros(FEATS, FIELDS, 2), "rank"),
    (torch.zeros(FEATS, FIELDS, 6), "rank"),
    (torch.zeros(FEATS, FIELDS, 36), "rank"),
    (torch.zeros(FEATS, FIELDS, 8)[:, :, ::2], "contiguous"),
    (torch.zeros(FIELDS, FEATS, 4).transpose(0, 1), "contiguous"),
], ids=["2d", "f64", "k0", "k2", "k6", "k36", "strided", "transposed"])
def test_ffm_rejects_bad_factor_tables(v, match):
    """a ValueError about v itself, raised before the CSR's device is looked at
    (the CSR is a host one) and before anything is launched"""
    csr, _ = _cpu_csr()
    with pytest.raises(ValueError, match=match):
        ops.ffm(csr, v)
    with pytest.raises(ValueError, match=match):
        ops.ffm_t(csr, torch.zeros(ROWS), v)
    with pytest.raises(ValueError, match=match):
        ops.csr_ffm(csr, v)


def test_ffm_rejects_a_csr_without_usable_fields():
    csr, _ = _cpu_csr()
    v = torch.zeros(FEATS, FIELDS, RANK)
    g = torch.zeros(ROWS)
    for bad in ({k: t for k, t in csr.items() if k != "field"}, dict(csr, field=None)):
        with pytest.raises(ValueError, match="no 'field'"):
            ops.ffm(bad, v)
        with pytest.raises(ValueError, match="no 'field'"):
            ops.ffm_t(bad, g, v)
    other = dict(csr, field=csr["field"].long())
    with pytest.raises(ValueError, match="index's dtype"):
        ops.ffm(other, v)
    with pytest.raises(ValueError, match="index's dtype"):
        ops.ffm_t(other, g, v)


def test_ffm_rejects_a_cpu_csr():
    csr, _ = _cpu_csr()
    v = torch.zeros(FEATS, FIELDS, RANK)
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.ffm(csr, v)
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.ffm_t(csr, torch.zeros(ROWS), v)
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.csr_ffm(csr, v)


def _loop64(csr, w, v, bias):
    """the definition as a plain double loop over the pairs of every row, in
    float64, and every row's sum of |term| (what "relative" is relative to)"""
    off = csr["offset"].tolist()
    idx, fld = csr["index"].tolist(), csr["field"].tolist()
    x = [1.0] * len(idx) if csr["value"] is None else csr["value"].double().tolist()
    w, v = w.detach().double(), v.detach().double()
    y, mag = [], []
    for r in range(len(off) - 1):
        s, m = float(bias), abs(float(bias))
        for a in range(off[r], off[r + 1]):
            t = x[a] * float(w[idx[a], 0])
            s, m = s + t, m + abs(t)
            for b in range(a + 1, off[r + 1]):
                prod = v[idx[a], fld[b]] * v[idx[b], fld[a]]
                s += x[a] * x[b] * float(prod.sum())
                m += abs(x[a] * x[b]) * float(prod.abs().sum())
        y.append(s)
        mag.append(m)
    return torch.tensor(y, dtype=torch.float64), torch.tensor(mag, dtype=torch.float64)


def _model(g, fields=FIELDS):
    m = SparseFFM(FEATS, fields, rank=RANK, seed=3)
    assert m.w.shape == (FEATS, 1) and m.bias.shape == (1,)
    assert m.v.shape == (FEATS, fields, RANK)
    assert torch.equal(m.v, SparseFFM(FEATS, fields, rank=RANK, seed=3).v)  # seeded
    assert 0 < float(m.v.detach().abs().max()) < 0.1 and not m.w.any() and not m.bias.any()
    with torch.no_grad():
        m.w.copy_(torch.randn(FEATS, 1, generator=g) * 0.3)
        m.v.copy_(torch.randn(FEATS, fields, RANK, generator=g) * 0.3)
        m.bias.fill_(0.2)
    return m


@pytest.mark.parametrize("value", [True, False])
def test_sparse_ffm_cpu_forward_matches_pair_loop(value):
    csr, g = _cpu_csr(1, value)
    m = _model(g)
    ref, mag = _loop64(csr, m.w, m.v, 0.2)
    got = m(csr).detach().double()
    assert got.shape == (ROWS,)
    # host f32 torch against f64: 1e-5 of each row's sum of |term|
    assert ((got - ref).abs() <= 1e-5 * mag).all()
    # an offset slice that does not start at row 0, beside the whole entry arrays
    sl = dict(csr, offset=csr["offset"][5:41])
    assert int(sl["offset"][0]) != 0
    got = m(sl).detach().double()
    assert ((got - ref[5:40]).abs() <= 1e-5 * mag[5:40]).all()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["logistic", "squared"])
def test_sparse_ffm_cpu_loss_backward(kind, weighted):
    csr, g = _cpu_csr(2)
    if weighted:
        csr["weight"] = torch.rand(ROWS, generator=g) + 0.5
    m = _model(g)
    loss = m.loss(csr, loss=kind)
    loss.backward()
    for t in (m.w.grad, m.v.grad, m.bias.grad):
        assert t is not None and torch.isfinite(t).all() and t.abs().sum() > 0
    assert m.v.grad.shape == m.v.shape
    # the same loss from the float64 pair loop
    y, _ = _loop64(csr, m.w, m.v, 0.2)
    lab = csr["label"].double()
    if kind == "logistic":
        each = torch.nn.functional.binary_cross_entropy_with_logits(y, lab, reduction="none")
    else:
        each = (y - lab) ** 2
    ref = (each * csr["weight"].double()).mean() if weighted else each.mean()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    with pytest.raises(ValueError, match="loss must be one of"):
        m.loss(csr, loss="hinge")


@pytest.mark.parametrize("value", [True, False])
def test_one_field_ffm_is_the_plain_fm(value):
    """num_fields == 1 and distinct ids per row: the pairwise term is SparseFM's
    0.5 * ((xV)^2 - x^2 V^2).sum(-1) on the densified batch"""
    csr, g = _cpu_csr(4, value, fields=1)
    m = _model(g, fields=1)
    x = torch.zeros(ROWS, FEATS, dtype=torch.float64)
    off = csr["offset"].tolist()
    for r in range(ROWS):
        for j in range(off[r], off[r + 1]):
            x[r, int(csr["index"][j])] += 1.0 if value is False else float(csr["value"][j])
    zero_w, zero_b = torch.zeros(FEATS, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    fm = SparseFM.reference(x, zero_w, m.v.detach().double()[:, 0, :], zero_b)
    got = SparseFFM.reference(csr, zero_w.float(), m.v.detach(), zero_b.float()).double()
    assert float((got - fm).abs().max()) <= 1e-5 * float(fm.abs().max())
