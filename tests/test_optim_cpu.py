"""Row-sparse steps without a GPU: the public surface and argument checks of
ops.compact_features / ops.lazy_update_, the extension's constants and
zero-size launches, RowSparseStep's parameter substitution, and the float64
reference formulas of lazy_reference.py against torch.optim.Adagrad.  The
kernels themselves run in test_gpu_compact.py and test_gpu_lazy_optim.py."""
import pytest
import torch

from dmlc_core_amd import _dmlc, ops, optim
from dmlc_core_amd.models import SparseLogReg
from lazy_reference import adagrad64, ftrl64


def test_new_names_are_exported():
    for name in ("compact_features", "lazy_update_"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    for name in ("LazyAdagrad", "LazyFTRL", "RowSparseStep"):
        assert name in optim.__all__ and callable(getattr(optim, name))
    for name in ("compact_mark", "compact_emit", "compact_max_features", "compact_scratch_bytes",
                 "lazy_update"):
        assert callable(getattr(_dmlc, name))


def test_extension_constants():
    assert _dmlc.compact_max_features() == 2 ** 32
    assert _dmlc.compact_err_index == 1 and _dmlc.lazy_err_ids == 1
    assert (_dmlc.lazy_adagrad, _dmlc.lazy_ftrl) == (0, 1)
    # bitmap + counts (each padded to an even number of words) + scan partials + 1
    assert _dmlc.compact_scratch_bytes(1) == 8 * (2 + 2 + 1 + 1)
    assert _dmlc.compact_scratch_bytes(64) == _dmlc.compact_scratch_bytes(1)
    assert _dmlc.compact_scratch_bytes(65) == 8 * (2 + 2 + 1 + 1)
    assert _dmlc.compact_scratch_bytes(129) == 8 * (4 + 4 + 1 + 1)
    f = 2 ** 26
    assert f // 4 <= _dmlc.compact_scratch_bytes(f) <= f // 4 + f // 4096 + 64  # ~ F / 4 bytes
    # a second scan tile (2048 words = 131 072 features) needs a second partial
    assert _dmlc.compact_scratch_bytes(131073) == _dmlc.compact_scratch_bytes(131072) + 8 * 5


def test_zero_size_launches_make_no_hip_call():
    """on a machine without a GPU any HIP call would fail: these return first"""
    view = (0, 0, 0, 0, 0, False, False)
    _dmlc.lazy_update(_dmlc.lazy_adagrad, 0, 0, 0, 0, 0, 10, 0, 4, 0.1, 1e-10, 0.0, 0.0, 0, 0)
    _dmlc.lazy_update(_dmlc.lazy_ftrl, 0, 0, 0, 0, 0, 10, 5, 0, 0.1, 1.0, 0.0, 0.0, 0, 0)
    # U3 without ids, U4 without entries, no row pointer asked for (scratch: any aligned address)
    _dmlc.compact_emit(view, 0, 0, 100, 16, 0, 0, 0, 0, 0)


def _cpu_csr():
    return {"offset": torch.tensor([0, 2, 3]), "index": torch.tensor([1, 4, 2], dtype=torch.int32),
            "value": torch.ones(3), "label": torch.tensor([0.0, 1.0])}


@pytest.mark.parametrize("nf", [0, -1, 2 ** 32 + 1, 3.0, True, None])
def test_compact_features_rejects_bad_num_features(nf):
    with pytest.raises(ValueError, match="num_features"):
        ops.compact_features(_cpu_csr(), nf)


def test_compact_features_rejects_bad_csr():
    csr = _cpu_csr()
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.compact_features(csr, 10)  # host tensors
    with pytest.raises(ValueError, match="32- or 64-bit integer"):
        ops.compact_features(dict(csr, index=csr["index"].to(torch.int16)), 10)
    with pytest.raises(ValueError, match="32- or 64-bit integer"):
        ops.compact_features(dict(csr, index=csr["index"].float()), 10)
    with pytest.raises(ValueError, match="64-bit row pointer"):
        ops.compact_features(dict(csr, offset=csr["offset"].to(torch.int32)), 10)
    with pytest.raises(ValueError, match="1-D tensor"):
        ops.compact_features(dict(csr, index=csr["index"].reshape(3, 1)), 10)
    with pytest.raises(ValueError, match="1-D tensor"):
        ops.compact_features(dict(csr, offset=None), 10)


def _lazy_args(width=4, rows=3, feats=10):
    shape = (feats, width) if width else (feats,)
    gshape = (rows,) + shape[1:]
    return (torch.zeros(shape), torch.arange(rows), torch.zeros(gshape), (torch.zeros(shape),))


def test_lazy_update_rejects_bad_arguments():
    p, ids, g, st = _lazy_args()
    with pytest.raises(ValueError, match="device tensor"):
        ops.lazy_update_(p, ids, g, st, "adagrad", lr=0.1)  # host tensors
    with pytest.raises(ValueError, match="rule must be one of"):
        ops.lazy_update_(p, ids, g, st, "adam", lr=0.1)
    with pytest.raises(ValueError, match="needs lr"):
        ops.lazy_update_(p, ids, g, st, "adagrad")
    with pytest.raises(ValueError, match="needs alpha"):
        ops.lazy_update_(p, ids, g, (st[0], st[0]), "ftrl")
    with pytest.raises(ValueError, match="takes"):
        ops.lazy_update_(p, ids, g, st, "adagrad", lr=0.1, beta=1.0)
    for bad in (-0.1, 0.0, float("nan"), "x", True):
        with pytest.raises(ValueError, match="lr must be"):
            ops.lazy_update_(p, ids, g, st, "adagrad", lr=bad)
    with pytest.raises(ValueError, match="l1 must be"):
        ops.lazy_update_(p, ids, g, (st[0], st[0]), "ftrl", alpha=0.1, l1=-1.0)
    with pytest.raises(ValueError, match="param must be a float32"):
        ops.lazy_update_(p.double(), ids, g, st, "adagrad", lr=0.1)
    with pytest.raises(ValueError, match="param must be a float32"):
        ops.lazy_update_(torch.zeros(()), None, g, st, "adagrad", lr=0.1)


def test_lazy_update_names_the_argument_of_a_wrong_shape_or_dtype():
    """shapes and dtypes are checked before devices, so host tensors do"""
    p, ids, g, st = _lazy_args()
    for bad in (ids.to(torch.int32), ids.float(), ids.reshape(3, 1), [0, 1, 2]):
        with pytest.raises(ValueError, match="ids must be a 1-D int64"):
            ops.lazy_update_(p, bad, g, st, "adagrad", lr=0.1)
    for bad in (g.double(), torch.zeros(2, 4), torch.zeros(3, 5), torch.zeros(3), torch.zeros(12),
                None):
        with pytest.raises(ValueError, match=r"grad must be float32 of shape \(3, 4\)"):
            ops.lazy_update_(p, ids, bad, st, "adagrad", lr=0.1)
    with pytest.raises(ValueError, match=r"grad must be float32 of shape \(10, 4\)"):
        ops.lazy_update_(p, None, g, st, "adagrad", lr=0.1)  # ids=None: one row per table row
    with pytest.raises(ValueError, match=r"grad must be float32 of shape \(3,\)"):
        ops.lazy_update_(torch.zeros(10), ids, g, (torch.zeros(10),), "adagrad", lr=0.1)
    for bad in ((), (st[0], st[0]), st[0], None):
        with pytest.raises(ValueError, match="takes a state of 1 tensor"):
            ops.lazy_update_(p, ids, g, bad, "adagrad", lr=0.1)
    with pytest.raises(ValueError, match="takes a state of 2 tensor"):
        ops.lazy_update_(p, ids, g, st, "ftrl", alpha=0.1)
    for bad in (torch.zeros(10, 3), torch.zeros(9, 4), torch.zeros(10, 4, dtype=torch.float64),
                torch.zeros(40), None):
        with pytest.raises(ValueError, match="state tensor must be float32 of param's shape"):
            ops.lazy_update_(p, ids, g, (bad,), "adagrad", lr=0.1)
        with pytest.raises(ValueError, match="state tensor must be float32 of param's shape"):
            ops.lazy_update_(p, ids, g, (st[0], bad), "ftrl", alpha=0.1)
    # all shapes right: what is left is the device
    with pytest.raises(ValueError, match="param must be a contiguous device tensor"):
        ops.lazy_update_(p, ids, g, st, "adagrad", lr=0.1)


def test_loaded_state_is_copied_and_keyed():
    opt = optim.LazyAdagrad(0.1)
    mine = (torch.full((4, 2), 3.0),)
    opt.load_state_dict({"rule": "adagrad", "hyper": opt.hyper, "state": {"w": mine}})
    sd = opt.state_dict()  # not used yet: still there, as a copy
    assert list(sd["state"]) == ["w"] and torch.equal(sd["state"]["w"][0], mine[0])
    assert sd["state"]["w"][0] is not mine[0]
    p = torch.nn.Parameter(torch.zeros(4, 2))
    got = opt._state_of(p, "w")
    assert torch.equal(got[0], mine[0]) and got[0].data_ptr() != mine[0].data_ptr()
    assert opt._state_of(p, "w") is got and opt._state_of(torch.zeros(4, 2), "w") is got
    other = optim.LazyAdagrad(0.1)
    other.load_state_dict({"rule": "adagrad", "hyper": opt.hyper, "state": {"w": mine}})
    assert other._state_of(p, "w")[0].data_ptr() != got[0].data_ptr()  # nothing shared
    with pytest.raises(ValueError, match="does not fit"):
        other.load_state_dict({"rule": "adagrad", "hyper": opt.hyper, "state": {"w": mine}})
        other._state_of(torch.zeros(5, 2), "w")
    # without keys: the order of first updates, whatever else has a key
    q, r = torch.zeros(3), torch.zeros(2)
    assert opt._state_of(q)[0].shape == (3,) and opt._state_of(r)[0].shape == (2,)
    assert opt._state_of(q) is opt._state[0] and opt._state_of(r) is opt._state[1]
    assert list(opt.state_dict()["state"]) == ["w", 0, 1]


def test_optimizers_check_their_hyper_parameters():
    with pytest.raises(ValueError, match="lr must be"):
        optim.LazyAdagrad(lr=0.0)
    with pytest.raises(ValueError, match="alpha must be"):
        optim.LazyFTRL(alpha=-1.0)
    with pytest.raises(ValueError, match="eps must be"):
        optim.LazyAdagrad(lr=0.1, eps=-1e-3)
    a = optim.LazyAdagrad(0.1, l2=0.01)
    assert a.hyper == {"lr": 0.1, "eps": 1e-10, "l2": 0.01}
    f = optim.LazyFTRL(0.2, l1=1.0)
    assert f.hyper == {"alpha": 0.2, "beta": 1.0, "l1": 1.0, "l2": 0.0}
    sd = f.state_dict()
    assert sd["rule"] == "ftrl" and sd["state"] == {}
    with pytest.raises(ValueError, match="rule"):
        a.load_state_dict(sd)
    g = optim.LazyFTRL(0.5)
    g.load_state_dict(sd)
    assert g.hyper == f.hyper


def test_substitution_restores_parameters_after_an_exception():
    m = SparseLogReg(7)
    weight, bias = m.weight, m.bias
    sub = {"weight": torch.ones(3), "bias": torch.zeros(1)}
    with optim._substituted(m, sub):
        assert m.weight is sub["weight"] and m.bias is sub["bias"]
    assert m.weight is weight and m.bias is bias
    with pytest.raises(RuntimeError, match="boom"):
        with optim._substituted(m, sub):
            raise RuntimeError("boom")
    assert m.weight is weight and m.bias is bias
    assert dict(m.named_parameters())["weight"] is weight
    with pytest.raises(KeyError):  # a name the model does not have: what was swapped is back
        with optim._substituted(m, {"weight": sub["weight"], "nope": sub["bias"]}):
            pass
    assert m.weight is weight


def test_row_sparse_step_restores_parameters_when_loss_raises():
    m = SparseLogReg(7)
    weight = m.weight
    step = optim.RowSparseStep(m, optim.LazyAdagrad(0.1))
    assert step.rows == ["weight"] and step.dense == ["bias"]
    with pytest.raises(ValueError):  # a host CSR: compact_features refuses it
        step.step(_cpu_csr())
    assert m.weight is weight

    class Boom(SparseLogReg):
        def loss(self, csr):
            assert self.weight.shape == (2,)  # the substituted slice
            raise RuntimeError("boom")

    b = Boom(7)
    weight = b.weight
    sub = {"weight": b.weight.detach()[torch.tensor([1, 4])].requires_grad_()}
    with pytest.raises(RuntimeError, match="boom"):
        with optim._substituted(b, sub):
            b.loss(None)
    assert b.weight is weight and isinstance(b.weight, torch.nn.Parameter)


def test_row_sparse_step_checks_row_names():
    m = SparseLogReg(1)  # bias [1] has shape[0] == num_features by chance
    assert optim.RowSparseStep(m, optim.LazyAdagrad(0.1)).rows == ["weight", "bias"]
    assert optim.RowSparseStep(m, optim.LazyAdagrad(0.1), rows=["weight"]).dense == ["bias"]
    with pytest.raises(ValueError, match="no parameter"):
        optim.RowSparseStep(m, optim.LazyAdagrad(0.1), rows=["w"])
    with pytest.raises(ValueError, match="shape"):
        optim.RowSparseStep(SparseLogReg(5), optim.LazyAdagrad(0.1), rows=["bias"])


def test_adagrad_reference_matches_torch_for_three_steps():
    """dense steps: torch.optim.Adagrad in float64 (lr_decay = 0, accumulator
    from 0, weight_decay = l2) is the same recurrence"""
    g = torch.Generator().manual_seed(5)
    for l2 in (0.0, 0.03):
        w0 = torch.randn(40, 3, generator=g, dtype=torch.float64)
        p = torch.nn.Parameter(w0.clone())
        opt = torch.optim.Adagrad([p], lr=0.1, eps=1e-10, weight_decay=l2)
        w, n = w0.clone(), torch.zeros_like(w0)
        for _ in range(3):
            grad = torch.randn(40, 3, generator=g, dtype=torch.float64)
            p.grad = grad.clone()
            opt.step()
            adagrad64(w, n, None, grad, 0.1, 1e-10, l2)
            torch.testing.assert_close(w, p.detach(), rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(n, opt.state[p]["sum"], rtol=1e-13, atol=0)


def test_lazy_adagrad_reference_equals_dense_with_scattered_gradient():
    """l2 = 0: a row with gradient 0 does not move, so steps on the touched
    rows equal dense steps on the scattered gradient"""
    g = torch.Generator().manual_seed(6)
    w0 = torch.randn(30, 2, generator=g, dtype=torch.float64)
    wl, nl = w0.clone(), torch.zeros_like(w0)
    wd, nd = w0.clone(), torch.zeros_like(w0)
    for _ in range(3):
        ids = torch.sort(torch.randperm(30, generator=g)[:7]).values
        gu = torch.randn(7, 2, generator=g, dtype=torch.float64)
        adagrad64(wl, nl, ids, gu, 0.1)
        dense = torch.zeros_like(w0)
        dense[ids] = gu
        adagrad64(wd, nd, None, dense, 0.1)
    assert torch.equal(wl, wd) and torch.equal(nl, nd)


def test_ftrl_reference_thresholds_and_signs():
    w, z, n = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), \
        torch.zeros(4, dtype=torch.float64)
    grad = torch.tensor([0.5, -0.5, 2.0, -2.0], dtype=torch.float64)
    ftrl64(w, z, n, None, grad, alpha=0.1, beta=1.0, l1=1.0, l2=0.0)
    assert torch.equal(z, grad) and torch.equal(n, grad * grad)
    assert w[0] == 0 and w[1] == 0          # |z| <= l1
    assert w[2] < 0 < w[3]                  # w has the sign of -z
    assert float(w[2]) == pytest.approx(-(2.0 - 1.0) / ((1.0 + 2.0) / 0.1))
