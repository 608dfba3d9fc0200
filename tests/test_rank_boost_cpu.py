"""ops.rank_grad_hess and SparseGBDT's rank objectives: names, checks, zero-group launch.  No GPU."""
import pytest
import torch

from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT


def test_names_and_zero_group_launch():
    assert "rank_grad_hess" in ops.__all__ and callable(ops.rank_grad_hess)
    for objective in ("rank:ndcg", "rank:pairwise"):
        model = SparseGBDT(8, objective=objective, rank_sigma=2, rank_normalize="pairs")
        assert (model.objective, model.rank_sigma) == (objective, 2.0)
    # no groups: accepted with null pointers, nothing is launched
    _dmlc.rank_boost(0, 0, 0, 0, 0, True, 1.0, False, 0, 0, 0, 0, 0)
    _dmlc.rank_boost(0, 0, 0, 0, 0, False, 2.5, True, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("change,match", [
    (dict(normalize="groups"), "normalize"), (dict(weighting="lambda"), "weighting"),
    (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"),
    (dict(score=torch.zeros(4).double()), "float32"), (dict(label=torch.zeros(4).long()), "float32"),
    (dict(group_ptr=torch.tensor([0, 4]).int()), "int64"),
    (dict(), "device")])  # everything right but on the host
def test_rank_grad_hess_checks_raise_before_any_launch(change, match):
    good = dict(score=torch.zeros(4), label=torch.zeros(4), group_ptr=torch.tensor([0, 4]))
    with pytest.raises(ValueError, match=match):
        ops.rank_grad_hess(**dict(good, **change))


def test_model_checks_raise_before_any_launch():
    model = SparseGBDT(8, objective="rank:ndcg")
    label, ptr = torch.zeros(4), torch.tensor([0, 4])
    for call in (lambda *a: model.boost({"rows": 4}, label, *a), lambda *a: model.loss(label, label, *a)):
        with pytest.raises(ValueError, match="needs group_ptr"):
            call()
        with pytest.raises(ValueError, match="takes no row weights"):
            call(torch.ones(4), ptr)
    assert model.trees == [] and model.margin is None
