"""Row-shuffled minibatches without a device: the epoch permutation
(data.row_order), RowBatches' batch arithmetic and checkpoint state on a stub
CSR, and ops.gather_rows' argument checks (the kernels run in
test_gpu_gather_rows.py)."""
import pytest
import torch

from dmlc_core_amd import data, ops


def _stub(n_rows):
    """host tensors: enough for everything RowBatches does before it gathers"""
    return {"offset": torch.zeros(n_rows + 1, dtype=torch.int64),
            "index": torch.zeros(0, dtype=torch.int32), "value": None}


@pytest.mark.parametrize("n", [0, 1, 2, 10, 1000])
def test_row_order_is_a_permutation(n):
    order = data.row_order(n, 3, 5)
    assert order.dtype == torch.int64 and order.device.type == "cpu" and order.shape == (n,)
    assert sorted(order.tolist()) == list(range(n))


def test_row_order_is_a_pure_function_of_its_arguments():
    a = data.row_order(1000, 7, 2)
    torch.manual_seed(12345)  # the global generator plays no part
    assert torch.equal(a, data.row_order(1000, 7, 2))
    assert not torch.equal(a, data.row_order(1000, 7, 3))  # another epoch
    assert not torch.equal(a, data.row_order(1000, 8, 2))  # another seed
    # seed and epoch do not trade places
    assert not torch.equal(data.row_order(1000, 0, 1), data.row_order(1000, 1, 0))
    # the documented construction
    g = torch.Generator(device="cpu")
    g.manual_seed((7 * 1000003 + 2) % 2 ** 32)
    assert torch.equal(a, torch.randperm(1000, generator=g))


@pytest.mark.parametrize("drop_last,bounds", [
    (False, [(0, 4), (4, 8), (8, 10)]),
    (True, [(0, 4), (4, 8)]),
])
def test_batch_boundaries(drop_last, bounds):
    it = data.RowBatches(_stub(10), 4, drop_last=drop_last)
    assert len(it) == len(bounds)
    assert [it.batch_bounds(k) for k in range(len(it))] == bounds
    with pytest.raises(IndexError):
        it.batch_bounds(len(it))


def test_batch_counts_at_the_edges():
    assert len(data.RowBatches(_stub(0), 4)) == 0
    assert len(data.RowBatches(_stub(8), 4)) == 2
    assert len(data.RowBatches(_stub(8), 4, drop_last=True)) == 2
    assert len(data.RowBatches(_stub(3), 4, drop_last=True)) == 0
    assert list(data.RowBatches(_stub(0), 4)) == []  # no batch, no device work
    with pytest.raises(ValueError):
        data.RowBatches(_stub(8), 0)
    with pytest.raises(ValueError):
        data.RowBatches(_stub(8), 4, buffers=0)


def test_state_dict_round_trip():
    a = data.RowBatches(_stub(10), 4, seed=9)
    a.set_epoch(3)
    a._next = 2  # as after two items of the epoch
    state = a.state_dict()
    assert state == {"seed": 9, "epoch": 3, "next_batch": 2, "batch_rows": 4, "n_rows": 10}
    b = data.RowBatches(_stub(10), 4, seed=9)
    b.load_state_dict(state)
    assert b.state_dict() == state
    b.set_epoch(4)  # a new epoch starts at its first batch
    assert b.state_dict()["next_batch"] == 0 and b.state_dict()["epoch"] == 4


@pytest.mark.parametrize("key,other", [("seed", 1), ("batch_rows", 5), ("n_rows", 11)])
def test_load_state_dict_refuses_a_mismatch(key, other):
    state = data.RowBatches(_stub(10), 4, seed=9).state_dict()
    kwargs = {"seed": 9, "batch_rows": 4, "n_rows": 10}
    kwargs[key] = other
    it = data.RowBatches(_stub(kwargs["n_rows"]), kwargs["batch_rows"], seed=kwargs["seed"])
    with pytest.raises(ValueError, match=key):
        it.load_state_dict(state)
    bad = dict(state, next_batch=4)  # 3 batches: 0..3 are positions
    with pytest.raises(ValueError, match="next_batch"):
        data.RowBatches(_stub(10), 4, seed=9).load_state_dict(bad)


def test_gather_rows_rejects_cpu_tensors():
    csr = {"offset": torch.tensor([0, 2, 3], dtype=torch.int64),
           "index": torch.tensor([1, 2, 3], dtype=torch.int32),
           "value": torch.ones(3)}
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops.gather_rows(csr, torch.tensor([1, 0]))
    assert "gather_rows" in ops.__all__
