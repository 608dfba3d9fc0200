"""ops.sort_rows / ops.row_order: names, caps, argument checks, zero-row launch.  No GPU."""
import pytest
import torch

from dmlc_core_amd import _dmlc, ops
from dmlc_core_amd.models import SparseGBDT


def test_names_caps_and_zero_row_launch():
    assert {"sort_rows", "row_order"} <= set(ops.__all__)
    assert callable(ops.sort_rows) and callable(ops.row_order)
    assert 64 <= _dmlc.sort_wave_row_entries() < _dmlc.sort_block_row_entries()
    # no rows: accepted with null pointers, nothing is launched
    view = (0, 0, 0, 0, 0, False, False)
    _dmlc.sort_rows(view, 0, False, 0, 0, 0, 0, 0, 0, 0)
    _dmlc.row_order(view, 0, False, 0, 0, 0)
    _dmlc.sort_rows_heads(view, 0, False, True, 0, 0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("change,kwargs,match", [
    (dict(), dict(by="value"), "by must be"),
    (dict(), dict(duplicates="mean"), "duplicates must be"),
    (dict(field=None), dict(by="field"), "needs csr\\['field'\\]"),
    (dict(value=None), dict(duplicates="sum"), "'first'"),
    (dict(value=torch.ones(4).double()), dict(), "float32"),
    (dict(field=torch.zeros(4).long()), dict(), "index's dtype"),
    (dict(offset=torch.tensor([0, 4]).int()), dict(), "64-bit row pointer"),
    (dict(), dict(), "device"),  # everything right but on the host
    (dict(), dict(by="field", duplicates="sum"), "device")])
def test_sort_rows_checks_raise_before_any_launch(change, kwargs, match):
    good = dict(offset=torch.tensor([0, 4]), index=torch.zeros(4).int(), value=torch.ones(4),
                field=torch.zeros(4).int())
    with pytest.raises(ValueError, match=match):
        ops.sort_rows(dict(good, **change), **kwargs)
    if "duplicates" not in kwargs:
        with pytest.raises(ValueError, match=match):
            ops.row_order(dict(good, **change), **kwargs)


def test_gbdt_check_rows_is_checked_on_the_device_csr_only():
    host = dict(offset=torch.tensor([0, 2]), index=torch.zeros(2).int(), label=torch.zeros(1))
    with pytest.raises(ValueError, match="device CSR"):
        SparseGBDT(8).fit(host, 1, check_rows=True)
