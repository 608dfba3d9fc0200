"""ops.level_splits is public and SparseGBDT checks split_search (no GPU needed)."""
import pytest

from dmlc_core_amd import ops
from dmlc_core_amd.models import SparseGBDT


def test_level_splits_is_public():
    assert "level_splits" in ops.__all__ and callable(ops.level_splits)


@pytest.mark.parametrize("kwargs, ok", [({}, True), ({"split_search": "histogram"}, True),
                                        ({"split_search": "fused"}, True),
                                        ({"split_search": "x"}, False),
                                        ({"split_search": "fused", "num_outputs": 2}, False)])
def test_split_search_is_checked(kwargs, ok):
    if ok:
        assert SparseGBDT(8, **kwargs).split_search == kwargs.get("split_search", "histogram")
    else:
        with pytest.raises(ValueError):
            SparseGBDT(8, **kwargs)
