"""The transpose's interleaved (index, value) pair layout as ops sees it,
checked on CPU tensors: which dicts the SpMV takes as pairs and which ones
the contiguity check rejects (the kernels themselves run in test_gpu_ops.py)."""
import pytest
import torch

from dmlc_core_amd import ops


def _pair_dict(nnz=37):
    pairs = torch.zeros((nnz, 2), dtype=torch.int32)
    pairs[:, 0] = torch.arange(nnz, dtype=torch.int32)
    pairs.view(torch.float32)[:, 1] = torch.linspace(-1, 1, nnz)
    return {"offset": torch.tensor([0, nnz], dtype=torch.int64), "index": pairs[:, 0],
            "value": pairs.view(torch.float32)[:, 1], "pairs": pairs}


def test_paired_views_are_recognised():
    d = _pair_dict()
    assert ops._paired(d)
    assert d["index"].stride(0) == 2 and d["value"].data_ptr() == d["index"].data_ptr() + 4
    # the pair views read back the values written through the pair buffer
    torch.testing.assert_close(d["value"], torch.linspace(-1, 1, 37))
    assert d["index"].tolist() == list(range(37))


def test_contiguous_or_unrelated_views_are_not_pairs():
    d = _pair_dict()
    assert not ops._paired({"offset": d["offset"], "index": d["index"].contiguous(),
                            "value": d["value"].contiguous()})
    # value from another buffer, or shifted by a whole pair
    other = torch.zeros((37, 2), dtype=torch.int32)
    assert not ops._paired({"offset": d["offset"], "index": d["index"],
                            "value": other.view(torch.float32)[:, 1]})
    assert not ops._paired({"offset": d["offset"], "index": d["pairs"][1:, 0],
                            "value": d["pairs"].view(torch.float32)[:-1, 1]})
    assert not ops._paired({"offset": d["offset"], "index": d["index"], "value": None})
    # 64-bit indices never form pairs
    p64 = torch.zeros((37, 2), dtype=torch.int64)
    assert not ops._paired({"offset": d["offset"], "index": p64[:, 0],
                            "value": p64.view(torch.float64)[:, 1]})


def test_descriptor_of_pairs_contiguous_copies_and_wide_indices():
    """the (offset, index, value, field, nrows, index64, paired) tuple every
    CSR op hands to the extension"""
    d = _pair_dict()
    off, idx, val, fld, nrows, index64, paired = ops._describe(d, pairs=True)
    assert paired is True and index64 is False
    assert val == idx + 4 and idx == d["pairs"].data_ptr() and off == d["offset"].data_ptr()
    assert (fld, nrows) == (0, 1)
    # an op without a pairs kernel never claims pairs
    assert ops._describe(d)[6] is False
    flat = {"offset": d["offset"], "index": d["index"].contiguous(),
            "value": d["value"].contiguous()}
    assert ops._describe(flat, pairs=True)[5:] == (False, False)
    wide = {"offset": d["offset"], "index": torch.arange(37, dtype=torch.int64), "value": None,
            "field": torch.zeros(37, dtype=torch.int64)}
    view = ops._describe(wide, pairs=True)
    assert view[2] == 0 and view[3] == wide["field"].data_ptr() and view[5:] == (True, False)


def test_launchers_refuse_an_inconsistent_view_before_anything_else():
    """no rows, so nothing would be launched or read: the view is checked first"""
    from dmlc_core_amd import _dmlc
    d = _pair_dict()
    idx, val = d["index"].data_ptr(), d["value"].data_ptr()
    both = (d["offset"].data_ptr(), idx, val, 0, 0, True, True)  # paired and index64
    with pytest.raises(_dmlc.DMLCError, match="pairs have 32-bit indices"):
        _dmlc.spmm(both, 0, 0, 4, 0, 0)
    with pytest.raises(_dmlc.DMLCError, match="takes no interleaved"):
        _dmlc.spmv_t(both, 0, 0, 0)
    pairs = both[:5] + (False, True)
    with pytest.raises(_dmlc.DMLCError, match="value is the float after its index"):
        _dmlc.spmv(pairs[:2] + (0,) + pairs[3:], 0, 0.0, 0, 0)  # pairs without values
    with pytest.raises(_dmlc.DMLCError, match="takes no interleaved"):
        _dmlc.ffm_forward(pairs, 0, 1, 1, 4, 0, 0, 0)
    _dmlc.spmv(pairs, 0, 0.0, 0, 0)  # a consistent view of no rows: accepted, nothing to do
    _dmlc.spmm(pairs, 0, 0, 4, 0, 0)


def test_check_rejects_cpu_and_strided_arrays():
    d = _pair_dict()
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops._check(d, pairs=True)  # CPU tensors: never a device CSR
    with pytest.raises(ValueError, match="contiguous device tensor"):
        ops._check(d)
