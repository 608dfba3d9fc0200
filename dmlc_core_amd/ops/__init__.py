"""HIP (gfx950) kernels exposed as PyTorch operations on device CSR data.

Every op launches a hand-written CDNA4 kernel from ``libdmlc.so`` on the
current torch stream (src/gpu/feature_kernels.hip, spmm_kernels.hip,
transpose_kernels.hip, gather_kernels.hip, ffm_kernels.hip, rank_kernels.hip,
compact_kernels.hip, optim_kernels.hip, gbdt_kernels.hip).
Histogram gradient-boosted trees run on the column-major binned matrix:
:func:`feature_cuts` -> :func:`bin_features` once, then per tree level
:func:`grad_histogram` -> :func:`best_splits` -> :func:`advance_rows`.
There is no PyTorch fallback: on a machine without the extension or a GPU these
functions raise.

CSR arguments are the dict returned by :func:`dmlc_core_amd.data.csr_to_torch`
(``offset`` int64/uint64 [rows+1], ``index`` int32/uint32 or 64-bit [nnz],
optional ``value`` float32 [nnz], optional ``field``).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import _dmlc

__all__ = ["spmv", "spmv_t", "hashed_dense", "SpMVFunction", "csr_spmv", "transpose",
           "gather_rows", "gather_buffers", "release_workspace",
           "compact_features", "lazy_update_",
           "spmm", "spmm_t", "SpMMFunction", "csr_spmm",
           "ffm", "ffm_t", "FFMFunction", "csr_ffm",
           "qid_groups", "group_rows", "rank_loss", "rank_loss_parts", "RankLossFunction", "ndcg",
           "feature_cuts", "bin_features", "gradient_scale", "grad_histogram", "best_splits",
           "advance_rows"]

# persistent transpose scratch per (device, stream), grow-only: a rebuild (a
# further shard, a refreshed batch) allocates no multi-GB scratch again
_WORKSPACE: Dict = {}


def _workspace(nbytes: int, dev) -> torch.Tensor:
    key = (dev.index, _stream())
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        _WORKSPACE.pop(key, None)  # free the smaller one first
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _WORKSPACE[key] = ws
    return ws


def release_workspace() -> None:
    """Free the persistent scratch of :func:`transpose` and :func:`gather_rows`
    (it is kept between calls so that later builds allocate only their outputs)."""
    _WORKSPACE.clear()


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def _paired(csr: Dict) -> bool:
    """index / value are the interleaved (int32 index, float32 value) pair
    views :func:`transpose` returns: value's storage is index's shifted by one
    4-byte word, both with stride 2"""
    idx, val = csr["index"], csr.get("value")
    return (val is not None and idx.element_size() == 4 and idx.dim() == 1 and val.dim() == 1
            and idx.stride(0) == 2 and val.stride(0) == 2 and idx.numel() == val.numel()
            and val.data_ptr() == idx.data_ptr() + 4 and idx.data_ptr() % 8 == 0)


def _check(csr: Dict, pairs: bool = False):
    """device CSR arrays the kernels can take: contiguous, or (``pairs``: the
    SpMV) the interleaved pair views of a transpose"""
    if pairs and _paired(csr) and csr["offset"].is_cuda and csr["offset"].is_contiguous():
        return
    for k in ("offset", "index"):
        t = csr[k]
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"csr[{k!r}] must be a contiguous device tensor")
    if csr.get("value") is not None and csr["value"].dtype != torch.float32:
        raise ValueError("csr['value'] must be float32")
    if csr.get("value") is not None and not csr["value"].is_contiguous():
        raise ValueError("csr['value'] must be contiguous")


def _unpair(csr: Dict) -> Dict:
    """a transpose's interleaved (index, value) pair views as separate
    contiguous arrays, for the kernels that take only contiguous CSR arrays
    (any other dict is returned as it is)"""
    if not _paired(csr):
        return csr
    out = dict(csr)
    out["index"], out["value"] = csr["index"].contiguous(), csr["value"].contiguous()
    out.pop("pairs", None)
    return out


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _describe(csr: Dict, pairs: bool = False) -> tuple:
    """``csr`` as every CSR op of ``_dmlc`` takes it (gpu::CsrView): the
    addresses of offset, index, value and field (0: none), the rows, whether
    the indices are 64-bit, and -- for an op that reads them (``pairs``) --
    whether index / value are a transpose's interleaved pairs"""
    field = csr.get("field")
    return (_ptr(csr["offset"]), _ptr(csr["index"]), _ptr(csr.get("value")),
            _ptr(field if isinstance(field, torch.Tensor) else None), csr["offset"].numel() - 1,
            csr["index"].element_size() == 8, pairs and _paired(csr))


def _view(csr: Dict, *, pairs: bool = False, fields=False):
    """check ``csr`` (:func:`_check`; ``fields``: the name of an op that needs a
    field per entry, :func:`_check_fields`) and return its :func:`_describe`
    tuple and row count.  The tuple holds addresses: ``csr`` must outlive the
    launch's enqueue, so the caller unpairs (:func:`_unpair`) and keeps the dict"""
    if fields:
        _check_fields(fields, csr)
    else:
        _check(csr, pairs)
    view = _describe(csr, pairs)
    return view, view[4]


def spmv(csr: Dict, w: torch.Tensor, bias: float = 0.0) -> torch.Tensor:
    """y[r] = sum_j value[j] * w[index[j]] + bias  (K11, 16 lanes per row).
    Takes contiguous arrays or a transpose's interleaved (index, value) pairs.
    Rows of any length (empty rows give ``bias``), any number of rows (none
    gives an empty result), 32- or 64-bit indices, ``value`` optional (1.0);
    ``offset`` may be a slice of a larger CSR's row pointer (``offset[0] !=
    0``) next to the whole ``index`` / ``value``.  Sums are f32, in no fixed
    order."""
    view, nrows = _view(csr, pairs=True)
    assert w.dtype == torch.float32 and w.is_cuda and w.is_contiguous()
    y = torch.empty(nrows, dtype=torch.float32, device=w.device)
    _dmlc.spmv(view, _ptr(w), float(bias), _ptr(y), _stream())
    return y


def spmv_t(csr: Dict, d: torch.Tensor, num_features: int) -> torch.Tensor:
    """g[index[j]] += value[j] * d[row(j)]  (transposed K11, f32 atomics).
    A transpose's pair views are unpaired into contiguous copies first.
    Takes the same CSR shapes as :func:`spmv`; rows whose ``d`` is +-0 are
    skipped (they add nothing), and a CSR of no rows gives zeros."""
    csr = _unpair(csr)
    view, _ = _view(csr)
    assert d.dtype == torch.float32 and d.is_cuda and d.is_contiguous()
    g = torch.zeros(num_features, dtype=torch.float32, device=d.device)
    _dmlc.spmv_t(view, _ptr(d), _ptr(g), _stream())
    return g


def _check_dense(name: str, m, bias=None) -> int:
    """the dense operand of :func:`spmm` / :func:`spmm_t` (and ``bias``), before
    anything is launched; returns its column count k"""
    if not isinstance(m, torch.Tensor) or m.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor [rows, k]")
    if m.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {m.dtype}")
    k, kmax = int(m.shape[1]), int(_dmlc.spmm_max_cols())
    if not 1 <= k <= kmax:
        raise ValueError(f"{name} must have 1 .. {kmax} columns, got {k}")
    if not m.is_contiguous():
        raise ValueError(f"{name} must be contiguous (row-major)")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 \
                or tuple(bias.shape) != (k,) or not bias.is_contiguous():
            raise ValueError(f"bias must be a contiguous float32 tensor of shape [{k}]")
    return k


def _check_device(name: str, t, csr: Dict) -> None:
    if t is not None and t.device != csr["index"].device:
        raise ValueError(f"{name} must be on the CSR's device ({csr['index'].device}), "
                         f"is on {t.device}")


def spmm(csr: Dict, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y[r, :] = sum_j value[j] * w[index[j], :] (+ bias)  (M1 / M1p,
    src/gpu/spmm_kernels.hip): the CSR times a dense ``[F, k]`` matrix, as
    float32 ``[rows, k]``.

    ``w``: a contiguous float32 device tensor ``[F, k]`` with k from 1 to
    ``_dmlc.spmm_max_cols()`` (256); ``bias``: None or a contiguous float32
    device tensor ``[k]``; anything else raises ``ValueError`` before a
    launch.  k a multiple of 4 reads ``w`` rows through 16-byte loads, other
    widths through 4-byte loads.  Takes the CSR shapes of :func:`spmv`
    (32- / 64-bit indices, ``value`` optional, ``offset`` a slice of a larger
    row pointer, empty rows, no rows) and a transpose's interleaved pair
    views.  Every feature id must be ``< w.shape[0]``: this precondition is
    not checked on the device.  No atomics and a summation order fixed by k:
    the same inputs give the same bytes."""
    k = _check_dense("w", w, bias)
    view, nrows = _view(csr, pairs=True)
    _check_device("w", w, csr)
    _check_device("bias", bias, csr)
    y = torch.empty((nrows, k), dtype=torch.float32, device=w.device)
    _dmlc.spmm(view, _ptr(w), _ptr(bias), k, _ptr(y), _stream())
    return y


def spmm_t(csr: Dict, d: torch.Tensor, num_features: int) -> torch.Tensor:
    """G[index[j], :] += value[j] * d[row(j), :]  (M2, no-return f32 atomics
    into a zeroed ``[num_features, k]`` result): X^T D without a transpose.
    ``d``: a contiguous float32 device tensor ``[rows, k]``, validated as
    :func:`spmm`'s ``w``.  A transpose's pair views are unpaired first.  Every
    feature id must be ``< num_features`` (not checked on the device).  The
    sums are in no fixed order."""
    k = _check_dense("d", d)
    csr = _unpair(csr)
    view, nrows = _view(csr)
    _check_device("d", d, csr)
    if d.shape[0] != nrows:
        raise ValueError(f"d has {d.shape[0]} rows, the CSR {nrows}")
    g = torch.zeros((int(num_features), k), dtype=torch.float32, device=d.device)
    _dmlc.spmm_t(view, _ptr(d), k, _ptr(g), _stream())
    return g


_FFM_ERR_INDEX, _FFM_ERR_FIELD = 1, 2  # kFFMErr* (src/gpu/kernels.h)


def _check_factors(v) -> int:
    """the factor table of :func:`ffm` / :func:`ffm_t`, before anything is
    launched; returns its rank k"""
    if not isinstance(v, torch.Tensor) or v.dim() != 3:
        raise ValueError("v must be a 3-D tensor [F, num_fields, k]")
    if v.dtype != torch.float32:
        raise ValueError(f"v must be float32, got {v.dtype}")
    k, kmax = int(v.shape[2]), int(_dmlc.ffm_max_rank())
    if k % 4 != 0 or not 4 <= k <= kmax:
        raise ValueError(f"v must have a rank k that is a multiple of 4 from 4 to {kmax}, got {k}")
    if v.shape[1] < 1:
        raise ValueError("v must have at least one field")
    if not v.is_contiguous():
        raise ValueError("v must be contiguous (row-major)")
    if v.data_ptr() % 16:
        raise ValueError("v must be 16-byte aligned (the kernels' 16-byte loads)")
    return k


def _check_fields(name: str, csr: Dict) -> None:
    """``csr`` as :func:`ffm` / :func:`ffm_t` take it: a contiguous device CSR
    with one ``field`` per entry, of the index's dtype"""
    if _paired(csr):
        raise ValueError(f"{name}: a transpose's pair views carry no fields "
                         "(a transpose has no field per entry)")
    field, index = csr.get("field"), csr["index"]
    if not isinstance(field, torch.Tensor):
        raise ValueError(f"{name}: csr has no 'field' tensor (parse with format=\"libfm\")")
    if field.dtype != index.dtype:
        raise ValueError(f"csr['field'] must have index's dtype ({index.dtype}), got {field.dtype}")
    _check(csr)
    if not field.is_cuda or not field.is_contiguous() or field.device != index.device:
        raise ValueError("csr['field'] must be a contiguous device tensor")
    if field.numel() != index.numel():
        raise ValueError(f"csr['field'] has {field.numel()} entries, csr['index'] {index.numel()}")
    if csr.get("value") is not None and csr["value"].numel() != index.numel():
        raise ValueError(f"csr['value'] has {csr['value'].numel()} entries, "
                         f"csr['index'] {index.numel()}")


def ffm(csr: Dict, v: torch.Tensor, validate: bool = True) -> torch.Tensor:
    """The pairwise term of a field-aware factorisation machine (FF1,
    src/gpu/ffm_kernels.hip), float32 ``[rows]``: over a row's entries a with
    id ``i_a``, field ``f_a`` and value ``x_a`` (1.0 without ``value``)

        p[r] = sum_{a < b} x_a x_b sum_c v[i_a, f_b, c] * v[i_b, f_a, c]

    Pairs run over entries, not distinct ids: two entries with the same id (or
    the same id and field) form a pair like any other; rows of 0 or 1 entries
    give 0.  ``csr``: a LibFM CSR (``csr_to_torch`` / ``gather_rows`` / a row
    slice) with a contiguous device ``field`` of index's dtype, one per entry;
    a transpose's pair views are rejected (a transpose has no fields).  ``v``:
    a contiguous float32 device tensor ``[F, num_fields, k]``, k a multiple of
    4 from 4 to ``_dmlc.ffm_max_rank()`` (32).  Anything else raises
    ``ValueError`` before a launch.

    An entry whose id is ``>= F`` or whose field is ``>= num_fields`` is
    skipped on the device (it takes part in no pair and no address is formed
    from it) and flagged: ``validate=True`` reads the flag word -- the one
    device-to-host read of the call -- and raises ``ValueError`` naming which
    of the two was out of range; ``validate=False`` reads nothing and returns
    the sums over the remaining entries.  Rows of up to
    ``_dmlc.ffm_staged_row_entries()`` entries are staged in LDS once, longer
    rows re-read global memory.  No atomics, a summation order fixed by the
    row's length and k: the same inputs give the same bytes."""
    k = _check_factors(v)
    view, nrows = _view(csr, fields="ffm")
    _check_device("v", v, csr)
    y = torch.empty(nrows, dtype=torch.float32, device=v.device)
    err = torch.zeros(1, dtype=torch.int32, device=v.device)
    _dmlc.ffm_forward(view, _ptr(v), int(v.shape[0]), int(v.shape[1]), k, _ptr(y), _ptr(err),
                      _stream())
    if validate:
        bits = int(err.item())
        if bits:
            what = [s for b, s in ((_FFM_ERR_INDEX, f"a feature id is >= F ({v.shape[0]})"),
                                   (_FFM_ERR_FIELD, f"a field is >= num_fields ({v.shape[1]})"))
                    if bits & b]
            raise ValueError("ffm: " + " and ".join(what))
    return y


def ffm_t(csr: Dict, g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """The gradient of :func:`ffm` in ``v`` for an upstream ``g`` (FF2, no-return
    f32 atomics into a zeroed ``[F, num_fields, k]`` result): for every ordered
    pair a != b of every row ``dV[i_a, f_b, :] += g[r] x_a x_b v[i_b, f_a, :]``.
    ``g``: a contiguous float32 device tensor ``[rows]``; ``csr`` and ``v`` as
    for :func:`ffm`.  Rows whose ``g`` is +-0 are skipped, out-of-range entries
    are skipped as in :func:`ffm` (nothing is read back here), and a CSR of no
    rows gives zeros.  The sums are in no fixed order: a deterministic,
    atomic-free gradient (a gather over the transpose that walks each row
    again) is not provided."""
    k = _check_factors(v)
    if not isinstance(g, torch.Tensor) or g.dim() != 1 or g.dtype != torch.float32 \
            or not g.is_contiguous():
        raise ValueError("g must be a contiguous float32 tensor [rows]")
    view, nrows = _view(csr, fields="ffm_t")
    _check_device("v", v, csr)
    _check_device("g", g, csr)
    if g.numel() != nrows:
        raise ValueError(f"g has {g.numel()} entries, the CSR {nrows} rows")
    dv = torch.zeros_like(v)
    _dmlc.ffm_backward(view, _ptr(g), _ptr(v), int(v.shape[0]), int(v.shape[1]), k, _ptr(dv),
                       _stream())
    return dv


def hashed_dense(csr: Dict, dim: int, seed: int = 0, fp8: bool = True,
                 scale: float = 1.0) -> torch.Tensor:
    """K9: signed feature hashing of every row into ``dim`` buckets.

    Returns float8_e4m3fn [rows, dim] (gfx950 OCP fp8, hardware conversion)
    when ``fp8`` else float32.  LibFM fields are folded into the hash key
    (``index ^ field << 40``, so field 0 is the same key as no field); a
    missing ``value`` counts 1.0 per entry.  ``dim``: a multiple of 4 from 4
    to 8192, anything else raises.

    fp8: each bucket's f32 sum times ``scale`` (one f32 product) is rounded
    to nearest, ties to even, subnormals included -- for ``|x| <= 464`` byte
    for byte torch's ``float32 -> float8_e4m3fn`` cast (464 still gives 448).
    Out of range, as produced by gfx950's conversion: a finite ``|x| > 464``
    and ``+-inf`` give the NaN code with the value's sign (0x7F / 0xFF; no
    saturation to 448; torch's cast gives the same bytes), and a NaN gives
    0xFF whatever its sign (torch's cast gives 0x7F for a positive NaN).
    Choose ``scale`` so that the sums stay within +-448.
    """
    csr = _unpair(csr)
    view, nrows = _view(csr)
    dev = csr["index"].device
    if fp8:
        out = torch.empty((nrows, dim), dtype=torch.uint8, device=dev)
    else:
        out = torch.empty((nrows, dim), dtype=torch.float32, device=dev)
    _dmlc.hashed_dense(view, int(dim), float(scale), int(seed) & 0xFFFFFFFF, _ptr(out), bool(fp8),
                       _stream())
    if fp8:
        return out.view(torch.float8_e4m3fn)
    return out


def transpose(csr: Dict, num_features: int, out: Optional[Dict] = None) -> Dict:
    """The CSR's transpose (CSC / inverted index) on the device, as a
    CSR-shaped dict whose rows are the features: ``offset`` int64
    [num_features + 1], ``index`` int32 row ids (ascending within every
    column), ``value`` (or None).  With values, ``index`` and ``value`` are
    the two columns of one interleaved [nnz, 2] buffer (``pairs``: int32 row,
    float32 bits), so each is a stride-2 view: the column scatter writes one
    8-byte pair per entry instead of a 4-byte store into each of two arrays,
    and :func:`spmv` reads the pairs directly (``.contiguous()`` gives
    separate copies).

    Built by the hand-written stable two-level counting sort of
    src/gpu/transpose_kernels.hip (bucket histogram -> scan -> stable bucket
    scatter -> per-bucket column histogram -> scan -> stable column scatter;
    ballot ranks, no atomics on the ordering), it turns the gradient X^T d into
    a gather SpMV (K11 over the transpose): every output is summed on chip and
    written once, instead of one memory-side f32 atomic per nonzero, which
    runs ~17x below the contiguous atomic rate when 64 lanes hit 64 different
    rows (MI355X_MICROARCH.md, Global float atomics).  Feature ids must be
    < num_features <= ``_dmlc.csr_transpose_max_features()`` (2^28: up to
    2^22 columns a two-level sort, above it three levels); an id outside
    raises.

    The sort's scratch (~10 bytes per entry) is a persistent per-device,
    per-stream workspace (:func:`release_workspace` frees it).  ``out``: a
    previous result of the same shape to overwrite instead of allocating
    the outputs (its ``index`` / ``value`` need at least nnz entries).  The
    input may itself be a transpose (its pair views are unpaired first)."""
    csr = _unpair(csr)
    view, nrows = _view(csr)
    offset, index, value = csr["offset"], csr["index"], csr.get("value")
    dev = index.device
    if num_features <= 0 or num_features > _dmlc.csr_transpose_max_features():
        raise ValueError(f"transpose: num_features must be in (0, "
                         f"{_dmlc.csr_transpose_max_features()}], got {num_features}")
    off = offset.view(torch.int64) if offset.dtype != torch.int64 else offset
    # the rows may be a slice of a larger CSR: entries [off[0], off[-1]) of index / value
    # (one device read for both ends)
    lo, hi = (int(v) for v in off[[0, -1]].tolist()) if nrows > 0 else (0, 0)
    nnz = hi - lo
    pairs = None
    if out is not None:
        col_ptr, rows, vals = out["offset"], out["index"], out.get("value")
        if (col_ptr.numel() != num_features + 1 or rows.numel() < nnz
                or (value is not None and (vals is None or vals.numel() < nnz))):
            raise ValueError("transpose: out= does not fit this CSR")
        if value is None:
            vals = None
        elif _paired(out):
            pairs = out.get("pairs")
        elif not (rows.is_contiguous() and vals.is_contiguous()):
            raise ValueError("transpose: out= index / value must be contiguous or a transpose's pairs")
    else:
        col_ptr = torch.empty(num_features + 1, dtype=torch.int64, device=dev)
        if value is not None:
            pairs = torch.empty((max(nnz, 1), 2), dtype=torch.int32, device=dev)
            rows, vals = pairs[:, 0], pairs.view(torch.float32)[:, 1]
        else:
            rows = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
            vals = None
    scratch = _workspace(_dmlc.csr_transpose_scratch_bytes(nnz, num_features), dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _dmlc.csr_transpose(view, lo, nnz, int(num_features), _ptr(col_ptr), _ptr(rows), _ptr(vals),
                        _ptr(scratch), _ptr(err), _stream())
    if int(err.item()) != 0:
        raise ValueError(f"transpose: a feature id is >= num_features ({num_features})")
    res = {"offset": col_ptr, "index": rows[:nnz],
           "value": vals[:nnz] if vals is not None else None}
    if pairs is not None:
        res["pairs"] = pairs
    return res


_ROW_COLUMNS = (("label", 4), ("weight", 4), ("qid", 8))  # per-row columns and their item sizes
_ERR_ROW, _ERR_CAPACITY, _ERR_SOURCE = 1, 2, 4  # kGatherErr* (src/gpu/kernels.h)


class _GatherOutTooSmall(ValueError):
    """``gather_rows(out=)``: the batch has ``nnz`` entries, the buffers fewer"""

    def __init__(self, msg: str, nnz: int):
        super().__init__(msg)
        self.nnz = nnz


def _gather_columns(csr: Dict, nrows: int) -> Dict:
    """the per-row columns of ``csr`` that are tensors, checked"""
    cols = {}
    for k, size in _ROW_COLUMNS:
        t = csr.get(k)
        if not isinstance(t, torch.Tensor):
            continue
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
            raise ValueError(f"csr[{k!r}] must be a contiguous device tensor")
        if t.element_size() != size or (size == 4 and t.dtype != torch.float32):
            raise ValueError(f"csr[{k!r}] must be {'float32' if size == 4 else '64-bit'}")
        if t.numel() < nrows:
            raise ValueError(f"csr[{k!r}] has {t.numel()} entries for {nrows} rows")
        cols[k] = t
    return cols


def gather_buffers(csr: Dict, max_rows: int, max_entries: int) -> Dict:
    """Buffers for :func:`gather_rows`'s ``out=``: room for a selection of up
    to ``max_rows`` rows with up to ``max_entries`` entries of ``csr`` (the
    same columns and dtypes; nothing is gathered)."""
    csr = _unpair(csr)
    _check(csr)
    dev = csr["index"].device
    # one slot more than the row pointer needs: every result's ``offset`` is
    # then a view of a larger buffer, which SpMVFunction's "auto" reads as a
    # batch made per step (atomic gradient, no transpose per batch)
    bufs = {"offset": torch.empty(max_rows + 2, dtype=torch.int64, device=dev),
            "index": torch.empty(max_entries, dtype=csr["index"].dtype, device=dev)}
    if csr.get("value") is not None:
        bufs["value"] = torch.empty(max_entries, dtype=torch.float32, device=dev)
    if csr.get("field") is not None:
        bufs["field"] = torch.empty(max_entries, dtype=csr["field"].dtype, device=dev)
    for k, t in _gather_columns(csr, 0).items():
        bufs[k] = torch.empty(max_rows, dtype=t.dtype, device=dev)
    return {"_buffers": bufs}


def gather_rows(csr: Dict, rows: torch.Tensor, out: Optional[Dict] = None) -> Dict:
    """Rows ``rows[0], rows[1], ...`` of a device CSR as a CSR batch (G1 / G2,
    src/gpu/gather_kernels.hip): the ragged-row gather behind row-shuffled
    minibatches of a resident shard.

    ``csr``: a ``csr_to_torch`` / ``value_torch`` dict, a row-slice dict
    (``offset[b:e + 1]`` next to the whole ``index`` / ``value``; row ids are
    then relative to the slice) or a transpose (unpaired first).  ``rows``: a
    1-D contiguous int64 or int32 device tensor of row ids, in any order,
    duplicates allowed, possibly empty.

    Returns ``offset`` int64 [n_sel + 1] from 0, ``index`` (the source's
    dtype) and ``value`` (None if the source has none: no 1.0 is made up)
    sliced to exactly nnz entries, ``field`` if the source dict has one, and
    ``label`` / ``weight`` / ``qid`` for each that is a tensor in ``csr``.
    The bytes are a pure function of the inputs (no atomics).  G1 writes each
    selected row's length and per-row columns, the K3 scan turns the lengths
    into the row pointer, and G2 copies the entries by output position: each
    wave owns ``_dmlc.csr_gather_run_entries()`` consecutive output entries.

    Runs on the current torch stream; the scan scratch is the persistent
    workspace :func:`transpose` uses.  Exactly one device-to-host read per
    call: one 16-byte copy holding the output nnz and the error word.  A row
    id outside ``[0, nrows)`` raises ``ValueError`` (a negative id does not
    count from the end).

    ``out``: an earlier result (or :func:`gather_buffers`) whose buffers are
    refilled in place; the full-capacity tensors travel under
    ``out["_buffers"]`` and the result holds views of them, so buffers may be
    larger than one batch needs.  ``offset`` needs n_sel + 1 slots, the per-row
    columns n_sel, ``index`` / ``value`` / ``field`` nnz entries: ``ValueError``
    if not.  G2 is bounded by the buffers' capacity, so nothing is written
    past a short buffer before the error is raised; the earlier result's
    contents are overwritten either way."""
    csr = _unpair(csr)
    view, nrows = _view(csr)
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or not rows.is_contiguous() \
            or rows.dim() != 1:
        raise ValueError("rows must be a 1-D contiguous device tensor")
    if rows.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"rows must be int64 or int32, got {rows.dtype}")
    offset, index, value, field = csr["offset"], csr["index"], csr.get("value"), csr.get("field")
    if offset.element_size() != 8 or offset.numel() < 1:
        raise ValueError("csr['offset'] must be a 64-bit row pointer of rows + 1 entries")
    if field is not None and (not field.is_cuda or not field.is_contiguous()
                              or field.dtype != index.dtype):
        raise ValueError("csr['field'] must be a contiguous device tensor of index's dtype")
    n_sel, dev = rows.numel(), index.device
    cols = _gather_columns(csr, nrows)
    src_entries = min(t.numel() for t in (index, value, field) if t is not None)
    entry_keys = ["index"] + (["value"] if value is not None else []) \
        + (["field"] if field is not None else [])
    if out is None:
        bufs = {"offset": torch.empty(n_sel + 2, dtype=torch.int64, device=dev)}  # gather_buffers
        for k, t in cols.items():
            bufs[k] = torch.empty(n_sel, dtype=t.dtype, device=dev)
    else:
        bufs = out.get("_buffers")
        if bufs is None:
            bufs = {k: out[k] for k in ["offset"] + entry_keys + list(cols) if out.get(k) is not None}
        for k in ["offset"] + entry_keys + list(cols):
            t = bufs.get(k)
            like = torch.int64 if k == "offset" else csr[k].dtype
            if t is None or t.dtype != like or t.device != dev or not t.is_contiguous():
                raise ValueError(f"gather_rows: out= has no {k!r} buffer of {like} on {dev}")
            if k == "offset" and t.data_ptr() % 16:
                raise ValueError("gather_rows: out= offset must be 16-byte aligned (the scan's loads)")
            if k not in entry_keys and t.numel() < n_sel + (k == "offset"):
                raise ValueError(f"gather_rows: out= does not fit this selection "
                                 f"({k!r}: {t.numel()} slots for {n_sel} rows)")
    status = torch.zeros(2, dtype=torch.int64, device=dev)  # [nnz, error word]
    scratch = _workspace(8 * _dmlc.csr_gather_scratch_words(n_sel), dev)
    rows64, stream = rows.dtype == torch.int64, _stream()
    _dmlc.csr_gather_count(_ptr(offset), nrows, src_entries, _ptr(rows), rows64, n_sel,
                           _ptr(cols.get("label")), _ptr(cols.get("weight")),
                           _ptr(cols.get("qid")), _ptr(bufs["offset"]), _ptr(bufs.get("label")),
                           _ptr(bufs.get("weight")), _ptr(bufs.get("qid")), _ptr(scratch),
                           _ptr(status), _ptr(status) + 8, stream)

    def fill(capacity: int) -> None:
        _dmlc.csr_gather_fill(view, src_entries, _ptr(rows), rows64, n_sel, _ptr(bufs["offset"]),
                              _ptr(status), _ptr(bufs["index"]), _ptr(bufs.get("value")),
                              _ptr(bufs.get("field")), capacity, _ptr(status) + 8, stream)

    if out is None:
        # the read comes between G1 and G2, to size the outputs
        nnz, err = status.tolist()
        if not err:
            for k in entry_keys:
                bufs[k] = torch.empty(nnz, dtype=csr[k].dtype, device=dev)
            fill(nnz)
    else:
        # G1, scan and G2 are queued back to back, G2 bounded by the buffers
        capacity = min(bufs[k].numel() for k in entry_keys)
        fill(capacity)
        nnz, err = status.tolist()
    if err & _ERR_ROW:
        raise ValueError(f"gather_rows: a row id is outside [0, nrows) (nrows = {nrows})")
    if err & _ERR_SOURCE:
        raise ValueError("gather_rows: csr['offset'] descends or points past index / value / field")
    if err & _ERR_CAPACITY:
        raise _GatherOutTooSmall(f"gather_rows: out= does not fit this selection "
                                 f"({capacity} entries for {nnz})", nnz)
    res = {"offset": bufs["offset"][:n_sel + 1], "index": bufs["index"][:nnz],
           "value": bufs["value"][:nnz] if value is not None else None}
    if "field" in csr:
        res["field"] = bufs["field"][:nnz] if field is not None else None
    for k in cols:
        res[k] = bufs[k][:n_sel]
    res["_buffers"] = bufs
    return res


def _source_key(csr: Dict, num_features: int):
    """identity of the tensors a cached transpose was built from: storage,
    size and in-place version of offset / index / value"""
    def one(t):
        return None if t is None else (int(t.data_ptr()), t.numel(), t._version)
    return (num_features, one(csr["offset"]), one(csr["index"]), one(csr.get("value")))


def _whole(csr: Dict) -> bool:
    """the dict is a whole CSR (its row pointer is a complete tensor of its
    own, as csr_to_torch returns), not a row slice of a larger one -- decided
    from the tensor's storage, without reading device memory"""
    off = csr["offset"]
    return off.storage_offset() == 0 and \
        off.numel() * off.element_size() == off.untyped_storage().nbytes()


def _cached_transpose(holder: Dict, csr: Dict, num_features: int, grad: str) -> Optional[Dict]:
    """The transpose a backward of ``csr`` (the tensors of the dict ``holder``)
    gathers over, or None for the atomic form.  Kept in ``holder['transpose']``
    with the identity of its source (``_transpose_key``), so :func:`csr_spmv`
    and :func:`csr_spmm` reuse each other's.  ``grad``: "atomic" never uses
    one; "transpose" builds it on the first call; "auto" builds it on the first
    call for a whole CSR and on the second through the same dict otherwise."""
    if grad == "atomic":
        return None
    key = _source_key(csr, num_features)
    t = holder.get("transpose")
    if t is not None and holder.get("_transpose_key") != key:
        t = None  # the dict now holds other tensors (or they were written in place)
    if t is None:
        uses = holder.get("_backward_calls", 0) + 1
        if holder.get("_calls_key") != key:
            uses = 1
        holder["_backward_calls"] = uses
        holder["_calls_key"] = key
        # auto: only feature spaces the counting-sort transpose takes
        # (<= 2^28 columns); wider models keep the atomic scatter, which
        # has no column limit.  "transpose" asked for it: transpose() raises
        fits = num_features <= _dmlc.csr_transpose_max_features()
        if grad == "transpose" or (fits and (uses >= 2 or _whole(csr))):
            t = transpose(csr, num_features)
            holder["transpose"] = t
            holder["_transpose_key"] = key
    return t


class SpMVFunction(torch.autograd.Function):
    """Autograd wrapper: forward = spmv, backward d/dw = X^T g -- a gather
    SpMV over the transpose cached in ``csr['transpose']``, or the f32-atomic
    spmv_t.  ``grad``: "transpose" builds the transpose on the first backward;
    "auto" builds it on the first backward of a whole CSR (it is reused every
    epoch) and on the second backward through the same dict otherwise (a
    batch made per step -- e.g. a row slice -- keeps the atomic form, which
    costs less than one transpose); "atomic" never builds it."""

    @staticmethod
    def forward(ctx, w, bias, csr_tuple, holder, grad):
        offset, index, value = csr_tuple
        ctx.csr = {"offset": offset, "index": index, "value": value}
        ctx.holder, ctx.grad = holder, grad
        ctx.num_features = w.numel()
        return spmv(ctx.csr, w, 0.0) + bias

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous().float()
        t = _cached_transpose(ctx.holder, ctx.csr, ctx.num_features, ctx.grad)
        if t is not None:
            gw = spmv(t, grad_out, 0.0)
        else:
            gw = spmv_t(ctx.csr, grad_out, ctx.num_features)
        gb = grad_out.sum().reshape(1)
        return gw, gb, None, None, None


class SpMMFunction(torch.autograd.Function):
    """Autograd wrapper: forward = spmm(csr, w, bias), backward d/dw = X^T G --
    the gather SpMM over the transpose cached in ``csr['transpose']`` (M1p),
    or the f32-atomic spmm_t (M2) -- and d/dbias = column sums of G.  ``grad``
    as for :class:`SpMVFunction`; both share one cache (:func:`_cached_transpose`)."""

    @staticmethod
    def forward(ctx, w, bias, csr_tuple, holder, grad):
        offset, index, value = csr_tuple
        ctx.csr = {"offset": offset, "index": index, "value": value}
        ctx.holder, ctx.grad = holder, grad
        ctx.num_features = w.shape[0]
        return spmm(ctx.csr, w.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous().float()
        gw = gb = None
        if ctx.needs_input_grad[0]:
            t = _cached_transpose(ctx.holder, ctx.csr, ctx.num_features, ctx.grad)
            if t is not None:
                gw = spmm(t, grad_out)
            else:
                gw = spmm_t(ctx.csr, grad_out, ctx.num_features)
        if ctx.needs_input_grad[1]:
            gb = grad_out.sum(0)
        return gw, gb, None, None, None


class FFMFunction(torch.autograd.Function):
    """Autograd wrapper: forward = ffm(csr, v), backward d/dv = ffm_t(csr, g, v)
    (FF2, f32 atomics).  The id / field check runs in forward only."""

    @staticmethod
    def forward(ctx, v, csr_tuple, validate):
        offset, index, value, field = csr_tuple
        ctx.csr = {"offset": offset, "index": index, "value": value, "field": field}
        ctx.save_for_backward(v)
        return ffm(ctx.csr, v.detach(), validate)

    @staticmethod
    def backward(ctx, grad_out):
        (v,) = ctx.saved_tensors
        gv = None
        if ctx.needs_input_grad[0]:
            gv = ffm_t(ctx.csr, grad_out.contiguous().float(), v.detach())
        return gv, None, None


def csr_ffm(csr: Dict, v: torch.Tensor, validate: bool = True) -> torch.Tensor:
    """Differentiable :func:`ffm` (its arguments and checks), differentiable in
    ``v``: the backward is :func:`ffm_t`, whose atomic sums are in no fixed
    order.  ``validate`` applies to the forward; the backward reads nothing
    back."""
    return FFMFunction.apply(v, (csr["offset"], csr["index"], csr.get("value"), csr.get("field")),
                             validate)


_RANK_ERR_GROUP, _RANK_ERR_LABEL = 1, 2  # kRankErr* (src/gpu/kernels.h)
_RANK_WEIGHTINGS = ("ndcg", "none")


def qid_groups(qid: torch.Tensor) -> torch.Tensor:
    """The group pointer of a ``qid`` column (Q1 / Q2, src/gpu/rank_kernels.hip):
    int64 ``[G + 1]`` with group g = rows ``[ptr[g], ptr[g + 1])``, one group per
    run of equal ids.  Rows of one query are taken to be adjacent, as ranking
    files are written: a qid that comes back after another starts a new group.

    ``qid``: a 1-D contiguous 64-bit device tensor (``csr_to_torch``'s int64 or
    a uint64 one; ids are only compared for equality, so values from 2^63 up
    are ids like any other); anything else raises ``ValueError``.  Q1 flags the
    run starts, the K3 scan numbers them, Q2 writes each start's row.  Exactly
    one device-to-host read, of G, between the scan and Q2 (it sizes the
    result); the flags live in the persistent workspace of :func:`transpose`.
    Empty input gives ``tensor([0])`` without a launch."""
    if not isinstance(qid, torch.Tensor) or qid.dim() != 1:
        raise ValueError("qid must be a 1-D tensor")
    if qid.dtype not in (torch.int64, torch.uint64):
        raise ValueError(f"qid must be a 64-bit integer tensor, got {qid.dtype}")
    if not qid.is_cuda or not qid.is_contiguous():
        raise ValueError("qid must be a contiguous device tensor")
    rows, dev = qid.numel(), qid.device
    if rows == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev)
    words = rows + int(_dmlc.qid_scan_words(rows)) + 1
    ws = _workspace(8 * words + 16, dev)
    # the scan reads its data, the flags, by 16-byte loads; its partials and
    # total are single-word accesses and follow the flags wherever they end
    flag = (_ptr(ws) + 15) // 16 * 16
    partials, total = flag + 8 * rows, flag + 8 * (words - 1)
    stream = _stream()
    _dmlc.qid_flags(_ptr(qid), rows, flag, partials, total, stream)
    tot = ws[total - _ptr(ws):total - _ptr(ws) + 8].view(torch.int64)
    groups = int(tot.item())
    ptr = torch.empty(groups + 1, dtype=torch.int64, device=dev)
    _dmlc.qid_group_ptr(_ptr(qid), rows, flag, total, groups, _ptr(ptr), stream)
    return ptr


def group_rows(group_ptr: torch.Tensor, groups: torch.Tensor):
    """The row ids of the groups ``groups[0], groups[1], ...`` of a group
    pointer, in that order, and their own pointer: ``(rows int64 [n], batch_ptr
    int64 [len(groups) + 1])`` on ``group_ptr``'s device.  With
    :func:`gather_rows` this gathers whole queries -- a group-shuffled
    minibatch whose ``batch_ptr`` is the batch's ``group_ptr``.  torch ops only
    (one read, of n, inside ``repeat_interleave``); group ids must be in
    ``[0, G)``, which is not checked."""
    if not isinstance(group_ptr, torch.Tensor) or group_ptr.dim() != 1 or group_ptr.numel() < 1 \
            or group_ptr.dtype != torch.int64:
        raise ValueError("group_ptr must be a 1-D int64 tensor [G + 1]")
    if not isinstance(groups, torch.Tensor) or groups.dim() != 1 \
            or groups.dtype not in (torch.int64, torch.int32):
        raise ValueError("groups must be a 1-D int64 or int32 tensor of group ids")
    sel = groups.to(device=group_ptr.device, dtype=torch.int64)
    start = group_ptr[sel]
    lens = group_ptr[sel + 1] - start
    batch_ptr = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=group_ptr.device)
    torch.cumsum(lens, 0, out=batch_ptr[1:])
    # row p of the batch belongs to selected group o: start[o] + (p - batch_ptr[o])
    owner = torch.repeat_interleave(torch.arange(sel.numel(), device=group_ptr.device), lens)
    rows = torch.arange(owner.numel(), device=group_ptr.device) - batch_ptr[owner] + start[owner]
    return rows, batch_ptr


def _check_rank(name: str, score, label, group_ptr) -> tuple:
    """the operands of :func:`rank_loss` / :func:`ndcg`, before anything is
    launched; returns (rows, groups)"""
    for what, t in (("score", score), ("label", label)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1:
            raise ValueError(f"{name}: {what} must be a 1-D tensor [rows]")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous")
    if not isinstance(group_ptr, torch.Tensor) or group_ptr.dim() != 1 or group_ptr.numel() < 1:
        raise ValueError(f"{name}: group_ptr must be a 1-D tensor [G + 1]")
    if group_ptr.dtype != torch.int64:
        raise ValueError(f"{name}: group_ptr must be int64, got {group_ptr.dtype}")
    if not group_ptr.is_contiguous():
        raise ValueError(f"{name}: group_ptr must be contiguous")
    if label.numel() != score.numel():
        raise ValueError(f"{name}: label has {label.numel()} entries, score {score.numel()}")
    for what, t in (("score", score), ("label", label), ("group_ptr", group_ptr)):
        if not t.is_cuda:
            raise ValueError(f"{name}: {what} must be a device tensor")
        if t.device != score.device:
            raise ValueError(f"{name}: {what} must be on score's device ({score.device}), "
                             f"is on {t.device}")
    return score.numel(), group_ptr.numel() - 1


def _check_rank_loss(score, label, group_ptr, weighting, sigma) -> tuple:
    """the two settings of the loss, then :func:`_check_rank`"""
    if weighting not in _RANK_WEIGHTINGS:
        raise ValueError(f"rank_loss: weighting must be one of {_RANK_WEIGHTINGS}, got {weighting!r}")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not sigma > 0:
        raise ValueError(f"rank_loss: sigma must be a number > 0, got {sigma!r}")
    return _check_rank("rank_loss", score, label, group_ptr)


def _raise_rank_errors(name: str, err: torch.Tensor, rows: int) -> None:
    """the one read of a validated call: the kernels' error word"""
    bits = int(err.item())
    if bits:
        what = [s for b, s in ((_RANK_ERR_GROUP, f"group_ptr descends or points past the rows ({rows}), "
                                                 "or a group spans 2^31 rows"),
                               (_RANK_ERR_LABEL, "a label is not an integer in "
                                                 f"[0, {int(_dmlc.rank_max_label())}]"))
                if bits & b]
        raise ValueError(f"{name}: " + " and ".join(what))


def rank_loss_parts(score: torch.Tensor, label: torch.Tensor, group_ptr: torch.Tensor,
                    weighting: str = "ndcg", sigma: float = 1.0, validate: bool = True):
    """The pairwise ranking loss of every query group and its gradient (RK1 /
    RK2, src/gpu/rank_kernels.hip), without autograd: ``(loss_g float32 [G],
    pairs_g int64 [G], grad float32 [rows])``.

    Group g is rows ``[group_ptr[g], group_ptr[g + 1])``, of any length from 0.
    Row i has score ``s_i``, label ``l_i`` (a float32 holding an integer in
    ``[0, _dmlc.rank_max_label()]`` = 31) and gain ``G_i = 2^l_i - 1``; ``r_i``
    is its 0-based position in a stable descending sort of the group by score,
    ``q_i`` by label, ``D(r) = 1 / log2(2 + r)`` and ``IDCG = sum_i G_i D(q_i)``.
    Over the pairs ``P = {(i, j) : l_i > l_j}`` with ``x_ij = sigma (s_i - s_j)``

        loss_g  = 1/|P| sum_P w_ij softplus(-x_ij)             (0 without pairs)
        grad[i] = sigma/|P| (- sum_{j: l_i > l_j} w_ij rho(x_ij)
                             + sum_{j: l_j > l_i} w_ji rho(x_ji)),  rho(z) = 1 / (1 + e^z)

    where ``weighting="none"`` (RankNet) has ``w_ij = 1`` and ``"ndcg"``
    (LambdaRank) ``w_ij = |G_i - G_j| |D(r_i) - D(r_j)| / IDCG``, treated as a
    constant: it is piecewise constant in s, so ``grad`` is d loss_g / d s_i
    almost everywhere.  ``pairs_g`` is ``|P|``.  Rows outside every group get
    gradient 0.  Row weights (``csr["weight"]``) are not used.

    One wave takes a group of up to ``_dmlc.rank_wave_group_rows()`` (256) rows
    staged in LDS, one workgroup a longer one (below 2^31 rows) in tiles; both
    kernels are launched once over all groups and no length is read back.  No
    sort and no atomics: ranks are counted, every row's sum has one owner, and
    the same inputs give the same bytes.  With ``"ndcg"`` a float per row of
    scratch comes from the persistent workspace of :func:`transpose`.

    ``score`` / ``label``: contiguous float32 device tensors ``[rows]``;
    ``group_ptr``: a contiguous int64 device tensor ``[G + 1]`` (it may start
    above 0 and end below ``rows``); ``sigma > 0``.  Anything else raises
    ``ValueError`` before a launch.  A group whose pointers descend or end past
    ``rows``, and a group with a label that is negative, fractional, NaN or
    above 31, forms no address and no pair: its loss and pairs are 0, its rows'
    gradient 0, and it is flagged.  ``validate=True`` reads the flag word --
    the one device-to-host read of the call -- and raises ``ValueError`` naming
    the check; ``validate=False`` reads nothing.  NaN scores violate a
    precondition: their group's outputs are unspecified."""
    rows, groups = _check_rank_loss(score, label, group_ptr, weighting, sigma)
    dev = score.device
    grad = torch.zeros(rows, dtype=torch.float32, device=dev)
    loss_g = torch.zeros(groups, dtype=torch.float32, device=dev)
    pairs_g = torch.zeros(groups, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    weighted = weighting == "ndcg"
    scratch = _workspace(4 * rows, dev) if weighted else None
    _dmlc.rank_loss(_ptr(score), _ptr(label), _ptr(group_ptr), groups, rows, weighted, float(sigma),
                    _ptr(scratch), _ptr(grad), _ptr(loss_g), _ptr(pairs_g), _ptr(err), _stream())
    if validate:
        _raise_rank_errors("rank_loss", err, rows)
    return loss_g, pairs_g, grad


class RankLossFunction(torch.autograd.Function):
    """Autograd wrapper of :func:`rank_loss_parts`: the forward launches RK1 and
    RK2 once and keeps the gradient; the backward scales it by the incoming
    gradient and by 1 / max(1, groups with pairs), which stays on the device."""

    @staticmethod
    def forward(ctx, score, label, group_ptr, weighting, sigma, validate):
        loss_g, pairs_g, grad = rank_loss_parts(score.detach(), label, group_ptr, weighting, sigma,
                                                validate)
        inv = 1.0 / (pairs_g > 0).sum().clamp(min=1).to(torch.float32)
        ctx.save_for_backward(grad, inv)
        return loss_g.sum() * inv

    @staticmethod
    def backward(ctx, grad_out):
        grad, inv = ctx.saved_tensors
        return grad * (grad_out * inv), None, None, None, None, None


def rank_loss(score: torch.Tensor, label: torch.Tensor, group_ptr: torch.Tensor,
              weighting: str = "ndcg", sigma: float = 1.0, validate: bool = True) -> torch.Tensor:
    """Differentiable mean pairwise ranking loss, ``sum_g loss_g / max(1, #{g :
    |P_g| > 0})``: :func:`rank_loss_parts` (its arguments, checks and
    definitions; row weights are not used) behind :class:`RankLossFunction`,
    differentiable in ``score``."""
    _check_rank_loss(score, label, group_ptr, weighting, sigma)
    return RankLossFunction.apply(score, label, group_ptr, weighting, sigma, validate)


def ndcg(score: torch.Tensor, label: torch.Tensor, group_ptr: torch.Tensor,
         k: Optional[int] = None, validate: bool = True) -> torch.Tensor:
    """NDCG@k of every query group, float32 ``[G]`` (RK1 / RK2 in metric mode:
    the rank counting of :func:`rank_loss_parts`, whose definitions and operand
    checks apply): ``sum_{i: r_i < k} G_i D(r_i) / sum_{i: q_i < k} G_i D(q_i)``;
    ``k=None`` is the whole group, and a group whose denominator is 0 (no rows,
    or only label 0) gives 1.0.  Ties in the scores are ranked by row position.
    Row weights are not used.  ``k``: None or an integer >= 1.  ``validate`` as
    for :func:`rank_loss_parts`; a refused group gives 0."""
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise ValueError(f"ndcg: k must be None or an integer >= 1, got {k!r}")
    rows, groups = _check_rank("ndcg", score, label, group_ptr)
    cut = 0xFFFFFFFF if k is None else min(int(k), 0xFFFFFFFF)
    dev = score.device
    out = torch.zeros(groups, dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _dmlc.rank_ndcg(_ptr(score), _ptr(label), _ptr(group_ptr), groups, rows, cut, _ptr(out),
                    _ptr(err), _stream())
    if validate:
        _raise_rank_errors("ndcg", err, rows)
    return out


_INDEX_DTYPES = (torch.int32, torch.uint32, torch.int64, torch.uint64)
_BATCH_COLUMNS = ("label", "weight", "qid", "group_ptr")  # passed through by compact_features


def _narrow_fields(field: torch.Tensor) -> torch.Tensor:
    """a slice of a ``field`` column as int32, the compact ``index``'s dtype:
    32-bit columns are reinterpreted, 64-bit ones converted, a field that does
    not fit becoming -1 (2^32 - 1 to the kernels: never a valid field)"""
    if field.element_size() == 4:
        return field if field.dtype == torch.int32 else field.view(torch.int32)
    f = field if field.dtype == torch.int64 else field.view(torch.int64)
    return torch.where((f < 0) | (f > 0x7FFFFFFF), torch.full_like(f, -1), f).to(torch.int32)


def compact_features(csr: Dict, num_features: int, validate: bool = True) -> Dict:
    """The batch with its feature ids renumbered to ``0 .. U-1``, U the number
    of distinct ids among its entries (U1 - U4, src/gpu/compact_kernels.hip):
    every CSR op then works on a ``[U, ...]`` slice of the parameters
    (``w[batch["ids"]]``) and returns compact ``[U, ...]`` gradients.

    ``csr``: a ``csr_to_torch`` / ``gather_rows`` dict or a row slice
    (``offset[b:e + 1]`` next to the whole ``index``: only the entries of the
    slice's rows count); 32- or 64-bit indices; a transpose's pair views are
    unpaired first.  ``num_features``: an int from 1 to
    ``_dmlc.compact_max_features()`` (2^32); the batch must have fewer than
    2^31 entries.  Anything else raises ``ValueError`` before a launch.

    Returns a batch dict: ``ids`` int64 ``[U]`` strictly ascending, ``index``
    int32 ``[nnz]`` (each entry's position in ``ids``, for 64-bit sources too),
    ``offset`` int64 ``[rows + 1]`` from 0 (a view of a buffer one slot larger,
    as :func:`gather_buffers` makes them: the "auto" gradient policy then keeps
    the atomic form for a batch made per step), ``value`` (the source's slice,
    None stays None), ``field`` if the source dict has one (the source's slice
    as int32, ``index``'s dtype), ``label`` / ``weight`` / ``qid`` /
    ``group_ptr`` passed through, and ``num_features`` = U.

    No sort: U1 sets a bit per touched id in a bitmap of ``num_features`` bits
    (testing the bit by a load before any atomic), U2 counts the bits of every
    64-bit word, the K3 scan numbers them, U3 writes the ids and U4 every
    entry's slot.  The bitmap, counts and scan scratch -- about
    ``num_features / 4`` bytes, ``_dmlc.compact_scratch_bytes()`` -- live in
    the persistent workspace of :func:`transpose` and the bitmap is cleared in
    the stream on every call.  The atomics build a set, so the output bytes are
    a pure function of the inputs.

    At most two device-to-host reads per call: the slice's ends
    ``offset[[0, -1]]`` (as :func:`transpose`), and one 16-byte copy holding U
    and the error word, between the scan and U3 (it sizes ``ids``).  An id
    ``>= num_features`` forms no address and is flagged: ``validate=True``
    raises ``ValueError``; ``validate=False`` does not, such an entry gets slot
    0 and what it contributes to a product or a gradient is unspecified (with
    U = 0 nothing may be indexed: it raises either way).  A batch without rows
    or entries gives U = 0 without a launch."""
    if isinstance(num_features, bool) or not isinstance(num_features, int):
        raise ValueError(f"compact_features: num_features must be an int, got {num_features!r}")
    fmax = int(_dmlc.compact_max_features())
    if not 1 <= num_features <= fmax:
        raise ValueError(f"compact_features: num_features must be in [1, {fmax}], "
                         f"got {num_features}")
    for k in ("offset", "index"):
        if not isinstance(csr.get(k), torch.Tensor) or csr[k].dim() != 1:
            raise ValueError(f"compact_features: csr[{k!r}] must be a 1-D tensor")
    csr = _unpair(csr)
    offset, index, value, field = csr["offset"], csr["index"], csr.get("value"), csr.get("field")
    if offset.dtype not in (torch.int64, torch.uint64) or offset.numel() < 1:
        raise ValueError("compact_features: csr['offset'] must be a 64-bit row pointer "
                         "of rows + 1 entries")
    if index.dtype not in _INDEX_DTYPES:
        raise ValueError(f"compact_features: csr['index'] must be a 32- or 64-bit integer "
                         f"tensor, got {index.dtype}")
    view, nrows = _view(csr)
    dev = index.device
    for k, t in (("value", value), ("field", field)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() \
                or t.dim() != 1 or t.device != dev:
            raise ValueError(f"compact_features: csr[{k!r}] must be a contiguous 1-D tensor "
                             "on index's device")
    if field is not None and field.dtype not in _INDEX_DTYPES:
        raise ValueError(f"compact_features: csr['field'] must be a 32- or 64-bit integer "
                         f"tensor, got {field.dtype}")
    off = offset.view(torch.int64) if offset.dtype != torch.int64 else offset
    lo, hi = (int(v) for v in off[[0, -1]].tolist()) if nrows > 0 else (0, 0)
    nnz = hi - lo
    entries = min(t.numel() for t in (index, value, field) if t is not None)
    if lo < 0 or nnz < 0 or hi > entries:
        raise ValueError(f"compact_features: csr['offset'] spans entries [{lo}, {hi}) of {entries}")
    if nnz >= 1 << 31:
        raise ValueError(f"compact_features: a batch must have fewer than 2^31 entries, has {nnz}")
    out_offset = torch.zeros(nrows + 2, dtype=torch.int64, device=dev)  # gather_buffers
    if nnz > 0:
        ws = _workspace(int(_dmlc.compact_scratch_bytes(num_features)) + 16, dev)
        scratch = (_ptr(ws) + 15) // 16 * 16
        status = torch.zeros(2, dtype=torch.int64, device=dev)  # [U, error word]
        stream = _stream()
        _dmlc.compact_mark(view, lo, nnz, num_features, scratch, _ptr(status), _ptr(status) + 8,
                           stream)
        n_ids, err = status.tolist()
        if err and (validate or n_ids == 0):
            raise ValueError(f"compact_features: a feature id is >= num_features ({num_features})")
        ids = torch.empty(n_ids, dtype=torch.int64, device=dev)
        slot = torch.empty(nnz, dtype=torch.int32, device=dev)
        _dmlc.compact_emit(view, lo, nnz, num_features, scratch, n_ids, _ptr(ids), _ptr(slot),
                           _ptr(out_offset), stream)
    else:
        n_ids = 0
        ids = torch.empty(0, dtype=torch.int64, device=dev)
        slot = torch.empty(0, dtype=torch.int32, device=dev)
    res = {"ids": ids, "index": slot, "offset": out_offset[:nrows + 1],
           "value": None if value is None else value[lo:hi]}
    if "field" in csr:
        res["field"] = None if field is None else _narrow_fields(field[lo:hi])
    for k in _BATCH_COLUMNS:
        if k in csr:
            res[k] = csr[k]
    res["num_features"] = n_ids
    return res


_LAZY_RULES = {"adagrad": (("lr", None), ("eps", 1e-10), ("l2", 0.0)),
               "ftrl": (("alpha", None), ("beta", 1.0), ("l1", 0.0), ("l2", 0.0))}


def _lazy_hyper(rule: str, hyper: Dict) -> list:
    """the four floats of ``_dmlc.lazy_update`` for ``rule`` from its keyword
    arguments, checked"""
    if rule not in _LAZY_RULES:
        raise ValueError(f"lazy_update_: rule must be one of {sorted(_LAZY_RULES)}, got {rule!r}")
    spec = _LAZY_RULES[rule]
    unknown = set(hyper) - {k for k, _ in spec}
    if unknown:
        raise ValueError(f"lazy_update_: {rule!r} takes {[k for k, _ in spec]}, "
                         f"not {sorted(unknown)}")
    vals = []
    for k, default in spec:
        v = hyper.get(k, default)
        if v is None:
            raise ValueError(f"lazy_update_: {rule!r} needs {k}=")
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v == v or v < 0:
            raise ValueError(f"lazy_update_: {k} must be a number >= 0, got {v!r}")
        if default is None and not v > 0:
            raise ValueError(f"lazy_update_: {k} must be > 0, got {v!r}")
        vals.append(float(v))
    return vals + [0.0] * (4 - len(vals))


def lazy_update_(param: torch.Tensor, ids: Optional[torch.Tensor], grad: torch.Tensor,
                 state: tuple, rule: str, validate: bool = True, **hyper) -> None:
    """One optimizer step, in place, on the rows ``ids`` of ``param`` and of
    its state tensors (L1, src/gpu/optim_kernels.hip): the fused update of a
    row-sparse minibatch step.  Rows not named in ``ids`` are neither read nor
    written.

    ``param``: a contiguous float32 device tensor ``[F, ...]`` (width = the
    product of the trailing dimensions, 1 without); ``ids``: int64 ``[U]``,
    strictly ascending, every id ``< F`` (:func:`compact_features`'s ``ids``),
    or None for the dense identity ``0 .. F-1`` (biases, small tensors);
    ``grad``: contiguous float32 ``[U, ...]`` with ``param``'s trailing shape;
    ``state``: a tuple of tensors shaped like ``param``.  Anything else raises
    ``ValueError`` before a launch.  Rules, f32 in exactly this order
    (``-ffp-contract=off``):

    ``"adagrad"`` (``lr, eps=1e-10, l2=0``), state ``(n,)``::

        g' = g + l2*w;  n += g'*g';  w -= lr * g' / (sqrt(n) + eps)

    torch's ``Adagrad`` with ``lr_decay=0`` and ``initial_accumulator_value=0``.
    With ``l2 = 0`` lazy steps equal dense steps exactly (an untouched row has
    gradient 0); with ``l2 > 0`` the decay is applied to a row only when it is
    touched -- the lazy regularisation of the dmlc CTR learners, not torch's
    ``weight_decay``.

    ``"ftrl"`` (``alpha, beta=1, l1=0, l2=0``), state ``(z, n)``::

        s = (sqrt(n + g*g) - sqrt(n)) / alpha;  z += g - s*w;  n += g*g
        w = 0 if |z| <= l1 else -(z - sign(z)*l1) / ((beta + sqrt(n))/alpha + l2)

    One thread per (row, 4 columns) with 16-byte accesses when width % 4 == 0
    and the tensors are 16-byte aligned, else one per element.  Distinct ids
    give every element one owner: no atomics, the same inputs give the same
    bytes.  A row whose id is ``>= F`` or not strictly between its neighbours'
    ids is skipped and flagged; ``validate=True`` reads the flag (the one
    device-to-host read) and raises ``ValueError``, ``validate=False`` reads
    nothing."""
    vals = _lazy_hyper(rule, hyper)
    # shapes and dtypes first, then devices and layout: a wrong argument is
    # named whatever device it is on
    if not isinstance(param, torch.Tensor) or param.dim() < 1 or param.dtype != torch.float32:
        raise ValueError("lazy_update_: param must be a float32 tensor [F, ...]")
    feats, trailing = int(param.shape[0]), tuple(param.shape[1:])
    width = 1
    for d in trailing:
        width *= int(d)
    if ids is not None and (not isinstance(ids, torch.Tensor) or ids.dim() != 1
                            or ids.dtype != torch.int64):
        raise ValueError("lazy_update_: ids must be a 1-D int64 tensor (or None)")
    nrows = feats if ids is None else int(ids.numel())
    if not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 \
            or tuple(grad.shape) != (nrows,) + trailing:
        raise ValueError(f"lazy_update_: grad must be float32 of shape "
                         f"{(nrows,) + trailing}")
    want = 1 if rule == "adagrad" else 2
    if not isinstance(state, (tuple, list)) or len(state) != want:
        raise ValueError(f"lazy_update_: {rule!r} takes a state of {want} tensor(s)")
    for s in state:
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or s.shape != param.shape:
            raise ValueError("lazy_update_: every state tensor must be float32 of param's "
                             f"shape {tuple(param.shape)}")
    if not param.is_cuda or not param.is_contiguous():
        raise ValueError("lazy_update_: param must be a contiguous device tensor")
    for name, t in (("ids", ids), ("grad", grad), *(("state", s) for s in state)):
        if t is not None and (not t.is_cuda or not t.is_contiguous() or t.device != param.device):
            raise ValueError(f"lazy_update_: {name} must be a contiguous tensor on param's device")
    if nrows == 0 or width == 0:
        return
    err = torch.zeros(1, dtype=torch.int32, device=param.device)
    _dmlc.lazy_update(int(_dmlc.lazy_adagrad if rule == "adagrad" else _dmlc.lazy_ftrl),
                      _ptr(param), _ptr(ids), _ptr(grad), _ptr(state[0]),
                      _ptr(state[1]) if want == 2 else 0, feats, nrows, width, *vals,
                      _ptr(err), _stream())
    if validate and int(err.item()):
        raise ValueError(f"lazy_update_: ids must be strictly ascending and < {feats}")


def csr_spmv(csr: Dict, w: torch.Tensor, bias: torch.Tensor, grad: str = "auto") -> torch.Tensor:
    """Differentiable y = X w + b for a device CSR batch.  X^T g runs as a
    gather SpMV over the CSR's transpose cached in ``csr['transpose']`` (one
    hand-written counting-sort transpose; ~16x faster than atomics on a
    10 M x 1 M batch) or as an
    f32-atomic scatter: grad="auto" (the default) builds the transpose on the
    first backward of a whole CSR and once a row-slice dict is seen a second
    time (only up to ``_dmlc.csr_transpose_max_features()`` = 2^28 columns;
    wider models stay on the atomic form), "transpose" at once, "atomic"
    never."""
    if grad not in ("auto", "transpose", "atomic"):
        raise ValueError(f"grad must be 'auto', 'transpose' or 'atomic', got {grad!r}")
    return SpMVFunction.apply(w, bias, (csr["offset"], csr["index"], csr.get("value")), csr, grad)


def csr_spmm(csr: Dict, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
             grad: str = "auto") -> torch.Tensor:
    """Differentiable Y = X W + b for a device CSR batch and a dense ``[F, k]``
    ``w`` (:func:`spmm`'s arguments and checks), differentiable in ``w`` and
    ``bias``.  X^T G runs as the gather SpMM over the transpose cached in
    ``csr['transpose']`` -- the one :func:`csr_spmv` uses, whichever of the two
    built it -- or as the atomic :func:`spmm_t`; ``grad`` as for
    :func:`csr_spmv`.  The "auto" policy is the one measured at k = 1."""
    if grad not in ("auto", "transpose", "atomic"):
        raise ValueError(f"grad must be 'auto', 'transpose' or 'atomic', got {grad!r}")
    return SpMMFunction.apply(w, bias, (csr["offset"], csr["index"], csr.get("value")), csr, grad)


# ------------------------------------------------------------ histogram GBDT
def _gbdt_index64(csr: Dict, lo: int, hi: int) -> torch.Tensor:
    """the feature ids of entries [lo, hi) as int64 (ids are < 2^28: checked by the transpose)"""
    idx = csr["index"][lo:hi]
    if idx.element_size() == 8:
        return idx if idx.dtype == torch.int64 else idx.view(torch.int64)
    idx = idx if idx.dtype == torch.int32 else idx.view(torch.int32)
    return idx.long() & 0xFFFFFFFF


def _check_cuts(name: str, cuts: Dict, num_features: int, dev) -> None:
    cut_ptr, cut = cuts.get("cut_ptr"), cuts.get("cut")
    if not isinstance(cut_ptr, torch.Tensor) or cut_ptr.dtype != torch.int64 \
            or tuple(cut_ptr.shape) != (num_features + 1,):
        raise ValueError(f"{name}: cut_ptr must be int64 [{num_features + 1}]")
    if not isinstance(cut, torch.Tensor) or cut.dtype != torch.float32 or cut.dim() != 1:
        raise ValueError(f"{name}: cut must be a 1-D float32 tensor")
    for k, t in (("cut_ptr", cut_ptr), ("cut", cut)):
        if t.device != dev or not t.is_contiguous():
            raise ValueError(f"{name}: {k} must be a contiguous tensor on {dev}")


def feature_cuts(csr: Dict, num_features: int, max_bins: int = 256) -> Dict:
    """The quantile cuts of every feature of a device CSR (GB1,
    src/gpu/gbdt_kernels.hip): ``{"cut_ptr": int64 [F + 1], "cut": float32
    [total]}``, feature j's cuts ascending at ``cut[cut_ptr[j]:cut_ptr[j + 1]]``.

    An absent entry is *missing*, not zero; a CSR without ``value`` reads every
    entry as 1.0.  With s the n present values of a feature, ascending, and B =
    ``max_bins`` (2 .. 256), the candidates are ``s[(i*n + B-1)//B - 1]`` for
    i = 1 .. B; equal candidates collapse, so the last cut is the column's
    maximum, n <= B makes every distinct value a cut, and n = 0 gives none.
    Values compare as floats (-0.0 is +0.0), +-inf are ordinary values, a NaN
    raises ``ValueError``.

    torch does the plumbing: :func:`transpose` (cached in ``csr`` as the
    gradients' is) gives the column counts and checks ``id < num_features <=
    _dmlc.csr_transpose_max_features()``, one ``torch.sort`` orders an int64 key
    per entry, ``(feature << 32) | order-preserving u32 of the value``.  GB1
    then picks and de-duplicates every column's candidates, one wave per
    column, in two runs around a ``cumsum`` of the counts.  Takes the CSR
    shapes of :func:`transpose` (32- / 64-bit indices, a row slice).  Three
    device-to-host reads: the slice's first entry ``offset[0]``, the total
    number of cuts and the error word (a transpose that is not cached yet reads
    the slice's ends once more)."""
    if isinstance(max_bins, bool) or not isinstance(max_bins, int) \
            or not 2 <= max_bins <= int(_dmlc.gbdt_max_bins()):
        raise ValueError(f"feature_cuts: max_bins must be an int in [2, "
                         f"{int(_dmlc.gbdt_max_bins())}], got {max_bins!r}")
    csr_u = _unpair(csr)
    t = _cached_transpose(csr, csr_u, int(num_features), "transpose")
    num_features = int(num_features)
    dev = csr_u["index"].device
    nnz = int(t["index"].numel())
    off = csr_u["offset"]
    off = off.view(torch.int64) if off.dtype != torch.int64 else off
    lo = int(off[0].item()) if off.numel() > 1 else 0
    cut_ptr = torch.zeros(num_features + 1, dtype=torch.int64, device=dev)
    if nnz == 0:
        return {"cut_ptr": cut_ptr, "cut": torch.empty(0, dtype=torch.float32, device=dev)}
    value = csr_u.get("value")
    if value is None:
        bits = torch.full((nnz,), 0x3F800000, dtype=torch.int64, device=dev)
    else:
        bits = (value[lo:lo + nnz] + 0.0).view(torch.int32).long()  # + 0.0: -0.0 becomes +0.0
    ordered = torch.where(bits < 0, ~bits, bits + 0x80000000)
    keys = torch.sort((_gbdt_index64(csr_u, lo, lo + nnz) << 32) | ordered).values
    del bits, ordered
    columns = {"offset": t["offset"], "index": t["index"], "value": t.get("value")}
    view = _describe(columns, pairs=True)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _stream()
    _dmlc.gbdt_cut_count(_ptr(keys), view, nnz, max_bins, _ptr(cut_ptr) + 8, _ptr(err), stream)
    cut_ptr[1:].cumsum_(0)
    total, bad = int(cut_ptr[-1].item()), int(err.item())
    if bad:
        raise ValueError("feature_cuts: a value is NaN")
    cut = torch.empty(total, dtype=torch.float32, device=dev)
    _dmlc.gbdt_cut_emit(_ptr(keys), view, nnz, max_bins, _ptr(cut_ptr), _ptr(cut), total, stream)
    return {"cut_ptr": cut_ptr, "cut": cut}


def bin_features(csr: Dict, cuts: Dict, num_features: int) -> Dict:
    """The column-major binned matrix of a device CSR under ``cuts`` (GB2):
    ``{"offset": int64 [F + 1], "row": int32 [nnz], "bin": uint8 [nnz],
    "cut_ptr", "cut", "rows": int}`` -- the :func:`transpose` (cached in
    ``csr``) with every value replaced by its bin; rows ascend within a column.

    ``bin = min(#cuts of the column that are < x, ncuts - 1)``: a value equal
    to a cut falls in that cut's bin, values below the first cut go to bin 0
    and values above the last to the last bin (data that the cuts were not
    trained on).  Entries of a feature without cuts get bin 0 and are ignored
    by every later step.  The global bin of an entry of feature f is
    ``cut_ptr[f] + bin``.  A NaN raises ``ValueError``, as does a feature with
    more than 256 cuts.  One workgroup per ``_dmlc.gbdt_segment_entries()``
    entries searches its columns' cuts in LDS.  Two device-to-host reads: the
    check of ``cut_ptr`` and the error word."""
    num_features = int(num_features)
    csr_u = _unpair(csr)
    dev = csr_u["index"].device
    _check_cuts("bin_features", cuts, num_features, dev)
    t = _cached_transpose(csr, csr_u, num_features, "transpose")
    cut_ptr, cut = cuts["cut_ptr"], cuts["cut"]
    widths = cut_ptr[1:] - cut_ptr[:-1]
    ok = (widths.min() >= 0) & (widths.max() <= int(_dmlc.gbdt_max_bins())) \
        & (cut_ptr[0] == 0) & (cut_ptr[-1] == cut.numel())
    if not bool(ok.item()):
        raise ValueError("bin_features: cut_ptr must ascend from 0 to len(cut) in steps of at most "
                         f"{int(_dmlc.gbdt_max_bins())}")
    nnz = int(t["index"].numel())
    row = torch.empty(nnz, dtype=torch.int32, device=dev)
    bins = torch.empty(nnz, dtype=torch.uint8, device=dev)
    if nnz > 0:
        columns = {"offset": t["offset"], "index": t["index"], "value": t.get("value")}
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _dmlc.gbdt_bin(_describe(columns, pairs=True), nnz, _ptr(cut_ptr), _ptr(cut), _ptr(row),
                       _ptr(bins), _ptr(err), _stream())
        if int(err.item()):
            raise ValueError("bin_features: a value is NaN")
    return {"offset": t["offset"], "row": row, "bin": bins, "cut_ptr": cut_ptr, "cut": cut,
            "rows": int(csr_u["offset"].numel() - 1)}


def _binned_arg(name: str, binned: Dict) -> tuple:
    """``binned`` as the GB3 / GB5 bindings take it (gpu::GbdtBinned), checked"""
    for k, dt in (("offset", torch.int64), ("row", torch.int32), ("bin", torch.uint8),
                  ("cut_ptr", torch.int64)):
        t = binned.get(k)
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_cuda \
                or not t.is_contiguous():
            raise ValueError(f"{name}: binned[{k!r}] must be a contiguous 1-D {dt} device tensor")
    offset, row, bins, cut_ptr = (binned[k] for k in ("offset", "row", "bin", "cut_ptr"))
    if offset.numel() < 2 or cut_ptr.numel() != offset.numel() or bins.numel() != row.numel():
        raise ValueError(f"{name}: binned's arrays do not fit each other")
    return (_ptr(offset), _ptr(row), _ptr(bins), _ptr(cut_ptr), offset.numel() - 1, row.numel(),
            int(binned["rows"]), int(binned["cut"].numel()))


def _check_rows(name: str, what: str, t, dtype, rows: int, dev) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (rows,) \
            or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} tensor [{rows}] on {dev}")


def _check_window(name: str, num_nodes, first_node) -> None:
    nmax = int(_dmlc.gbdt_max_nodes())
    if isinstance(num_nodes, bool) or not isinstance(num_nodes, int) or not 1 <= num_nodes <= nmax:
        raise ValueError(f"{name}: num_nodes must be an int in [1, {nmax}], got {num_nodes!r}")
    if isinstance(first_node, bool) or not isinstance(first_node, int) \
            or not 0 <= first_node < (1 << 30):
        raise ValueError(f"{name}: first_node must be an int in [0, 2^30), got {first_node!r}")


def gradient_scale(grad: torch.Tensor, hess: torch.Tensor) -> float:
    """The power of two ``2**e`` that :func:`grad_histogram` quantises with:
    ``e = 61 - ceil(log2(S))``, ``S = max(sum|g|, sum|h|)`` summed in float64
    (1.0 for S = 0): every sum of quantised values stays below 2^62.  One
    device-to-host read."""
    import math
    s = float(torch.stack([grad.double().abs().sum(), hess.double().abs().sum()]).max().item())
    if not math.isfinite(s):
        raise ValueError("gradient_scale: the gradients are not finite")
    if s == 0.0:
        return 1.0
    m, k = math.frexp(s)  # s = m 2^k, m in [0.5, 1): ceil(log2 s) = k, or k - 1 at a power of two
    return math.ldexp(1.0, 61 - (k - 1 if m == 0.5 else k))


def grad_histogram(binned: Dict, grad: torch.Tensor, hess: torch.Tensor, pos: torch.Tensor,
                   num_nodes: int, scale: float, first_node: int = 0) -> torch.Tensor:
    """The gradient histograms of ``num_nodes`` tree nodes (GB3), int64
    ``[num_nodes, total_bins, 2]``: a row r with ``n = pos[r] - first_node`` in
    ``[0, num_nodes)`` adds ``(llrint(g[r] * scale), llrint(h[r] * scale))``
    (float64 product, ties to even) at ``[n, cut_ptr[f] + bin, :]`` for each of
    its entries; other rows are skipped.  Cells nothing fell in are 0.

    ``grad`` / ``hess``: float32 ``[rows]``, ``pos``: int32 ``[rows]``,
    ``scale``: :func:`gradient_scale`'s.  The sums are 64-bit integers, so they
    do not depend on the order: two runs give the same bytes and a parent's
    histogram is exactly the sum of its children's.  One workgroup per
    ``_dmlc.gbdt_segment_entries()`` entries of the column-major matrix keeps
    its (node, bin) sums in LDS, tiling the nodes when they do not fit, and
    writes each cell once: by a plain store for a column inside one segment,
    by one 64-bit atomic per non-zero cell for a column that spans several.
    Nothing is read back."""
    arg = _binned_arg("grad_histogram", binned)
    _check_window("grad_histogram", num_nodes, first_node)
    rows, total, dev = arg[6], arg[7], binned["row"].device
    _check_rows("grad_histogram", "grad", grad, torch.float32, rows, dev)
    _check_rows("grad_histogram", "hess", hess, torch.float32, rows, dev)
    _check_rows("grad_histogram", "pos", pos, torch.int32, rows, dev)
    if not float(scale) > 0:
        raise ValueError(f"grad_histogram: scale must be > 0, got {scale!r}")
    hist = torch.zeros((num_nodes, total, 2), dtype=torch.int64, device=dev)
    if rows > 0 and total > 0 and arg[5] > 0:
        _dmlc.gbdt_histogram(arg, _ptr(grad), _ptr(hess), _ptr(pos), first_node, num_nodes,
                             float(scale), _ptr(hist), _stream())
    return hist


def best_splits(hist: torch.Tensor, node_sum: torch.Tensor, cut_ptr: torch.Tensor, scale: float,
                reg_lambda: float = 1.0, gamma: float = 0.0,
                min_child_weight: float = 1.0) -> Dict:
    """The best split of every node (GB4): ``{"feature": int64 [N], "bin":
    int32 [N], "default_left": bool [N], "gain": float64 [N]}``, ``feature``
    -1 (bin 0, gain 0) for a node without a split.

    ``hist``: :func:`grad_histogram`'s ``[N, total_bins, 2]``; ``node_sum``:
    int64 ``[N, 2]``, the quantised totals of each node's rows, rows without an
    entry in a feature included.  For a feature with c >= 1 cuts every
    threshold t in 0 .. c-1 and both sides for the missing rows is a candidate:
    left = bins <= t (plus ``node_sum - column total`` when missing goes left),
    right = the rest; the integer sums become float64 and are divided by
    ``scale``; valid with ``HL, HR >= min_child_weight``;
    ``gain = 0.5*(GL^2/(HL+l) + GR^2/(HR+l) - G^2/(H+l)) - gamma``.  The answer
    is the valid candidate of greatest gain if that is > 0; equal gains go to
    the lowest (feature, bin), then to missing-right -- a total order, so
    every run gives the same answer.  The float threshold of a split is
    ``cut[cut_ptr[feature] + bin]``.  ``reg_lambda`` must be > 0."""
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() != 3 \
            or hist.shape[2] != 2 or not hist.is_cuda or not hist.is_contiguous():
        raise ValueError("best_splits: hist must be a contiguous int64 device tensor [N, bins, 2]")
    n, total, dev = int(hist.shape[0]), int(hist.shape[1]), hist.device
    if not isinstance(node_sum, torch.Tensor) or node_sum.dtype != torch.int64 \
            or tuple(node_sum.shape) != (n, 2) or node_sum.device != dev \
            or not node_sum.is_contiguous():
        raise ValueError(f"best_splits: node_sum must be a contiguous int64 tensor [{n}, 2] on {dev}")
    if not isinstance(cut_ptr, torch.Tensor) or cut_ptr.dtype != torch.int64 or cut_ptr.dim() != 1 \
            or cut_ptr.numel() < 2 or cut_ptr.device != dev or not cut_ptr.is_contiguous():
        raise ValueError(f"best_splits: cut_ptr must be a contiguous int64 tensor [F + 1] on {dev}")
    if not float(reg_lambda) > 0:
        raise ValueError(f"best_splits: reg_lambda must be > 0, got {reg_lambda!r}")
    if not float(scale) > 0:
        raise ValueError(f"best_splits: scale must be > 0, got {scale!r}")
    if n > int(_dmlc.gbdt_max_nodes()):
        raise ValueError(f"best_splits: at most {int(_dmlc.gbdt_max_nodes())} nodes, got {n}")
    nfeat = cut_ptr.numel() - 1
    res = {"feature": torch.full((n,), -1, dtype=torch.int64, device=dev),
           "bin": torch.zeros(n, dtype=torch.int32, device=dev),
           "default_left": torch.zeros(n, dtype=torch.bool, device=dev),
           "gain": torch.zeros(n, dtype=torch.float64, device=dev)}
    if n > 0:
        ws = _workspace(int(_dmlc.gbdt_split_scratch_bytes(n, nfeat)) + 16, dev)
        _dmlc.gbdt_best_splits(_ptr(hist), _ptr(node_sum), _ptr(cut_ptr), nfeat, total, n,
                               float(scale), float(reg_lambda), float(gamma),
                               float(min_child_weight), (_ptr(ws) + 15) // 16 * 16,
                               _ptr(res["feature"]), _ptr(res["bin"]), _ptr(res["default_left"]),
                               _ptr(res["gain"]), _stream())
    return res


def advance_rows(binned: Dict, pos: torch.Tensor, split: Dict, left: torch.Tensor,
                 right: torch.Tensor, first_node: int = 0) -> torch.Tensor:
    """Every row's node after the splits of one tree level (GB5), a new int32
    ``[rows]``: a row in node n of the window (``pos[r] == first_node + n``, n <
    N) goes to ``left[n]`` if ``split["feature"][n] < 0``; else, with an entry
    in that column, to ``left[n]`` when its bin is ``<= split["bin"][n]`` and
    to ``right[n]`` otherwise; and without an entry to the side
    ``split["default_left"][n]`` names.  Rows outside the window keep their
    ``pos``.  ``left`` / ``right``: int32 ``[N]``, the ids the children get.

    One pass over ``pos``, then only the split columns are read, filtered by
    ``pos == n`` (two nodes may split on the same feature).  A row's feature
    ids are taken to be distinct; with a repeated id the result is
    unspecified.  Nothing is read back."""
    arg = _binned_arg("advance_rows", binned)
    rows, dev = arg[6], binned["row"].device
    _check_rows("advance_rows", "pos", pos, torch.int32, rows, dev)
    feature = split.get("feature")
    if not isinstance(feature, torch.Tensor) or feature.dim() != 1:
        raise ValueError("advance_rows: split['feature'] must be a 1-D tensor")
    n = int(feature.numel())
    _check_window("advance_rows", max(n, 1), first_node)
    _check_rows("advance_rows", "split['feature']", feature, torch.int64, n, dev)
    _check_rows("advance_rows", "split['bin']", split.get("bin"), torch.int32, n, dev)
    _check_rows("advance_rows", "split['default_left']", split.get("default_left"), torch.bool, n,
                dev)
    _check_rows("advance_rows", "left", left, torch.int32, n, dev)
    _check_rows("advance_rows", "right", right, torch.int32, n, dev)
    out = torch.empty_like(pos)
    if rows > 0:
        _dmlc.gbdt_advance(arg, _ptr(pos), _ptr(feature), _ptr(split["bin"]),
                           _ptr(split["default_left"]), _ptr(left), _ptr(right), first_node, n,
                           _ptr(out), _stream())
    return out
