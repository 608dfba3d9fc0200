"""NumPy reference of the histogram-GBDT ops (ops.feature_cuts, bin_features,
gradient_scale, grad_histogram, best_splits, advance_rows), written from their
definitions; tests/test_gbdt_cpu.py checks it on the CPU and
tests/test_gpu_gbdt.py compares the HIP kernels with it."""
import math

import numpy as np


def column_values(off, idx, val, num_features):
    """per feature the (row, value) pairs of the CSR rows, rows ascending; an
    absent entry is missing, a CSR without values reads 1.0"""
    lo, hi = int(off[0]), int(off[-1])
    idx = np.asarray(idx[lo:hi]).astype(np.int64)
    val = np.ones(hi - lo, np.float32) if val is None else np.asarray(val[lo:hi], np.float32)
    if idx.size and (idx.min() < 0 or idx.max() >= num_features):
        raise ValueError("a feature id is >= num_features")
    if np.isnan(val).any():
        raise ValueError("a value is NaN")
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(np.asarray(off, np.int64)))
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(idx, minlength=num_features)
    col_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return col_ptr, rows[order].astype(np.int32), val[order]


def feature_cuts(off, idx, val, num_features, max_bins=256):
    col_ptr, _, v = column_values(off, idx, val, num_features)
    cut_ptr, cuts = [0], []
    for f in range(num_features):
        s = np.sort(v[col_ptr[f]:col_ptr[f + 1]] + np.float32(0.0))  # + 0.0: -0.0 is +0.0
        n = s.size
        if n:
            i = np.arange(1, max_bins + 1, dtype=np.int64)
            cuts.append(np.unique(s[(i * n + max_bins - 1) // max_bins - 1]))
        cut_ptr.append(cut_ptr[-1] + (cuts[-1].size if n else 0))
    cut = np.concatenate(cuts).astype(np.float32) if cuts else np.zeros(0, np.float32)
    return np.asarray(cut_ptr, np.int64), cut


def bin_features(off, idx, val, num_features, cut_ptr, cut):
    col_ptr, rows, v = column_values(off, idx, val, num_features)
    bins = np.zeros(v.size, np.uint8)
    for f in range(num_features):
        c = cut[cut_ptr[f]:cut_ptr[f + 1]]
        if c.size:
            x = v[col_ptr[f]:col_ptr[f + 1]]
            bins[col_ptr[f]:col_ptr[f + 1]] = np.minimum(np.searchsorted(c, x, side="left"),
                                                         c.size - 1)
    return {"offset": col_ptr, "row": rows, "bin": bins, "cut_ptr": cut_ptr, "cut": cut,
            "rows": len(off) - 1}


def gradient_scale(g, h):
    s = max(np.abs(np.asarray(g, np.float64)).sum(), np.abs(np.asarray(h, np.float64)).sum())
    if s == 0:
        return 1.0
    m, k = math.frexp(float(s))  # ceil(log2 s) without a rounded logarithm
    return math.ldexp(1.0, 61 - (k - 1 if m == 0.5 else k))


def quantise(x, scale):
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * scale).astype(np.int64)


def entry_global_bins(binned):
    """(feature, global bin, counted) of every entry; entries of a feature
    without cuts are not counted"""
    col_ptr, cut_ptr = binned["offset"], binned["cut_ptr"]
    feat = np.repeat(np.arange(len(col_ptr) - 1), np.diff(col_ptr))
    ncuts = np.diff(cut_ptr)[feat]
    return feat, cut_ptr[feat] + binned["bin"].astype(np.int64), ncuts > 0


def grad_histogram(binned, g, h, pos, num_nodes, scale, first_node=0):
    total = int(binned["cut_ptr"][-1])
    hist = np.zeros((num_nodes, total, 2), np.int64)
    _, gb, counted = entry_global_bins(binned)
    r = binned["row"].astype(np.int64)
    node = np.asarray(pos, np.int64)[r] - first_node
    keep = counted & (node >= 0) & (node < num_nodes)
    qg, qh = quantise(g, scale), quantise(h, scale)
    np.add.at(hist[:, :, 0], (node[keep], gb[keep]), qg[r[keep]])
    np.add.at(hist[:, :, 1], (node[keep], gb[keep]), qh[r[keep]])
    return hist


def node_sums(g, h, pos, num_nodes, scale, first_node=0):
    out = np.zeros((num_nodes, 2), np.int64)
    node = np.asarray(pos, np.int64) - first_node
    keep = (node >= 0) & (node < num_nodes)
    np.add.at(out[:, 0], node[keep], quantise(g, scale)[keep])
    np.add.at(out[:, 1], node[keep], quantise(h, scale)[keep])
    return out


def _gain(lg, lh, ng, nh, scale, lam, gamma, mcw, terms=False):
    """float64 gain of integer left sums (lg, lh) under node sums (ng, nh);
    -inf where a child is lighter than min_child_weight"""
    gl, hl = lg.astype(np.float64) / scale, lh.astype(np.float64) / scale
    gr, hr = (ng - lg).astype(np.float64) / scale, (nh - lh).astype(np.float64) / scale
    g, h = np.float64(ng) / scale, np.float64(nh) / scale
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b, p = gl * gl / (hl + lam), gr * gr / (hr + lam), g * g / (h + lam)
        gain = 0.5 * (a + b - p) - gamma
    if terms:
        return np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(p))
    return np.where((hl >= mcw) & (hr >= mcw), gain, -np.inf)


def gain_table(hist, node_sum, cut_ptr, scale, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0,
               terms=False):
    """[N, total_bins, 2]: the gain of splitting node n at global bin b with
    the missing rows going right (0) or left (1); -inf where invalid.
    ``terms``: instead the largest of |GL^2/(HL+l)|, |GR^2/(HR+l)|, |G^2/(H+l)|,
    the magnitude a tolerance on the gain is relative to"""
    n_nodes, total = hist.shape[0], hist.shape[1]
    feat = np.repeat(np.arange(len(cut_ptr) - 1), np.diff(cut_ptr))
    table = np.full((n_nodes, total, 2), -np.inf)
    for n in range(n_nodes):
        csum = np.cumsum(hist[n], axis=0)
        before = np.concatenate([np.zeros((1, 2), np.int64), csum])[cut_ptr[:-1]]  # per feature
        col_total = np.concatenate([np.zeros((1, 2), np.int64), csum])[cut_ptr[1:]] - before
        left = csum - before[feat]
        miss = (node_sum[n] - col_total)[feat]
        for d in (0, 1):
            ls = left + d * miss
            table[n, :, d] = _gain(ls[:, 0], ls[:, 1], node_sum[n, 0], node_sum[n, 1], scale,
                                   reg_lambda, gamma, min_child_weight, terms)
    return table


def best_splits(hist, node_sum, cut_ptr, scale, reg_lambda=1.0, gamma=0.0, min_child_weight=1.0):
    table = gain_table(hist, node_sum, cut_ptr, scale, reg_lambda, gamma, min_child_weight)
    n_nodes, total = table.shape[0], table.shape[1]
    feat = np.repeat(np.arange(len(cut_ptr) - 1), np.diff(cut_ptr))
    out = {"feature": np.full(n_nodes, -1, np.int64), "bin": np.zeros(n_nodes, np.int32),
           "default_left": np.zeros(n_nodes, bool), "gain": np.zeros(n_nodes, np.float64)}
    for n in range(n_nodes):
        flat = table[n].reshape(-1)  # (global bin, side): the tie-break order, the first maximum
        if total == 0 or not (flat.max() > 0):
            continue
        k = int(np.argmax(flat))
        b, d = k // 2, k % 2
        out["feature"][n], out["bin"][n] = feat[b], b - cut_ptr[feat[b]]
        out["default_left"][n], out["gain"][n] = bool(d), flat[k]
    return out


def best_splits_brute(hist, node_sum, cut_ptr, scale, reg_lambda=1.0, gamma=0.0,
                      min_child_weight=1.0):
    """the same answer by a loop over every (node, feature, bin, side)"""
    n_nodes = hist.shape[0]
    out = {"feature": np.full(n_nodes, -1, np.int64), "bin": np.zeros(n_nodes, np.int32),
           "default_left": np.zeros(n_nodes, bool), "gain": np.zeros(n_nodes, np.float64)}
    for n in range(n_nodes):
        best = 0.0
        ng, nh = int(node_sum[n, 0]), int(node_sum[n, 1])
        for f in range(len(cut_ptr) - 1):
            col = hist[n, cut_ptr[f]:cut_ptr[f + 1]]
            tg, th = int(col[:, 0].sum()), int(col[:, 1].sum())
            lg = lh = 0
            for t in range(col.shape[0]):
                lg, lh = lg + int(col[t, 0]), lh + int(col[t, 1])
                for d in (0, 1):
                    a, b = lg + d * (ng - tg), lh + d * (nh - th)
                    gl, hl, gr, hr = a / scale, b / scale, (ng - a) / scale, (nh - b) / scale
                    if hl < min_child_weight or hr < min_child_weight:
                        continue
                    g, h = ng / scale, nh / scale
                    gain = 0.5 * (gl * gl / (hl + reg_lambda) + gr * gr / (hr + reg_lambda)
                                  - g * g / (h + reg_lambda)) - gamma
                    if gain > best:
                        best = gain
                        out["feature"][n], out["bin"][n] = f, t
                        out["default_left"][n], out["gain"][n] = bool(d), gain
    return out


def advance_rows(binned, pos, split, left, right, first_node=0):
    pos = np.asarray(pos, np.int32)
    out = pos.copy()
    col_ptr = binned["offset"]
    for n in range(len(split["feature"])):
        here = pos == first_node + n
        f = int(split["feature"][n])
        if f < 0:
            out[here] = left[n]
            continue
        out[here] = left[n] if split["default_left"][n] else right[n]
        rows = binned["row"][col_ptr[f]:col_ptr[f + 1]]
        bins = binned["bin"][col_ptr[f]:col_ptr[f + 1]]
        sel = here[rows]
        out[rows[sel]] = np.where(bins[sel] <= split["bin"][n], left[n], right[n])
    return out
