"""The weighted quantile cuts of ops.feature_cuts(weight=) in NumPy with Python
integers, written from the rule; tests/test_gpu_weighted_cuts.py compares GB1w
(src/gpu/gbdt_cut_kernels.hip) with it, tests/test_weighted_cuts_cpu.py checks
it against the unweighted reference."""
import math

import numpy as np

from gbdt_ref import column_values


def weight_scale(weight):
    s = float(np.asarray(weight, np.float64).sum())
    if s == 0:
        return 1.0
    m, k = math.frexp(s)  # ceil(log2 s) without a rounded logarithm
    return math.ldexp(1.0, 52 - (k - 1 if m == 0.5 else k))


def feature_cuts(off, idx, val, num_features, max_bins, weight):
    col_ptr, rows, v = column_values(off, idx, val, num_features)
    q = np.rint(np.asarray(weight, np.float64) * weight_scale(weight)).astype(np.int64)
    cut_ptr, cut = [0], []
    for f in range(num_features):
        x = v[col_ptr[f]:col_ptr[f + 1]] + np.float32(0.0)  # + 0.0: -0.0 is +0.0
        qx = q[rows[col_ptr[f]:col_ptr[f + 1]]]
        order = np.argsort(x, kind="stable")
        xs, cs = x[order], np.cumsum(qx[order])  # C at every entry: below 2^54, exact
        total, t_prev = int(qx.sum()), 0
        ends = np.flatnonzero(np.append(xs[1:] != xs[:-1], True)) if total > 0 else ()
        for j in ends:  # the last entry of every distinct value
            t = int(cs[j]) * max_bins // total
            if t > t_prev:
                cut.append(xs[j])
            t_prev = t
        cut_ptr.append(len(cut))
    return np.asarray(cut_ptr, np.int64), np.asarray(cut, np.float32)
