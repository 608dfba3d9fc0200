"""NumPy reference of ops.predict_forest: a row as a dict id -> value walked by the bin rule of
GB2 / GB5 (bin = min(#cuts < x, ncuts - 1), left iff bin <= the node's); no float threshold."""
import numpy as np


def walk(off, idx, val, trees, cut_ptr, cut, seen=None):
    """int32 [rows, T] end nodes; ``seen``: the default sides taken, "last" (bin) / "value" splits"""
    seen = set() if seen is None else seen
    out = np.zeros((off.size - 1, len(trees)), np.int32)
    for r in range(off.size - 1):
        row = {int(idx[j]): (1.0 if val is None else val[j]) for j in range(off[r], off[r + 1])}
        for t, tree in enumerate(trees):
            i, feature = 0, tree["feature"]
            while 2 * i + 2 < feature.size and feature[i] >= 0:
                f = int(feature[i])
                c = cut[cut_ptr[f]:cut_ptr[f + 1]]
                if f in row:
                    left = min(int((c < row[f]).sum()), c.size - 1) <= tree["bin"][i]
                    seen.add("last" if tree["bin"][i] == c.size - 1 else "value")
                else:
                    left = bool(tree["default_left"][i])
                    seen.add("left" if left else "right")
                i = 2 * i + (1 if left else 2)
            out[r, t] = i
    return out
