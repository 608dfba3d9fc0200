#!/usr/bin/env python3
"""End-to-end demonstrator of multiclass boosting with vector-leaf trees:
LibSVM (labels are class ids 0 .. K-1) -> GPU parser -> CSR resident in HBM ->
cuts and bins (once) -> one tree per round whose leaves hold K values, grown by
the K-channel kernels GB3m / GB4m and GB5 on the first 90 % of the rows; the
rest is held out and scored in row order (GB6 leaf ids, vector leaves gathered),
one process on one MI355X.

    python examples/train_sparse_gbdt_softmax.py data/train.libsvm --classes 5 --rounds 20

Without a data path a synthetic shard is written: every class has 4 marker
features of which a row holds 2 (one of them from another class with
probability --flip), among 12 noise features out of 1000.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_classes(path, rows, classes, flip, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    label = rng.integers(0, classes, rows)
    with open(path, "w") as out:
        for r in range(rows):
            shown = np.where(rng.random(2) < flip, rng.integers(0, classes, 2), label[r])
            ids = set((4 * shown + rng.integers(0, 4, 2)).tolist())
            ids.update((4 * classes + rng.integers(0, 1000, 12)).tolist())
            vals = rng.standard_normal(len(ids))
            out.write(f"{label[r]} " + " ".join(f"{i}:{v:.4f}" for i, v in zip(sorted(ids), vals))
                      + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("uri", nargs="?", default=None)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--rows", type=int, default=50_000, help="synthetic rows")
    ap.add_argument("--flip", type=float, default=0.2, help="synthetic: misleading markers")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-bins", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.3)
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseGBDT

    uri = args.uri
    if uri is None:
        uri = os.path.join(tempfile.mkdtemp(prefix="dmlc_gbdt_softmax_"), "shard.libsvm")
        write_classes(uri, args.rows, args.classes, args.flip)

    t0 = time.perf_counter()
    csr = data.GPUParser(uri).parse_all()
    torch.cuda.synchronize()
    t_parse = time.perf_counter() - t0
    num_features = int(csr.max_index) + 1
    whole = data.csr_to_torch(csr)
    ntrain = max(int(csr.rows) * 9 // 10, 1)
    t = dict(whole, offset=whole["offset"][:ntrain + 1])  # row slices of the same arrays
    held = dict(whole, offset=whole["offset"][ntrain:])
    label, held_label = whole["label"][:ntrain].float(), whole["label"][ntrain:].float()
    model = SparseGBDT(num_features, max_bins=args.max_bins, max_depth=args.max_depth,
                       learning_rate=args.lr, objective="softmax", num_outputs=args.classes)

    t0 = time.perf_counter()
    model.cuts = ops.feature_cuts(t, num_features, args.max_bins)
    binned = ops.bin_features(t, model.cuts, num_features)
    torch.cuda.synchronize()
    t_bin = time.perf_counter() - t0
    history = []
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        margin = model.boost(binned, label)
        history.append(float(model.loss(margin, label)))
    torch.cuda.synchronize()
    t_boost = time.perf_counter() - t0
    result = {"rows": int(csr.rows), "nnz": int(csr.nnz), "num_features": num_features,
              "classes": args.classes, "total_bins": int(model.cuts["cut"].numel()),
              "parse_sec": round(t_parse, 4), "cuts_and_bins_sec": round(t_bin, 4),
              "boost_sec_per_round": round(t_boost / max(args.rounds, 1), 4),
              "train_accuracy": round(float((margin.argmax(1) == label.long()).float().mean()), 4),
              "loss_per_round": [round(x, 5) for x in history]}
    if held["offset"].numel() > 1:
        scores = model.predict(held, method="rows")
        result["held_out_rows"] = int(csr.rows) - ntrain
        result["held_out_loss"] = round(float(model.loss(scores, held_label)), 5)
        result["held_out_accuracy"] = round(
            float((scores.argmax(1) == held_label.long()).float().mean()), 4)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
