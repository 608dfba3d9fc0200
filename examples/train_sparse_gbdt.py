#!/usr/bin/env python3
"""End-to-end demonstrator: LibSVM -> GPU parser -> CSR resident in HBM ->
quantile cuts and the column-major binned matrix (once) -> histogram
gradient-boosted trees (HIP kernels GB1 - GB5), one process on one MI355X.

    python examples/train_sparse_gbdt.py data/train.libsvm --rounds 20 --max-depth 6

Without a data path a synthetic shard is generated.  An absent entry is a
missing value: every split learns the side such rows go to.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("uri", nargs="?", default=None)
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-bins", type=int, default=256)
    ap.add_argument("--lr", type=float, default=0.3)
    ap.add_argument("--objective", choices=("logistic", "squared"), default="logistic")
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseGBDT

    uri = args.uri
    if uri is None:
        tmp = tempfile.mkdtemp(prefix="dmlc_gbdt_")
        uri = os.path.join(tmp, "shard.libsvm")
        data.write_synthetic(uri, 0, args.rows, seed=7, nthread=8)

    t0 = time.perf_counter()
    csr = data.GPUParser(uri).parse_all()
    torch.cuda.synchronize()
    t_parse = time.perf_counter() - t0
    num_features = int(csr.max_index) + 1
    t = data.csr_to_torch(csr)
    label = t["label"].float()
    model = SparseGBDT(num_features, max_bins=args.max_bins, max_depth=args.max_depth,
                       learning_rate=args.lr, objective=args.objective)

    t0 = time.perf_counter()
    model.cuts = ops.feature_cuts(t, num_features, args.max_bins)
    binned = ops.bin_features(t, model.cuts, num_features)
    torch.cuda.synchronize()
    t_bin = time.perf_counter() - t0
    history = []
    t0 = time.perf_counter()
    for _ in range(args.rounds):
        margin = model.boost(binned, label, t.get("weight"))
        history.append(float(model.loss(margin, label, t.get("weight"))))
    torch.cuda.synchronize()
    t_boost = time.perf_counter() - t0
    splits = sum(int((tree["feature"] >= 0).sum()) for tree in model.trees)
    print(json.dumps({"rows": int(csr.rows), "nnz": int(csr.nnz), "num_features": num_features,
                      "total_bins": int(model.cuts["cut"].numel()),
                      "parse_sec": round(t_parse, 4), "cuts_and_bins_sec": round(t_bin, 4),
                      "boost_sec_per_round": round(t_boost / max(args.rounds, 1), 4),
                      "splits": splits, "loss_per_round": [round(x, 5) for x in history]}),
          flush=True)


if __name__ == "__main__":
    main()
