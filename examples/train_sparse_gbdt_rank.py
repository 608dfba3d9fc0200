#!/usr/bin/env python3
"""LambdaMART demonstrator: LibSVM with ``qid:`` tokens (``label qid:id
index:value ...``, the rows of one query adjacent) -> GPU parser -> CSR with its
qid column resident in HBM -> ops.qid_groups (the group pointer) -> a share of
the *queries* held out (ops.group_rows + ops.gather_rows: whole groups, never
rows of one) -> SparseGBDT(objective="rank:ndcg"): every round takes the
per-row gradients and hessians of the pairwise objective from RK1 / RK2 in
boost mode (ops.rank_grad_hess) and grows one tree on them (GB3 - GB5).  NDCG@10
of the training and of the held-out queries after every round, the latter
scored in row order by the fused forest kernel (GB6).  One process, one MI355X.

    python examples/train_sparse_gbdt_rank.py data/mslr.libsvm --rounds 50

Without a data path a synthetic shard with 16-row queries is generated and
graded 0 .. 4 by the quantiles of a fixed random linear teacher.  Labels must
be integers in [0, 31].
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
    ap.add_argument("--objective", choices=("rank:ndcg", "rank:pairwise"), default="rank:ndcg")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--normalize", choices=("none", "pairs"), default="none")
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows")
    ap.add_argument("--features", type=int, default=200, help="synthetic feature ids")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--lr", type=float, default=0.3)
    ap.add_argument("--held-out", type=float, default=0.1, help="share of the queries held out")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseGBDT

    uri = args.uri
    if uri is None:
        uri = os.path.join(tempfile.mkdtemp(prefix="dmlc_gbdt_rank_"), "shard.libsvm")
        data.write_synthetic(uri, 0, args.rows - args.rows % 16, format="libsvm", seed=7,
                             num_features=args.features, qid=True, nthread=8)
    csr = data.GPUParser(uri).parse_all()
    num_features = int(csr.max_index) + 1
    t = data.csr_to_torch(csr)
    if t.get("qid") is None:
        raise SystemExit("the file has no qid: tokens")
    group_ptr = ops.qid_groups(t["qid"])
    groups = group_ptr.numel() - 1
    if args.uri is None:
        g = torch.Generator(device="cpu").manual_seed(11)
        score = ops.spmv(t, torch.randn(num_features, generator=g).cuda())
        cuts = torch.quantile(score[:1_000_000], torch.tensor([0.5, 0.75, 0.9, 0.97], device="cuda"))
        label = torch.bucketize(score, cuts).float()
    else:
        label = t["label"].float()
    shard = {"offset": t["offset"], "index": t["index"], "value": t["value"], "label": label}

    # whole queries on either side of the split, each side in file order
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    order = torch.randperm(groups, generator=gen, device="cuda")
    nheld = min(int(groups * args.held_out), groups - 1)
    parts = []
    for ids in (order[nheld:].sort().values, order[:nheld].sort().values):
        rows, ptr = ops.group_rows(group_ptr, ids)
        part = ops.gather_rows(shard, rows)
        part["group_ptr"] = ptr
        parts.append(part)
    train, held = parts

    model = SparseGBDT(num_features, max_depth=args.max_depth, learning_rate=args.lr,
                       objective=args.objective, rank_sigma=args.sigma,
                       rank_normalize=args.normalize)
    model.cuts = ops.feature_cuts(train, num_features)
    binned = ops.bin_features(train, model.cuts, num_features)
    ops.ndcg(torch.zeros_like(train["label"]), train["label"], train["group_ptr"], 10)  # labels checked
    torch.cuda.synchronize()
    ndcg_train, ndcg_held, t_boost = [], [], 0.0
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        margin = model.boost(binned, train["label"], None, train["group_ptr"])
        torch.cuda.synchronize()
        t_boost += time.perf_counter() - t0
        ndcg_train.append(float(ops.ndcg(margin, train["label"], train["group_ptr"], 10).mean()))
        ndcg_held.append(float(model.ndcg(held, k=10)) if nheld else None)
        print("round %d: NDCG@10 train %.5f held-out %s" % (len(ndcg_train), ndcg_train[-1],
              ndcg_held[-1] if ndcg_held[-1] is None else "%.5f" % ndcg_held[-1]), file=sys.stderr)
    print(json.dumps({"rows": int(csr.rows), "nnz": int(csr.nnz), "num_features": num_features,
                      "queries": groups, "held_out_queries": nheld, "objective": args.objective,
                      "normalize": args.normalize,
                      "boost_sec_per_round": round(t_boost / max(args.rounds, 1), 4),
                      "ndcg10_train_per_round": [round(x, 5) for x in ndcg_train],
                      "ndcg10_held_out_per_round": [x if x is None else round(x, 5)
                                                    for x in ndcg_held]}), flush=True)


if __name__ == "__main__":
    main()
