#!/usr/bin/env python3
"""Learning-to-rank demonstrator: sharded LibSVM with ``qid:`` tokens (``label
qid:id index:value ...``, the rows of one query adjacent) -> GPU parser -> CSR
with its qid column resident in HBM -> ops.qid_groups (Q1 / Q2: the group
pointer) -> group-shuffled minibatches of whole queries (ops.group_rows +
ops.gather_rows) -> SparseRanker (ops.csr_spmv scores, ops.rank_loss: RK1 / RK2
LambdaRank or RankNet) -> RCCL gradient all-reduce -> SGD, one process per
MI355X; NDCG@10 of the shard after every epoch (ops.ndcg).

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 \
        examples/train_sparse_rank.py data/ --weighting ndcg

Without a data path a synthetic LibSVM shard with 16-row queries is generated
per rank and graded 0 .. 4 by the quantiles of a fixed random linear teacher.
Labels must be integers in [0, 31]; a shard must not split a query (shard the
files on query boundaries).  Plain SGD on the LambdaRank gradient wants a large
step: every pair weight is divided by the group's ideal DCG and the sum by the
pair count (boosted rankers divide by a second derivative instead), hence the
default --lr of 1000 for --weighting ndcg.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("uri", nargs="?", default=None)
    ap.add_argument("--weighting", choices=["ndcg", "none"], default="ndcg",
                    help="pair weights: ndcg (LambdaRank) or none (RankNet)")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows per rank")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch-groups", type=int, default=512, help="queries per minibatch")
    ap.add_argument("--lr", type=float, default=None,
                    help="SGD step (default: 1000 for ndcg, 2 for none -- the ndcg pair weights "
                         "divide the gradient by the group's ideal DCG)")
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--shuffle-seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseRanker
    from dmlc_core_amd.parallel import dist

    info = dist.init()
    rank, world = info["rank"], info["world_size"]
    uri = args.uri
    if uri is None:
        uri = os.path.join(tempfile.mkdtemp(prefix="dmlc_rank_"), "shard.libsvm")
        rows = args.rows - args.rows % 16  # whole 16-row queries
        data.write_synthetic(uri, rank * rows, (rank + 1) * rows, format="libsvm", seed=7,
                             num_features=20_000, qid=True, nthread=8)
        part, nparts = 0, 1
    else:
        part, nparts = rank, world

    csr = data.GPUParser(uri, part, nparts).parse_all()
    (rows, nnz), max_index = dist.global_stats([csr.rows, csr.nnz], csr.max_index)
    num_features = max_index + 1
    t = data.csr_to_torch(csr)
    if t.get("qid") is None:
        raise SystemExit("the file has no qid: tokens")
    group_ptr = ops.qid_groups(t["qid"])
    groups = group_ptr.numel() - 1
    if args.uri is None:
        g = torch.Generator(device="cpu").manual_seed(11)  # the same teacher on every rank
        score = ops.spmv(t, torch.randn(num_features, generator=g).cuda())
        cuts = torch.quantile(score[:1_000_000], torch.tensor([0.5, 0.75, 0.9, 0.97], device="cuda"))
        label = torch.bucketize(score, cuts).float()
    else:
        label = t["label"].float()
    shard = {"offset": t["offset"], "index": t["index"], "value": t["value"], "label": label,
             "group_ptr": group_ptr}
    model = SparseRanker(num_features).cuda()
    ops.ndcg(model(shard).detach(), label, group_ptr, 10)  # labels and pointers checked once
    reducer = dist.GradAllReducer(model.parameters(), bucket_mb=args.bucket_mb)
    lr = args.lr if args.lr is not None else (1000.0 if args.weighting == "ndcg" else 2.0)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    gen = torch.Generator(device="cuda").manual_seed(args.shuffle_seed * world + rank)
    # every rank takes the same number of steps (the all-reduce is collective)
    (_,), steps = dist.global_stats([0], (groups + args.batch_groups - 1) // args.batch_groups)
    history, ndcg10 = [], []
    for epoch in range(args.epochs):
        order = torch.randperm(groups, generator=gen, device="cuda")
        tot, cnt = 0.0, 0
        for step in range(steps):
            sel = order[step * args.batch_groups:(step + 1) * args.batch_groups]
            rows_sel, batch_ptr = ops.group_rows(group_ptr, sel)
            batch = ops.gather_rows(shard, rows_sel)  # whole queries, in the shuffled order
            batch["group_ptr"] = batch_ptr
            loss = model.loss(batch, weighting=args.weighting, sigma=args.sigma, validate=False)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            reducer.synchronize()
            opt.step()
            tot += float(loss.detach()) * sel.numel()
            cnt += sel.numel()
        (loss_sum, seen, nd), _ = dist.global_stats(
            [tot, cnt, float(model.ndcg(shard, k=10)) * groups], 0)
        (all_groups,), _ = dist.global_stats([groups], 0)
        history.append(loss_sum / max(1, seen))
        ndcg10.append(nd / max(1, all_groups))
    if rank == 0:
        print(json.dumps({"world": world, "rows": int(rows), "nnz": int(nnz),
                          "num_features": num_features, "weighting": args.weighting,
                          "loss_per_epoch": [round(x, 5) for x in history],
                          "ndcg10_per_epoch": [round(x, 5) for x in ndcg10]}), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
