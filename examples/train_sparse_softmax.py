#!/usr/bin/env python3
"""Multiclass demonstrator: sharded LibSVM with labels 0 .. C-1 -> GPU parser
-> CSR resident in HBM -> HIP SpMM softmax regression (ops.csr_spmm: M1
forward, gather or atomic X^T G backward) -> RCCL gradient all-reduce -> SGD,
one process per MI355X.

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 \
        examples/train_sparse_softmax.py data/ --num-classes 10

Without a data path a synthetic shard is generated per rank and labelled with
the argmax of a fixed random projection of its rows (itself one ops.spmm).
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
    ap.add_argument("--num-classes", type=int, default=4)
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows per rank")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--lr", type=float, default=0.5)
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--shuffle-rows", action="store_true",
                    help="a fresh row permutation of the resident CSR every epoch "
                         "(data.RowBatches: device row gather) instead of file order")
    ap.add_argument("--shuffle-seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseSoftmaxReg
    from dmlc_core_amd.parallel import dist

    info = dist.init()
    rank, world = info["rank"], info["world_size"]
    uri = args.uri
    if uri is None:
        uri = os.path.join(tempfile.mkdtemp(prefix="dmlc_softmax_"), "shard.libsvm")
        data.write_synthetic(uri, rank * args.rows, (rank + 1) * args.rows, seed=7, nthread=8)
        part, nparts = 0, 1
    else:
        part, nparts = rank, world

    csr = data.GPUParser(uri, part, nparts).parse_all()
    (rows, nnz), max_index = dist.global_stats([csr.rows, csr.nnz], csr.max_index)
    num_features = max_index + 1
    t = data.csr_to_torch(csr)
    if args.uri is None:
        g = torch.Generator(device="cpu").manual_seed(11)  # the same projection on every rank
        proj = torch.randn(num_features, args.num_classes, generator=g).cuda()
        label = ops.spmm(t, proj).argmax(1).float()
    else:
        label = t["label"].float()
    model = SparseSoftmaxReg(num_features, args.num_classes).cuda()
    model.check_labels(label)  # once for the shard; the steps below skip it
    reducer = dist.GradAllReducer(model.parameters(), bucket_mb=args.bucket_mb)
    opt = torch.optim.SGD(model.parameters(), lr=args.lr)
    n = csr.rows
    history = []
    shuffled = None
    if args.shuffle_rows:
        # every rank permutes its own rows; the seed differs per rank
        shuffled = data.RowBatches({"offset": t["offset"], "index": t["index"], "value": t["value"],
                                    "label": label}, args.batch_rows,
                                   seed=args.shuffle_seed * world + rank)

    def file_order():
        for b in range(0, n, args.batch_rows):
            e = min(n, b + args.batch_rows)
            yield {"offset": t["offset"][b:e + 1], "index": t["index"], "value": t["value"],
                   "label": label[b:e]}

    for epoch in range(args.epochs):
        tot, cnt = 0.0, 0
        if shuffled is not None:
            shuffled.set_epoch(epoch)
        for batch in (shuffled if shuffled is not None else file_order()):
            loss = model.loss(batch, validate=False)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            reducer.synchronize()
            opt.step()
            rows_in = batch["label"].numel()
            tot += float(loss.detach()) * rows_in
            cnt += rows_in
        (loss_sum, rows_seen), _ = dist.global_stats([tot, cnt], 0)
        history.append(loss_sum / rows_seen)
    if rank == 0:
        print(json.dumps({"world": world, "rows": int(rows), "nnz": int(nnz),
                          "num_features": num_features, "num_classes": args.num_classes,
                          "loss_per_epoch": [round(x, 5) for x in history]}), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
