#!/usr/bin/env python3
"""End-to-end demonstrator: sharded LibSVM ->
GPU parser -> CSR resident in HBM -> HIP SpMV logistic regression -> RCCL
gradient all-reduce -> SGD, one process per MI355X.

    # one node, 8 GPUs, torchrun rendezvous
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_sparse_logreg.py data/
    # or through the dmlc tracker
    scripts/dmlc-submit --cluster local --num-workers 8 --gpus-per-node 8 \
        python examples/train_sparse_logreg.py data/

Without a data path a synthetic shard is generated per rank.
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
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows per rank")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--lr", type=float, default=None,
                    help="sgd: the step size (default 0.5); lazy-adagrad: lr, "
                         "lazy-ftrl: alpha (default 0.05)")
    ap.add_argument("--optimizer", choices=("sgd", "lazy-adagrad", "lazy-ftrl"), default="sgd",
                    help="lazy-*: row-sparse steps (optim.RowSparseStep) that touch only "
                         "the batch's features; one process only")
    ap.add_argument("--bucket-mb", type=float, default=64.0)
    ap.add_argument("--shuffle-rows", action="store_true",
                    help="a fresh row permutation of the resident CSR every epoch "
                         "(data.RowBatches: device row gather) instead of file order")
    ap.add_argument("--shuffle-seed", type=int, default=0)
    args = ap.parse_args()

    import torch
    from dmlc_core_amd import data
    from dmlc_core_amd.models import SparseLogReg
    from dmlc_core_amd.parallel import dist

    info = dist.init()
    rank, world = info["rank"], info["world_size"]
    lazy = args.optimizer != "sgd"
    if lazy and world > 1:
        sys.exit(f"--optimizer {args.optimizer} runs on one process: a row-sparse all-reduce "
                 f"over {world} ranks needs the union of their feature ids, which is not built")
    lr = args.lr if args.lr is not None else (0.05 if lazy else 0.5)
    tmp = None
    uri = args.uri
    if uri is None:
        tmp = tempfile.mkdtemp(prefix="dmlc_logreg_")
        uri = os.path.join(tmp, "shard.libsvm")
        data.write_synthetic(uri, rank * args.rows, (rank + 1) * args.rows, seed=7, nthread=8)
        part, nparts = 0, 1
    else:
        part, nparts = rank, world

    t0 = time.perf_counter()
    csr = data.GPUParser(uri, part, nparts).parse_all()
    torch.cuda.synchronize()
    t_parse = time.perf_counter() - t0
    (rows, nnz), max_index = dist.global_stats([csr.rows, csr.nnz], csr.max_index)
    num_features = max_index + 1
    t = data.csr_to_torch(csr)
    label = t["label"].float()
    model = SparseLogReg(num_features).cuda()
    reducer = dist.GradAllReducer(model.parameters(), bucket_mb=args.bucket_mb)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    stepper = None
    if lazy:
        from dmlc_core_amd import optim
        stepper = optim.RowSparseStep(model, optim.LazyAdagrad(lr) if args.optimizer == "lazy-adagrad"
                                      else optim.LazyFTRL(lr))
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
            if stepper is not None:
                loss = stepper.step(batch)
            else:
                logits = model(batch)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, batch["label"])
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
                          "num_features": num_features, "parse_sec_rank0": round(t_parse, 4),
                          "loss_per_epoch": [round(x, 5) for x in history]}), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
