#!/usr/bin/env python3
"""Field-aware FM demonstrator: sharded LibFM (``label field:index:value ...``)
-> GPU parser -> CSR with a field per entry resident in HBM -> SparseFFM
(ops.csr_ffm: FF1 forward, FF2 atomic backward; ops.csr_spmv for the linear
term) -> RCCL gradient all-reduce -> SGD, one process per MI355X.

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 \
        examples/train_sparse_ffm.py data/ --rank 8

Without a data path a synthetic LibFM shard is generated per rank and labelled
by a fixed random field-aware model of the same shape (one ops.spmv plus one
ops.ffm).
The number of fields is the parsed CSR's ``max_field + 1``.
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
    ap.add_argument("--rank", type=int, default=4, help="factor rank: a multiple of 4 up to 32")
    ap.add_argument("--rows", type=int, default=200_000, help="synthetic rows per rank")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch-rows", type=int, default=8192)
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
    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseFFM
    from dmlc_core_amd.parallel import dist

    info = dist.init()
    rank, world = info["rank"], info["world_size"]
    lazy = args.optimizer != "sgd"
    if lazy and world > 1:
        sys.exit(f"--optimizer {args.optimizer} runs on one process: a row-sparse all-reduce "
                 f"over {world} ranks needs the union of their feature ids, which is not built")
    lr = args.lr if args.lr is not None else (0.05 if lazy else 0.5)
    uri = args.uri
    if uri is None:
        uri = os.path.join(tempfile.mkdtemp(prefix="dmlc_ffm_"), "shard.libfm")
        # 20 .. 60 entries per row over 20 000 ids in 16 fields (field = id mod 16)
        data.write_synthetic(uri, rank * args.rows, (rank + 1) * args.rows, format="libfm", seed=7,
                             num_features=20_000, num_fields=16, nthread=8)
        part, nparts = 0, 1
    else:
        part, nparts = rank, world

    csr = data.GPUParser(uri, part, nparts, format="libfm").parse_all()
    (rows, nnz), max_index = dist.global_stats([csr.rows, csr.nnz], csr.max_index)
    _, max_field = dist.global_stats([0], csr.max_field)
    num_features, num_fields = max_index + 1, max_field + 1
    t = data.csr_to_torch(csr)
    if args.uri is None:
        g = torch.Generator(device="cpu").manual_seed(11)  # the same teacher on every rank
        lin = torch.randn(num_features, generator=g).cuda()
        teacher = torch.randn(num_features, num_fields, 4, generator=g).cuda() * 0.3
        score = ops.spmv(t, lin) + ops.ffm(t, teacher)
        label = (score > score.median()).float()
        del lin, teacher
    else:
        label = t["label"].float()
    model = SparseFFM(num_features, num_fields, rank=args.rank).cuda()
    ops.ffm(t, model.v.detach())  # ids and fields checked once for the shard
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
                                    "field": t["field"], "label": label}, args.batch_rows,
                                   seed=args.shuffle_seed * world + rank)

    def file_order():
        for b in range(0, n, args.batch_rows):
            e = min(n, b + args.batch_rows)
            yield {"offset": t["offset"][b:e + 1], "index": t["index"], "value": t["value"],
                   "field": t["field"], "label": label[b:e]}

    for epoch in range(args.epochs):
        tot, cnt = 0.0, 0
        if shuffled is not None:
            shuffled.set_epoch(epoch)
        for batch in (shuffled if shuffled is not None else file_order()):
            if stepper is not None:
                loss = stepper.step(batch)
            else:
                loss = model.loss(batch)
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
                          "num_features": num_features, "num_fields": num_fields,
                          "rank": args.rank,
                          "loss_per_epoch": [round(x, 5) for x in history]}), flush=True)
    dist.finalize()


if __name__ == "__main__":
    main()
