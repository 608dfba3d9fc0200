#!/usr/bin/env python3
"""Dense against row-sparse training steps on one batch of a resident shard.

A shard of --shard-rows rows (10 M) is made on the device from a seed: 20 .. 60
entries per row (39 for the FFM shape, one per field), ids uniform in [0, F).
One batch of --batch-rows rows (65 536) is gathered from it with
ops.gather_rows, and the same batch is stepped on repeatedly:

  dense  today's path: model.loss (csr_spmv with the atomic gradient; for
         SparseFFM also csr_ffm) + backward + torch.optim.Adagrad.step
  lazy   optim.RowSparseStep(model, optim.LazyAdagrad).step

for SparseLogReg at F = 2^20, 2^24, 2^26, for SparseLogReg at F = 2^24 with a
batch in which one id occurs in every row ("skewed"), and for SparseFFM at 1 M
ids x 39 fields x k = 4.  Every step gets a fresh copy of the batch dict, as a
batch made per step is.  Before timing, one step of each path from the same
parameters is compared (largest |difference| of any parameter).

Also timed alone: ops.compact_features(batch, F) against
torch.unique(batch["index"], return_inverse=True) on the device.

Every figure is a time per step (or call): the median (and the fastest) of
--iters host-clock windows, each around --window consecutive steps (20) and
ending in a device synchronise, divided by the steps in it, after --warmup
steps of the same shape.  The two paths are timed in alternating blocks, twice;
the better block's median is reported and both are kept (``*_runs_ms``).
Prints one JSON object; a line per shape goes to stderr.

usage: python scripts/bench_lazy.py [--shard-rows N] [--batch-rows N] [--shapes a,b,...]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"logreg_2^20": ("logreg", 1 << 20), "logreg_2^24": ("logreg", 1 << 24),
          "logreg_2^26": ("logreg", 1 << 26), "logreg_2^24_skewed": ("skewed", 1 << 24),
          "ffm_1M_39x4": ("ffm", 1_000_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shard-rows", type=int, default=10_000_000)
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--iters", type=int, default=15, help="timed windows per block")
    ap.add_argument("--window", type=int, default=20, help="steps (calls) per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.05)
    args = ap.parse_args()
    for s in args.shapes.split(","):
        if s not in SHAPES:
            raise SystemExit(f"unknown shape {s!r}; known: {sorted(SHAPES)}")
    import torch

    from dmlc_core_amd import ops, optim
    from dmlc_core_amd.models import SparseFFM, SparseLogReg

    assert torch.cuda.is_available(), "bench_lazy.py measures on a GPU"
    dev = torch.device("cuda")
    fields, rank = 39, 4

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            for _ in range(args.window):
                fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.window)
        ms.sort()
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3)}

    def make_batch(kind, feats, gen):
        """the shard, then one gathered batch of it (the shard is freed)"""
        rows = args.shard_rows
        if kind == "ffm":
            lens = torch.full((rows,), fields, dtype=torch.int64, device=dev)
        else:
            lens = torch.randint(20, 61, (rows,), device=dev, generator=gen)
        offset = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offset[1:])
        nnz = int(offset[-1])
        shard = {"offset": offset,
                 "index": torch.randint(0, feats, (nnz,), device=dev, generator=gen,
                                        dtype=torch.int32),
                 "value": torch.rand(nnz, device=dev, generator=gen) + 0.5,
                 "label": (torch.rand(rows, device=dev, generator=gen) < 0.5).float()}
        if kind == "ffm":
            shard["field"] = torch.arange(fields, dtype=torch.int32, device=dev).repeat(rows)
        if kind == "skewed":
            shard["index"][offset[:-1]] = 7  # the first entry of every row
        pick = torch.randperm(rows, device=dev, generator=gen)[:args.batch_rows]
        batch = ops.gather_rows(shard, pick)
        batch.pop("_buffers", None)
        return batch

    def models(kind, feats):
        if kind == "ffm":
            return (SparseFFM(feats, fields, rank=rank, seed=1).cuda(),
                    SparseFFM(feats, fields, rank=rank, seed=1).cuda())
        return SparseLogReg(feats, grad="atomic").cuda(), SparseLogReg(feats, grad="atomic").cuda()

    res = {"shard_rows": args.shard_rows, "batch_rows": args.batch_rows, "iters": args.iters,
           "window": args.window, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        kind, feats = SHAPES[shape]
        gen = torch.Generator(device=dev).manual_seed(0)
        batch = make_batch(kind, feats, gen)
        torch.cuda.empty_cache()
        dense, lazy = models(kind, feats)
        opt = torch.optim.Adagrad(dense.parameters(), lr=args.lr, eps=1e-10)
        stepper = optim.RowSparseStep(lazy, optim.LazyAdagrad(args.lr))

        def dense_step():
            loss = dense.loss(dict(batch))
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()

        def lazy_step():
            stepper.step(dict(batch))

        # the same step first
        dense_step()
        lazy_step()
        diff = max(float((a.detach() - b.detach()).abs().max())
                   for a, b in zip(dense.parameters(), lazy.parameters()))
        nnz = batch["index"].numel()
        r = {"model": "SparseFFM" if kind == "ffm" else "SparseLogReg", "features": feats,
             "batch_nnz": nnz, "distinct_ids": int(ops.compact_features(batch, feats)["num_features"]),
             "param_bytes": sum(p.numel() * 4 for p in dense.parameters()),
             "first_step_max_abs_diff": diff}
        # alternate the two paths' timing blocks: others share the machine
        a1, b1 = timed(dense_step), timed(lazy_step)
        a2, b2 = timed(dense_step), timed(lazy_step)
        r["dense_step"], r["lazy_step"] = min(a1, a2, key=lambda t: t["ms"]), \
            min(b1, b2, key=lambda t: t["ms"])
        r["dense_step_runs_ms"], r["lazy_step_runs_ms"] = [a1["ms"], a2["ms"]], [b1["ms"], b2["ms"]]
        r["dense_over_lazy"] = round(r["dense_step"]["ms"] / r["lazy_step"]["ms"], 2)
        if kind != "ffm":
            index = batch["index"]
            got = ops.compact_features(batch, feats)
            ids, inv = torch.unique(index, return_inverse=True)
            assert torch.equal(got["ids"], ids.long()) and torch.equal(got["index"].long(), inv)
            r["compact_features"] = timed(lambda: ops.compact_features(batch, feats))
            r["torch_unique"] = timed(lambda: torch.unique(index, return_inverse=True))
            r["unique_over_compact"] = round(r["torch_unique"]["ms"] / r["compact_features"]["ms"], 2)
        res[shape] = r
        print(f"{shape}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del dense, lazy, opt, stepper, batch
        ops.release_workspace()
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
