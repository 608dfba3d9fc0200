#!/usr/bin/env python3
"""RK1 / RK2 in boost mode against their loss mode on the same inputs:
ops.rank_grad_hess(..., validate=False) next to ops.rank_loss_parts(...,
validate=False), random f32 scores with labels 0 .. 4 made on the device from a
seed, for two shapes of query groups:

  len24   --rows rows (10 M) in groups of 24: every group on RK1 (one wave each)
  long    --long-groups (512) groups of --long-rows (3000) rows: every group on
          RK2 (one workgroup each)

Per shape and weighting it checks first that the boost mode's gradient with
normalize="pairs" is torch.equal to the loss mode's and that hess >= 0, then
times both: the median of --iters device-event timings of one call after
--warmup calls, the fastest next to it (zero fills of the outputs included:
two [rows] fills for the boost mode; one and two [groups] fills for the loss
mode).  Prints one JSON object.

usage: python scripts/bench_rank_boost.py [--rows N] [--shapes len24,long]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-groups", type=int, default=512)
    ap.add_argument("--long-rows", type=int, default=3000)
    ap.add_argument("--shapes", default="len24,long")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=1.0)
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import ops

    assert torch.cuda.is_available(), "bench_rank_boost.py measures on a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3)}

    res = {"sigma": args.sigma, "iters": args.iters, "warmup": args.warmup,
           "wave_group_rows": int(ops._dmlc.rank_wave_group_rows()),
           "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        if shape == "len24":
            n, groups = 24, args.rows // 24
        elif shape == "long":
            n, groups = args.long_rows, args.long_groups
        else:
            raise SystemExit(f"unknown shape {shape!r}")
        rows = n * groups
        score = torch.randn(rows, device=dev, generator=gen)
        label = torch.randint(0, 5, (rows,), device=dev, generator=gen).float()
        ptr = torch.arange(groups + 1, device=dev, dtype=torch.int64) * n
        r = {"rows": rows, "groups": groups, "group_rows": n, "pair_evals": groups * n * n}
        for weighting in ("ndcg", "none"):
            grad, hess = ops.rank_grad_hess(score, label, ptr, weighting, args.sigma, "pairs")
            assert torch.equal(grad, ops.rank_loss_parts(score, label, ptr, weighting, args.sigma)[2])
            assert float(hess.min()) >= 0 and float(hess.max()) > 0
            del grad, hess
            loss = timed(lambda: ops.rank_loss_parts(score, label, ptr, weighting, args.sigma,
                                                     validate=False))
            boost = timed(lambda: ops.rank_grad_hess(score, label, ptr, weighting, args.sigma,
                                                     "none", validate=False))
            boost["Gpairs_per_s"] = round(r["pair_evals"] / boost["ms"] / 1e6, 2)
            r[f"rank_loss_{weighting}"], r[f"rank_grad_hess_{weighting}"] = loss, boost
            r[f"boost_over_loss_{weighting}"] = round(boost["ms"] / loss["ms"], 3)
        res[shape] = r
        print(f"{shape}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del score, label, ptr
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
