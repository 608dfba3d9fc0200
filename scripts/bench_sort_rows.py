#!/usr/bin/env python3
"""ops.sort_rows (SR0 - SR3) on two resident shards whose rows were shuffled:

  linear  the bench_linear.py shard: --linear-rows rows of the synthetic LibSVM
          set parsed into HBM (ragged rows), sorted by id
  ffm     the bench_ffm.py shard: --ffm-rows rows of 39 entries, one per field,
          ids uniform in 1 M, made on the device from a seed, sorted by field

For each: sort_rows against the only formulation stock torch offers, one global
stable torch.sort of (row << 32 | key) over all entries with the row id rebuilt
per entry (repeat_interleave) and the columns gathered through the permutation;
the outputs are compared first.  For ffm also ops.ffm_t (FF2, k = 4) on the
shuffled rows against the same rows after sort_rows(by="field"), the sort's
cost in FF2 gradient calls, and the calls after which sorting once has paid.
Every figure is the median of --iters HIP-event timings after --warmup calls,
with the fastest next to it.  Prints one JSON object.

usage: python scripts/bench_sort_rows.py [--linear-rows N] [--ffm-rows N] [--skip-linear]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--linear-rows", type=int, default=10_000_000)
    ap.add_argument("--ffm-rows", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--data", default="/tmp/dmlc_linear_bench")
    ap.add_argument("--skip-linear", action="store_true")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import data, ops

    assert torch.cuda.is_available(), "bench_sort_rows.py measures on a GPU"
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

    def row_ids(csr):
        rows = csr["offset"].numel() - 1
        return torch.repeat_interleave(torch.arange(rows, device=dev), csr["offset"].diff())

    def torch_sort(csr, by):
        """the same outputs from one global sort (the row pointer does not change)"""
        key = csr["index"].long()
        if by == "field":  # (row, field, id): fields < 64, ids < 2^32
            key = ((row_ids(csr) * 64 + csr["field"].long()) << 32) | key
        else:
            key = (row_ids(csr) << 32) | key
        perm = torch.sort(key, stable=True)[1]
        return {k: csr[k][perm] for k in ("index", "value", "field") if csr.get(k) is not None}

    def shuffled_rows(csr):
        perm = torch.sort((row_ids(csr) << 32) | torch.randint(
            0, 1 << 31, (csr["index"].numel(),), device=dev, generator=gen))[1]
        return dict(csr, **{k: csr[k][perm].contiguous() for k in ("index", "value", "field")
                            if csr.get(k) is not None})

    def measure(csr, by):
        got, want = ops.sort_rows(csr, by), torch_sort(csr, by)
        same = all(torch.equal(got[k], want[k]) for k in want)
        del got, want
        r = {"rows": csr["offset"].numel() - 1, "nnz": csr["index"].numel(), "by": by,
             "same_outputs_as_torch": same}
        r["sort_rows"] = timed(lambda: ops.sort_rows(csr, by))
        r["torch_sort"] = timed(lambda: torch_sort(csr, by))
        r["speedup"] = round(r["torch_sort"]["ms"] / r["sort_rows"]["ms"], 2)
        r["row_order"] = timed(lambda: ops.row_order(csr, by))
        return r

    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup}
    if not args.skip_linear:
        os.makedirs(args.data, exist_ok=True)
        nfiles = 16
        per = (args.linear_rows + nfiles - 1) // nfiles
        for i in range(nfiles):
            f = os.path.join(args.data, f"part-{i:03d}.libsvm")
            if not os.path.exists(f):
                data.write_synthetic(f + ".tmp", i * per, min(args.linear_rows, (i + 1) * per),
                                     seed=0, nthread=16)
                os.replace(f + ".tmp", f)
        t = data.csr_to_torch(data.GPUParser(args.data).parse_all())
        signed = torch.int32 if t["index"].element_size() == 4 else torch.int64  # torch indexes these
        t = shuffled_rows({"offset": t["offset"].view(torch.int64),
                           "index": t["index"].view(signed), "value": t.get("value")})
        res["linear"] = measure(t, "index")
        del t
        ops.release_workspace()
        torch.cuda.empty_cache()

    rows, n, nfeat, k = args.ffm_rows, 39, 1_000_000, 4
    csr = {"offset": torch.arange(0, rows * n + 1, n, dtype=torch.int64, device=dev),
           "index": torch.randint(0, nfeat, (rows * n,), device=dev, generator=gen,
                                  dtype=torch.int32),
           "field": torch.arange(n, dtype=torch.int32, device=dev).repeat(rows),
           "value": torch.randn(rows * n, device=dev, generator=gen)}
    shuffled = shuffled_rows(csr)
    del csr
    r = measure(shuffled, "field")
    ordered = ops.sort_rows(shuffled, "field")
    g = torch.randn(rows, device=dev, generator=gen)
    v = torch.randn(nfeat, n, k, device=dev, generator=gen) * 0.1
    r["ffm_t_shuffled"] = timed(lambda: ops.ffm_t(shuffled, g, v))
    r["ffm_t_sorted"] = timed(lambda: ops.ffm_t(ordered, g, v))
    r["sort_in_ffm_t_calls"] = round(r["sort_rows"]["ms"] / r["ffm_t_sorted"]["ms"], 2)
    saved = r["ffm_t_shuffled"]["ms"] - r["ffm_t_sorted"]["ms"]
    r["calls_until_paid"] = round(r["sort_rows"]["ms"] / saved, 2) if saved > 0 else None
    res["ffm"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
