#!/usr/bin/env python3
"""Row gather (G1 / G2, ops.gather_rows) on the synthetic 10 M-row LibSVM set
parsed into HBM: (a) a 65 536-row random batch into reused out= buffers, (b) a
whole-shard permutation, and (c) the same outputs built from stock torch ops
(cumsum / repeat_interleave / advanced indexing) -- what a user could do
without the kernels, the baseline.  A clone() of the same number of entry
bytes is the copy yardstick.  Every time is a host clock around calls that end
in a device synchronise (gather_rows reads its 16-byte status itself), after
warm-up; GB/s counts bytes read plus bytes written of index, value and the
row pointers.  Prints one JSON object.

usage: python scripts/bench_gather.py [--rows N] [--batch-rows B] [--shape S] [--iters K]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUM_PARTS = 16


def ensure_data(d, rows, shape):
    from dmlc_core_amd import data

    os.makedirs(d, exist_ok=True)
    per = (rows + NUM_PARTS - 1) // NUM_PARTS
    for p in range(NUM_PARTS):
        f = os.path.join(d, f"part-{p:05d}.libsvm")
        if not os.path.exists(f):
            data.write_synthetic(f + ".tmp", p * per, min(rows, (p + 1) * per), format="libsvm",
                                 seed=0, nthread=16, shape=shape)
            os.replace(f + ".tmp", f)


def torch_gather(t, rows):
    """gather_rows' offset / index / value from stock torch ops"""
    import torch

    off = t["offset"].view(torch.int64)
    start = off[rows]
    lens = off[rows + 1] - start
    out_off = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rows.device)
    torch.cumsum(lens, 0, out=out_off[1:])
    nnz = int(out_off[-1])  # the one host read, as in gather_rows
    src = torch.repeat_interleave(start - out_off[:-1], lens, output_size=nnz)
    src += torch.arange(nnz, dtype=torch.int64, device=rows.device)
    return {"offset": out_off, "index": t["index"].view(torch.int32)[src], "value": t["value"][src]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--shape", default="uniform", choices=["uniform", "skewed", "mixed"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--data", default="/tmp/dmlc_gather_bench")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import data, ops

    assert torch.cuda.is_available(), "bench_gather.py measures on the GPU only"
    d = os.path.join(args.data, f"libsvm_{args.rows}r_{args.shape}")
    ensure_data(d, args.rows, args.shape)
    csr = data.GPUParser(d).parse_all()
    t = data.csr_to_torch(csr)
    src = {"offset": t["offset"], "index": t["index"], "value": t["value"]}
    nrows = csr.rows
    off = t["offset"].view(torch.int64)

    def timed(fn, iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    def case(name, rows, iters):
        nnz = int((off[rows + 1] - off[rows]).sum())
        n_sel = rows.numel()
        # index + value read and written, per row: its id, two source row
        # pointers read, one batch row pointer written
        nbytes = nnz * 16 + n_sel * 32
        res = {"rows": n_sel, "nnz": nnz, "bytes": nbytes}
        out = ops.gather_rows(src, rows)
        ref = torch_gather(src, rows)
        same = all(torch.equal(out[k].view(torch.int32) if k != "offset" else out[k],
                               ref[k].view(torch.int32) if k != "offset" else ref[k])
                   for k in ("offset", "index", "value"))
        res["matches_torch_composite"] = bool(same)
        del ref
        yard_i = torch.empty(nnz, dtype=torch.int32, device="cuda")
        yard_v = torch.empty(nnz, dtype=torch.float32, device="cuda")
        box = {}

        def clone():
            box["i"], box["v"] = yard_i.clone(), yard_v.clone()

        def composite():
            box["c"] = torch_gather(src, rows)

        # alternate the three so that drift hits them alike
        ms = {"gather_rows_out": [], "gather_rows_alloc": [], "torch_composite": [], "clone": []}
        for _ in range(3):
            ms["gather_rows_out"].append(timed(lambda: ops.gather_rows(src, rows, out=out), iters))
            ms["gather_rows_alloc"].append(timed(lambda: ops.gather_rows(src, rows), iters))
            ms["torch_composite"].append(timed(composite, max(1, iters // 4)))
            box.clear()
            ms["clone"].append(timed(clone, iters))
            box.clear()
        for k, v in ms.items():
            best = min(v)
            by = nnz * 16 if k == "clone" else nbytes
            res[k] = {"ms": round(best, 4), "ms_runs": [round(x, 4) for x in v],
                      "GBps": round(by / best / 1e6, 1)}
        res["speedup_vs_torch_composite"] = round(
            res["torch_composite"]["ms"] / res["gather_rows_out"]["ms"], 2)
        print(f"# {name}: {json.dumps(res)}", file=sys.stderr, flush=True)
        return res

    g = torch.Generator().manual_seed(0)
    batch = torch.randint(0, nrows, (min(args.batch_rows, nrows),), generator=g).cuda()
    result = {"rows": nrows, "nnz": csr.nnz, "shape": args.shape,
              "run_entries": ops._dmlc.csr_gather_run_entries(),
              "device": torch.cuda.get_device_name(0),
              "batch": case("batch", batch, args.iters),
              "permutation": case("permutation", data.row_order(nrows, 0, 0).cuda(),
                                  max(3, args.iters // 4))}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
