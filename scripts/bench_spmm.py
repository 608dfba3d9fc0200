#!/usr/bin/env python3
"""M1 / M1p / M2 at scripts/bench_linear.py's shape: a 10 M x 1 M CSR with
400 M entries (20 .. 60 per row, uniform ids, as data.write_synthetic's
default), made on the device from a seed.  For k in 4, 16, 64, 256:

  spmm          ops.spmm(X, W)                      (M1)
  spmm_t        ops.spmm_t(X, D, F)                 (M2, atomic X^T D)
  spmm_gather   ops.spmm(transpose(X), D)           (M1p, gather X^T D)

against what the project offered before (k calls of ops.spmv / ops.spmv_t, one
per column, without the cost of cutting columns out of W; actually run for
k <= 16, k times one call above that and marked so) and torch.sparse.mm over
data.to_sparse_csr.  Every figure is the median of --iters HIP-event timings
after --warmup calls of the same shape, with the fastest next to it; GB/s
are the bytes the product needs over that time: the CSR, plus nnz * 4k
gathered (added, for spmm_t), plus out_rows * 4k written (read, for spmm_t).
Prints one JSON object.

usage: python scripts/bench_spmm.py [--rows N] [--features F] [--iters K] [--ks 4,16,64,256]
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
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="4,16,64,256")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.sparse.mm yardstick")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import data, ops

    assert torch.cuda.is_available(), "bench_spmm.py measures on a GPU"
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    lens = torch.randint(20, 61, (args.rows,), device=dev, generator=g)
    offset = torch.zeros(args.rows + 1, dtype=torch.int64, device=dev)
    offset[1:] = torch.cumsum(lens, 0)
    nnz, nrows, nfeat = int(offset[-1]), args.rows, args.features
    t = {"offset": offset,
         "index": torch.randint(0, nfeat, (nnz,), device=dev, generator=g, dtype=torch.int32),
         "value": torch.randn(nnz, device=dev, generator=g)}
    del lens

    def timed(fn, iters=args.iters, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3)}

    def with_rate(r, nbytes):
        r["GBps"] = round(nbytes / r["ms"] / 1e6, 1)
        return r

    csr_bytes = nnz * 8 + (nrows + 1) * 8
    csc_bytes = nnz * 8 + (nfeat + 1) * 8
    res = {"rows": nrows, "nnz": nnz, "num_features": nfeat, "iters": args.iters,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    tt = ops.transpose(t, nfeat)
    w1 = torch.randn(nfeat, device=dev) * 0.01
    d1 = torch.randn(nrows, device=dev)
    res["spmv"] = timed(lambda: ops.spmv(t, w1))
    res["spmv_t"] = timed(lambda: ops.spmv_t(t, d1, nfeat))
    res["spmv_gather"] = timed(lambda: ops.spmv(tt, d1))
    xs = None if args.no_torch else data.to_sparse_csr(t, nfeat)
    for k in (int(s) for s in args.ks.split(",")):
        w = torch.randn(nfeat, k, device=dev) * 0.01
        d = torch.randn(nrows, k, device=dev)
        gathered = nnz * 4 * k
        r = {"spmm": with_rate(timed(lambda: ops.spmm(t, w)), csr_bytes + gathered + nrows * 4 * k),
             "spmm_t": with_rate(timed(lambda: ops.spmm_t(t, d, nfeat)),
                                 csr_bytes + gathered + nrows * 4 * k),
             "spmm_gather": with_rate(timed(lambda: ops.spmm(tt, d)),
                                      csc_bytes + gathered + nfeat * 4 * k)}
        if k <= 16:
            def k_spmv():
                for _ in range(k):
                    ops.spmv(t, w1)

            def k_spmv_t():
                for _ in range(k):
                    ops.spmv_t(t, d1, nfeat)

            def k_gather():
                for _ in range(k):
                    ops.spmv(tt, d1)

            r["k_spmv_calls"] = dict(timed(k_spmv), run=True)
            r["k_spmv_t_calls"] = dict(timed(k_spmv_t, iters=3, warmup=1), run=True)
            r["k_spmv_gather_calls"] = dict(timed(k_gather), run=True)
        else:
            for name, one in (("k_spmv_calls", "spmv"), ("k_spmv_t_calls", "spmv_t"),
                              ("k_spmv_gather_calls", "spmv_gather")):
                r[name] = {"ms": round(k * res[one]["ms"], 3), "run": False}
        if xs is not None:
            try:
                r["torch_sparse_mm"] = with_rate(timed(lambda: torch.sparse.mm(xs, w)),
                                                 csr_bytes + gathered + nrows * 4 * k)
            except RuntimeError as err:  # say so; no figure is made up
                r["torch_sparse_mm"] = {"error": str(err)[:200]}
        res[f"k{k}"] = r
        print(f"k={k}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del w, d
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
