#!/usr/bin/env python3
"""The histogram-GBDT ops on a resident shard, each against stock torch ops.

--shard parsed (the default) is bench_linear.py's shard: --shard-rows rows
(10 M) of data.write_synthetic LibSVM text in 16 files under --data (shared
with bench_linear.py, written on the first run), parsed into HBM by the GPU
parser -- about 1 M features and 400 M entries.  --shard device makes
bench_lazy.py's instead, on the device from a seed, without a file: 20 .. 60
entries per row, ids uniform in [0, --features), values in [0.5, 1.5).
--max-bins defaults to 16: a histogram is 16 bytes per (node, bin), and at 256
cuts for each of 1 M features 64 nodes would need 262 GB.

  one-time   ops.transpose, ops.feature_cuts and ops.bin_features (both on the
             cached transpose); torch: the per-column sort as two torch.sort
             (by value, then stable by column) -- the order alone, no cuts
  histogram  ops.grad_histogram at 1, 8 and 64 nodes; torch: an int64
             index_add_ per plane (g, h) over pos[row] * total_bins + global bin
             with the entries' global bins made beforehand, not timed.  The
             results are compared exactly, and 64 sampled columns are summed
             again by small torch ops.  `stream_share`: the time 5 bytes per entry take
             at the measured device copy rate, over the measured time
  splits     ops.best_splits at 8 nodes; torch: cumsum + argmax over the
             missing-right candidates only (half of GB4's work)
  advance    ops.advance_rows with those splits, per call over windows of 50
             calls back to back (a single call is mostly launch and synchronise)
  boost      one depth-6 SparseGBDT.boost (logistic)

Every figure is the median (and the fastest) of --iters host-clock windows
around one call each, ending in a device synchronise, after one warm-up call.
Prints one JSON object; a line per section goes to stderr.

usage: python scripts/bench_gbdt.py [--shard parsed|device] [--shard-rows N] [--max-bins B]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shard", choices=("parsed", "device"), default="parsed")
    ap.add_argument("--data", default="/tmp/dmlc_linear_bench", help="--shard parsed: the files")
    ap.add_argument("--shard-rows", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=1_000_000, help="--shard device only")
    ap.add_argument("--max-bins", type=int, default=16)
    ap.add_argument("--nodes", default="1,8,64")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import data, ops
    from dmlc_core_amd.models import SparseGBDT

    assert torch.cuda.is_available(), "bench_gbdt.py measures on a GPU"
    dev = torch.device("cuda")
    rows, feats = args.shard_rows, args.features

    def timed(fn, iters=args.iters):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3)}

    def note(name, r):
        res[name] = r
        print(f"{name}: {json.dumps(r)}", file=sys.stderr, flush=True)

    def ratio(a, b):
        return round(a["ms"] / b["ms"], 2)

    gen = torch.Generator(device=dev).manual_seed(0)
    if args.shard == "parsed":
        if args.shard_rows != 10_000_000:
            args.data = f"{args.data}_{args.shard_rows}"
        os.makedirs(args.data, exist_ok=True)
        nfiles = 16
        per = (rows + nfiles - 1) // nfiles
        for i in range(nfiles):
            f = os.path.join(args.data, f"part-{i:03d}.libsvm")
            if not os.path.exists(f):
                data.write_synthetic(f + ".tmp", i * per, min(rows, (i + 1) * per), seed=0,
                                     nthread=16)
                os.replace(f + ".tmp", f)
        parsed = data.GPUParser(args.data).parse_all()  # owns the arrays: kept to the end
        csr = data.csr_to_torch(parsed)
        rows, nnz, feats = int(parsed.rows), int(parsed.nnz), int(parsed.max_index) + 1
        csr["label"] = csr["label"].float()
    else:
        lens = torch.randint(20, 61, (rows,), device=dev, generator=gen)
        offset = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offset[1:])
        nnz = int(offset[-1])
        csr = {"offset": offset,
               "index": torch.randint(0, feats, (nnz,), device=dev, generator=gen,
                                      dtype=torch.int32),
               "value": torch.rand(nnz, device=dev, generator=gen) + 0.5,
               "label": (torch.rand(rows, device=dev, generator=gen) < 0.5).float()}
        del lens
    res = {"shard": args.shard, "rows": rows, "features": feats, "nnz": nnz, "max_bins": args.max_bins,
           "iters": args.iters, "device": torch.cuda.get_device_name(0)}

    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy = timed(lambda: dst.copy_(src))
    res["copy_gb_s"] = round(2 * src.numel() / copy["ms"] / 1e6, 1)  # bytes read + written
    del src, dst
    stream_ms = 5 * nnz / (res["copy_gb_s"] * 1e6)
    res["stream_ms"] = round(stream_ms, 3)

    # ------------------------------------------------------------ one-time costs
    note("transpose", timed(lambda: ops.transpose(csr, feats), 2))
    cuts = ops.feature_cuts(csr, feats, args.max_bins)  # caches the transpose in csr
    note("feature_cuts", timed(lambda: ops.feature_cuts(csr, feats, args.max_bins), 2))
    note("bin_features", timed(lambda: ops.bin_features(csr, cuts, feats), 2))
    if not args.skip_torch and csr.get("value") is not None:
        index = csr["index"]
        if index.dtype == torch.uint32:
            index = index.view(torch.int32)  # ids < 2^31: the same order

        def torch_column_sort():
            v, i1 = torch.sort(csr["value"][:nnz])
            _, i2 = torch.sort(index[:nnz][i1], stable=True)
            return v[i2]
        note("torch_column_sort", timed(torch_column_sort, 2))
        res["column_sort_over_feature_cuts"] = ratio(res["torch_column_sort"], res["feature_cuts"])
    binned = ops.bin_features(csr, cuts, feats)
    total = int(cuts["cut"].numel())
    res["total_bins"] = total
    del csr["transpose"]
    ops.release_workspace()
    torch.cuda.empty_cache()

    # ---------------------------------------------------------------- histogram
    g = torch.randn(rows, device=dev, generator=gen)
    h = torch.rand(rows, device=dev, generator=gen)
    scale = ops.gradient_scale(g, h)
    if not args.skip_torch:
        counts = binned["offset"][1:] - binned["offset"][:-1]
        gbin = torch.repeat_interleave(binned["cut_ptr"][:-1], counts) + binned["bin"].long()
        row64 = binned["row"].long()
        del counts
    qg = torch.round(g.double() * scale).long()
    qh = torch.round(h.double() * scale).long()

    def sampled_columns_equal(hist, pos, n, samples=64):
        """the histogram's cells of `samples` features against sums over each
        one's few hundred entries: small torch ops only"""
        col_ptr, cut_ptr = binned["offset"], binned["cut_ptr"]
        picks = torch.randint(0, feats, (samples,), generator=torch.Generator().manual_seed(n))
        ends = torch.stack([col_ptr[picks.to(dev)], col_ptr[picks.to(dev) + 1],
                            cut_ptr[picks.to(dev)], cut_ptr[picks.to(dev) + 1]]).tolist()
        for lo, hi, c0, c1 in zip(*ends):
            r = binned["row"][lo:hi].long()
            cell = pos[r].long() * (c1 - c0) + binned["bin"][lo:hi].long()
            want = torch.zeros((2, n * (c1 - c0)), dtype=torch.int64, device=dev)
            want[0].index_add_(0, cell, qg[r])
            want[1].index_add_(0, cell, qh[r])
            got = hist[:, c0:c1, :].permute(2, 0, 1).reshape(2, -1)
            if not torch.equal(want, got):
                return False
        return True

    hist8 = pos8 = None
    for n in (int(s) for s in args.nodes.split(",")):
        pos = torch.randint(0, n, (rows,), device=dev, generator=gen, dtype=torch.int32)
        r = timed(lambda: ops.grad_histogram(binned, g, h, pos, n, scale))
        r["stream_share"] = round(stream_ms / r["ms"], 3)
        r["hist_gb"] = round(n * total * 16 / 1e9, 2)
        note(f"grad_histogram_{n}", r)
        hist = ops.grad_histogram(binned, g, h, pos, n, scale)
        res[f"grad_histogram_{n}_sampled_columns_equal"] = sampled_columns_equal(hist, pos, n)
        if not args.skip_torch:
            def torch_hist():
                # one plane each for g and h, 1-D gathers: the 2-D form (q[row] with q
                # [rows, 2] and 400 M row ids) gave sums no input can produce when measured
                flat = pos[binned["row"]].long() * total + gbin
                out = torch.zeros((2, n * total), dtype=torch.int64, device=dev)
                out[0].index_add_(0, flat, qg[row64])
                out[1].index_add_(0, flat, qh[row64])
                return out
            try:
                want = torch_hist()
                res[f"grad_histogram_{n}_equal"] = bool(
                    torch.equal(want[0].view(n, total), hist[..., 0])
                    and torch.equal(want[1].view(n, total), hist[..., 1]))
                del want
                note(f"torch_index_add_{n}", timed(torch_hist, 3))
                res[f"index_add_over_histogram_{n}"] = ratio(res[f"torch_index_add_{n}"], r)
            except torch.cuda.OutOfMemoryError:
                res[f"torch_index_add_{n}"] = "out of memory"
                torch.cuda.empty_cache()
        if n == 8 or hist8 is None:
            hist8, pos8 = hist, pos
        del hist

    # ------------------------------------------------------------------- splits
    n8 = hist8.shape[0]
    qgh = torch.stack([torch.round(g.double() * scale), torch.round(h.double() * scale)], 1).long()
    node_sum = torch.zeros((n8, 2), dtype=torch.int64, device=dev)
    node_sum.index_add_(0, pos8.long(), qgh)
    cut_ptr = binned["cut_ptr"]
    note(f"best_splits_{n8}", timed(lambda: ops.best_splits(hist8, node_sum, cut_ptr, scale)))
    split = ops.best_splits(hist8, node_sum, cut_ptr, scale)
    res["splits_found"] = int((split["feature"] >= 0).sum())
    if not args.skip_torch:
        feat_of_bin = torch.repeat_interleave(torch.arange(feats, device=dev),
                                              cut_ptr[1:] - cut_ptr[:-1])
        base_at = cut_ptr[:-1][feat_of_bin]

        def torch_splits():
            csum = torch.cumsum(hist8, 1)
            zero = torch.zeros((n8, 1, 2), dtype=torch.int64, device=dev)
            before = torch.cat([zero, csum], 1)[:, base_at]
            left = (csum - before).double() / scale
            tot = node_sum.double()[:, None, :] / scale
            right = tot - left
            gain = 0.5 * (left[..., 0] ** 2 / (left[..., 1] + 1.0)
                          + right[..., 0] ** 2 / (right[..., 1] + 1.0)
                          - tot[..., 0] ** 2 / (tot[..., 1] + 1.0))
            gain = torch.where((left[..., 1] >= 1.0) & (right[..., 1] >= 1.0), gain,
                               torch.full_like(gain, -1.0))
            return torch.argmax(gain, 1)
        try:
            note(f"torch_cumsum_argmax_{n8}", timed(torch_splits, 3))
            res["cumsum_argmax_over_best_splits"] = ratio(res[f"torch_cumsum_argmax_{n8}"],
                                                          res[f"best_splits_{n8}"])
        except torch.cuda.OutOfMemoryError:
            res[f"torch_cumsum_argmax_{n8}"] = "out of memory"
            torch.cuda.empty_cache()
        del feat_of_bin, base_at, gbin, row64

    # ------------------------------------------------------------------ advance
    ids = torch.arange(n8, dtype=torch.int32, device=dev)
    left, right = (n8 + 2 * ids).contiguous(), (n8 + 2 * ids + 1).contiguous()
    def advance_window(calls=50):  # a sub-0.1 ms op: one window of back-to-back calls per figure
        for _ in range(calls):
            ops.advance_rows(binned, pos8, split, left, right)
    r = timed(advance_window)
    note(f"advance_rows_{n8}", {"ms": round(r["ms"] / 50, 4), "ms_min": round(r["ms_min"] / 50, 4),
                                "calls_per_window": 50})
    del hist8, pos8
    torch.cuda.empty_cache()

    # -------------------------------------------------------------------- boost
    model = SparseGBDT(feats, max_bins=args.max_bins, max_depth=6)
    note("boost_depth6", timed(lambda: model.boost(binned, csr["label"]), 2))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
