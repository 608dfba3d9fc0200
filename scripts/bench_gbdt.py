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
  predict    8 depth-6 trees over the shard: SparseGBDT.predict(method="levels")
             (bin_features on the cached transpose, then a GB5 launch per tree
             and level) against method="rows" (GB6, one launch, the packed forest
             cached) and ops.pack_forest alone.  The two margin vectors must be
             equal bit for bit.  `rows_share`: the time one pass over the CSR's
             bytes takes at the measured device copy rate, over the measured time
             --vector-leaves K[,K..]: the same trees with random [size, K] leaves in
             a softmax model (a K-output histogram of 1 M features does not fit):
             method="rows" (GB6m, one launch) against what it replaced, GB6's leaf
             ids and a torch gather and add per tree; the margins must be equal

  --outputs K  instead of the sections after `one-time`: ops.grad_histogram_multi
             and ops.best_splits_multi (GB3m / GB4m, K gradients per row) at each
             of --nodes, against K calls of the scalar op on the K columns made
             contiguous beforehand (for the splits: on the K planes of the
             histogram), which is how the same sums were had without them.  The
             histograms are compared exactly

  --fused    instead of the sections after `one-time`: ops.level_splits (GB9) against
             ops.grad_histogram + ops.best_splits at each of --nodes, their windows
             alternating, and the outputs compared exactly; then a depth-6
             SparseGBDT.boost with split_search "fused" and "histogram" (the trees
             compared).  `peak_allocated_gb`: torch's peak during one level_splits
             call, the shard, the binned matrix and the scratch included.
             --fused only: level_splits alone, for a shape whose histogram does not fit

Every figure is the median (and the fastest, the slowest) of --iters host-clock windows
around one call each, ending in a device synchronise, after one warm-up call.
Prints one JSON object; a line per section goes to stderr.

usage: python scripts/bench_gbdt.py [--shard parsed|device] [--shard-rows N] [--max-bins B]
                                    [--outputs K]
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
    ap.add_argument("--vector-leaves", default="", help="the predict section: these K too")
    ap.add_argument("--outputs", type=int, default=0,
                    help="K > 0: only the one-time section and the K-output ops")
    ap.add_argument("--fused", nargs="?", const="on", default="off", choices=("off", "on", "only"),
                    help="only the one-time section and ops.level_splits (GB9) against "
                         "grad_histogram + best_splits; 'only': without the two-step path")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import _dmlc, data, ops
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
        return {"ms": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3),
                "ms_max": round(ms[-1], 3)}

    def timed_pair(a, b):
        """`timed` for two ways to the same result, their windows alternating"""
        a(), b()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(args.iters):
            for fn, out in zip((a, b), ms):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
        return [{"ms": round(sorted(m)[len(m) // 2], 3), "ms_min": round(min(m), 3),
                 "ms_max": round(max(m), 3)} for m in ms]

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

    # ------------------------------------------------- K outputs (--outputs only)
    if args.outputs > 0:
        K = args.outputs
        res["outputs"] = K
        gk = torch.randn((rows, K), device=dev, generator=gen)
        hk = torch.rand((rows, K), device=dev, generator=gen)
        scale = ops.gradient_scale(gk, hk)
        qgh = torch.stack([torch.round(gk.double() * scale), torch.round(hk.double() * scale)],
                          2).long()
        cols = [(gk[:, k].contiguous(), hk[:, k].contiguous()) for k in range(K)]  # not timed
        cut_ptr = binned["cut_ptr"]

        for n in (int(s) for s in args.nodes.split(",")):
            pos = torch.randint(0, n, (rows,), device=dev, generator=gen, dtype=torch.int32)

            def scalar_histograms():
                for g1, h1 in cols:
                    ops.grad_histogram(binned, g1, h1, pos, n, scale)
            r, r1 = timed_pair(lambda: ops.grad_histogram_multi(binned, gk, hk, pos, n, scale),
                               scalar_histograms)
            r["hist_gb"] = round(n * total * K * 16 / 1e9, 2)
            note(f"grad_histogram_multi_{n}", r)
            note(f"grad_histogram_x{K}_{n}", r1)
            res[f"scalar_over_multi_histogram_{n}"] = ratio(r1, r)
            hist = ops.grad_histogram_multi(binned, gk, hk, pos, n, scale)
            per_k = [hist[:, :, k].contiguous() for k in range(K)]
            res[f"grad_histogram_multi_{n}_equal"] = all(
                torch.equal(per_k[k], ops.grad_histogram(binned, *cols[k], pos, n, scale))
                for k in range(K))
            node_sum = torch.zeros((n, K, 2), dtype=torch.int64, device=dev)
            node_sum.index_add_(0, pos.long(), qgh)
            sums_k = [node_sum[:, k].contiguous() for k in range(K)]

            def scalar_splits():
                for k in range(K):
                    ops.best_splits(per_k[k], sums_k[k], cut_ptr, scale)
            r, r1 = timed_pair(lambda: ops.best_splits_multi(hist, node_sum, cut_ptr, scale),
                               scalar_splits)
            note(f"best_splits_multi_{n}", r)
            note(f"best_splits_x{K}_{n}", r1)
            res[f"scalar_over_multi_splits_{n}"] = ratio(r1, r)
            split = ops.best_splits_multi(hist, node_sum, cut_ptr, scale)
            res[f"splits_found_multi_{n}"] = int((split["feature"] >= 0).sum())
            del hist, per_k, node_sum, sums_k
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        return

    # ------------------------------------------- fused level search (--fused only)
    if args.fused != "off":
        g = torch.randn(rows, device=dev, generator=gen)
        h = torch.rand(rows, device=dev, generator=gen)
        scale = ops.gradient_scale(g, h)
        qgh = torch.stack([torch.round(g.double() * scale), torch.round(h.double() * scale)],
                          1).long()
        cut_ptr = binned["cut_ptr"]
        lens = binned["offset"][1:] - binned["offset"][:-1]
        res["long_columns"] = int((lens > int(_dmlc.gbdt_segment_entries())).sum())
        del lens
        for n in (int(s) for s in args.nodes.split(",")):
            pos = torch.randint(0, n, (rows,), device=dev, generator=gen, dtype=torch.int32)
            node_sum = torch.zeros((n, 2), dtype=torch.int64, device=dev)
            node_sum.index_add_(0, pos.long(), qgh)

            def fused():
                return ops.level_splits(binned, g, h, pos, node_sum, scale)

            def two_step():
                return ops.best_splits(ops.grad_histogram(binned, g, h, pos, n, scale), node_sum,
                                       cut_ptr, scale)
            if args.fused == "only":  # a shape whose histogram does not fit
                r = timed(fused)
            else:
                r, r1 = timed_pair(fused, two_step)
                note(f"histogram_then_best_splits_{n}", r1)
                res[f"two_step_over_fused_{n}"] = ratio(r1, r)
                got, want = fused(), two_step()
                res[f"level_splits_{n}_equal"] = all(torch.equal(got[k], want[k]) for k in got)
            r["hist_gb"] = round(n * total * 16 / 1e9, 2)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            fused()  # its workspace is warm: the figure is what stays allocated, scratch included
            torch.cuda.synchronize()
            r["peak_allocated_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
            note(f"level_splits_{n}", r)
            res[f"splits_found_{n}"] = int((fused()["feature"] >= 0).sum())
            torch.cuda.empty_cache()
        if args.fused == "on":
            models = [SparseGBDT(feats, max_bins=args.max_bins, max_depth=6, split_search=s)
                      for s in ("fused", "histogram")]
            r, r1 = timed_pair(*(lambda m=m: m.boost(binned, csr["label"]) for m in models))
            note("boost_depth6_fused", r)
            note("boost_depth6_histogram", r1)
            res["boost_trees_equal"] = all(
                torch.equal(a[k], b[k]) for a, b in zip(models[0].trees, models[1].trees) for k in a)
        print(json.dumps(res), flush=True)
        return

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

    # ------------------------------------------------------------------ predict
    while len(model.trees) < 8:
        model.boost(binned, csr["label"])
    del model.trees[8:]
    del binned
    torch.cuda.empty_cache()
    note("predict_levels_8", timed(lambda: model.predict(csr), 3))
    csr.pop("transpose", None)  # the levels path's, cached by its first call
    ops.release_workspace()
    torch.cuda.empty_cache()
    note("pack_forest_8", timed(lambda: ops.pack_forest(model.trees, model.cuts)))
    r = timed(lambda: model.predict(csr, method="rows"))
    csr_bytes = sum(csr[k].numel() * csr[k].element_size() for k in ("offset", "index", "value")
                    if csr.get(k) is not None)
    r["rows_share"] = round(csr_bytes / (res["copy_gb_s"] * 1e6) / r["ms"], 3)
    note("predict_rows_8", r)
    res["levels_over_rows"] = ratio(res["predict_levels_8"], r)
    res["predict_trees_with_splits"] = sum(int(t["feature"][0]) >= 0 for t in model.trees)
    assert torch.equal(model.predict(csr, method="rows"), model.predict(csr)), \
        "predict: the rows path and the levels path differ"
    for K in (int(s) for s in args.vector_leaves.split(",") if s):
        multi = SparseGBDT(feats, max_bins=args.max_bins, max_depth=6, objective="softmax",
                           num_outputs=K)
        multi.cuts = model.cuts
        multi.trees = [dict(t, leaf=torch.randn((t["leaf"].numel(), K), device=dev, generator=gen))
                       for t in model.trees]

        def gathered():  # method="rows" before GB6m; model's forest: the same nodes, cached
            ids = ops.predict_forest(csr, model._forest(), "leaf")
            margin = torch.zeros((rows, K), dtype=torch.float32, device=dev)
            for t, tree in enumerate(multi.trees):
                margin = margin + tree["leaf"][ids[:, t].long()]
            return margin
        r, r1 = timed_pair(lambda: multi.predict(csr, method="rows"), gathered)
        note(f"predict_rows_8_K{K}", r)
        note(f"predict_leaf_ids_torch_gather_8_K{K}", r1)
        res[f"gather_over_rows_K{K}"] = ratio(r1, r)
        assert torch.equal(multi.predict(csr, method="rows"), gathered()), \
            "predict: GB6m and the gathered leaves differ"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
