#!/usr/bin/env python3
"""Q1 / Q2 and RK1 / RK2 (ops.qid_groups, ops.rank_loss_parts, ops.ndcg) on
--rows rows (10 M) of random scores with labels 0 .. 4, made on the device from
a seed, for three shapes of query groups:

  len24      every group 24 rows (the Yahoo set's typical query)
  len120     lengths uniform in 60 .. 180
  long_tail  lengths uniform in 1 .. 79, and one group in a thousand uniform in
             300 .. 3000: those run on RK2 (one workgroup per group)

Per shape it times

  qid_groups       ops.qid_groups(qid)                      (Q1, K3 scan, Q2, one read)
  rank_loss_ndcg   ops.rank_loss_parts(..., "ndcg", validate=False)
  rank_loss_none   ops.rank_loss_parts(..., "none", validate=False)
  ndcg10           ops.ndcg(..., k=10, validate=False)

against the same outputs from stock torch ops on the same device: the groups
sorted by length and padded to the longest of their chunk, a chunk holding as
many groups as keep one [groups, L, L] f32 intermediate within --torch-mb MB;
ranks by comparison counts, the pair terms as [groups, L, L] tensors
(softplus / sigmoid), the gradient scattered back to the rows.  The chunk plan
is made once, outside the timed region.  Both sets of outputs are compared
first (largest difference over the largest magnitude).  Every HIP figure is the
median of --iters device-event timings after --warmup calls of the same shape,
with the fastest next to it; the torch figures take --torch-iters after one
warm-up.  pair_evals is sum n^2 over the groups, the pair terms the gather form
evaluates, and Gpairs_per_s that over the median.  Prints one JSON object.

usage: python scripts/bench_rank.py [--rows N] [--shapes len24,len120,long_tail] [--torch-mb MB]
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
    ap.add_argument("--shapes", default="len24,len120,long_tail")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--torch-mb", type=float, default=64.0,
                    help="size of one [groups, L, L] f32 intermediate of the torch formulation")
    ap.add_argument("--sigma", type=float, default=1.0)
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import ops

    assert torch.cuda.is_available(), "bench_rank.py measures on a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, sigma = args.rows, args.sigma
    score = torch.randn(rows, device=dev, generator=gen)
    label = torch.randint(0, 5, (rows,), device=dev, generator=gen).float()

    def lengths(shape):
        """group lengths that sum to `rows` exactly (the last one is cut)"""
        if shape == "len24":
            lens = torch.full(((rows + 23) // 24,), 24, dtype=torch.int64, device=dev)
        elif shape == "len120":
            lens = torch.randint(60, 181, (rows // 60 + 1,), device=dev, generator=gen)
        elif shape == "long_tail":
            lens = torch.randint(1, 80, (rows // 20 + 1,), device=dev, generator=gen)
            tail = torch.rand(lens.numel(), device=dev, generator=gen) < 1e-3
            lens = torch.where(tail, torch.randint(300, 3001, lens.shape, device=dev, generator=gen),
                               lens)
        else:
            raise SystemExit(f"unknown shape {shape!r}")
        end = lens.cumsum(0)
        keep = int((end < rows).sum()) + 1
        lens = lens[:keep].clone()
        lens[-1] -= end[keep - 1] - rows
        return lens

    def timed(fn, iters, warmup):
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

    def plan(ptr, lens):
        """chunks of groups in order of length: (group ids, row index [g, L], mask [g, L])"""
        budget = int(args.torch_mb * 2 ** 20) // 4
        order = lens.argsort()
        sorted_lens = lens[order].tolist()
        chunks, b = [], 0
        while b < len(sorted_lens):
            e = b + 1
            # ascending lengths: the chunk's L is its last group's
            while e < len(sorted_lens) and (e + 1 - b) * sorted_lens[e] ** 2 <= budget:
                e += 1
            ids = order[b:e]
            span = max(1, sorted_lens[e - 1])
            pos = torch.arange(span, device=dev)
            mask = pos[None, :] < lens[ids][:, None]
            idx = (ptr[ids][:, None] + pos[None, :]).clamp(max=rows - 1)
            chunks.append((ids, idx, mask))
            b = e
        return chunks

    def torch_ranks(s, lab, mask):
        span = s.shape[1]
        pos = torch.arange(span, device=dev)
        before = pos[None, :] < pos[:, None]  # [i, j]: j < i
        mj = mask[:, None, :]
        r = (((s[:, None, :] > s[:, :, None]) | ((s[:, None, :] == s[:, :, None]) & before))
             & mj).sum(2)
        q = (((lab[:, None, :] > lab[:, :, None]) | ((lab[:, None, :] == lab[:, :, None]) & before))
             & mj).sum(2)
        return r, q

    def torch_loss(chunks, weighting):
        loss = torch.zeros(groups, device=dev)
        pairs = torch.zeros(groups, dtype=torch.int64, device=dev)
        grad = torch.zeros(rows, device=dev)
        for ids, idx, mask in chunks:
            s, lab = score[idx], label[idx]
            pair = (lab[:, :, None] > lab[:, None, :]) & mask[:, :, None] & mask[:, None, :]
            npairs = pair.sum((1, 2))
            x = sigma * (s[:, :, None] - s[:, None, :])
            w = pair.float()
            if weighting == "ndcg":
                r, q = torch_ranks(s, lab, mask)
                gain = (torch.exp2(lab) - 1) * mask
                d = 1 / torch.log2(2.0 + r)
                idcg = (gain / torch.log2(2.0 + q)).sum(1).clamp(min=1e-30)
                w = w * (gain[:, :, None] - gain[:, None, :]).abs() \
                    * (d[:, :, None] - d[:, None, :]).abs() / idcg[:, None, None]
            scale = 1 / npairs.clamp(min=1).float()
            loss[ids] = (w * torch.nn.functional.softplus(-x)).sum((1, 2)) * scale
            pairs[ids] = npairs
            gr = w * torch.sigmoid(-x)
            g = (gr.sum(1) - gr.sum(2)) * (sigma * scale)[:, None]
            grad[idx[mask]] = g[mask]
        return loss, pairs, grad

    def torch_ndcg(chunks, k):
        out = torch.zeros(groups, device=dev)
        for ids, idx, mask in chunks:
            s, lab = score[idx], label[idx]
            r, q = torch_ranks(s, lab, mask)
            gain = (torch.exp2(lab) - 1) * mask
            dcg = (gain / torch.log2(2.0 + r) * (r < k)).sum(1)
            ideal = (gain / torch.log2(2.0 + q) * (q < k)).sum(1)
            out[ids] = torch.where(ideal > 0, dcg / ideal.clamp(min=1e-30), torch.ones_like(dcg))
        return out

    def rel(got, want):
        return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))

    res = {"rows": rows, "labels": "0..4", "sigma": sigma, "torch_mb": args.torch_mb,
           "iters": args.iters, "warmup": args.warmup, "torch_iters": args.torch_iters,
           "wave_group_rows": int(ops._dmlc.rank_wave_group_rows()),
           "device": torch.cuda.get_device_name(0)}
    for shape in args.shapes.split(","):
        lens = lengths(shape)
        groups = lens.numel()
        qid = torch.repeat_interleave(torch.arange(groups, device=dev) * 7919 + 13, lens)
        ptr = ops.qid_groups(qid)
        want_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
        assert torch.equal(ptr, want_ptr), "qid_groups disagrees with the lengths"
        pair_evals = int((lens * lens).sum())
        r = {"groups": groups, "longest": int(lens.max()),
             "groups_on_rk2": int((lens > res["wave_group_rows"]).sum()), "pair_evals": pair_evals}
        chunks = plan(ptr, lens)
        r["torch_chunks"] = len(chunks)
        # the same outputs first
        for weighting in ("ndcg", "none"):
            got = ops.rank_loss_parts(score, label, ptr, weighting, sigma)
            want = torch_loss(chunks, weighting)
            assert torch.equal(got[1], want[1]), "pair counts differ"
            r[f"loss_{weighting}_max_rel_diff"] = rel(got[0], want[0])
            r[f"grad_{weighting}_max_rel_diff"] = rel(got[2], want[2])
            del got, want
        r["ndcg10_max_abs_diff"] = float((ops.ndcg(score, label, ptr, 10)
                                          - torch_ndcg(chunks, 10)).abs().max())
        r["qid_groups"] = timed(lambda: ops.qid_groups(qid), args.iters, args.warmup)
        for weighting in ("ndcg", "none"):
            hip = timed(lambda: ops.rank_loss_parts(score, label, ptr, weighting, sigma,
                                                    validate=False), args.iters, args.warmup)
            hip["Gpairs_per_s"] = round(pair_evals / hip["ms"] / 1e6, 2)
            r[f"rank_loss_{weighting}"] = hip
            r[f"torch_loss_{weighting}"] = timed(lambda: torch_loss(chunks, weighting),
                                                 args.torch_iters, 1)
            r[f"loss_{weighting}_speedup"] = round(r[f"torch_loss_{weighting}"]["ms"] / hip["ms"], 2)
        r["ndcg10"] = timed(lambda: ops.ndcg(score, label, ptr, 10, validate=False), args.iters,
                            args.warmup)
        r["torch_ndcg10"] = timed(lambda: torch_ndcg(chunks, 10), args.torch_iters, 1)
        r["ndcg10_speedup"] = round(r["torch_ndcg10"]["ms"] / r["ndcg10"]["ms"], 2)
        res[shape] = r
        print(f"{shape}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del chunks, qid, ptr, lens
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
