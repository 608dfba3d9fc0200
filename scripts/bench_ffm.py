#!/usr/bin/env python3
"""FF1 / FF2 (ops.ffm / ops.ffm_t) at the Criteo shape: --rows rows (2 M) of
--fields entries (39), one per field with the fields ascending, ids uniform in
--features (1 M), made on the device from a seed.  For k in --ks (4, 8):

  ffm            ops.ffm(X, V, validate=False)            (FF1)
  ffm_t          ops.ffm_t(X, g, V)                       (FF2, fields ascending)
  ffm_t_shuffled the same rows with the entries of every row in a random order
                 (the same sums; what the access shape of FF2 buys)

against the same outputs from stock torch ops on the same device: gather
V[i_a, f_b] and V[i_b, f_a] as [rows, n, n, k] tensors, their product summed
over k, and index_put_(accumulate=True) for the gradient, on as many rows as
keep one such intermediate within --torch-mb MB (16 373 rows at k = 4, 8 186
at k = 8), scaled per row.  (torch.einsum("rabk,rabk->rab") in place of the
product and sum was tried first and dropped: at these shapes it took 190x
longer and did not return the same values.)  The
HIP results on those rows are compared with torch's first.  Every figure is
the median of --iters HIP-event timings after --warmup calls of the same
shape, with the fastest next to it.  added_GBps is the bytes FF2 adds
(rows * n * (n - 1) * 4k) over its time, next to the ~1300 GB/s the memory-side
f32 atomics reach (MI355X_MICROARCH.md, Global float atomics).  Prints one JSON
object.

usage: python scripts/bench_ffm.py [--rows N] [--features F] [--ks 4,8] [--torch-mb MB]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--torch-mb", type=float, default=380.0,
                    help="size of one [rows, n, n, k] f32 intermediate of the torch formulation")
    args = ap.parse_args()
    import torch

    from dmlc_core_amd import ops

    assert torch.cuda.is_available(), "bench_ffm.py measures on a GPU"
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, n, nfeat = args.rows, args.fields, args.features
    nnz = rows * n
    offset = torch.arange(0, nnz + 1, n, dtype=torch.int64, device=dev)
    index = torch.randint(0, nfeat, (rows, n), device=dev, generator=gen, dtype=torch.int32)
    field = torch.arange(n, dtype=torch.int32, device=dev).repeat(rows, 1)
    value = torch.randn(rows, n, device=dev, generator=gen)
    order = torch.rand(rows, n, device=dev, generator=gen).argsort(1)
    t = {"offset": offset, "index": index.reshape(-1), "field": field.reshape(-1),
         "value": value.reshape(-1)}
    shuffled = {"offset": offset, "index": index.gather(1, order).reshape(-1),
                "field": field.gather(1, order).reshape(-1),
                "value": value.gather(1, order).reshape(-1)}
    del order
    g = torch.randn(rows, device=dev, generator=gen)

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

    # the torch formulation, on the first `tr` rows
    offdiag = ~torch.eye(n, dtype=torch.bool, device=dev)

    def torch_forward(v, ia, fa, xx):
        va = v[ia[:, :, None], fa[:, None, :]]  # V[i_a, f_b]
        vb = v[ia[:, None, :], fa[:, :, None]]  # V[i_b, f_a]
        return 0.5 * ((va * vb).sum(-1) * xx).sum((1, 2))

    def torch_backward(v, ia, fa, xx, gr):
        tr = ia.shape[0]
        vb = v[ia[:, None, :], fa[:, :, None]]
        term = (gr[:, None, None] * xx)[:, :, :, None] * vb
        dv = torch.zeros_like(v)
        dv.index_put_((ia[:, :, None].expand(tr, n, n), fa[:, None, :].expand(tr, n, n)), term,
                      accumulate=True)
        return dv

    res = {"rows": rows, "entries_per_row": n, "nnz": nnz, "num_features": nfeat,
           "torch_mb": args.torch_mb, "iters": args.iters, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "atomic_ceiling_GBps": 1300}
    for k in (int(s) for s in args.ks.split(",")):
        tr = max(1, min(rows, int(args.torch_mb * 2 ** 20) // (n * n * k * 4)))
        scale = rows / tr
        head = {key: (a[:tr + 1] if key == "offset" else a) for key, a in t.items()}
        ia, fa, xa = index[:tr].long(), field[:tr].long(), value[:tr]
        xx = xa[:, :, None] * xa[:, None, :] * offdiag
        gt = g[:tr].contiguous()
        v = torch.randn(nfeat, n, k, device=dev, generator=gen) * 0.1
        added = rows * n * (n - 1) * 4 * k
        r = {}
        # the same outputs first (largest difference over the largest magnitude)
        want = torch_forward(v, ia, fa, xx)
        got = ops.ffm(head, v)
        r["forward_max_rel_diff"] = float((got - want).abs().max() / want.abs().max())
        want = torch_backward(v, ia, fa, xx, gt)
        got = ops.ffm_t(head, gt, v)
        r["backward_max_rel_diff"] = float((got - want).abs().max() / want.abs().max())
        del want, got
        r["ffm"] = timed(lambda: ops.ffm(t, v, validate=False))
        r["ffm_t"] = timed(lambda: ops.ffm_t(t, g, v))
        r["ffm_t"]["added_GBps"] = round(added / r["ffm_t"]["ms"] / 1e6, 1)
        r["ffm_t_shuffled"] = timed(lambda: ops.ffm_t(shuffled, g, v))
        r["ffm_t_shuffled"]["added_GBps"] = round(added / r["ffm_t_shuffled"]["ms"] / 1e6, 1)
        r["ffm_shuffled"] = timed(lambda: ops.ffm(shuffled, v, validate=False))
        zero = timed(lambda: torch.zeros_like(v))  # part of ffm_t and of the torch gradient
        r["zero_fill"] = zero
        tf = timed(lambda: torch_forward(v, ia, fa, xx))
        tb = timed(lambda: torch_backward(v, ia, fa, xx, gt))
        r["torch_forward"] = dict(tf, rows=tr, ms_scaled=round(tf["ms"] * scale, 3))
        # the zero fill of dV does not grow with the rows: scale what is left
        r["torch_backward"] = dict(tb, rows=tr, ms_scaled=round(
            (tb["ms"] - zero["ms"]) * scale + zero["ms"], 3))
        r["forward_speedup"] = round(r["torch_forward"]["ms_scaled"] / r["ffm"]["ms"], 2)
        r["backward_speedup"] = round(r["torch_backward"]["ms_scaled"] / r["ffm_t"]["ms"], 2)
        res[f"k{k}"] = r
        print(f"k={k}: {json.dumps(r)}", file=sys.stderr, flush=True)
        del v, ia, fa, xa, xx, gt, head
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
