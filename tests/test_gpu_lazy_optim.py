"""L1 (src/gpu/optim_kernels.hip) through ops.lazy_update_, the optimizers and
RowSparseStep, against the float64 formulas of lazy_reference.py.

Tolerance, derived: a step applies at most 6 f32 operations to an element, each
correctly rounded or within 2.5 ulp, so 16 * 2^-24 relative per step and, over
the three steps of a test, REL = 3 * 16 * 2^-24 -- on ``n``, and on the
accumulated change of ``w`` (the sum over the steps of |w_after - w_before| in
the reference) -- plus half an ulp of ``w`` per step (2^-24 |w_after|, summed
over the three steps: ``slack`` of _run) for the final subtraction.  The case
grid (widths x U) runs AdaGrad at l2 = 0 and FTRL against exactly these bounds.

Two quantities outside that grid take a bound of their own, because a sum in
them cancels and the error is then relative to the magnitudes summed, not to
the result (``mag`` of _run).  The additional AdaGrad cases with l2 > 0
(test_adagrad_with_l2): ``g' = g + l2*w`` can lose bits, so ``n`` is bounded
by REL * sum (|g| + l2 |w|)^2 instead of REL * n (the two are equal at l2 = 0);
``w`` keeps the bound above.  And FTRL's ``z``, which the bound above does not
cover (it speaks of ``n`` and ``w``): FTRL's
``z += g - s*w`` with ``s`` a difference of two square roots gives ``z`` the
bound REL * sum (|g| + (sqrt(n + g*g) + sqrt(n)) / alpha * |w|) plus half an
ulp of ``z`` per step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dmlc_core_amd import data, ops, optim
from dmlc_core_amd.models import SparseFFM, SparseLogReg
from lazy_reference import adagrad64, ftrl64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 1000
WIDTHS = [1, 3, 4, 8, 156]
COUNTS = [0, 1, 64, 65, 257]
STEPS = 3
REL = STEPS * 16 * 2.0 ** -24
HALF_ULP = 2.0 ** -24


def _ids(u, step, g):
    """u distinct ascending ids of [0, F), different per step, with 0 and F-1"""
    if u == 0:
        return torch.zeros(0, dtype=torch.int64)
    if u == 1:
        return torch.tensor([(0, F - 1, 17)[step]])
    inner = torch.randperm(F - 2, generator=g)[:u - 2] + 1
    return torch.sort(torch.cat([torch.tensor([0, F - 1]), inner])).values


def _shape(rows, width):
    return (rows,) if width == 0 else (rows, width)


def _run(rule, width, u, hyper, dense=False, misalign=False, l_seed=0):
    """three steps on the device and in float64; returns the device tensors,
    the float64 ones and the reference's accumulated |change| of each"""
    g = torch.Generator().manual_seed(1000 * width + u + l_seed)
    n_state = 1 if rule == "adagrad" else 2

    def dev(t):
        if not misalign:
            return t.cuda()
        buf = torch.empty(t.numel() + 1, device="cuda")  # 4 bytes off a 16-byte boundary
        out = buf[1:].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out

    w0 = torch.randn(_shape(F, width), generator=g)
    w = dev(w0)
    state = tuple(dev(torch.zeros(_shape(F, width))) for _ in range(n_state))
    w64 = w0.double()
    s64 = tuple(torch.zeros(_shape(F, width), dtype=torch.float64) for _ in range(n_state))
    moved = [torch.zeros_like(w64) for _ in range(1 + n_state)]
    slack, mag = torch.zeros_like(w64), torch.zeros_like(w64)
    for step in range(STEPS):
        ids = None if dense else _ids(u, step, g)
        rows = F if dense else u
        grad = torch.randn(_shape(rows, width), generator=g)
        before = [t.clone() for t in (w, *state)]
        ops.lazy_update_(w, None if dense else ids.cuda(), dev(grad), state, rule, **hyper)
        before64 = [t.clone() for t in (w64, *s64)]
        r, g64 = (slice(None) if dense else ids), grad.double()
        if rule == "adagrad":
            mag[r] += (g64.abs() + hyper.get("l2", 0.0) * w64[r].abs()) ** 2
        else:
            n_r = s64[1][r]
            mag[r] += g64.abs() + ((n_r + g64 * g64).sqrt() + n_r.sqrt()) / hyper["alpha"] * w64[r].abs()
        if rule == "adagrad":
            adagrad64(w64, s64[0], ids, grad.double(), **hyper)
        else:
            ftrl64(w64, s64[0], s64[1], ids, grad.double(), **hyper)
        for m, a, b in zip(moved, (w64, *s64), before64):
            m += (a - b).abs()
        slack += HALF_ULP * w64.abs()
        # rows not named in ids: neither read nor written
        untouched = torch.ones(F, dtype=torch.bool)
        if ids is None:
            untouched[:] = False
        else:
            untouched[ids] = False
        for t, b in zip((w, *state), before):
            assert torch.equal(t.cpu()[untouched], b.cpu()[untouched])
    return (w, *state), (w64, *s64), moved, slack, mag


def _assert_within(name, got, ref, bound):
    err = (got.cpu().double() - ref).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, "
          f"worst err / bound {worst:.3f}")
    assert (err <= bound).all(), name


@pytest.mark.parametrize("u", COUNTS)
@pytest.mark.parametrize("width", [0] + WIDTHS)
def test_adagrad_three_steps(width, u):
    """the whole grid at l2 = 0; width 0: a 1-D parameter ``[F]`` (no trailing
    dimension)"""
    hyper = {"lr": 0.1, "eps": 1e-10, "l2": 0.0}
    (w, n), (w64, n64), (dw, dn), slack, _ = _run("adagrad", width, u, hyper)
    _assert_within("n", n, n64, REL * n64.abs())
    _assert_within("w", w, w64, REL * dw + slack)


@pytest.mark.parametrize("width,u", [(0, 257), (3, 65), (4, 257), (156, 65)])
def test_adagrad_with_l2(width, u):
    """additional cases, l2 > 0: ``n`` against the magnitude bound of the
    module docstring, ``w`` against the grid's"""
    hyper = {"lr": 0.1, "eps": 1e-10, "l2": 0.02}
    (w, n), (w64, n64), (dw, dn), slack, mag = _run("adagrad", width, u, hyper)
    assert (mag >= n64).all()
    _assert_within("n", n, n64, REL * mag)
    _assert_within("w", w, w64, REL * dw + slack)


@pytest.mark.parametrize("u", COUNTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_ftrl_three_steps(width, u):
    hyper = {"alpha": 0.1, "beta": 1.0, "l1": 0.05, "l2": 0.01}
    (w, z, n), (w64, z64, n64), (dw, dz, dn), slack, mag = _run("ftrl", width, u, hyper)
    # w is continuous in z at the threshold |z| = l1 (it reaches 0 there), so a z that
    # falls on the other side of it in f32 moves w by no more than its own error
    _assert_within("n", n, n64, REL * n64.abs())
    _assert_within("z", z, z64, REL * mag + STEPS * HALF_ULP * z64.abs())
    _assert_within("w", w, w64, REL * dw + slack)


@pytest.mark.parametrize("rule,hyper", [("adagrad", {"lr": 0.1}), ("ftrl", {"alpha": 0.1, "l1": 0.05})])
@pytest.mark.parametrize("width", [0, 3, 4, 156])
def test_dense_identity_and_unaligned_tensors(rule, hyper, width):
    """ids=None, and width % 4 == 0 tensors off a 16-byte boundary (one thread
    per element)"""
    got, ref, moved, slack, _ = _run(rule, width, F, hyper, dense=True)
    _assert_within("w", got[0], ref[0], REL * moved[0] + slack)
    _assert_within("n", got[-1], ref[-1], REL * ref[-1].abs())
    if width and width % 4 == 0:
        off, ref, moved, slack, _ = _run(rule, width, 65, hyper, misalign=True)
        _assert_within("w unaligned", off[0], ref[0], REL * moved[0] + slack)
        # the same arithmetic per element as the 16-byte path
        vec = _run(rule, width, 65, hyper)[0]
        for a, b in zip(off, vec):
            assert torch.equal(a, b)


@pytest.mark.parametrize("width", [0, 3, 8])
def test_lazy_adagrad_equals_dense_steps_on_the_scattered_gradient(width):
    g = torch.Generator().manual_seed(7 + width)
    w0 = torch.randn(_shape(F, width), generator=g)
    wl, nl = w0.cuda(), torch.zeros(_shape(F, width)).cuda()
    wd, nd = w0.cuda(), torch.zeros(_shape(F, width)).cuda()
    for step in range(STEPS):
        ids = _ids(257, step, g).cuda()
        gu = torch.randn(_shape(257, width), generator=g).cuda()
        ops.lazy_update_(wl, ids, gu, (nl,), "adagrad", lr=0.1)
        dense = torch.zeros_like(wd)
        dense[ids] = gu
        ops.lazy_update_(wd, None, dense, (nd,), "adagrad", lr=0.1)
    assert torch.equal(wl, wd) and torch.equal(nl, nd)
    # the same inputs give the same bytes
    w2, n2 = w0.cuda(), torch.zeros_like(nl)
    g = torch.Generator().manual_seed(7 + width)
    torch.randn(_shape(F, width), generator=g)
    for step in range(STEPS):
        ids = _ids(257, step, g).cuda()
        ops.lazy_update_(w2, ids, torch.randn(_shape(257, width), generator=g).cuda(), (n2,),
                         "adagrad", lr=0.1)
    assert torch.equal(w2, wl) and torch.equal(n2, nl)


def test_ftrl_l1_threshold_and_signs():
    g = torch.Generator().manual_seed(11)
    grad = torch.randn(F, 4, generator=g)
    grad[grad.abs() < 1e-3] = 0.5
    ids = torch.arange(F).cuda()
    # an l1 above every |z|: exact zeros, whatever w was
    w, z, n = torch.randn(F, 4, generator=g).cuda(), torch.zeros(F, 4).cuda(), torch.zeros(F, 4).cuda()
    ops.lazy_update_(w, ids, grad.cuda(), (z, n), "ftrl", alpha=0.1, l1=1e6)
    assert float(z.abs().max()) < 1e6 and not w.any()
    assert torch.equal(w, torch.zeros_like(w)) and not torch.signbit(w).any()
    # from zero state z = g exactly: w has the sign of -z wherever |z| > l1
    w, z, n = torch.zeros(F, 4).cuda(), torch.zeros(F, 4).cuda(), torch.zeros(F, 4).cuda()
    ops.lazy_update_(w, ids, grad.cuda(), (z, n), "ftrl", alpha=0.1, l1=0.25)
    assert torch.equal(z.cpu(), grad) and torch.equal(n.cpu(), grad * grad)
    big = grad.abs() > 0.25
    assert big.any() and (~big).any() and (grad[big] > 0).any() and (grad[big] < 0).any()
    assert torch.equal(torch.sign(w.cpu()[big]), -torch.sign(grad[big]))
    assert not w.cpu()[~big].any()


@pytest.mark.parametrize("rule", ["adagrad", "ftrl"])
@pytest.mark.parametrize("ids,flagged", [
    ([2, 5, 3, 9], [5, 3]),          # descending: both rows of the pair
    ([2, 7, 7, 9], [7]),             # a duplicate
    ([2, 9, F], []),                 # an id >= F
    ([2, 9, 2 ** 40], []),
    ([-1, 2, 9], [2]),               # a negative id is a huge one; 2 is not above it
], ids=["descending", "duplicate", "equal-F", "huge", "negative"])
def test_bad_ids_raise_and_their_rows_stay(rule, ids, flagged):
    g = torch.Generator().manual_seed(13)
    for width in (3, 4):
        w0 = torch.randn(F, width, generator=g)
        w = w0.cuda()
        state = tuple(torch.zeros(F, width).cuda() for _ in range(1 if rule == "adagrad" else 2))
        grad = (torch.randn(len(ids), width, generator=g) + 3.0).cuda()
        hyper = {"lr": 0.1} if rule == "adagrad" else {"alpha": 0.1}
        with pytest.raises(ValueError, match="strictly ascending"):
            ops.lazy_update_(w, torch.tensor(ids).cuda(), grad, state, rule, **hyper)
        good = [i for i in ids if 0 <= i < F and i not in flagged]
        stay = torch.ones(F, dtype=torch.bool)
        stay[good] = False
        assert torch.equal(w.cpu()[stay], w0[stay])          # flagged rows and all others
        assert not any(s.cpu()[stay].any() for s in state)
        assert (w.cpu()[good] != w0[good]).all()             # the valid rows were updated
        # validate=False reads nothing and does not raise
        ops.lazy_update_(w, torch.tensor(ids).cuda(), grad, state, rule, validate=False, **hyper)
        assert torch.equal(w.cpu()[stay], w0[stay])


def test_optimizer_state_and_state_dict():
    opt = optim.LazyAdagrad(0.1)
    p = torch.nn.Parameter(torch.ones(F, 4).cuda())
    q = torch.nn.Parameter(torch.ones(3).cuda())
    ids = torch.tensor([0, 5, F - 1]).cuda()
    opt.update_rows_(p, ids, torch.full((3, 4), 2.0).cuda())
    opt.update_(q, torch.full((3,), 2.0).cuda())
    sd = opt.state_dict()
    assert {k: tuple(s[0].shape) for k, s in sd["state"].items()} == {0: (F, 4), 1: (3,)}
    assert sd["state"][0][0][ids.cpu()].eq(4.0).all() and float(sd["state"][0][0].sum()) == 48.0
    assert float(p.detach()[5, 0]) ==pytest.approx(1.0 - 0.1, rel=1e-6)
    # a fresh optimizer that loads the state continues exactly like the first
    other = optim.LazyAdagrad(0.5)
    other.load_state_dict(sd)
    p2 = torch.nn.Parameter(p.detach().clone())
    q2 = torch.nn.Parameter(q.detach().clone())
    for o, a, b in ((opt, p, q), (other, p2, q2)):
        o.update_rows_(a, ids, torch.full((3, 4), 1.0).cuda())
        o.update_(b, torch.full((3,), 1.0).cuda())
    assert other.hyper == opt.hyper and torch.equal(p, p2) and torch.equal(q, q2)
    # the loaded dict's tensors were copied, not adopted: sd still holds the old state
    assert float(sd["state"][0][0].sum()) == 48.0 and float(sd["state"][1][0].sum()) == 12.0
    # RowSparseStep keys the state by parameter name
    m = SparseLogReg(F).cuda()
    named = optim.LazyAdagrad(0.1)
    batch = {"offset": torch.tensor([0, 2, 3]).cuda(),
             "index": torch.tensor([1, 4, 2], dtype=torch.int32).cuda(), "value": None,
             "label": torch.tensor([0.0, 1.0]).cuda()}
    optim.RowSparseStep(m, named).step(batch)
    assert sorted(named.state_dict()["state"]) == ["bias", "weight"]


def _bce64(y, label):
    return torch.nn.functional.binary_cross_entropy_with_logits(y, label)


def _distance(params, ref):
    return max(float((p.detach().cpu().double() - r.detach()).abs().max())
               for p, r in zip(params, ref))


def test_row_sparse_logreg_matches_todays_path(tmp_path):
    """F = 5000, five steps over 512-row batches of a synthetic LibSVM shard:
    RowSparseStep(SparseLogReg, LazyAdagrad) and today's path (csr_spmv with the
    atomic gradient + torch.optim.Adagrad) against a float64 replay"""
    nf, rows_per, steps, lr = 5000, 512, 5, 0.1
    path = str(tmp_path / "shard.libsvm")
    data.write_synthetic(path, 0, rows_per * steps, format="libsvm", seed=5, num_features=nf)
    csr = data.GPUParser(path, chunk_mb=1).parse_all()
    assert csr.rows == rows_per * steps and int(csr.max_index) < nf
    t = data.csr_to_torch(csr)
    label = (t["label"].float() > 0).float()
    host = {"offset": t["offset"].cpu(), "index": t["index"].cpu(),
            "value": None if t["value"] is None else t["value"].cpu()}

    def batches():
        for b in range(0, rows_per * steps, rows_per):
            yield b, {"offset": t["offset"][b:b + rows_per + 1], "index": t["index"],
                      "value": t["value"], "label": label[b:b + rows_per]}

    lazy = SparseLogReg(nf).cuda()
    stepper = optim.RowSparseStep(lazy, optim.LazyAdagrad(lr))
    assert stepper.rows == ["weight"] and stepper.dense == ["bias"]
    dense = SparseLogReg(nf, grad="atomic").cuda()
    opt = torch.optim.Adagrad(dense.parameters(), lr=lr, eps=1e-10)
    w64, b64 = torch.zeros(nf, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    nw, nb = torch.zeros_like(w64), torch.zeros_like(b64)
    for b, batch in batches():
        loss_lazy = stepper.step(batch)
        loss = dense.loss(batch)
        opt.zero_grad()
        loss.backward()
        opt.step()
        x = data.to_sparse_csr(dict(host, offset=host["offset"][b:b + rows_per + 1]),
                               nf).to_dense().double()
        w, bias = w64.clone().requires_grad_(), b64.clone().requires_grad_()
        loss64 = _bce64(x @ w + bias, batch["label"].cpu().double())
        gw, gb = torch.autograd.grad(loss64, (w, bias))
        adagrad64(w64, nw, None, gw, lr)
        adagrad64(b64, nb, None, gb, lr)
        assert float(loss_lazy) == pytest.approx(float(loss64.detach()), rel=1e-4)
    assert isinstance(lazy.weight, torch.nn.Parameter) and lazy.weight.shape == (nf,)
    e_dense = _distance((dense.weight, dense.bias), (w64, b64))
    e_lazy = _distance((lazy.weight, lazy.bias), (w64, b64))
    print(f"logreg: e_dense {e_dense:.3e}  e_lazy {e_lazy:.3e}")
    assert float(lazy.weight.detach().abs().max()) > 0.01
    assert e_lazy <= 4 * e_dense + 1e-7


def test_row_sparse_ffm_matches_todays_path():
    """the same equivalence for SparseFFM (F = 200, 5 fields, k = 4, 64-row
    batches), the replay being SparseFFM.reference in float64"""
    nf, nfields, k, rows_per, steps, lr = 200, 5, 4, 64, 5, 0.05
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 13, rows_per * steps)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    nnz = int(off[-1])
    host = {"offset": off, "index": torch.from_numpy(rng.integers(0, nf, nnz).astype(np.int32)),
            "field": torch.from_numpy(rng.integers(0, nfields, nnz).astype(np.int32)),
            "value": torch.from_numpy(rng.standard_normal(nnz).astype(np.float32))}
    label = torch.from_numpy(rng.integers(0, 2, rows_per * steps).astype(np.float32))
    dev = {k_: v.cuda() for k_, v in host.items()}

    lazy = SparseFFM(nf, nfields, rank=k, seed=2).cuda()
    stepper = optim.RowSparseStep(lazy, optim.LazyAdagrad(lr))
    assert stepper.rows == ["w", "v"] and stepper.dense == ["bias"]
    dense = SparseFFM(nf, nfields, rank=k, seed=2).cuda()
    opt = torch.optim.Adagrad(dense.parameters(), lr=lr, eps=1e-10)
    ref = [p.detach().cpu().double() for p in (dense.bias, dense.w, dense.v)]
    acc = [torch.zeros_like(p) for p in ref]
    for b in range(0, rows_per * steps, rows_per):
        sl = slice(b, b + rows_per + 1)
        batch = dict(dev, offset=dev["offset"][sl], label=label[b:b + rows_per].cuda())
        stepper.step(batch)
        loss = dense.loss(batch)
        opt.zero_grad()
        loss.backward()
        opt.step()
        leaves = [p.clone().requires_grad_() for p in ref]
        y = SparseFFM.reference(dict(host, offset=host["offset"][sl]), leaves[1], leaves[2],
                                leaves[0])
        grads = torch.autograd.grad(_bce64(y, label[b:b + rows_per].double()), leaves)
        for p, n, g in zip(ref, acc, grads):
            adagrad64(p, n, None, g, lr)
    e_dense = _distance((dense.bias, dense.w, dense.v), ref)
    e_lazy = _distance((lazy.bias, lazy.w, lazy.v), ref)
    print(f"ffm: e_dense {e_dense:.3e}  e_lazy {e_lazy:.3e}")
    assert e_lazy <= 4 * e_dense + 1e-7


def test_train_sparse_logreg_lazy_adagrad():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "DMLC_TRACKER_URI"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_sparse_logreg.py"),
                        "--rows", "20000", "--epochs", "3", "--batch-rows", "4096",
                        "--shuffle-rows", "--optimizer", "lazy-adagrad"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    losses = out["loss_per_epoch"]
    assert out["rows"] == 20000
    assert losses[-1] < losses[0], losses
