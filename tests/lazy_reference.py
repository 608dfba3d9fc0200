"""Float64 references of the lazy optimizer rules (ops.lazy_update_, kernel L1),
shared by test_optim_cpu.py (which checks them against torch.optim.Adagrad) and
test_gpu_lazy_optim.py.  Tensors are float64 host tensors, updated in place on
the rows ``ids`` (None: every row)."""
import torch


def _rows(ids, n):
    return torch.arange(n) if ids is None else ids.to(torch.int64).cpu()


def adagrad64(w, n, ids, g, lr, eps=1e-10, l2=0.0):
    """g' = g + l2*w;  n += g'*g';  w -= lr * g' / (sqrt(n) + eps)"""
    r = _rows(ids, w.shape[0])
    gp = g + l2 * w[r]
    n[r] = n[r] + gp * gp
    w[r] = w[r] - lr * gp / (n[r].sqrt() + eps)


def ftrl64(w, z, n, ids, g, alpha, beta=1.0, l1=0.0, l2=0.0):
    """s = (sqrt(n + g*g) - sqrt(n)) / alpha;  z += g - s*w;  n += g*g;
    w = 0 if |z| <= l1 else -(z - sign(z)*l1) / ((beta + sqrt(n))/alpha + l2)"""
    r = _rows(ids, w.shape[0])
    s = ((n[r] + g * g).sqrt() - n[r].sqrt()) / alpha
    z[r] = z[r] + (g - s * w[r])
    n[r] = n[r] + g * g
    zr = z[r]
    new = -(zr - torch.sign(zr) * l1) / ((beta + n[r].sqrt()) / alpha + l2)
    w[r] = torch.where(zr.abs() <= l1, torch.zeros_like(zr), new)
