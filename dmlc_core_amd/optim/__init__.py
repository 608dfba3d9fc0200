"""Row-sparse minibatch steps: lazy AdaGrad / FTRL on the touched rows only.

A step on a per-step batch of a resident CSR costs O(batch), not O(features):
:func:`dmlc_core_amd.ops.compact_features` renumbers the batch's feature ids to
``0 .. U-1``, the CSR ops run unchanged on the ``[U, ...]`` slices of the
parameters and return compact gradients, and
:func:`dmlc_core_amd.ops.lazy_update_` (HIP kernel L1) applies them to the
touched rows of the full tables and of the optimizer state.

Not covered: multi-rank training (a row-sparse all-reduce needs the union of
the ranks' ids first), :class:`~dmlc_core_amd.models.HashedFM` (dense by
construction), and a HIP gather for ``p[ids]`` (torch indexing is used).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Iterable, List, Optional

import torch

from .. import ops

__all__ = ["LazyAdagrad", "LazyFTRL", "RowSparseStep"]


class _LazyOptimizer:
    """Per-parameter state (zeros on first use) around ``ops.lazy_update_``.
    A parameter's state is kept under the ``key`` given with its updates
    (:class:`RowSparseStep` gives the parameter's name), or, without one,
    under its position in the order of first updates."""

    rule = ""
    n_state = 0

    def __init__(self, **hyper):
        ops._lazy_hyper(self.rule, hyper)  # raises on a bad value
        self.hyper = hyper
        self._keys: Dict[int, object] = {}   # id(param) -> key, for updates without a key
        self._params: List[torch.Tensor] = []  # kept alive: their ids are in _keys
        self._state: Dict[object, tuple] = {}
        self._loaded: Dict[object, tuple] = {}

    def _state_of(self, param: torch.Tensor, key=None) -> tuple:
        if key is None:
            key = self._keys.get(id(param))
            if key is None:
                key = len(self._params)
                self._keys[id(param)] = key
                self._params.append(param)
        st = self._state.get(key)
        if st is None:
            if key in self._loaded:
                # copies: the loaded dict's tensors are not updated in place
                st = tuple(t.detach().to(device=param.device, dtype=torch.float32, copy=True)
                           .contiguous() for t in self._loaded.pop(key))
                if len(st) != self.n_state or any(t.shape != param.shape for t in st):
                    raise ValueError(f"loaded optimizer state {key!r} does not fit a parameter "
                                     f"of shape {tuple(param.shape)}")
            else:
                st = tuple(torch.zeros_like(param.detach(), memory_format=torch.contiguous_format)
                           for _ in range(self.n_state))
            self._state[key] = st
        return st

    def update_rows_(self, param: torch.Tensor, ids: Optional[torch.Tensor], grad_u: torch.Tensor,
                     validate: bool = True, key=None) -> None:
        """One step on rows ``ids`` of ``param`` from the compact gradient
        ``grad_u`` ``[U, ...]`` (``ops.lazy_update_``'s arguments and checks).
        ``key`` names the parameter's state (any hashable; the same one at
        every update); without it ``param`` must be the same object every
        time, and its state is known by the order of first updates."""
        ops.lazy_update_(param.detach(), ids, grad_u.detach().contiguous(),
                         self._state_of(param, key), self.rule, validate=validate, **self.hyper)

    def update_(self, param: torch.Tensor, grad: torch.Tensor, key=None) -> None:
        """One dense step on every row of ``param`` (biases, small tensors)"""
        self.update_rows_(param, None, grad, validate=False, key=key)

    def state_dict(self) -> Dict:
        """``rule``, ``hyper`` and ``state``: key -> tuple of copies of the
        state tensors (loaded state not used yet included)"""
        state = {k: tuple(t.clone() for t in st) for k, st in self._loaded.items()}
        state.update({k: tuple(t.clone() for t in st) for k, st in self._state.items()})
        return {"rule": self.rule, "hyper": dict(self.hyper), "state": state}

    def load_state_dict(self, state: Dict) -> None:
        """Take over ``state_dict()``'s hyper-parameters and state.  Each
        parameter gets a copy of the state under its key at its next update."""
        if state.get("rule") != self.rule:
            raise ValueError(f"state is for rule {state.get('rule')!r}, optimizer is {self.rule!r}")
        ops._lazy_hyper(self.rule, state["hyper"])
        self.hyper = dict(state["hyper"])
        self._loaded = {k: tuple(st) for k, st in state["state"].items()}
        self._keys, self._params, self._state = {}, [], {}


class LazyAdagrad(_LazyOptimizer):
    """AdaGrad on touched rows: ``g' = g + l2*w; n += g'*g'; w -= lr * g' /
    (sqrt(n) + eps)`` -- torch's ``Adagrad`` with ``lr_decay=0`` and
    ``initial_accumulator_value=0``.  With ``l2 = 0`` it equals the dense step
    exactly; ``l2 > 0`` decays a row only when it is touched."""

    rule, n_state = "adagrad", 1

    def __init__(self, lr: float, eps: float = 1e-10, l2: float = 0.0):
        super().__init__(lr=lr, eps=eps, l2=l2)


class LazyFTRL(_LazyOptimizer):
    """FTRL-Proximal on touched rows, state ``(z, n)``: ``s = (sqrt(n + g*g) -
    sqrt(n)) / alpha; z += g - s*w; n += g*g; w = 0 if |z| <= l1 else -(z -
    sign(z)*l1) / ((beta + sqrt(n))/alpha + l2)``."""

    rule, n_state = "ftrl", 2

    def __init__(self, alpha: float, beta: float = 1.0, l1: float = 0.0, l2: float = 0.0):
        super().__init__(alpha=alpha, beta=beta, l1=l1, l2=l2)


@contextlib.contextmanager
def _substituted(model: torch.nn.Module, tensors: Dict[str, torch.Tensor]):
    """Inside the block the parameters ``tensors`` names (``named_parameters``
    names) are those tensors, for every method of ``model`` -- ``loss`` too,
    which ``torch.func.functional_call`` does not reach.  The model's own
    parameters are back afterwards, also after an exception."""
    saved = []
    try:
        for name, t in tensors.items():
            owner, _, leaf = name.rpartition(".")
            mod = model.get_submodule(owner) if owner else model
            saved.append((mod, leaf, mod._parameters[leaf]))
            mod._parameters[leaf] = t
        yield model
    finally:
        for mod, leaf, p in reversed(saved):
            mod._parameters[leaf] = p


class RowSparseStep:
    """Training steps that touch only a batch's features.

    ``model``: a module with ``num_features`` and ``loss(batch, **kw)`` whose
    device path takes its sizes from the parameter tensors --
    ``SparseLogReg``, ``SparseSoftmaxReg``, ``SparseFM``, ``SparseFFM``,
    ``SparseRanker``.  ``optimizer``: a :class:`LazyAdagrad` or
    :class:`LazyFTRL`.  ``rows``: the names of the parameters indexed by feature
    id; by default every parameter whose ``shape[0] == model.num_features``
    (name them when another tensor, such as a ``[C]`` bias with C == F, has
    that length by chance).  The other parameters get dense steps."""

    def __init__(self, model: torch.nn.Module, optimizer: _LazyOptimizer,
                 rows: Optional[Iterable[str]] = None):
        self.model, self.optimizer = model, optimizer
        self.num_features = int(model.num_features)
        named = dict(model.named_parameters())
        if rows is None:
            rows = [n for n, p in named.items() if p.dim() >= 1 and p.shape[0] == self.num_features]
        self.rows = list(rows)
        for n in self.rows:
            if n not in named:
                raise ValueError(f"RowSparseStep: the model has no parameter {n!r}")
            if named[n].dim() < 1 or named[n].shape[0] != self.num_features:
                raise ValueError(f"RowSparseStep: parameter {n!r} has shape "
                                 f"{tuple(named[n].shape)}, not [{self.num_features}, ...]")
        self.dense = [n for n in named if n not in set(self.rows)]
        self._named = named

    def step(self, csr: Dict, **loss_kw) -> torch.Tensor:
        """One step on the batch ``csr`` (a device CSR dict with its labels):
        compact the feature ids, evaluate ``model.loss`` on the ``[U, ...]``
        slices of the row parameters, backpropagate, and update the touched
        rows (and the dense parameters).  Returns the detached loss."""
        batch = ops.compact_features(csr, self.num_features)
        ids = batch["ids"]
        sub = {n: self._named[n].detach()[ids].requires_grad_() for n in self.rows}
        for n in self.dense:
            self._named[n].grad = None
        with _substituted(self.model, sub):
            loss = self.model.loss(batch, **loss_kw)
        loss.backward()
        for n in self.rows:
            if sub[n].grad is not None:
                # ids come from compact_features: ascending and < F by construction
                self.optimizer.update_rows_(self._named[n], ids, sub[n].grad, validate=False, key=n)
        for n in self.dense:
            p = self._named[n]
            if p.grad is not None:
                self.optimizer.update_(p, p.grad, key=n)
                p.grad = None
        return loss.detach()
