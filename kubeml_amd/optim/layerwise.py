"""Layer-wise adaptive optimizers over the flat parameter space: fused LAMB and LARS.

The large-batch recipes (LARS for ResNet, LAMB for BERT) scale each parameter tensor's update by
a trust ratio of two 2-norms taken over that tensor.  On a GPU a step is two launches per flat
space (``csrc/kernels/layerwise.hip``): the first reduces every tensor's norms over a chunk table
of the space, deterministically and independent of the grid, and leaves the ratios on the device;
the second applies the update and refreshes the bf16 shadow.  Learning rate, weight decay and
``adapt`` are a row per *tensor* of a small fp32 device table, so there is no limit on the number
of parameter groups and a captured step follows ``set_lr`` without re-capture; step count,
first-step flag and clip coefficient are device scalars as in the other fused optimizers.

LAMB (You et al. 2020; apex ``FusedLAMB`` with decoupled decay and bias correction), per tensor p::

    m = b1*m + (1-b1)*g'          v = b2*v + (1-b2)*g'^2
    u = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + wd*w
    r = |w_p| / |u_p|   if adapt and |w_p| > 0 and |u_p| > 0, else 1
    w -= lr * r * u

LARS (You, Gitman, Ginsburg 2017; the "scale" form of apex ``LARC`` around momentum SGD)::

    r = trust_coefficient * |w_p| / (|g'_p| + wd*|w_p| + eps)   if adapt and both norms > 0, else 1
    d = r * (g' + wd*w)
    buf = d on the first step after a reset, else momentum*buf + (1-dampening)*d
    w -= lr * (d + momentum*buf if nesterov else buf)

``g' = grad_scale * clip * g``; a NaN norm gives a NaN ratio (it reaches the weights, as a NaN clip
coefficient does).  The update inside the ZeRO-1 shard step would need a cross-rank sum of the
chunk norms, as clipping does: both classes report no ranged step, so those plans run as the exact
all-reduce plan.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from . import FusedOptimizer, _Tables

__all__ = ["LAMB", "LARS", "layerwise_groups"]


def _ratio(adapt, wn, other, value):
    """The guard both formulas share: ``value()`` when adapting and both norms are positive, NaN when
    a norm is NaN (never clamped to 1), else 1."""
    if not adapt:
        return 1.0
    if math.isnan(wn) or math.isnan(other):
        return float("nan")
    return float(value()) if wn > 0 and other > 0 else 1.0


class _Layerwise(FusedOptimizer):
    _per_group = ("lr", "weight_decay", "adapt")
    _max_groups = None

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._ratios_host: Dict[int, float] = {}   # CPU / loose path: id(p) -> last ratio

    # --- per-tensor table ---------------------------------------------------------------
    def _hp_rows(self, sp):
        """One (lr, weight_decay, adapt, 0) per tensor of ``sp``, in the space's parameter order.  A
        tensor of the space in no group of this optimizer gets zeros: its weights do not move."""
        of = {}
        for g in self.param_groups:
            row = [float(g["lr"]), float(g["weight_decay"]), 1.0 if g["adapt"] else 0.0, 0.0]
            for p in g["params"]:
                of[id(p)] = row
        return [of.get(id(p), [0.0, 0.0, 0.0, 0.0]) for p in sp.params]

    def layer_tables(self, sp) -> _Tables:
        """Tables of GPU space ``sp`` (built once; scratch like the clip scalars, not optimizer
        state).  An eager step refreshes the hyper-parameter rows when ``param_groups`` were written
        directly; a captured step reads them as they stand, so between replays use :meth:`set_lr`."""
        from ..ops import kernels as K
        tb = self._tables.get(id(sp))
        rows = self._hp_rows(sp)
        if tb is None:
            tb = self._tables[id(sp)] = _Tables(sp, rows)
            tb.chunks, tb.ranges = K.layer_tables(sp.offsets, sp.numel, sp.device)
            tb.part = torch.zeros(2 * tb.chunks.shape[0], dtype=torch.float32, device=sp.device)
            tb.ratio = torch.ones(len(rows), dtype=torch.float32, device=sp.device)
        else:
            tb.refresh(rows)
        return tb

    _prepare_tables = layer_tables

    def _lr_outputs(self):
        """A row per tensor of every GPU space: column 0 of its [T, 4] table (a tensor in no group: None)."""
        of = {id(p): k for k, g in enumerate(self.param_groups) for p in g["params"]}
        return [(tb.hp, len(tb.space.params), 4, [of.get(id(p)) for p in tb.space.params])
                for tb in self._tables.values()]

    def trust_ratios(self) -> torch.Tensor:
        """The last step's trust ratio of every tensor as one fp32 tensor: on a GPU the device tensor
        the step wrote (no synchronisation), in the flat space's parameter order (``space.params``);
        otherwise a CPU tensor in parameter-group order.  Ones before the first step."""
        spaces, loose = self._flat_groups()
        gpu = [sp for sp, _ in spaces if sp.device.type == "cuda"]
        if gpu:
            if len(gpu) != 1 or loose:
                raise ValueError("trust_ratios on a GPU needs every parameter in one flat space")
            return self.layer_tables(gpu[0]).ratio
        ps = [p for g in self.param_groups for p in g["params"]]
        return torch.tensor([self._ratios_host.get(id(p), 1.0) for p in ps], dtype=torch.float32)

    # --- no ranged steps: a tensor's norms need all of its gradient -------------------------
    def supports_ranges(self) -> bool:
        return False

    def step_range(self, *a, **k):
        raise ValueError(f"{type(self).__name__} cannot step by ranges (a tensor's norms need its whole gradient)")


class LAMB(_Layerwise):
    kind = "lamb"
    _STATE_NAMES = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adapt=True,
                 max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adapt=adapt,
                                      max_grad_norm=max_grad_norm))

    def _begin_space(self, sp, new_device):
        if new_device:          # one count per device, whatever its spaces
            self._step_dev_inc(sp.device)

    def _step_space(self, sp, clip):
        from ..ops import kernels as K
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        st = self.step_tensor(sp.device)
        bufs = self.state_buffers(sp)
        tb = self.layer_tables(sp)
        K.lamb_moments_(sp.master, sp.grad, bufs["exp_avg"], bufs["exp_avg_sq"], tb.chunks, tb.ranges, tb.hp,
                        tb.part, tb.ratio, 0.0, b1, b2, g["eps"], self._grad_scale, step_dev=st, clip_dev=clip)
        K.lamb_apply_(sp.master, bufs["exp_avg"], bufs["exp_avg_sq"], sp.shadow, tb.chunks, tb.hp, tb.ratio, 0.0,
                      b1, b2, g["eps"], step_dev=st)

    def _step_loose(self, group, params, scale):
        _torch_lamb(params, group, self.state, scale, self._ratios_host)

    def _finish_step(self, devices):
        self._step_host += 1


class LARS(_Layerwise):
    kind = "lars"

    @property
    def _STATE_NAMES(self):
        return ("momentum",) if self.param_groups[0]["momentum"] != 0 else ()

    def __init__(self, params, lr, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
                 trust_coefficient=1e-3, eps=1e-8, adapt=True, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, trust_coefficient=trust_coefficient, eps=eps, adapt=adapt,
                                      max_grad_norm=max_grad_norm))

    def _step_space(self, sp, clip):
        from ..ops import kernels as K
        g = self.param_groups[0]
        mom = self.state_buffers(sp).get("momentum")
        first = self.first_tensor(sp.device) if mom is not None else None
        tb = self.layer_tables(sp)
        K.lars_norms_(sp.master, sp.grad, tb.chunks, tb.ranges, tb.hp, tb.part, tb.ratio,
                      trust_coefficient=g["trust_coefficient"], eps=g["eps"], grad_scale=self._grad_scale,
                      clip_dev=clip)
        K.lars_apply_(sp.master, sp.grad, mom, sp.shadow, tb.chunks, tb.hp, tb.ratio, momentum=g["momentum"],
                      dampening=g["dampening"], nesterov=g["nesterov"], first=self._first,
                      grad_scale=self._grad_scale, first_dev=first, clip_dev=clip)

    def _step_loose(self, group, params, scale):
        _torch_lars(params, group, self.state, scale, self._ratios_host)

    _finish_step = FusedOptimizer._clear_first


def _torch_lamb(params, g, state, grad_scale, ratios):
    """Per-tensor torch form of the two LAMB launches (CPU spaces, loose parameters)."""
    b1, b2 = g["betas"]
    for p in params:
        if p.grad is None:
            continue
        st = state.setdefault(p, {})
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        st["step"] += 1
        t = st["step"]
        gr = p.grad * grad_scale
        st["exp_avg"].mul_(b1).add_(gr, alpha=1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(gr, gr, value=1 - b2)
        denom = (st["exp_avg_sq"] / (1 - b2 ** t)).sqrt_().add_(g["eps"])
        u = (st["exp_avg"] / (1 - b1 ** t)).div_(denom).add_(p, alpha=g["weight_decay"])
        wn, un = float(p.norm()), float(u.norm())
        r = _ratio(g["adapt"], wn, un, lambda: wn / un)
        ratios[id(p)] = r
        p.add_(u, alpha=-g["lr"] * r)


def _torch_lars(params, g, state, grad_scale, ratios):
    """Per-tensor torch form of the two LARS launches (CPU spaces, loose parameters)."""
    for p in params:
        if p.grad is None:
            continue
        gr = p.grad * grad_scale
        wn, gn = float(p.norm()), float(gr.norm())
        r = _ratio(g["adapt"], wn, gn,
                   lambda: g["trust_coefficient"] * wn / (gn + g["weight_decay"] * wn + g["eps"]))
        ratios[id(p)] = r
        d = gr.add(p, alpha=g["weight_decay"]).mul_(r)
        if g["momentum"]:
            st = state.setdefault(p, {})
            buf = st.get("momentum_buffer")
            if buf is None:
                buf = d.clone().detach()
                st["momentum_buffer"] = buf
            else:
                buf.mul_(g["momentum"]).add_(d, alpha=1 - g["dampening"])
            d = d.add(buf, alpha=g["momentum"]) if g["nesterov"] else buf
        p.add_(d, alpha=-g["lr"])


def layerwise_groups(module: torch.nn.Module, weight_decay: float):
    """The two parameter groups of :func:`~kubeml_amd.optim.no_decay_groups` for LAMB / LARS: weights
    (``ndim > 1``) at ``weight_decay`` with the trust ratio, then biases and BN / LayerNorm weights
    (``ndim <= 1``) without decay and without adaptation (``adapt=False``: ratio 1), the usual
    exclusion of the large-batch recipes."""
    from . import no_decay_groups
    groups = no_decay_groups(module, weight_decay)
    for g in groups:
        g["adapt"] = any(p.ndim > 1 for p in g["params"])
    return groups
