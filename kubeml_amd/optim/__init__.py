"""Fused optimizers over the flat parameter space (one HIP launch per step).

``SGD`` / ``Adam`` / ``AdamW`` accept the same arguments as their ``torch.optim``
counterparts.  When the parameters live in :class:`~kubeml_amd.nn.flat.FlatParamSpace`
buffers (the GPU path) the step is one ``kml_sgd`` / ``kml_adam`` launch per space
that also refreshes the bf16 shadow copy; otherwise (CPU) it defers to the stock
torch implementation so CPU-only plumbing tests share the exact same semantics.

The learning rate lives in a device scalar (``lr_tensor``) so a graph-captured step
follows LR changes (``set_lr``) without re-capture, and Adam's step counter is a
device scalar incremented inside the captured region.

``reset_state()`` implements the reference's per-round optimizer reset under K-step
averaging (python/kubeml/kubeml/network.py:121-128): a memset of the state buffers,
Adam's device step counter back to 0 and SGD's device first-step flag back to 1 — all
read by the kernels at replay time, so a captured step honours a reset between replays.

``state_tensors()`` lists every device tensor a step mutates (state buffers, step
counters, flags); graph capture snapshots and restores them around its warm-up so
capturing a step never applies an update (engine/step.py).

``max_grad_norm=`` turns on global-norm gradient clipping (torch's ``clip_grad_norm_`` with
the L2 norm) as part of the step: one deterministic ``kml_grad_norm`` launch over the flat
gradient leaves the clip coefficient on the device and the fused update multiplies it into
its gradient scale — no extra pass over the gradient.  The threshold is a device scalar
(``set_max_grad_norm``), so a captured step follows a changed threshold; clipping on or off
is fixed at construction (it decides the step's launches).  ``grad_norm_tensor`` is the
norm of the last step's averaged gradient.

Parameter groups may differ in ``lr`` and ``weight_decay`` (the no-decay idiom for biases and
norm weights, layer-wise LR decay); every other hyper-parameter is one value for the optimizer.
A grouped step is still one launch (``kml_sgd_groups`` / ``kml_adam_groups``): a byte per
64-element granule of the flat space names its group and a small fp32 device table holds the
groups' (lr, weight_decay), so a captured step follows ``set_lr([...])`` as it follows the single
LR scalar.  A single-group optimizer launches exactly what it always did.
:func:`no_decay_groups` builds the usual two groups of a module.

``LAMB`` / ``LARS`` (:mod:`kubeml_amd.optim.layerwise`) are the layer-wise adaptive optimizers of the
large-batch recipes: two launches per step (per-tensor norms, then the update), a table row per
tensor instead of the granule bytes, everything else as above.

:class:`~kubeml_amd.optim.lr_schedule.LRSchedule` moves the learning rate every step from the device: one
single-block launch writes ``base * f(position)`` into the words the launches above read, so a captured
step follows a warm-up / decay schedule without host work between replays.

:class:`~kubeml_amd.optim.ema.EMA` keeps an exponential moving average of the flat state prefix (weights
and BN statistics) in one launch per step, for validation, checkpoints and inference.

``from_torch(opt)`` converts a user's ``torch.optim.SGD/Adam/AdamW`` (what
``KubeModel.configure_optimizers`` returns in reference code) into the fused one
with identical hyper-parameters, group by group.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List

import torch

__all__ = ["SGD", "Adam", "AdamW", "LAMB", "LARS", "from_torch", "with_max_grad_norm", "no_decay_groups",
           "layerwise_groups", "FusedOptimizer", "EMA", "LRSchedule", "lr_factor"]

MAX_GROUPS = 8            # rows of the kernels' hyper-parameter table (KML_MAX_GROUPS)
_PER_GROUP = ("lr", "weight_decay")     # what may differ between parameter groups


def _spaces(params):
    """Group params by their flat space (None for params without one)."""
    groups: Dict[int, tuple] = {}
    loose = []
    for p in params:
        sp = getattr(p, "_kml_flat", None)
        if sp is None:
            loose.append(p)
        else:
            groups.setdefault(id(sp), (sp, []))[1].append(p)
    return [g for g in groups.values()], loose


class _Tables:
    """Device tables of the launches over one GPU flat space: the fp32 hyper-parameter table ``hp``,
    the host ``rows`` it holds, and whatever else the class's launches index (granule bytes, chunks)."""

    def __init__(self, space, rows):
        self.space, self.rows = space, rows
        self.hp = torch.tensor(rows, dtype=torch.float32).to(space.device)
        self.scheduled = False     # column 0 (the LR) is written on the device by an LRSchedule

    def refresh(self, rows):
        """hp := rows when they changed.  A capturing stream reads the table as it stands.  The LR
        column of a scheduled table is the schedule's: host values never overwrite it."""
        if rows != self.rows and not torch.cuda.is_current_stream_capturing():
            new = torch.tensor(rows, dtype=torch.float32)
            if self.scheduled:
                self.hp[:, 1:].copy_(new[:, 1:])
            else:
                self.hp.copy_(new)
            self.rows = rows


class FusedOptimizer(torch.optim.Optimizer):
    """The step skeleton, device scalars and tables every fused optimizer shares.  A subclass gives
    the launches over one GPU space (:meth:`_step_space`) and their torch form (:meth:`_step_loose`)."""
    kind = "base"
    _per_group = _PER_GROUP      # the keys that may differ between this class's parameter groups
    _max_groups = MAX_GROUPS     # None: no limit (a table row per tensor, not per group)
    _STATE_NAMES = ()            # the per-element fp32 state buffers of a flat space
    _cpu_ranges = False          # step_range also has a torch form over a CPU flat space
    _lr_schedule = None          # the attached optim.LRSchedule: it owns the device LR words

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._state_bufs: Dict[int, Dict[str, torch.Tensor]] = {}
        self._scalars: Dict[tuple, torch.Tensor] = {}      # (name, device) -> fp32 device tensor
        self._tables: Dict[int, _Tables] = {}              # id(space) -> the launches' tables
        self._grad_scale = 1.0
        self._first = True
        self._step_host = 0
        self._norm_host = None     # CPU / loose-parameter path: the last step's norm
        mgn = self.defaults.get("max_grad_norm")
        if mgn is not None and not float(mgn) > 0.0:
            raise ValueError("max_grad_norm must be a positive number or None")
        self._check_groups()

    # --- parameter groups ---------------------------------------------------------------
    @property
    def grouped(self) -> bool:
        """True with more than one parameter group (per-group ``lr`` / ``weight_decay``)."""
        return len(self.param_groups) > 1

    def _check_groups(self):
        """Groups may differ in lr and weight_decay only, there are at most MAX_GROUPS of them,
        and on a GPU all their parameters share one flat space (the one launch's range)."""
        groups = self.param_groups
        if self._max_groups is not None and len(groups) > self._max_groups:
            raise ValueError(f"{len(groups)} parameter groups: the fused optimizers take at most {MAX_GROUPS}")
        for key in self.defaults:
            if key in self._per_group:
                continue
            for g in groups[1:]:
                a, b = groups[0][key], g[key]
                if (tuple(a) != tuple(b)) if isinstance(a, (tuple, list)) else (a != b):
                    raise ValueError(f"parameter groups differ in {key!r}: only {' and '.join(self._per_group)} "
                                     f"may differ between the groups of a fused optimizer")
        if self.grouped and self._max_groups is not None:
            spaces, loose = self._flat_groups()
            if any(p.is_cuda for g in groups for p in g["params"]) and (len(spaces) != 1 or loose):
                raise ValueError("a GPU optimizer with several parameter groups needs every parameter in one "
                                 "flat space (nn.flatten_module)")

    def _hp_rows(self, sp):
        """The rows of the hyper-parameter table over space ``sp``: a (lr, weight_decay) per group."""
        return [[float(g["lr"]), float(g["weight_decay"])] for g in self.param_groups]

    def add_param_group(self, param_group):
        """torch's, then the checks of the constructor; the cached tables are rebuilt."""
        if self._lr_schedule is not None:
            raise ValueError("add_param_group after an LR schedule was attached: the schedule wrote this "
                             "optimizer's LR tables; attach it after the last group")
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):          # (torch's constructor adds the first groups itself)
            self._tables.clear()
            self._check_groups()

    def group_ids(self, sp) -> torch.Tensor:
        """uint8 CPU tensor, one group index per 64-element granule of flat space ``sp`` (regions
        are 64-aligned; a region's padding belongs to its parameter's group).  Granules of
        parameters of the space that are in no group of this optimizer stay at 0: the launch
        covers the whole space, as the single-group launch does, so they see group 0's values
        (their gradient is zero unless something else writes it)."""
        from ..nn.flat import ALIGN
        gid = torch.zeros(sp.numel // ALIGN, dtype=torch.uint8)
        for k, g in enumerate(self.param_groups):
            for p in g["params"]:
                region = sp.region_of(p)
                if region is None:
                    raise ValueError("parameter groups need every parameter in one flat space")
                o, n = region
                gid[o // ALIGN:(o + n) // ALIGN] = k
        return gid

    def group_tables(self, sp):
        """(gid, hp) device tensors of the grouped launches over GPU space ``sp``: the granule
        bytes and the fp32 [G, 2] rows of (lr, weight_decay).  Scratch like the clip scalars, not
        optimizer state.  An eager step refreshes hp when ``param_groups[k]["lr"]`` or
        ``["weight_decay"]`` were written directly (an LR scheduler); a captured step reads the
        table as it stands, so between replays use :meth:`set_lr` or call this method."""
        tb = self._tables.get(id(sp))
        rows = self._hp_rows(sp)
        if tb is None:
            spaces, loose = self._flat_groups()
            if len(spaces) != 1 or loose or spaces[0][0] is not sp:
                raise ValueError("a GPU optimizer with several parameter groups needs every parameter in one "
                                 "flat space")
            tb = self._tables[id(sp)] = _Tables(sp, rows)
            tb.gid = self.group_ids(sp).to(sp.device)
        else:
            tb.refresh(rows)
        return tb.gid, tb.hp

    def _elem_values(self, sp, start, end):
        """(lr, weight_decay) per element of [start, end) of a CPU flat space, as fp32 vectors."""
        from ..nn.flat import ALIGN
        hp = torch.tensor(self._hp_rows(sp), dtype=torch.float32)
        idx = self.group_ids(sp).long().repeat_interleave(ALIGN)[start:end]
        return hp[idx, 0], hp[idx, 1]

    def _members(self, params):
        """[(group, its parameters among ``params``)], in group order."""
        ids = {id(p) for p in params}
        return [(g, [p for p in g["params"] if id(p) in ids]) for g in self.param_groups]

    # --- device scalars -------------------------------------------------------------
    def _scalar(self, name, device, init=0.0, n=1):
        """Get or create this optimizer's fp32 tensor ``name`` on ``device``: [n], filled with ``init``."""
        t = self._scalars.get((name, device))
        if t is None:
            t = self._scalars[(name, device)] = torch.full((n,), float(init), dtype=torch.float32, device=device)
        return t

    def _scalars_named(self, name):
        return [t for (nm, _), t in self._scalars.items() if nm == name]

    def lr_tensor(self, device):
        """fp32 device scalar the single-group launches read the learning rate from."""
        return self._scalar("lr", device, self.param_groups[0]["lr"])

    def first_tensor(self, device):
        """fp32 device flag: 1 until the first fused step after a reset clears it."""
        return self._scalar("first", device, 1.0)

    def step_tensor(self, device):
        """fp32 device step count of the bias corrections, advanced inside the step."""
        return self._scalar("step", device)

    def max_norm_tensor(self, device):
        """fp32 device scalar the norm launch reads its threshold from."""
        return self._scalar("max_norm", device, self.param_groups[0]["max_grad_norm"])

    def _norm_out_tensor(self, device):
        """fp32 [3] scratch of the norm launch: sum of squares, norm, clip coefficient."""
        return self._scalar("norm_out", device, n=3)

    def _step_dev_inc(self, device):
        from ..ops import kernels as K
        t = self.step_tensor(device)
        K.increment_(t, 1.0)
        return t

    def set_lr(self, lr):
        """A number sets every group's LR; a sequence sets one LR per group (in group order).
        The device scalar (group 0's LR) and the launches' tables follow, so a captured
        step runs with the new values without re-capture.  With an :class:`LRSchedule` attached these
        are the base (peak) LRs: the schedule rewrites the current LR at its unchanged position."""
        if self._lr_schedule is not None:
            if isinstance(lr, (list, tuple)) or (isinstance(lr, torch.Tensor) and lr.dim() > 0):
                lrs = [float(v) for v in lr]
                if len(lrs) != len(self.param_groups):
                    raise ValueError(f"set_lr: {len(lrs)} learning rates for {len(self.param_groups)} parameter "
                                     f"groups")
            else:
                lrs = [float(lr)] * len(self.param_groups)
            self._lr_schedule._set_base(lrs)
            return
        if isinstance(lr, (list, tuple)) or (isinstance(lr, torch.Tensor) and lr.dim() > 0):
            lrs = [float(v) for v in lr]
            if len(lrs) != len(self.param_groups):
                raise ValueError(f"set_lr: {len(lrs)} learning rates for {len(self.param_groups)} parameter groups")
            for g, v in zip(self.param_groups, lrs):
                g["lr"] = v
            lr = lrs[0]
        else:
            for g in self.param_groups:
                g["lr"] = lr
        for t in self._scalars_named("lr"):
            t.fill_(float(lr))
        for tb in self._tables.values():
            tb.refresh(self._hp_rows(tb.space))

    def _lr_outputs(self):
        """[(tensor, rows, row stride, parameter-group index per row)]: the device words the launches over
        the GPU spaces read their LR from (after :meth:`prepare`), for an :class:`LRSchedule`."""
        if self.grouped:
            n = len(self.param_groups)
            return [(tb.hp, n, 2, list(range(n))) for tb in self._tables.values()]
        return [(t, 1, 1, [0]) for t in self._scalars_named("lr")]

    def set_grad_scale(self, s: float):
        """Folded into the step: the DP all-reduce SUMs, the optimizer averages."""
        self._grad_scale = float(s)

    # --- global-norm clipping ---------------------------------------------------------
    @property
    def clips(self) -> bool:
        """True when the step clips the global gradient norm (``max_grad_norm`` given)."""
        return self.param_groups[0].get("max_grad_norm") is not None

    def set_max_grad_norm(self, v: float):
        """Change the clip threshold (a captured step follows it without re-capture).  Only on
        an optimizer built with ``max_grad_norm``: clipping on / off is a different step."""
        if not self.clips:
            raise ValueError("this optimizer was built without max_grad_norm; create it with one to clip")
        if v is None or not float(v) > 0.0:
            raise ValueError("max_grad_norm must be a positive number")
        for g in self.param_groups:
            g["max_grad_norm"] = float(v)
        for t in self._scalars_named("max_norm"):
            t.fill_(float(v))

    def grad_norm_tensor(self, device=None):
        """The last step's global norm of the averaged gradient (before clipping) as a one-element
        tensor: a view of the norm launch's output on a GPU (no synchronisation), a CPU tensor
        otherwise."""
        if not self.clips:
            raise ValueError("this optimizer does not clip: no gradient norm is computed")
        if device is None:
            spaces, _ = self._flat_groups()
            device = spaces[0][0].device if spaces else "cpu"
        device = torch.device(device)
        if device.type == "cuda":
            return self._norm_out_tensor(device)[1:2]
        return torch.tensor([float("nan") if self._norm_host is None else self._norm_host])

    def _clip_dev(self, sp, loose):
        """Launch the norm over GPU space ``sp`` and return the device coefficient for the fused
        update.  Clipping on a GPU needs every parameter in that one flat space."""
        spaces, _ = self._flat_groups()
        if len(spaces) != 1 or loose:
            raise ValueError("max_grad_norm on a GPU needs every parameter in one flat space")
        from ..ops import kernels as K
        out = self._norm_out_tensor(sp.device)
        K.grad_norm_(sp.grad, out, self.max_norm_tensor(sp.device), grad_scale=self._grad_scale)
        return out[2:3]

    def _clip_loose(self, params):
        """torch form of the norm launch for CPU spaces / loose parameters: the coefficient
        (a python float, 1.0 when nothing clips) for gradients scaled by grad_scale."""
        grads = [p.grad for p in params if p.grad is not None]
        if not grads:
            return 1.0
        ss = torch.stack([(g.float() * g.float()).sum() for g in grads]).sum()
        nrm = self._grad_scale * torch.sqrt(ss)
        self._norm_host = float(nrm)
        c = self.param_groups[0]["max_grad_norm"] / (nrm + 1e-6)
        return float(torch.clamp(c, max=1.0))

    # --- the step -----------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, **kw):
        """One step over every parameter.  Per GPU flat space, in this order: the space's deferred
        gradient folds, :meth:`_begin_space`, the clip launch, :meth:`_step_space`; then
        :meth:`_finish_step`; then the torch form over CPU spaces and loose parameters.  ``kw``:
        what the subclass's launch does once per step (SGD's ``advance``), so space 0 alone gets it."""
        loss = closure() if closure is not None else None
        spaces, loose = self._flat_groups()
        devices = []
        for k, (sp, members) in enumerate(spaces):
            if sp.device.type != "cuda":
                loose += members
                continue
            sp.finish_grads()
            new_device = sp.device not in devices
            if new_device:
                devices.append(sp.device)
            self._begin_space(sp, new_device)
            clip = self._clip_dev(sp, loose) if self.clips else None
            self._step_space(sp, clip, **(kw if k == 0 else {}))
        self._finish_step(devices)
        if loose:
            coef = self._clip_loose(loose) if self.clips else 1.0
            for group, params in self._members(loose):
                self._step_loose(group, params, self._grad_scale * coef)
        return loss

    def _begin_space(self, sp, new_device):
        """Before the launches over GPU space ``sp``; new_device: the step's first space on its device."""

    def _step_space(self, sp, clip, **kw):
        """The update launches over GPU space ``sp``; clip: the device clip coefficient or None."""
        raise NotImplementedError

    def _step_loose(self, group, params, scale):
        """torch form of the update for ``params`` of ``group``, gradients scaled by ``scale``."""
        raise NotImplementedError

    def _finish_step(self, devices):
        """After the last GPU space (``devices``: theirs): the class's host bookkeeping."""

    def _clear_first(self, devices=()):
        """End of a momentum step: the first-step flag goes down, on ``devices`` and on the host."""
        if self.param_groups[0]["momentum"] != 0:
            from ..ops import kernels as K
            for dev in devices:
                K.fill_(self.first_tensor(dev), 0.0)
        self._first = False

    # ---- per-range steps (optimizer overlapped with backward, engine/dp.py) -------------
    def supports_ranges(self) -> bool:
        """True when :meth:`step_range` can apply the step: every parameter lives in one flat space
        (no loose parameters; on a GPU unless the class has a CPU range path) and nothing clips."""
        spaces, loose = self._flat_groups()
        return (len(spaces) == 1 and not loose and not self.clips
                and (self._cpu_ranges or spaces[0][0].device.type == "cuda"))

    def supports_shard_range(self) -> bool:
        """One :meth:`step_range` per step over this rank's chunk (engine/dp.py shard plan)."""
        return self.supports_ranges()

    def begin_ranges(self):
        """Start of a step applied through ``step_range`` calls (no-op unless overridden)."""

    def _range_space(self, start, end):
        """The one flat space of a ``step_range`` over [start, end), after the checks they share."""
        if self.clips:     # the global norm needs the whole gradient before any element is updated
            raise ValueError("a clipping optimizer cannot step by ranges (the norm needs the whole gradient)")
        spaces, loose = self._flat_groups()
        if len(spaces) != 1 or loose:
            raise ValueError("step_range needs all parameters in one flat space")
        if self.grouped and (start % 64 or (end - start) % 64):
            raise ValueError(f"a grouped step_range covers whole 64-element granules from an aligned start "
                             f"(got [{start}, {end}))")
        return spaces[0][0]

    # --- state --------------------------------------------------------------------------
    def _flat_groups(self):
        ps = [p for g in self.param_groups for p in g["params"]]
        return _spaces(ps)

    def zero_grad(self, set_to_none: bool = False):
        spaces, loose = self._flat_groups()
        for sp, _ in spaces:
            sp.zero_grad()
        for p in loose:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def reset_state(self):
        """Zero every optimizer state buffer (K-AVG round boundary)."""
        from ..ops import kernels as K
        for bufs in self._state_bufs.values():
            for t in bufs.values():
                if t.is_cuda:
                    K.memset_(t)
                else:
                    t.zero_()
        self.state.clear()
        self._first = True
        self._step_host = 0
        for t in self._scalars_named("step"):
            t.zero_()
        for t in self._scalars_named("first"):
            t.fill_(1.0)

    def prepare(self):
        """Allocate every device state buffer now (not lazily inside a first step), so
        :meth:`state_tensors` is complete before a graph capture."""
        spaces, _ = self._flat_groups()
        for sp, _ in spaces:
            if sp.device.type != "cuda":
                continue
            self.state_buffers(sp)
            self.lr_tensor(sp.device)
            self.first_tensor(sp.device)
            self.step_tensor(sp.device)
            if self.clips:            # scratch of the norm launch, not optimizer state
                self.max_norm_tensor(sp.device)
                self._norm_out_tensor(sp.device)
            self._prepare_tables(sp)
        return self

    def _prepare_tables(self, sp):
        if self.grouped:          # the grouped launches' tables: scratch as well
            self.group_tables(sp)

    def state_tensors(self) -> List[torch.Tensor]:
        """Every device tensor :meth:`step` mutates: the state buffers, the step count and the
        first-step flag (not the lr, clip or table scratch)."""
        out = [t for bufs in self._state_bufs.values() for t in bufs.values()]
        return out + self._scalars_named("step") + self._scalars_named("first")

    def state_buffers(self, sp) -> Dict[str, torch.Tensor]:
        """The per-element fp32 state buffers of flat space ``sp`` by name (allocated on first use)."""
        d = self._state_bufs.get(id(sp))
        if d is None:
            d = {n: torch.zeros(sp.numel, dtype=torch.float32, device=sp.device) for n in self._STATE_NAMES}
            self._state_bufs[id(sp)] = d
        return d

    def host_state(self):
        """The host side of the step bookkeeping, for a snapshot (:meth:`load_host_state` restores it)."""
        return self._first, self._step_host

    def load_host_state(self, host):
        self._first, self._step_host = host

    @property
    def stepped(self) -> bool:
        """True once a step was applied since construction or the last :meth:`reset_state`."""
        return self._step_host > 0 or not self._first


# mom, first, lr: the momentum buffer, the first-step flag and the learning-rate scalar of the space's
# device (the first two None without momentum); then the first parameter group's scalars
SgdOperands = namedtuple("SgdOperands", "mom first lr wd momentum dampening nesterov")


class SGD(FusedOptimizer):
    """``step(advance=(ctr, batch, n))`` folds the data-counter advance into the launch (see
    :meth:`fuse_advance`)."""
    kind = "sgd"
    _cpu_ranges = True

    @property
    def _STATE_NAMES(self):
        return ("momentum",) if self.param_groups[0]["momentum"] != 0 else ()

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 max_grad_norm=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov, max_grad_norm=max_grad_norm))

    def fuse_advance(self, ctr, batch, n) -> bool:
        """Can ``step(advance=(ctr, batch, n))`` advance the on-device data-sampler counter
        ``ctr`` (``ops.kernels.advance_counter_``) inside its SGD launch instead of a
        one-thread launch of its own?  False when no GPU flat space holds the counter's
        device.  Nothing is attached to the optimizer: the advance is per call."""
        spaces, _ = self._flat_groups()
        return bool(spaces and spaces[0][0].device.type == "cuda" and ctr.device == spaces[0][0].device)

    def sgd_operands(self, sp) -> SgdOperands:
        """What an SGD launch over flat space ``sp`` takes from this optimizer, for the launches that
        carry the update themselves (the shard collective, the rider slices) as for its own."""
        g = self.param_groups[0]
        mom = self.state_buffers(sp).get("momentum")
        first = self.first_tensor(sp.device) if mom is not None else None
        return SgdOperands(mom, first, self.lr_tensor(sp.device), g["weight_decay"], g["momentum"], g["dampening"],
                           g["nesterov"])

    def _launch(self, sp, start, end, max_blocks, clip, advance):
        """The one SGD launch over [start, end) of GPU space ``sp``."""
        from ..ops import kernels as K
        op = self.sgd_operands(sp)
        if self.grouped and end <= start:      # nothing to launch; a folded advance still happens
            if advance is not None:
                K.advance_counter_(*advance)
            return
        w, gr, mom, shadow = (None if t is None else t[start:end] for t in (sp.master, sp.grad, op.mom, sp.shadow))
        kw = dict(momentum=op.momentum, dampening=op.dampening, nesterov=op.nesterov, first=self._first,
                  grad_scale=self._grad_scale, first_dev=op.first, max_blocks=max_blocks, advance=advance,
                  clip_dev=clip)
        if self.grouped:
            gid, hp = self.group_tables(sp)
            K.sgd_groups_(w, gr, mom, shadow, gid, hp, start, **kw)
        else:
            K.sgd_(w, gr, mom, shadow, self.param_groups[0]["lr"], wd=op.wd, lr_dev=op.lr, **kw)

    def _step_space(self, sp, clip, advance=None):
        self._launch(sp, 0, sp.numel, 0, clip, advance)

    def _step_loose(self, group, params, scale):
        _torch_sgd(params, group, self.state, scale)

    _finish_step = FusedOptimizer._clear_first

    @torch.no_grad()
    def step_range(self, start: int, end: int, max_blocks: int = 0, advance_step: bool = True, advance=None):
        """The fused step restricted to flat elements [start, end): the gradients of a
        finished backward stage are applied while earlier stages still run backward.  The
        first-step flag stays set until :meth:`finish_ranges` (every range of the step
        reads the same value); the union of one step's ranges must cover the space once.
        advance_step: accepted for the ranged-step protocol (SGD keeps no step counter).
        advance: (ctr, batch, n) data-counter advance folded into this launch (as :meth:`step`)."""
        sp = self._range_space(start, end)
        if sp.device.type != "cuda":
            g = self.param_groups[0]
            if self.grouped:      # the same ops with each element's own lr and weight decay
                lr, wd = self._elem_values(sp, start, end)
                g = dict(g, lr=lr, weight_decay=wd)
            _sgd_range_cpu(sp, start, end, g, self.state_buffers(sp).get("momentum"), self._first, self._grad_scale)
            return
        sp.finish_grads_range(start, end)
        self._launch(sp, start, end, max_blocks or _RANGE_BLOCKS, None, advance)

    @torch.no_grad()
    def finish_ranges(self):
        """End of a step applied through :meth:`step_range`: clear the first-step flag."""
        spaces, _ = self._flat_groups()
        dev = spaces[0][0].device
        self._clear_first([dev] if dev.type == "cuda" else [])


# grid cap of a range update (it runs beside the backward on a side stream)
_RANGE_BLOCKS = 64


def _sgd_range_cpu(sp, start, end, g, mom, first, grad_scale):
    """torch form of k_sgd over [start, end) of a CPU flat space (same math as the kernel).
    Through ``.data``: parameters are views of the flat buffer and share its autograd version
    counter, which a range update must not bump while other stages' backward still runs."""
    w, gr = sp.master.data[start:end], sp.grad.data[start:end]
    d = gr * grad_scale if grad_scale != 1.0 else gr          # op for op as _torch_sgd
    per_elem = isinstance(g["lr"], torch.Tensor)    # a grouped optimizer: lr / weight decay vectors
    if per_elem:
        d = d + g["weight_decay"] * w
    elif g["weight_decay"]:
        d = d.add(w, alpha=g["weight_decay"])
    if mom is not None:
        m = mom.data[start:end]
        if first:
            m.copy_(d)
        else:
            m.mul_(g["momentum"]).add_(d, alpha=1 - g["dampening"])
        d = d.add(m, alpha=g["momentum"]) if g["nesterov"] else m
    if per_elem:
        w.sub_(g["lr"] * d)
    else:
        w.add_(d, alpha=-g["lr"])
    if sp.shadow is not None:
        sp.shadow.data[start:end].copy_(w)


def _torch_sgd(params, g, state, grad_scale):
    for p in params:
        if p.grad is None:
            continue
        d = p.grad * grad_scale if grad_scale != 1.0 else p.grad
        if g["weight_decay"]:
            d = d.add(p, alpha=g["weight_decay"])
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


class Adam(FusedOptimizer):
    kind = "adam"
    decoupled = False
    _STATE_NAMES = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm))

    def _launch(self, sp, start, end, max_blocks, clip):
        """The one Adam launch over [start, end) of GPU space ``sp`` (none over an empty range)."""
        from ..ops import kernels as K
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        bufs = self.state_buffers(sp)
        if end <= start:
            return
        w, gr, m, v, shadow = (None if t is None else t[start:end]
                               for t in (sp.master, sp.grad, bufs["exp_avg"], bufs["exp_avg_sq"], sp.shadow))
        kw = dict(step_dev=self.step_tensor(sp.device), max_blocks=max_blocks, clip_dev=clip)
        if self.grouped:
            gid, hp = self.group_tables(sp)
            K.adam_groups_(w, gr, m, v, shadow, gid, hp, 0.0, start, b1, b2, g["eps"], self.decoupled,
                           self._grad_scale, **kw)
        else:
            K.adam_(w, gr, m, v, shadow, g["lr"], 0.0, b1, b2, g["eps"], g["weight_decay"], self.decoupled,
                    self._grad_scale, lr_dev=self.lr_tensor(sp.device), **kw)

    def _begin_space(self, sp, new_device):
        self._step_dev_inc(sp.device)

    def _step_space(self, sp, clip):
        self._launch(sp, 0, sp.numel, 0, clip)

    def _step_loose(self, group, params, scale):
        _torch_adam(params, group, self.state, scale, self.decoupled)

    def _finish_step(self, devices):
        self._step_host += 1

    @torch.no_grad()
    def begin_ranges(self):
        """Start of a step applied as several ranges (engine/dp.py ``opt_overlap``): advance the
        bias-correction step once; every stage's :meth:`step_range` then runs with
        ``advance_step=False``, so a step split into ranges equals one whole step."""
        spaces, _ = self._flat_groups()
        self._step_host += 1
        self._step_dev_inc(spaces[0][0].device)

    def finish_ranges(self):
        """End of a ranged step (nothing to clear: the counter advanced in begin_ranges)."""

    @torch.no_grad()
    def step_range(self, start: int, end: int, max_blocks: int = 0, advance_step: bool = True):
        """The fused step over flat elements [start, end) only.  advance_step=True (a sharded
        update: this rank owns that chunk of the master and its moments, one range per step)
        advances the step counter; False (one of several stage ranges of a step, after
        :meth:`begin_ranges`) reuses it."""
        sp = self._range_space(start, end)
        if advance_step:
            self._step_host += 1
            self._step_dev_inc(sp.device)
        sp.finish_grads_range(start, end)
        self._launch(sp, start, end, max_blocks or (0 if advance_step else _RANGE_BLOCKS), None)


class AdamW(Adam):
    kind = "adamw"
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm)


def _torch_adam(params, g, state, grad_scale, decoupled):
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
        if decoupled:
            p.mul_(1 - g["lr"] * g["weight_decay"])
        elif g["weight_decay"]:
            gr = gr.add(p, alpha=g["weight_decay"])
        st["exp_avg"].mul_(b1).add_(gr, alpha=1 - b1)
        st["exp_avg_sq"].mul_(b2).addcmul_(gr, gr, value=1 - b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        denom = (st["exp_avg_sq"].sqrt() / (bc2 ** 0.5)).add_(g["eps"])
        p.addcdiv_(st["exp_avg"], denom, value=-g["lr"] / bc1)


def from_torch(opt: torch.optim.Optimizer) -> FusedOptimizer:
    """Fused equivalent of a stock torch optimizer: the same parameter groups with the same
    hyper-parameters.  Groups may differ in lr and weight_decay; a difference in anything else
    (betas, eps, momentum, ...) has no fused form and raises ValueError (never dropped silently)."""
    if isinstance(opt, FusedOptimizer):
        return opt
    if isinstance(opt, torch.optim.AdamW):
        cls, keys = AdamW, ("lr", "betas", "eps", "weight_decay")
    elif isinstance(opt, torch.optim.Adam):
        cls, keys = Adam, ("lr", "betas", "eps", "weight_decay")
    elif isinstance(opt, torch.optim.SGD):
        cls, keys = SGD, ("lr", "momentum", "dampening", "weight_decay", "nesterov")
    else:
        raise TypeError(f"no fused equivalent for {type(opt).__name__}")
    groups = [dict({k: g[k] for k in keys}, params=list(g["params"])) for g in opt.param_groups]
    return cls(groups, **{k: opt.param_groups[0][k] for k in keys})


def with_max_grad_norm(opt: FusedOptimizer, max_grad_norm) -> FusedOptimizer:
    """A fresh fused optimizer of the same class, parameter groups and hyper-parameters as ``opt``
    that clips the global gradient norm at ``max_grad_norm`` (None: does not clip)."""
    mgn = None if max_grad_norm is None else float(max_grad_norm)
    groups = [dict({k: g[k] for k in opt.defaults}, params=list(g["params"]), max_grad_norm=mgn)
              for g in opt.param_groups]
    kw = {k: opt.param_groups[0][k] for k in opt.defaults}
    kw["max_grad_norm"] = mgn
    new = type(opt)(groups, **kw)
    new.set_grad_scale(opt._grad_scale)
    return new


def no_decay_groups(module: torch.nn.Module, weight_decay: float):
    """The usual two parameter groups of ``module`` for an optimizer's first argument: weights
    (``ndim > 1``) at ``weight_decay``, then biases and BN / LayerNorm weights (``ndim <= 1``) at 0."""
    decay, no_decay = [], []
    for p in module.parameters():
        if p.requires_grad:
            (no_decay if p.ndim <= 1 else decay).append(p)
    groups = [{"params": decay, "weight_decay": float(weight_decay)}, {"params": no_decay, "weight_decay": 0.0}]
    return [g for g in groups if g["params"]]


from .layerwise import LAMB, LARS, layerwise_groups  # noqa: E402  (needs FusedOptimizer above)
from .ema import EMA  # noqa: E402
from .lr_schedule import LRSchedule, lr_factor  # noqa: E402
