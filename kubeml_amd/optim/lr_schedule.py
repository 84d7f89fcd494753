"""Per-step learning-rate schedules whose LR is written on the device.

Every fused launch reads its learning rate from device memory (the ``lr_tensor`` scalar, column 0 of
the grouped ``[G, 2]`` table, column 0 of the layer-wise ``[T, 4]`` table; the SGD riders and the update
inside the ZeRO-1 collective read the scalar too).  :class:`LRSchedule` owns those words once it is
attached to a :class:`~kubeml_amd.optim.FusedOptimizer`: one single-block launch per step
(``kml_lr_schedule``, csrc/kernels/lr_schedule.hip) writes ``base * f(x)`` into them, with the step
counter ``t``, the position ``(x0, dx)`` and the base (peak) LRs in device memory.  A captured train
step (``engine.dp.make_train_step(..., lr_schedule=)``) therefore carries one launch that moves the LR
every replay, with no host ``fill_`` or table copy between replays.

Position and factor::

    x = x0 + float(t) * dx                                  (fp32: product, then sum)
    x < warmup:  f = warmup_start + (1 - warmup_start) * (x / warmup)
    else:        q = clamp((x - warmup) / (total - warmup), 0, 1),  f = min_ratio + (1 - min_ratio) * d

    constant    d = 1
    linear      d = 1 - q
    polynomial  d = (1 - q) ** power            (power == 1 is the linear path)
    cosine      d = 0.5 * (1 + cos(pi q))
    step        f = gamma ** k, k = number of milestones <= x   (total and min_ratio unused)

``(x0, dx) = (0, 1)`` counts optimizer steps; ``KubeModel`` measures position in epochs and sets
``(epoch, 1 / steps_of_the_task)`` at the start of every train task, so a worker crosses ``[e, e + 1)``
once per epoch whatever its shard size, K or the epoch's parallelism.

``step()`` follows torch's convention: call it after ``optimizer.step()``; it writes the LR of the next
step.  Attaching writes ``lr(0)``, so optimizer step ``s`` (0-based) runs with ``base * f(s)``, as with
``torch.optim.lr_scheduler.LambdaLR``.  From then on ``optimizer.set_lr`` sets the base (peak) LR and
the current LR is rewritten at the unchanged ``t``.

:func:`lr_factor` is the stock-torch fp32 twin of the kernel: the same bits for ``constant``, ``linear``
and ``step`` (every rounding is spelled out on both sides); ``cosine`` and a general ``power`` go
through ``cosf`` / ``powf`` on the device and agree to a few ulp.  CPU flat spaces and loose parameters
are served by the twin: it sets ``param_groups[k]["lr"]`` to the fp32 product ``base_k * f``.  With every
parameter in a GPU flat space ``param_groups[k]["lr"]`` keeps the base LR and :meth:`LRSchedule.last_lr`
reads the current one.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch

__all__ = ["LRSchedule", "lr_factor", "KINDS", "MAX_MILESTONES", "MAX_T"]

F32 = torch.float32
KINDS = ("constant", "linear", "polynomial", "cosine", "step")
MAX_MILESTONES = 8
MAX_T = 1 << 24          # float(t) is exact below


def _f32(v) -> torch.Tensor:
    return torch.as_tensor(v, dtype=F32).reshape(()).cpu() if torch.is_tensor(v) else torch.tensor(float(v), dtype=F32)


def _check_shape(kind, warmup, total, min_ratio, warmup_start, power, gamma, milestones):
    if kind not in KINDS:
        raise ValueError(f"LR schedule: kind is one of {KINDS}, got {kind!r}")
    ms = tuple(float(v) for v in milestones)
    if len(ms) > MAX_MILESTONES:
        raise ValueError(f"LR schedule: at most {MAX_MILESTONES} milestones, got {len(ms)}")
    if any(b < a for a, b in zip(ms, ms[1:])):
        raise ValueError("LR schedule: milestones must ascend")
    warmup = float(warmup)
    if not warmup >= 0.0:
        raise ValueError(f"LR schedule: warmup must be >= 0, got {warmup!r}")
    if kind == "step":
        total = 0.0 if total is None else float(total)
    else:
        if total is None or not float(total) > warmup:
            raise ValueError(f"LR schedule: total must be greater than warmup (total {total!r}, warmup {warmup!r})")
        total = float(total)
    if not 0.0 <= float(min_ratio) <= 1.0 or not 0.0 <= float(warmup_start) <= 1.0:
        raise ValueError("LR schedule: min_ratio and warmup_start are fractions of the base LR in [0, 1]")
    if not float(power) > 0.0 or not float(gamma) > 0.0:
        raise ValueError("LR schedule: power and gamma must be positive")
    return dict(kind=kind, warmup=warmup, total=total, min_ratio=float(min_ratio), warmup_start=float(warmup_start),
                power=float(power), gamma=float(gamma), milestones=ms)


def _position(t, x0, dx) -> torch.Tensor:
    """x = x0 + float(t) * dx in fp32, two roundings."""
    t = int(t)
    if not 0 <= t < MAX_T:
        raise ValueError(f"LR schedule: step index {t} outside [0, 2^24): float(t) would not be exact")
    return _f32(x0) + _f32(t) * _f32(dx)


def _factor(x: torch.Tensor, s: dict) -> torch.Tensor:
    """f(x) for a 0-d fp32 position, operation for operation as the kernel."""
    one = _f32(1.0)
    w = _f32(s["warmup"])
    if s["warmup"] > 0.0 and bool(x < w):
        ws = _f32(s["warmup_start"])
        return ws + (one - ws) * (x / w)
    if s["kind"] == "step":
        d, g = one.clone(), _f32(s["gamma"])
        for ms in s["milestones"]:
            if bool(_f32(ms) <= x):
                d = d * g
        return d
    q = torch.clamp((x - w) / (_f32(s["total"]) - w), 0.0, 1.0)
    kind, power = s["kind"], _f32(s["power"])
    if kind == "linear" or (kind == "polynomial" and float(power) == 1.0):
        d = one - q
    elif kind == "polynomial":
        d = torch.pow(one - q, power)
    elif kind == "cosine":
        d = _f32(0.5) * (one + torch.cos(_f32(3.14159265358979323846) * q))
    else:
        d = one
    m = _f32(s["min_ratio"])
    return m + (one - m) * d


def lr_factor(t, x0, dx, kind, warmup=0.0, total=None, min_ratio=0.0, warmup_start=0.0, power=1.0, gamma=0.1,
              milestones=()) -> torch.Tensor:
    """The factor ``f`` the kernel writes for step index ``t`` at position ``(x0, dx)``, computed with
    stock torch fp32 operations: a 0-d fp32 CPU tensor.  ``torch.tensor(base, dtype=torch.float32) * f`` is
    the LR.  Bit for bit the kernel's value for ``constant``, ``linear``, ``step`` and ``polynomial`` with
    ``power == 1``; within a few ulp for ``cosine`` and other powers."""
    s = _check_shape(kind, warmup, total, min_ratio, warmup_start, power, gamma, milestones)
    return _factor(_position(t, x0, dx), s)


class LRSchedule:
    """``LRSchedule(optimizer, kind, warmup=0, total=None, min_ratio=0, warmup_start=0, power=1, gamma=0.1,
    milestones=())`` attaches to a fused optimizer (SGD, Adam, AdamW, LAMB, LARS; one group or several).

    The groups' current LRs become the base LRs and ``lr(0)`` is written at once.  Either every parameter
    lives in GPU flat spaces of one device (one launch per LR table: one per step for a model in one flat
    space) or none does (the twin).  Device state: ``ctl`` int32 [4] = [t, 0, 0, 0], ``pos`` fp32 [2] =
    [x0, dx], ``last`` fp32 [2] = [x, f] of the LR just written, and one fp32 base vector per table.
    """

    def __init__(self, optimizer, kind: str, warmup: float = 0.0, total=None, min_ratio: float = 0.0,
                 warmup_start: float = 0.0, power: float = 1.0, gamma: float = 0.1, milestones: Sequence[float] = ()):
        from . import FusedOptimizer
        if not isinstance(optimizer, FusedOptimizer):
            raise TypeError("LRSchedule attaches to a kubeml_amd.optim fused optimizer (optim.from_torch converts "
                            "a torch.optim.SGD / Adam / AdamW)")
        if getattr(optimizer, "_lr_schedule", None) is not None:
            raise ValueError("this optimizer already has an LR schedule")
        self.shape = _check_shape(kind, warmup, total, min_ratio, warmup_start, power, gamma, milestones)
        self.optimizer = optimizer
        self.base_lrs = [float(g["lr"]) for g in optimizer.param_groups]
        spaces, loose = optimizer._flat_groups()
        gpu = [sp for sp, _ in spaces if sp.device.type == "cuda"]
        host = bool(loose) or len(gpu) != len(spaces)
        if gpu and (host or len({sp.device for sp in gpu}) != 1):
            raise ValueError("LRSchedule: every parameter in GPU flat spaces of one device, or none")
        self.device = gpu[0].device if gpu else torch.device("cpu")
        self.ctl = torch.zeros(4, dtype=torch.int32, device=self.device)
        self.pos = torch.tensor([0.0, 1.0], dtype=F32, device=self.device)
        self.last = torch.zeros(2, dtype=F32, device=self.device)
        self._bound = 0            # host upper bound of t (a captured replay advances it without the host)
        # (out, rows, stride, base, group index per row) of every LR table on the device
        self._outs: List[tuple] = []
        if gpu:
            optimizer.prepare()
            self._outs = [(out, rows, stride, torch.zeros(rows, dtype=F32, device=self.device), of)
                          for out, rows, stride, of in optimizer._lr_outputs()]
            for tb in optimizer._tables.values():
                tb.scheduled = True
        optimizer._lr_schedule = self
        self._upload_base()
        self._write(0)

    # --- base LRs ---------------------------------------------------------------------------
    def _upload_base(self):
        for _, _, _, base, of in self._outs:
            base.copy_(torch.tensor([0.0 if k is None else self.base_lrs[k] for k in of], dtype=F32))

    def _set_base(self, lrs):
        """``optimizer.set_lr`` with a schedule attached: new base LRs, the current LR rewritten at the
        unchanged ``t``."""
        self.base_lrs = [float(v) for v in lrs]
        if self._outs:
            for g, v in zip(self.optimizer.param_groups, self.base_lrs):
                g["lr"] = v
            self._upload_base()
        self._write(0)

    # --- the launch ---------------------------------------------------------------------------
    @torch.no_grad()
    def _write(self, advance: int):
        """``t += advance`` and the LR of step ``t`` into every table: the launches on a GPU, the twin
        elsewhere.  No host bookkeeping: this is what a captured step records."""
        if self._outs:
            from ..ops import kernels as K
            for i, (out, rows, stride, base, _) in enumerate(self._outs):
                K.lr_schedule_(out, rows, stride, base, self.ctl, self.pos, self.last, advance if i == 0 else 0,
                               **self.shape)
            return
        t = int(self.ctl[0]) + advance
        x = _position(t, self.pos[0], self.pos[1])
        f = _factor(x, self.shape)
        for g, b in zip(self.optimizer.param_groups, self.base_lrs):
            g["lr"] = float(_f32(b) * f)
        self.ctl[0] = t
        self.last[0], self.last[1] = x, f

    def _count(self, n: int = 1):
        self._bound += n
        if self._bound >= MAX_T:
            raise ValueError(f"LR schedule: step index {self._bound} reaches 2^24, float(t) would stop being exact "
                             f"(set_position restarts the count)")

    def step(self):
        """After ``optimizer.step()``: advance ``t`` and write the LR of the next step."""
        self._count()
        self._write(1)

    def _replayed(self):
        """Host side of one replay of a captured step that carries the launch."""
        self._count()

    # --- accessors ----------------------------------------------------------------------------
    def state_tensors(self) -> List[torch.Tensor]:
        """Every device tensor :meth:`step` mutates: the counter, ``last`` and the LR words themselves
        (graph capture snapshots and restores them, so capturing a step neither advances the schedule
        nor leaves the LR of a later step behind)."""
        return [self.ctl, self.last] + [out for out, *_ in self._outs]

    @property
    def t(self) -> int:
        """The step index of the LR now in place (one device read)."""
        return int(self.ctl[0])

    def last_factor(self) -> float:
        return float(self.last[1])

    def last_lr(self) -> List[float]:
        """The LR now in place, one per parameter group: the fp32 products ``base_k * f`` of the factor
        the last launch left in ``last`` (one device read)."""
        f = self.last[1:2].to("cpu")[0]
        return [float(_f32(b) * f) for b in self.base_lrs]

    @torch.no_grad()
    def set_position(self, x0: float, dx: float):
        """``x = x0 + t * dx`` from now on, with ``t`` back at 0; the LR of that position is written."""
        self.pos.copy_(torch.tensor([float(x0), float(dx)], dtype=F32))
        self.ctl.zero_()
        self._bound = 0
        self._write(0)

    def state_dict(self) -> Dict:
        pos = self.pos.to("cpu")
        return {"t": self.t, "x0": float(pos[0]), "dx": float(pos[1]), "base_lrs": list(self.base_lrs),
                "shape": dict(self.shape, milestones=list(self.shape["milestones"]))}

    @torch.no_grad()
    def load_state_dict(self, sd: Dict):
        shape = sd.get("shape")
        if shape is not None and dict(shape, milestones=tuple(shape["milestones"])) != self.shape:
            raise ValueError("LRSchedule.load_state_dict: the saved schedule has another shape")
        t = int(sd["t"])
        if not 0 <= t < MAX_T:
            raise ValueError(f"LRSchedule.load_state_dict: t = {t} outside [0, 2^24)")
        if len(sd["base_lrs"]) != len(self.base_lrs):
            raise ValueError("LRSchedule.load_state_dict: another number of parameter groups")
        self.pos.copy_(torch.tensor([float(sd["x0"]), float(sd["dx"])], dtype=F32))
        self.ctl.copy_(torch.tensor([t, 0, 0, 0], dtype=torch.int32))
        self._bound = t
        self._set_base(sd["base_lrs"])
