"""Exponential moving average of the weights, for validation, checkpoints and inference.

The parameters (in storage layout) and the fp32 module buffers (BN running statistics) of a
flattened model are one contiguous fp32 prefix of ``FlatParamSpace.state`` (``[0, i64_off)``), so
the average is ONE buffer of that size and ONE streaming launch per step (``kml_ema_update``,
csrc/kernels/ema.hip), issued after every update of the master.  The int64 counters stay the live
model's.

Everything that changes per step lives on the device: ``ctl = [ticks, updates, applied, 0]`` (int32)
gates the launch (``update_every``) and drives timm's decay warm-up ``min(decay, (1 + updates) /
(10 + updates))``; ``aout[0]`` is the weight ``a = 1 - d`` of the last launch.  A captured train step
(``engine.dp.make_train_step(..., ema=)``) therefore carries one EMA launch that follows both
without re-capture.  The element update is ``e + (w - e) * a`` with three fp32 roundings, which is
what :func:`update_twin` computes with stock torch operations, bit for bit.

Evaluating with the averaged weights exchanges the two buffers in place (:meth:`EMA.swap`,
:meth:`EMA.applied`): the forward kernels read the bf16 shadow and the BatchNorm statistics as
views of the state buffer, so captured eval graphs are reused as they are, and two swaps restore
every bit of the live model.

K-AVG: the EMA is linear in the weights, so the mean of the workers' EMAs (:meth:`EMA.average_`)
is the EMA of the mean trajectory as long as every worker takes part in every averaging round;
only ragged tail rounds (a worker without data contributes no steps) depart from that.

An un-flattened CPU module (the CPU workers' models) is served through a gathered copy of its
fp32 tensors: same methods, same arithmetic, nothing about the module changes.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Iterator, List, Tuple

import torch

__all__ = ["EMA", "update_twin", "decay_weight"]

F32 = torch.float32
CTL_KEY = "ema.__ctl__"
# grid cap of the update launch: every block takes a ticket on one word (about 20 ns apiece, one
# after the other), so the launch runs fastest with one block per CU: 45 us at 256 blocks against
# 112 us at the kernel's own cap of 2048 over the ResNet-34 prefix, 239 against 369 us over the
# BERT-base space, 128 blocks slower again (profiles/r16/ema.md).  The result does not depend on it.
UPDATE_BLOCKS = 256
PREFIX = "ema."


def decay_weight(decay: float, updates: int, warmup: bool) -> torch.Tensor:
    """``a = 1 - d`` as the kernel forms it, every operation in fp32: ``d = min(decay, (1 + updates) /
    (10 + updates))`` under ``warmup``, else ``decay``.  A 0-d fp32 CPU tensor."""
    d = torch.tensor(float(decay), dtype=F32)
    if warmup:
        d = torch.minimum(d, torch.tensor(updates + 1, dtype=F32) / torch.tensor(updates + 10, dtype=F32))
    return torch.tensor(1.0, dtype=F32) - d


@torch.no_grad()
def update_twin(ema, w, decay, every, warmup, ctl, aout, a=None):
    """Stock-torch form of ``kml_ema_update`` on any device: the same gate, the same fp32 ``a``
    (or the given one) and the same three-operation element form.  Reads ``ctl`` on the host."""
    ticks, updates = int(ctl[0]), int(ctl[1])
    apply = (ticks + 1) % int(every) == 0
    if a is None:
        a = decay_weight(decay, updates, warmup)
    a = torch.as_tensor(a, dtype=F32).reshape(()).to(ema.device)
    if apply:
        ema.copy_(ema + (w - ema) * a)
    ctl[0], ctl[1], ctl[2] = ticks + 1, updates + int(apply), int(apply)
    aout[0] = a


class _LooseState:
    """The fp32 parameters and buffers of an un-flattened CPU module behind the attributes the EMA
    reads from a flat space: ``state`` is a gathered copy (:meth:`pull` / :meth:`push`)."""
    shadow = None

    def __init__(self, module: torch.nn.Module):
        self.module = module
        live = self._live()
        if any(t.device.type != "cpu" for _, t in live):
            raise ValueError("EMA: a GPU module must be flattened first (nn.flatten_module)")
        self.entries: List[Tuple[str, int, int]] = []
        off = 0
        for name, t in live:
            self.entries.append((name, off, t.numel()))
            off += t.numel()
        self.numel = sum(t.numel() for _, t in live if isinstance(t, torch.nn.Parameter))
        self.i64_off = -(-off // 4) * 4
        self.device = torch.device("cpu")
        self.state = torch.zeros(max(self.i64_off, 4), dtype=F32)
        self.pull()

    def _live(self):
        sd = self.module.state_dict(keep_vars=True)
        ts = [(k, v) for k, v in sd.items() if v.dtype == F32]
        # parameters first, as in the flat layout
        return ([kv for kv in ts if isinstance(kv[1], torch.nn.Parameter)] +
                [kv for kv in ts if not isinstance(kv[1], torch.nn.Parameter)])

    @torch.no_grad()
    def pull(self):
        for (_, o, n), (_, t) in zip(self.entries, self._live()):
            self.state[o:o + n].copy_(t.detach().reshape(-1))

    @torch.no_grad()
    def push(self):
        for (_, o, n), (_, t) in zip(self.entries, self._live()):
            t.data.copy_(self.state[o:o + n].view(t.shape))


class EMA:
    """``EMA(module_or_space, decay=0.9999, update_every=1, warmup=True)``.

    One fp32 buffer ``ema`` of ``space.i64_off`` elements, initialised from the live state, plus the
    device words ``ctl``, ``aout`` and ``ticket``.  ``update()`` is one launch on a GPU space and
    :func:`update_twin` elsewhere; call it after every optimizer step (a captured step built with
    ``make_train_step(..., ema=ema)`` does).  ``named_tensors`` / ``state_dict`` need the module.
    """

    def __init__(self, module_or_space, decay: float = 0.9999, update_every: int = 1, warmup: bool = True):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"EMA: decay must be in [0, 1], got {decay!r}")
        if isinstance(update_every, bool) or not isinstance(update_every, int) or update_every < 1:
            raise ValueError(f"EMA: update_every must be an integer >= 1, got {update_every!r}")
        self.decay, self.update_every, self.warmup = float(decay), update_every, bool(warmup)
        self.module = None
        if isinstance(module_or_space, torch.nn.Module):
            self.module = module_or_space
            space = getattr(module_or_space, "_kml_flat", None)
            if space is None:
                space = _LooseState(module_or_space)
        else:
            space = module_or_space
        if getattr(space, "state", None) is None:
            raise ValueError("EMA: needs a module or its FlatParamSpace")
        self.space = space
        self.n = int(space.i64_off)
        dev = space.state.device
        self.ema = space.state[:self.n].detach().clone()
        self.ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        self.aout = torch.zeros(1, dtype=F32, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.max_blocks = UPDATE_BLOCKS
        self.swapped = False       # True between the two swaps of an evaluation pass

    # --- the live state ---------------------------------------------------------------------
    @property
    def _loose(self) -> bool:
        return isinstance(self.space, _LooseState)

    def _live(self) -> torch.Tensor:
        """The fp32 prefix the EMA follows (a view of the flat state; current after ``pull``)."""
        if self._loose:
            self.space.pull()
        return self.space.state[:self.n]

    # --- update -----------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        """One EMA step (gated by ``update_every``, warmed up by the update count)."""
        if self.swapped:
            raise RuntimeError("EMA.update() inside applied(): the live weights are swapped out")
        if self.ema.is_cuda:
            from ..ops import kernels as K
            K.ema_update_(self.ema, self.space.state[:self.n], self.decay, self.update_every, self.warmup,
                          self.ctl, self.aout, self.ticket, max_blocks=self.max_blocks)
        else:
            update_twin(self.ema, self._live(), self.decay, self.update_every, self.warmup, self.ctl, self.aout)

    @torch.no_grad()
    def reset(self):
        """``ema := state``, counters back to 0."""
        self.ema.copy_(self._live())
        self.ctl.zero_()
        self.aout.zero_()

    def state_tensors(self) -> List[torch.Tensor]:
        """Every device tensor :meth:`update` mutates (graph capture snapshots them)."""
        return [self.ema, self.ctl, self.aout, self.ticket]

    @property
    def updates(self) -> int:
        """Applied updates so far (one device read)."""
        return int(self.ctl[1])

    @property
    def last_decay(self) -> float:
        """The decay the last launch ran with, ``1 - aout[0]`` (one device read)."""
        return 1.0 - float(self.aout[0])

    # --- evaluation with the averaged weights -------------------------------------------------
    @torch.no_grad()
    def swap(self):
        """Exchange the live state prefix and the EMA; the bf16 shadow follows the new state."""
        sp = self.space
        if self.ema.is_cuda:
            from ..ops import kernels as K
            K.ema_swap_(sp.state[:self.n], self.ema, sp.shadow, sp.numel)
        else:
            live = self._live()
            tmp = live.clone()
            live.copy_(self.ema)
            self.ema.copy_(tmp)
            if self._loose:
                sp.push()
            else:
                sp.refresh_shadow()
        self.swapped = not self.swapped

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied():`` the model runs with the averaged weights and BN statistics; the
        live model is back, bit for bit, on exit (also when the body raises)."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # --- names --------------------------------------------------------------------------------
    def named_tensors(self) -> Iterator[Tuple[str, torch.Tensor]]:
        """(state_dict name, view of ``ema``) for every fp32 tensor of the module the EMA covers, with
        the shape and strides of the module's own tensor (a conv weight's KRSC storage shows as the
        same strided ``[Cout, Cin, KH, KW]`` view the flat space binds to ``p.data``)."""
        if self.module is None:
            raise ValueError("EMA.named_tensors needs the module (EMA(module, ...))")
        if self._loose:
            at = {name: (o, n) for name, o, n in self.space.entries}
            for name, t in self.module.state_dict(keep_vars=True).items():     # in state_dict order
                if name in at:
                    o, n = at[name]
                    yield name, self.ema[o:o + n].view(t.shape)
            return
        state = self.space.state
        base, lo = state.untyped_storage().data_ptr(), state.storage_offset()
        for name, t in self.module.state_dict(keep_vars=True).items():
            t = t.data
            if t.dtype != F32 or t.device != state.device or t.untyped_storage().data_ptr() != base:
                continue
            off = t.storage_offset() - lo
            if 0 <= off < self.n:
                yield name, self.ema.as_strided(t.shape, t.stride(), self.ema.storage_offset() + off)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """``ema.<name>`` dense CPU copies plus ``ema.__ctl__`` (the int32 counters)."""
        out = {PREFIX + k: v.detach().to("cpu").contiguous().clone() for k, v in self.named_tensors()}
        out[CTL_KEY] = self.ctl.detach().to("cpu").clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        missing = []
        for name, v in self.named_tensors():
            src = sd.get(PREFIX + name)
            if src is None:
                missing.append(name)
            else:
                v.copy_(src.to(v.device, v.dtype))
        if strict and (missing or CTL_KEY not in sd):
            raise KeyError(f"EMA.load_state_dict: missing {missing or CTL_KEY}")
        if CTL_KEY in sd:
            self.ctl.copy_(sd[CTL_KEY].to(self.ctl.device, torch.int32))

    # --- data-parallel workers ------------------------------------------------------------------
    @torch.no_grad()
    def broadcast_(self, comm, src: int = 0):
        """Every worker takes rank ``src``'s EMA and counters."""
        if comm.world == 1:
            return
        comm.broadcast_(self.ema, src)
        comm.broadcast_(self.ctl, src)

    @torch.no_grad()
    def average_(self, comm):
        """Mean of the workers' EMAs (all-reduce SUM times ``1 / world``; nothing at world 1).  The
        EMA is linear in the weights, so after K-AVG rounds in which every worker took part this is
        the EMA of the mean trajectory; ragged tail rounds are the only departure."""
        if comm.world == 1:
            return
        comm.all_reduce_(self.ema)
        if self.ema.is_cuda:
            from ..ops import kernels as K
            K.scale_(self.ema, 1.0 / comm.world)
        else:
            self.ema.mul_(1.0 / comm.world)
