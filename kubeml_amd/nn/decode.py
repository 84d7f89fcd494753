"""Decode-time state of a decoder LM: the per-layer key / value cache and the per-sequence
bookkeeping that one captured decode step reads and advances on the device."""
from __future__ import annotations

import torch


class KVCache:
    """Keys and values of ``layers`` attention layers for ``B`` sequences of up to ``Lcap``
    tokens (rounded up to a multiple of 64), head dim 64.

    * ``k[i]``, ``v[i]``: ``[B, H, Lcap, 64]``, head-major — one (b, h) key stream is contiguous
      128-byte rows.  bf16 and uninitialised on the GPU (rows past ``lens[b]`` are never read);
      zeros of ``dtype`` on the CPU.
    * ``lens`` int32 ``[B]``: index of the newest token of each sequence (its key is row
      ``lens[b]`` once the step has appended it).
    * ``tokens`` int64 ``[B, Lcap]``: prompt and generated tokens; ``next_ids`` int64 ``[B]``: the
      token the next step feeds; ``finished`` int32 ``[B]``: eos seen.
    * ``ctl`` int32 ``[seed, step, eos (-1: none), 0]`` and ``temp`` fp32 ``[temperature]``: what
      the sampler reads; ``ws``: the chunk partials of the decode attention (GPU only).
    """

    def __init__(self, layers, B, H, Lcap, device, dtype=None):
        device = torch.device(device)
        self.layers, self.B, self.H = int(layers), int(B), int(H)
        self.Lcap = -(-int(Lcap) // 64) * 64
        self.device = device
        gpu = device.type == "cuda"
        self.dtype = torch.bfloat16 if gpu else (dtype or torch.float32)
        shape = (self.B, self.H, self.Lcap, 64)
        make = torch.empty if gpu else torch.zeros
        self.k = [make(shape, dtype=self.dtype, device=device) for _ in range(self.layers)]
        self.v = [make(shape, dtype=self.dtype, device=device) for _ in range(self.layers)]
        self.lens = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.tokens = torch.zeros((self.B, self.Lcap), dtype=torch.int64, device=device)
        self.next_ids = torch.zeros(self.B, dtype=torch.int64, device=device)
        self.finished = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.ctl = torch.tensor([0, 0, -1, 0], dtype=torch.int32, device=device)
        self.temp = torch.ones(1, dtype=torch.float32, device=device)
        self.ws = None
        if gpu:
            from ..ops import decode as D
            self.ws = D.attn_decode_workspace(self.B, self.H, self.Lcap, device)
        self.sample = False   # Gumbel-max sampling at temp[0] instead of the argmax
        self.gen = None       # CPU sampling: the torch.Generator the draws come from
        self._graphs = {}     # (advance, sample) -> (captured step, its logits)

    def reset(self, seed=0, temperature=0.0, eos_token_id=None):
        """Empty the cache for a new batch (the K / V rows are simply no longer covered by lens)."""
        self.lens.zero_()
        self.tokens.zero_()
        self.next_ids.zero_()
        self.finished.zero_()
        eos = -1 if eos_token_id is None else int(eos_token_id)
        self.ctl.copy_(torch.tensor([int(seed) & 0x7FFFFFFF, 0, eos, 0], dtype=torch.int32))
        self.temp.fill_(float(temperature) if temperature > 0 else 1.0)
        self.sample = temperature > 0
        if self.device.type != "cuda":
            self.gen = torch.Generator().manual_seed(int(seed))

    # ------------------------------------------------------------------ CPU path (plain tensors)
    def append_cpu(self, i, qkv, Lq, decode):
        """K / V thirds of a ``[B*Lq, 3*H*64]`` buffer into layer i: rows 0..Lq-1 (prefill) or
        row ``lens[b]`` (decode, Lq = 1); rows at or past Lcap are dropped."""
        B, H, D = self.B, self.H, self.H * 64
        k = qkv[:, D:2 * D].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
        v = qkv[:, 2 * D:].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
        if not decode:
            n = min(Lq, self.Lcap)
            self.k[i][:, :, :n] = k[:, :, :n]
            self.v[i][:, :, :n] = v[:, :, :n]
            return
        for b in range(B):
            r = int(self.lens[b])
            if 0 <= r < self.Lcap:
                self.k[i][b, :, r] = k[b, :, 0]
                self.v[i][b, :, r] = v[b, :, 0]

    def attend_cpu(self, i, qkv):
        """softmax(q Kᵀ / 8) V over cache rows 0..lens[b] of layer i; q = the first third of qkv."""
        B, H = self.B, self.H
        q = qkv[:, :H * 64].reshape(B, H, 1, 64)
        s = (q @ self.k[i].transpose(-1, -2)) / 8.0                          # [B, H, 1, Lcap]
        past = torch.arange(self.Lcap)[None, :] > self.lens[:, None].long()  # [B, Lcap]
        s = s.masked_fill(past[:, None, None, :], float("-inf"))
        return (s.softmax(-1) @ self.v[i]).reshape(B, H * 64)
