"""Decode-time state of a decoder LM: the per-layer key / value cache and the per-sequence
bookkeeping that one captured decode step reads and advances on the device."""
from __future__ import annotations

import torch


def filter_logits(logits, tokens, lens, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0):
    """Stock-torch twin of the filters of ``kml_decode_sample``, in HF's processor order.

    ``logits [B, classes]``; ``tokens [B, L]`` int64 and ``lens [B]``: row b's history is
    ``tokens[b, 0 .. lens[b]]``.  Returns ``(penalised logits, keep mask)``.

    1. Repetition penalty, once per distinct id of the history inside ``[0, classes)``: a logit v
       becomes ``v / penalty`` if positive, else ``v * penalty``.  bf16 input takes the kernel's
       arithmetic: ``bf16(fp32(v) * fp32(1 / penalty))`` and ``bf16(fp32(v) * fp32(penalty))``.
    2. Columns are compared as values: ``-0.0 == +0.0``, NaN is never kept.
    3. ``0 < top_k < classes``: keep what is ``>=`` the k-th largest value (its ties included).
    4. ``top_p < 1``: with ``w = exp((v - vmax) / T)`` over the survivors (fp64) and Z their sum,
       walk the classes of equal value downwards and keep the smallest prefix of whole classes
       whose mass is ``>= fp32(top_p) * Z``; the class of the maximum always stays.
    The temperature is taken as the fp32 number the kernel reads."""
    B, C = logits.shape
    z = logits.clone()
    if penalty != 1.0:
        pen = torch.tensor(float(penalty), dtype=torch.float32)
        inv = torch.tensor(1.0 / float(penalty), dtype=torch.float32)
        for b in range(B):
            ids = tokens[b, :max(int(lens[b]) + 1, 0)].cpu()
            ids = torch.unique(ids[(ids >= 0) & (ids < C)]).to(z.device)
            v = z[b, ids]
            if z.dtype == torch.bfloat16:
                f = v.float()
                z[b, ids] = torch.where(f > 0, f * inv.to(f.device), f * pen.to(f.device)).to(torch.bfloat16)
            else:
                z[b, ids] = torch.where(v > 0, v / float(penalty), v * float(penalty))
    x = z.double().cpu() + 0.0   # -0.0 + 0.0 = +0.0
    T = float(torch.tensor(float(temperature), dtype=torch.float32))
    p = float(torch.tensor(float(top_p), dtype=torch.float32))
    valid = ~torch.isnan(x)
    xs = torch.where(valid, x, torch.full_like(x, float("-inf")))
    keep = valid.clone()
    if 0 < top_k < C:
        kth = xs.topk(int(top_k), dim=-1).values[:, -1:]
        keep &= xs >= kth
    if p < 1.0:
        for b in range(B):
            if not bool(keep[b].any()):
                continue
            v = xs[b][keep[b]]
            vals, inverse = torch.unique(v, return_inverse=True)   # ascending classes
            vmax = vals[-1]
            w = torch.where(vals == vmax, torch.ones_like(vals), torch.exp((vals - vmax) / T))
            mass = torch.zeros_like(vals).index_add_(0, inverse, w[inverse]).flip(0)   # descending
            cum = mass.cumsum(0)
            reach = (cum >= p * cum[-1]).nonzero()
            idx = int(reach[0]) if reach.numel() else vals.numel() - 1
            keep[b] &= xs[b] >= vals.flip(0)[idx]
    return z, keep.to(z.device)


def lookup_draft_reference(tokens, lens, k, max_ngram=2):
    """Stock-torch twin of ``kml_draft_lookup`` (prompt-lookup drafting, HF's
    ``prompt_lookup_num_tokens``): ``k`` draft tokens per sequence from its own history
    ``tokens[b, 0 .. L]``, ``L = lens[b]``.

    For ``g = min(max_ngram, L)`` down to 1 the suffix of ``g`` tokens ending at ``L`` is searched
    among the starts ``s <= L - g`` (an earlier occurrence with at least one token after it); the
    most recent one wins.  The draft is the tokens that follow it, never past ``L``; the remaining
    slots repeat the last copied token.  Without a match at any ``g`` every slot is
    ``tokens[b, L]``.  Returns int64 ``[B, k]`` on the device of ``tokens``."""
    B, Lcap = tokens.shape
    rows, ls = tokens.cpu().tolist(), lens.cpu().tolist()
    out = []
    for b in range(B):
        L = min(max(int(ls[b]), 0), Lcap - 1)
        h = rows[b]
        start = L
        for g in range(min(int(max_ngram), L), 0, -1):
            suffix = h[L - g + 1:L + 1]
            hit = next((s for s in range(L - g, -1, -1) if h[s:s + g] == suffix), None)
            if hit is not None:
                start = hit + g
                break
        out.append([h[min(start + j, L)] for j in range(int(k))])
    return torch.tensor(out, dtype=torch.int64, device=tokens.device).reshape(B, int(k))


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
    * ``fpar`` fp32 ``[temperature, top_p, penalty, 1 / penalty]`` and ``ipar`` int32 ``[top_k]``:
      what the filtered sampler (``kml_decode_sample``) reads; ``info`` fp32 ``[B, 4]``: what it
      reports per row (threshold value, kept columns, kept mass share, row maximum).
    * speculative decoding (``reset(draft_tokens=k)``, None before): ``start`` / ``limit`` int32
      ``[B]`` — the index of each sequence's last prompt token (the origin of its sampling steps)
      and the index ``lens[b]`` never passes; ``draft`` int64 ``[B, k]``: the tokens the next verify
      round checks; ``pick`` int32 ``[B * (k + 1)]``: what the round chose per row; ``stats`` int32
      ``[accepted drafts, committed tokens, max(limit - lens), 0]``; ``ws_multi``: the attention
      partials of ``k + 1`` queries per (sequence, head) (GPU only).
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
        self.fpar = torch.tensor([1.0, 1.0, 1.0, 1.0], dtype=torch.float32, device=device)
        self.ipar = torch.zeros(1, dtype=torch.int32, device=device)
        self.info = torch.zeros((self.B, 4), dtype=torch.float32, device=device)
        self.ws = None
        if gpu:
            from ..ops import decode as D
            self.ws = D.attn_decode_workspace(self.B, self.H, self.Lcap, device)
        self.sample = False   # Gumbel-max sampling at temp[0] instead of the argmax
        self.filtered = False   # a repetition penalty, top-k or top-p is on: the filtered sampler picks
        self.filters = (1.0, 0, 1.0, 1.0)   # host copy: temperature, top_k, top_p, penalty
        self.gen = None       # CPU sampling: the torch.Generator the draws come from
        self._graphs = {}     # (advance, sample, filtered) -> (captured step, its logits)
        # verify rounds (reset(draft_tokens=k) allocates them)
        self.draft_tokens = 0
        self.start = self.limit = self.draft = self.pick = self.stats = self.ws_multi = None
        self.ublocks = {}     # CPU sampling in verify rounds: new-token index -> its [B, vocab] uniforms

    def reset(self, seed=0, temperature=0.0, eos_token_id=None, top_k=0, top_p=1.0, repetition_penalty=1.0,
              start=None, limit=None, draft_tokens=0):
        """Empty the cache for a new batch (the K / V rows are simply no longer covered by lens)
        and set the sampling state; ``top_k`` 0, ``top_p`` 1 and ``repetition_penalty`` 1 are off.

        ``draft_tokens = k > 0`` prepares verify rounds of ``k + 1`` rows per sequence: ``start``
        (``[B]``: ``prompt_len[b] - 1``, default 0) is where a sequence's sampling steps count from
        and ``limit`` (``[B]``, default ``Lcap - 1``) the index its ``lens`` never passes.  With the
        default 0 nothing of this is allocated or touched."""
        from ..ops.decode import sampling_params
        fpar, ipar = sampling_params(temperature, top_k, top_p, repetition_penalty, sample=temperature > 0)
        self.lens.zero_()
        self.tokens.zero_()
        self.next_ids.zero_()
        self.finished.zero_()
        eos = -1 if eos_token_id is None else int(eos_token_id)
        self.ctl.copy_(torch.tensor([int(seed) & 0x7FFFFFFF, 0, eos, 0], dtype=torch.int32))
        self.temp.fill_(float(temperature) if temperature > 0 else 1.0)
        self.sample = temperature > 0
        self.fpar.copy_(torch.tensor(fpar, dtype=torch.float32))
        self.ipar.copy_(torch.tensor(ipar, dtype=torch.int32))
        self.filters = (fpar[0], ipar[0], fpar[1], fpar[2])
        self.filtered = ipar[0] != 0 or fpar[1] != 1.0 or fpar[2] != 1.0
        if self.device.type != "cuda":
            self.gen = torch.Generator().manual_seed(int(seed))
        k = int(draft_tokens)
        if k == 0:
            if start is not None or limit is not None:
                raise ValueError("reset: start / limit belong to verify rounds (draft_tokens >= 1)")
            return
        if k < 0 or self.B * (k + 1) > 16:
            raise ValueError(f"reset: {k} draft tokens for {self.B} sequences; B * (k + 1) must be in 2..16")
        if self.filtered:
            raise ValueError("reset: verify rounds do not run behind top-k, top-p or a repetition penalty")
        dev = self.device
        if self.draft_tokens != k:
            self.draft_tokens = k
            self.draft = torch.zeros((self.B, k), dtype=torch.int64, device=dev)
            self.pick = torch.zeros(self.B * (k + 1), dtype=torch.int32, device=dev)
            self.ws_multi = None
            if dev.type == "cuda":
                from ..ops import decode as D
                self.ws_multi = D.attn_decode_multi_workspace(self.B, self.H, self.Lcap, k + 1, dev)
        if self.start is None:
            self.start = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.limit = torch.zeros(self.B, dtype=torch.int32, device=dev)
            self.stats = torch.zeros(4, dtype=torch.int32, device=dev)
        def per_sequence(v, default):
            if v is None:
                return torch.full((self.B,), default, dtype=torch.int32)
            return torch.as_tensor(v).reshape(self.B).to(torch.int32).cpu()
        self.start.copy_(per_sequence(start, 0))
        self.limit.copy_(per_sequence(limit, self.Lcap - 1).clamp(max=self.Lcap - 1))
        self.draft.zero_()
        self.stats.zero_()
        self.ublocks = {}

    # ------------------------------------------------------------------ CPU path (plain tensors)
    def append_cpu(self, i, qkv, Lq, decode):
        """K / V thirds of a ``[B*Lq, 3*H*64]`` buffer into layer i: rows 0..Lq-1 (prefill) or
        rows ``lens[b] + t`` (decode: Lq = 1 in a plain step, the rows of a verify round
        otherwise); rows at or past Lcap are dropped."""
        B, H, D = self.B, self.H, self.H * 64
        k = qkv[:, D:2 * D].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
        v = qkv[:, 2 * D:].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
        if not decode:
            n = min(Lq, self.Lcap)
            self.k[i][:, :, :n] = k[:, :, :n]
            self.v[i][:, :, :n] = v[:, :, :n]
            return
        for b in range(B):
            for t in range(Lq):
                r = int(self.lens[b]) + t
                if 0 <= r < self.Lcap:
                    self.k[i][b, :, r] = k[b, :, t]
                    self.v[i][b, :, r] = v[b, :, t]

    def attend_cpu(self, i, qkv, Lq=1):
        """softmax(q Kᵀ / 8) V of layer i; q = the first third of qkv ``[B*Lq, 3*H*64]``: row
        ``b*Lq + t`` sees cache rows ``0 .. lens[b] + t``.  The queries of a sequence are taken one
        at a time, each with the shapes of the one-query call, so row t has the bits of a plain
        step at that length."""
        B, H = self.B, self.H
        kt = self.k[i].transpose(-1, -2)
        cols = torch.arange(self.Lcap)[None, :]
        q = qkv[:, :H * 64].reshape(B, Lq, H, 1, 64)
        out = []
        for t in range(Lq):
            s = (q[:, t] @ kt) / 8.0                                           # [B, H, 1, Lcap]
            past = cols > (self.lens[:, None].long() + t).clamp(max=self.Lcap - 1)   # [B, Lcap]
            s = s.masked_fill(past[:, None, None, :], float("-inf"))
            out.append((s.softmax(-1) @ self.v[i]).reshape(B, H * 64))
        return out[0] if Lq == 1 else torch.stack(out, 1).reshape(B * Lq, H * 64)

    def uniforms_cpu(self, t, shape):
        """The uniform block plain CPU sampling consumes for new-token index ``t`` (0 is the
        prefill's pick, drawn by the prefill itself): blocks are drawn once, in increasing ``t``,
        from the cache's generator and kept until :meth:`forget_uniforms_cpu` drops them."""
        have = max(self.ublocks, default=0)
        for n in range(have + 1, t + 1):
            self.ublocks[n] = torch.rand(shape, generator=self.gen, dtype=torch.float64).clamp_(1e-300, 1.0 - 1e-16)
        return self.ublocks[t]

    def forget_uniforms_cpu(self, below):
        """Drop the kept blocks of index < ``below`` (never the newest: it marks what was drawn)."""
        newest = max(self.ublocks, default=0)
        for n in [n for n in self.ublocks if n < below and n != newest]:
            del self.ublocks[n]
