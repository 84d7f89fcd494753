"""Decode-time state of a decoder LM: the per-layer key / value cache and the per-sequence
bookkeeping that one captured decode step reads and advances on the device; and
:class:`DecodeMixin`, the model-independent half of ``generate`` that the decoder LMs share."""
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
      128-byte rows.  ``kv_heads = Hkv`` (grouped-query models; None: ``H``) makes them ``[B, Hkv,
      Lcap, 64]``: query head h reads K/V head ``h // (H // Hkv)``; the workspace stays sized for
      the ``H`` query heads.  bf16 and uninitialised on the GPU (rows past ``lens[b]`` are never read);
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

    def __init__(self, layers, B, H, Lcap, device, dtype=None, kv_heads=None):
        device = torch.device(device)
        self.layers, self.B, self.H = int(layers), int(B), int(H)
        self.Hkv = self.H if kv_heads is None else int(kv_heads)
        if self.Hkv < 1 or self.H % self.Hkv:
            raise ValueError(f"KVCache: kv_heads {kv_heads} must divide the {self.H} heads")
        self.Lcap = -(-int(Lcap) // 64) * 64
        self.device = device
        gpu = device.type == "cuda"
        self.dtype = torch.bfloat16 if gpu else (dtype or torch.float32)
        shape = (self.B, self.Hkv, self.Lcap, 64)
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
            self.ws = (D.attn_decode_workspace if kv_heads is None else D.attn_decode_gqa_workspace)(
                self.B, self.H, self.Lcap, device)
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
        """K / V parts of a ``[B*Lq, (H + 2*Hkv)*64]`` buffer (thirds when ``Hkv == H``) into layer
        i: rows 0..Lq-1 (prefill) or rows ``lens[b] + t`` (decode: Lq = 1 in a plain step, the rows
        of a verify round otherwise); rows at or past Lcap are dropped."""
        B, H, D, E = self.B, self.Hkv, self.H * 64, self.Hkv * 64
        k = qkv[:, D:D + E].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
        v = qkv[:, D + E:].reshape(B, Lq, H, 64).permute(0, 2, 1, 3)
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
        """softmax(q Kᵀ / 8) V of layer i; q = the first ``H*64`` columns of qkv ``[B*Lq, (H +
        2*Hkv)*64]``: row ``b*Lq + t`` sees cache rows ``0 .. lens[b] + t``.  The queries of a
        sequence are taken one at a time, each with the shapes of the one-query call, so row t has
        the bits of a plain step at that length.  With ``Hkv < H`` every K/V head serves its group
        of ``H // Hkv`` query heads."""
        B, H = self.B, self.H
        kc, vc = self.k[i], self.v[i]
        if self.Hkv != H:
            kc, vc = (t.repeat_interleave(H // self.Hkv, 1) for t in (kc, vc))
        kt = kc.transpose(-1, -2)
        cols = torch.arange(self.Lcap)[None, :]
        q = qkv[:, :H * 64].reshape(B, Lq, H, 1, 64)
        out = []
        for t in range(Lq):
            s = (q[:, t] @ kt) / 8.0                                           # [B, H, 1, Lcap]
            past = cols > (self.lens[:, None].long() + t).clamp(max=self.Lcap - 1)   # [B, Lcap]
            s = s.masked_fill(past[:, None, None, :], float("-inf"))
            out.append((s.softmax(-1) @ vc).reshape(B, H * 64))
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


def draft_count(k, max_ngram):
    """``prompt_lookup_num_tokens`` as an int (None: 0), both options checked."""
    k = 0 if k is None else k
    if isinstance(k, bool) or not isinstance(k, (int, float)) or int(k) != k or k < 0:
        raise ValueError(f"prompt_lookup_num_tokens must be an integer >= 0, got {k!r}")
    if isinstance(max_ngram, bool) or not isinstance(max_ngram, (int, float)) or int(max_ngram) != max_ngram \
            or max_ngram < 1:
        raise ValueError(f"max_matching_ngram_size must be an integer >= 1, got {max_ngram!r}")
    return int(k)


def advance_cpu(cache, logits, gen):
    """Stock-torch twin of ``kml_decode_advance`` / ``kml_decode_sample`` on a CPU cache."""
    eos = int(cache.ctl[2])
    keep = None
    if cache.filtered:
        T, k, p, pen = cache.filters
        logits, keep = filter_logits(logits, cache.tokens, cache.lens, T, k, p, pen)
    if cache.sample:
        u = torch.rand(logits.shape, generator=gen, dtype=torch.float64).clamp_(1e-300, 1.0 - 1e-16)
        key = logits.double() / float(cache.temp[0]) - torch.log(-torch.log(u))
        if keep is not None:
            key = key.masked_fill(~keep, float("-inf"))
        tok = key.argmax(-1)
    elif keep is not None:   # the argmax of the penalised row; NaN never wins, an all-NaN row gives 0
        tok = logits.masked_fill(torch.isnan(logits), float("-inf")).argmax(-1)
    else:
        tok = logits.argmax(-1)
    if eos >= 0:
        tok = torch.where(cache.finished.bool(), torch.full_like(tok, eos), tok)
        cache.finished |= (tok == eos).to(torch.int32)
    cache.next_ids.copy_(tok)
    nxt = cache.lens.long() + 1
    ok = nxt < cache.Lcap
    cache.tokens[torch.arange(cache.B)[ok], nxt[ok]] = tok[ok]
    cache.lens.copy_(nxt.clamp(max=cache.Lcap - 1).to(torch.int32))
    cache.ctl[1] += 1


class DecodeMixin:
    """The model-independent half of KV-cache decoding, shared by the decoder LMs.  A model supplies

    * ``vocab``, ``_decode_max_pos`` (positions it can address) and ``_decode_table`` (its token
      table parameter: the device, dtype and shadow address a captured step is bound to);
    * ``new_cache(B, Lcap, device)``;
    * ``_prefill(ids, attention_mask, cache)``: the prompt through the training kernels, every
      layer's K / V appended, ``lens[b] = prompt_len[b] - 1``, returns the last prompt logits;
    * ``_step(cache, advance)``: one step from ``cache.next_ids`` at position ``lens[b]``; on the GPU
      it ends with :meth:`_pick` when ``advance``, on the CPU with :func:`advance_cpu`;
    * optionally ``_generate_lookup`` (prompt-lookup speculative decoding).

    Inference only (no autograd, no dropout whatever the module's mode).  GPU: the prompt runs the
    training kernels once, every later token one captured step of the decode kernels
    (csrc/kernels/decode.hip).  CPU: the same steps in stock torch on a cache of plain tensors."""

    def _pick(self, cache, logits):
        """The GPU step's last launch: the plain sampler, or the filtered one when the cache has
        a repetition penalty, top-k or top-p on."""
        from ..ops import decode as D
        if cache.filtered:
            D.decode_sample(logits, self.vocab, cache.ctl, cache.fpar, cache.ipar, cache.next_ids, cache.tokens,
                            cache.lens, cache.finished, sample=cache.sample, info=cache.info)
        else:
            D.decode_advance(logits, self.vocab, cache.ctl, cache.temp, cache.next_ids, cache.tokens, cache.lens,
                             cache.finished, sample=cache.sample)

    def quantize_decode_weights(self, dtype="int8"):
        """Weight-only quantisation of the decode step: every :class:`~kubeml_amd.nn.Linear` the step
        reaches (the attention and MLP projections and the output head, a tied one included) gets
        an int8 copy of its current bf16 shadow weight with one fp32 scale per output row
        (``Linear.quantize_small``), and ``forward_small`` — the captured step and the verify
        round — streams that copy through the int8 skinny GEMMs.  Activations, sums, the token
        gather, the prefill and training keep bf16.  ``dtype=None`` undoes it.

        This is a speed feature: a step reads half the weight bytes.  The bf16 weights stay
        resident, so memory grows by the int8 copies instead of shrinking.  The copies are a
        snapshot: after training or ``load_state_dict`` call this again.  Needs a flattened model
        on the GPU in eval mode (``ValueError`` otherwise: there is no int8 CPU path).  Every call
        retires the captured steps, which hold weight addresses.  Returns the names of the layers
        left in bf16: an input width that is no multiple of 16, or a shape at which the int8 kernel
        measured slower (``nn.modules._SMALL_W8_SLOWER``: the 576-wide Llama's, whose step is
        launch-bound, stays bf16 altogether)."""
        from .modules import Linear
        if dtype not in (None, "int8"):
            raise ValueError(f"quantize_decode_weights: dtype {dtype!r} (\"int8\" or None)")
        if dtype is not None:
            if not self._decode_table.is_cuda:
                raise ValueError("quantize_decode_weights: the int8 decode kernels are GPU only")
            if getattr(self, "_kml_flat", None) is None or self.training:
                raise ValueError("quantize_decode_weights: needs a flattened model (nn.flatten_module) in eval mode")
        left = [name for name, m in self.named_modules() if isinstance(m, Linear) and not m.quantize_small(dtype)]
        # a new stamp: no step captured before this call is replayed (_graphs_of), and generate's
        # own caches go with their captures
        self.__dict__["_kml_w8_stamp"] = self.__dict__.get("_kml_w8_stamp", 0) + 1
        self.__dict__.get("_kml_decode_caches", {}).clear()
        return left if dtype is not None else []

    def _graphs_of(self, cache):
        """``cache._graphs``, emptied first if its steps were captured under another quantisation
        state of the model than the current one (they hold the addresses of the weights they read)."""
        stamp = self.__dict__.get("_kml_w8_stamp", 0)
        if getattr(cache, "_w8_stamp", 0) != stamp:
            cache._graphs.clear()
            cache._w8_stamp = stamp
        return cache._graphs

    def _replay(self, cache, advance):
        """The GPU step as one captured graph per (cache, advance, sampling, filtered); captured
        on first use after an eager warm-up whose effect on the decode state is rolled back.  The
        filter parameters live in device memory: other values replay the same graph."""
        key = (bool(advance), bool(cache.sample), bool(cache.filtered))
        ent = self._graphs_of(cache).get(key)
        if ent is None:
            from ..engine.step import capture_graph
            state = [cache.lens, cache.tokens, cache.next_ids, cache.finished, cache.ctl]
            keep = [t.clone() for t in state]
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._step(cache, advance)   # re-appends the same K / V row: idempotent
            cur.wait_stream(side)
            for t, k in zip(state, keep):
                t.copy_(k)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with capture_graph(g, capture_error_mode="thread_local"):
                logits = self._step(cache, advance)
            ent = cache._graphs[key] = (g, logits)
        ent[0].replay()
        return ent[1]

    def decode_step(self, cache):
        """Feed ``cache.next_ids``, append its keys / values, pick the next token (greedy or
        Gumbel-max, behind the cache's repetition penalty / top-k / top-p if any is on) and
        advance ``lens``.  Returns the logits."""
        if cache.lens.is_cuda:
            return self._replay(cache, True)
        return self._step(cache, True)

    def prefill(self, ids, attention_mask, cache):
        """Run the right-padded prompt, fill the cache and pick each sequence's first new token
        (``cache.next_ids``, ``cache.tokens[b, prompt_len[b]]``).  Returns the prompt's last logits."""
        logits = self._prefill(ids, attention_mask, cache)
        if ids.is_cuda:
            self._pick(cache, logits)
        else:
            advance_cpu(cache, logits, cache.gen)
        return logits

    def prefill_logits(self, ids, attention_mask, cache):
        """Teacher-forced :meth:`prefill`: fills the cache, samples nothing.  ``[B, vocab]``."""
        return self._prefill(ids, attention_mask, cache)[:, :self.vocab]

    @torch.no_grad()
    def decode_logits(self, cache, ids):
        """Teacher-forced :meth:`decode_step`: appends the GIVEN token ``ids[b]`` at the next
        position of every sequence and returns its logits ``[B, vocab]`` (a new tensor)."""
        cache.lens.add_(1).clamp_(max=cache.Lcap - 1)
        cache.next_ids.copy_(ids.reshape(-1))
        logits = self._replay(cache, False) if cache.lens.is_cuda else self._step(cache, False)
        return logits[:, :self.vocab].clone()

    def _generate_lookup(self, *args):
        raise ValueError(f"generate: prompt_lookup_num_tokens > 0 (speculative decoding) is not implemented for "
                         f"{type(self).__name__}")

    @torch.no_grad()
    def generate(self, ids, attention_mask=None, max_new_tokens=32, temperature=0.0, eos_token_id=None, seed=0,
                 top_k=0, top_p=1.0, repetition_penalty=1.0, prompt_lookup_num_tokens=0, max_matching_ngram_size=2):
        """Continue each right-padded prompt by ``max_new_tokens`` tokens: greedy at
        ``temperature == 0``, else Gumbel-max sampling reproducible from ``seed``.  HF's processor
        chain runs on the device ahead of the pick: ``repetition_penalty`` (1: off) over the prompt
        and everything generated, ``top_k`` (0: off; ties at the k-th value stay) and ``top_p`` (1:
        off; whole classes of equal value).  A sequence that
        draws ``eos_token_id`` keeps emitting it.  Returns int64 ``[B, Lprompt_max +
        max_new_tokens]``: row b is its prompt, its new tokens, then ``eos_token_id`` (0 without
        one) up to the common width.

        ``prompt_lookup_num_tokens = k >= 1`` turns on prompt-lookup speculative decoding (HF's
        option of that name) on the models that implement it (GPT-2; the others raise
        ``ValueError``): an n-gram lookup in each sequence's own history (n-grams of up to
        ``max_matching_ngram_size`` tokens) drafts ``k`` tokens and one round of ``k + 1`` rows per
        sequence verifies them (``draft_lookup``, ``verify_step``), so a round emits 1 to
        ``k + 1`` tokens per sequence.  The result is, element for element, what the same call
        returns with ``k = 0``, greedy or sampled; ``last_generate_stats`` then holds ``rounds``,
        ``accepted`` (draft tokens accepted) and ``tokens`` (tokens the rounds committed), both
        summed over the sequences.  Limits: ``B <= 4``, ``B * (k + 1) <= 16``, no ``top_k`` /
        ``top_p`` / ``repetition_penalty``."""
        from .flat import shadow_of
        table, max_pos = self._decode_table, self._decode_max_pos
        B, L = ids.shape
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if B > 16:
            raise ValueError(f"generate: batch {B} > 16 (the decode GEMMs take at most 16 rows)")
        plen = torch.full((B,), L, dtype=torch.int64) if attention_mask is None else attention_mask.long().sum(1).cpu()
        if int(plen.max()) + max_new_tokens > max_pos:
            raise ValueError(f"generate: prompt {int(plen.max())} + {max_new_tokens} new tokens exceeds max_pos "
                             f"{max_pos}")
        k = draft_count(prompt_lookup_num_tokens, max_matching_ngram_size)
        if k:
            return self._generate_lookup(ids, attention_mask, plen, max_new_tokens, temperature, eos_token_id, seed,
                                         top_k, top_p, repetition_penalty, k, int(max_matching_ngram_size))
        Lcap = -(-(L + max_new_tokens) // 64) * 64
        sample = temperature > 0
        caches = self.__dict__.setdefault("_kml_decode_caches", {})
        # the captured step holds the addresses of the bf16 shadows: a model moved or flattened
        # again gets a new cache (and capture)
        stamp = shadow_of(table).data_ptr() if ids.is_cuda else 0
        key = (B, Lcap, sample, ids.device, table.dtype, stamp)
        cache = caches.get(key)
        if cache is None:
            cache = caches[key] = self.new_cache(B, Lcap, ids.device)
        cache.reset(seed=seed, temperature=temperature, eos_token_id=eos_token_id, top_k=top_k, top_p=top_p,
                    repetition_penalty=repetition_penalty)
        if ids.is_cuda:
            for p in self.parameters():   # bf16 shadows current before the captured step reads them
                shadow_of(p)
        self.prefill(ids, attention_mask, cache)
        for _ in range(max_new_tokens - 1):
            self.decode_step(cache)
        W = L + max_new_tokens
        out = cache.tokens[:, :W].clone()
        fill = 0 if eos_token_id is None else int(eos_token_id)
        end = (plen + max_new_tokens).to(out.device)
        out.masked_fill_(torch.arange(W, device=out.device)[None] >= end[:, None], fill)
        return out
