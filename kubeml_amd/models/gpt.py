"""GPT-2 decoder-only language model (HuggingFace ``GPT2LMHeadModel`` architecture and
``state_dict`` names: ``transformer.wte.weight``, ``transformer.h.{i}.attn.c_attn.weight``, ...,
``lm_head.weight`` tied to the token table) on the MI355X layers:

* token-major bf16 activations ``[B*L, hidden]``; fused QKV projection, GELU-epilogue FFN1,
  FFN2's dgrad carrying FFN1's GELU backward, tied-embedding decoder GEMM — all gemm.hip, as in
  models/bert.py;
* causal flash attention (csrc/kernels/attention.hip, ``CAUSAL``): the key tiles above the
  diagonal are never computed; attention-probability dropout inside the kernels;
* the pre-LN residual stream is a chain of :meth:`LayerNorm.add_norm` — each block's ``ln_2``,
  the next block's ``ln_1`` and ``ln_f`` take ``(branch output, stream)`` and return
  ``(normalised, new stream)``: the residual sums, the hidden dropout and the gradient sums
  run inside the LayerNorm kernels, no add kernel forward or backward;
* next-token labels from one launch (``kml_lm_shift_labels``); vocab-padded logits go to the
  cross-entropy kernels in place;
* inference: ``generate`` / ``prefill`` / ``decode_step`` on a :class:`~kubeml_amd.nn.KVCache` —
  the prompt through the kernels above, then one captured step per token on the decode kernels
  (csrc/kernels/decode.hip: cache append, one-query attention, skinny GEMMs, sampling);
  ``generate(prompt_lookup_num_tokens=k)`` / ``draft_lookup`` / ``verify_step``: speculative
  decoding, k n-gram drafts verified per captured round of k + 1 rows, same tokens as without.

FFN activation: ``activation="gelu"`` (the erf GELU, HF ``activation_function="gelu"``; the
default) or ``activation="gelu_tanh"`` (the tanh approximation, HF ``gelu_new`` /
``gelu_pytorch_tanh`` — what every released GPT-2 checkpoint was trained with).  Both run in the
GEMM epilogues forward and backward and in the skinny decode GEMM.  For released weights build the
model from the checkpoint's ``config.json`` with :meth:`GPT2LMHeadModel.from_hf_config`, which
picks the activation, then ``load_state_dict``.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as tnn
from torch.autograd import Function

from ..nn.decode import KVCache, filter_logits, lookup_draft_reference
from ..nn.flat import grad_storage_of, shadow_of
from ..nn.modules import Linear, cross_entropy
from ..nn.transformer import Dropout, LayerNorm, RNGState, SelfAttention, _bf, gather_rows


class _Emb2Fn(Function):
    """Token + position embedding: one gather launch; backward = the word / position kernels."""

    @staticmethod
    def forward(ctx, ids, wte, wpe, L):
        from ..ops import transformer as T
        ctx.save = (ids, wte, wpe)
        ctx.L = L
        return T.embed2_fwd(ids, shadow_of(wte), shadow_of(wpe), L)

    @staticmethod
    def backward(ctx, dsum):
        from ..ops import transformer as T
        ids, wte, wpe = ctx.save
        T.embed_bwd(ids, None, _bf(dsum).contiguous(), grad_storage_of(wte), grad_storage_of(wpe), None, ctx.L)
        ctx.save = None
        return None, None, None, None


class GPT2Attention(SelfAttention):
    """Causal self-attention with HF GPT-2 names: the fused ``qkv`` Linear is ``c_attn`` and the
    output projection ``c_proj``.  HF keeps both as ``Conv1D`` ([in, out]), so the save / load
    hooks transpose the weights (they replace SelfAttention's BERT renaming)."""

    _NAMES = (("qkv", "c_attn"), ("out", "c_proj"))

    def __init__(self, hidden, heads, attn_dropout, rng):
        super().__init__(hidden, heads, attn_dropout=attn_dropout, rng=rng, causal=True)
        self._state_dict_hooks.clear()
        self._load_state_dict_pre_hooks.clear()
        self._register_state_dict_hook(GPT2Attention._sd_hook)
        self._register_load_state_dict_pre_hook(GPT2Attention._load_hook, with_module=True)

    @staticmethod
    def _sd_hook(mod, sd, prefix, local_metadata):
        for ours, hf in GPT2Attention._NAMES:
            sd[prefix + hf + ".weight"] = sd.pop(prefix + ours + ".weight").t()
            sd[prefix + hf + ".bias"] = sd.pop(prefix + ours + ".bias")
        return sd

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        for ours, hf in GPT2Attention._NAMES:
            if prefix + hf + ".weight" in sd:
                sd[prefix + ours + ".weight"] = sd.pop(prefix + hf + ".weight").t()
            if prefix + hf + ".bias" in sd:
                sd[prefix + ours + ".bias"] = sd.pop(prefix + hf + ".bias")


ACTIVATIONS = ("gelu", "gelu_tanh")   # Linear's act names: erf GELU, tanh-approximated GELU


class GPT2MLP(tnn.Module):
    def __init__(self, hidden, inter, activation="gelu"):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: one of {ACTIVATIONS}")
        self.activation = activation
        self.c_fc = Linear(hidden, inter)
        self.c_proj = Linear(inter, hidden)
        # c_proj is the only consumer of c_fc's GELU output: its dgrad applies the GELU backward
        # and sums c_fc's bias gradient in its epilogue (nn/modules.py)
        object.__setattr__(self.c_proj, "_kml_gelu_producer", self.c_fc)
        self._register_state_dict_hook(GPT2MLP._sd_hook)
        self._register_load_state_dict_pre_hook(GPT2MLP._load_hook, with_module=True)

    @staticmethod
    def _sd_hook(mod, sd, prefix, local_metadata):   # HF Conv1D layout: [in, out]
        for n in ("c_fc", "c_proj"):
            sd[prefix + n + ".weight"] = sd[prefix + n + ".weight"].t()
        return sd

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        for n in ("c_fc", "c_proj"):
            if prefix + n + ".weight" in sd:
                sd[prefix + n + ".weight"] = sd[prefix + n + ".weight"].t()

    def forward(self, x):
        return self.c_proj(self.c_fc(x, act=self.activation))   # the GELU in the GEMM epilogue


class GPT2Block(tnn.Module):
    """``h += drop(attn(ln_1(h)))``, ``h += drop(mlp(ln_2(h)))``.  The block receives
    ``ln_1(h)`` already computed (by the previous block's closing add-and-normalise) and
    returns its MLP branch and the stream; the caller's next ``add_norm`` closes it."""

    def __init__(self, hidden, heads, inter, eps, dropout, rng, activation="gelu"):
        super().__init__()
        self.ln_1 = LayerNorm(hidden, eps=eps)
        self.attn = GPT2Attention(hidden, heads, dropout, rng)
        self.ln_2 = LayerNorm(hidden, eps=eps)
        self.mlp = GPT2MLP(hidden, inter, activation)
        self.drop1 = Dropout(dropout, rng)   # resid_pdrop after the attention projection
        self.drop2 = Dropout(dropout, rng)   # ... and after the MLP
        # ln_2's branch input is the attention projection's output alone: that Linear's bias
        # gradient is summed inside the LayerNorm backward (nn/transformer.py)
        object.__setattr__(self.ln_2, "_kml_in_linear", self.attn.out)

    def forward(self, x, s, B: int, L: int, bias=None):
        """x = ln_1(s).  Returns (MLP branch output, stream after the attention branch)."""
        a = self.attn(x, B, L, bias)
        x2, s2 = self.ln_2.add_norm(a, residual=s, dropout=self.drop1)
        return self.mlp(x2), s2


class GPT2Model(tnn.Module):
    def __init__(self, vocab, hidden, layers, heads, inter, max_pos, eps, dropout, rng, activation="gelu"):
        super().__init__()
        self.wte = tnn.Embedding(vocab, hidden)
        self.wpe = tnn.Embedding(max_pos, hidden)
        self.drop = Dropout(dropout, rng)   # embd_pdrop
        self.h = tnn.ModuleList([GPT2Block(hidden, heads, inter, eps, dropout, rng, activation)
                                 for _ in range(layers)])
        self.ln_f = LayerNorm(hidden, eps=eps)
        self.max_pos = max_pos
        # storage rows padded to 8 so the tied lm_head Linear can share the token table
        vp = -(-vocab // 8) * 8
        self.wte.weight._kml_storage_shape = (vp, hidden)
        self.wte.weight._kml_view = lambda st: st[:vocab, :hidden]
        # the LayerNorm closing block i (block i+1's ln_1, or ln_f) reads block i's c_proj output
        closers = [blk.ln_1 for blk in self.h[1:]] + [self.ln_f]
        for blk, ln in zip(self.h, closers):
            object.__setattr__(ln, "_kml_in_linear", blk.mlp.c_proj)

    def forward(self, ids, attention_mask=None):
        B, L = ids.shape
        if L > self.max_pos:
            raise ValueError(f"sequence length {L} exceeds max_pos {self.max_pos}")
        bias = None
        if attention_mask is not None:
            bias = ((1.0 - attention_mask.float()) * -10000.0).reshape(B, L).contiguous()
        if not ids.is_cuda:
            pos = torch.arange(L, device=ids.device)
            e = (self.wte(ids) + self.wpe(pos)[None]).reshape(B * L, -1)
            if bias is not None:
                bias = bias.to(e.dtype)
        else:
            e = _Emb2Fn.apply(ids.reshape(-1).contiguous(), self.wte.weight, self.wpe.weight, L)
        # embedding dropout inside block 0's ln_1 launch; from here on (x, s) = (LN(s), stream)
        x, s = self.h[0].ln_1.add_norm(e, residual=None, dropout=self.drop)
        closers = [blk.ln_1 for blk in self.h[1:]] + [self.ln_f]
        for blk, ln in zip(self.h, closers):
            m, s = blk(x, s, B, L, bias)
            x, s = ln.add_norm(m, residual=s, dropout=blk.drop2)
        return x


class GPT2LMHeadModel(tnn.Module):
    def __init__(self, vocab=50257, hidden=768, layers=12, heads=12, inter=3072, max_pos=1024, eps=1e-5,
                 dropout=0.1, seed: int = 0, activation: str = "gelu"):
        super().__init__()
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: \"gelu\" (erf) or \"gelu_tanh\" (the tanh approximation "
                             "that HF calls gelu_new; use activation=\"gelu_tanh\" for released GPT-2 weights, or "
                             "GPT2LMHeadModel.from_hf_config, which maps HF's activation_function)")
        self.activation = activation
        self.rng = RNGState(seed)
        self.vocab = vocab
        self.transformer = GPT2Model(vocab, hidden, layers, heads, inter, max_pos, eps, dropout, self.rng,
                                     activation)
        self.lm_head = Linear(hidden, vocab, bias=False)
        # weight tying (HF tie_word_embeddings): lm_head.weight IS the token table
        self.lm_head.weight = self.transformer.wte.weight
        self._init_weights(layers)
        self._register_load_state_dict_pre_hook(GPT2LMHeadModel._load_hook, with_module=True)

    _HF_ACT = {"gelu_new": "gelu_tanh", "gelu_pytorch_tanh": "gelu_tanh", "gelu": "gelu"}

    @classmethod
    def from_hf_config(cls, config, **overrides):
        """Build the model a HuggingFace GPT-2 ``config`` describes: a ``GPT2Config``, a dict, or the
        path of a ``config.json``.  ``activation_function`` picks the FFN activation (``gelu_new``
        and ``gelu_pytorch_tanh``: "gelu_tanh"; ``gelu``: "gelu"), ``n_inner`` defaults to
        ``4 n_embd``.  Raises ``ValueError`` for what this model does not implement: another
        activation, dropout rates that differ (there is one), ``scale_attn_by_inverse_layer_idx``,
        ``reorder_and_upcast_attn``.  ``overrides`` replace constructor arguments (``seed=...``).
        Follow with ``load_state_dict(hf_model.state_dict())`` for the weights."""
        if isinstance(config, (str, os.PathLike)):
            with open(config) as f:
                config = json.load(f)
        elif hasattr(config, "to_dict"):
            config = config.to_dict()
        if not isinstance(config, dict):
            raise TypeError(f"from_hf_config: a GPT2Config, a dict or a path, got {type(config).__name__}")
        c = config
        act = c.get("activation_function", "gelu_new")
        if act not in cls._HF_ACT:
            raise ValueError(f"from_hf_config: activation_function {act!r} (supported: {sorted(cls._HF_ACT)})")
        drop = c.get("resid_pdrop", 0.1)
        for k in ("embd_pdrop", "attn_pdrop"):
            if c.get(k, 0.1) != drop:
                raise ValueError(f"from_hf_config: {k} = {c.get(k, 0.1)} differs from resid_pdrop = {drop}; "
                                 "the model has one dropout rate")
        for k in ("scale_attn_by_inverse_layer_idx", "reorder_and_upcast_attn"):
            if c.get(k, False):
                raise ValueError(f"from_hf_config: {k} is not implemented")
        hidden = c.get("n_embd", 768)
        inter = c.get("n_inner")
        kw = dict(vocab=c.get("vocab_size", 50257), hidden=hidden, layers=c.get("n_layer", 12),
                  heads=c.get("n_head", 12), inter=4 * hidden if inter is None else inter,
                  max_pos=c.get("n_positions", 1024), eps=c.get("layer_norm_epsilon", 1e-5), dropout=drop,
                  activation=cls._HF_ACT[act])
        kw.update(overrides)
        return cls(**kw)

    def _init_weights(self, layers):
        for m in self.modules():
            if isinstance(m, (Linear, tnn.Embedding)):
                if m is self.lm_head:
                    continue
                tnn.init.normal_(m.weight, 0.0, 0.02)
                if isinstance(m, Linear) and m.bias is not None:
                    tnn.init.zeros_(m.bias)
            elif isinstance(m, LayerNorm):
                tnn.init.ones_(m.weight)
                tnn.init.zeros_(m.bias)
        for blk in self.transformer.h:   # GPT-2: residual projections scaled by 1/sqrt(2 layers)
            for lin in (blk.attn.out, blk.mlp.c_proj):
                tnn.init.normal_(lin.weight, 0.0, 0.02 / (2 * layers) ** 0.5)

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        if prefix + "lm_head.weight" not in sd and prefix + "transformer.wte.weight" in sd:
            sd[prefix + "lm_head.weight"] = sd[prefix + "transformer.wte.weight"]
        for k in [k for k in sd if k.startswith(prefix) and k.endswith((".attn.bias", ".attn.masked_bias"))]:
            sd.pop(k)   # HF's causal-mask buffers (older checkpoints store them)

    def forward(self, ids, attention_mask=None, labels=None, return_correct=False):
        """ids [B, L]; labels [B, L] (may be ``ids`` itself): position t is scored against
        labels[:, t + 1], the last position of every sequence is ignored.  Returns logits
        ``[B*L, vocab]``, or the mean loss (and the correct count) when labels are given."""
        if self.training and ids.is_cuda:
            self.rng.advance(ids.device)
        z = self.transformer(ids, attention_mask)
        if labels is None:
            return self.lm_head(z)
        if ids.is_cuda:
            from ..ops import transformer as T
            tgt = T.lm_shift_labels(labels, -100)   # one launch: no stock indexing kernels in the step
        else:
            tgt = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], 1)
        # vocab-padded logits used in place (no slice copy / gradient re-pad of [T, 50264])
        logits = self.lm_head(z, keep_pad=True)
        return cross_entropy(logits, tgt.reshape(-1), ignore_index=-100, return_correct=return_correct,
                             classes=self.vocab)

    # ------------------------------------------------------------------ KV-cache decoding
    # Inference only (no autograd, no dropout whatever the module's mode).  GPU: the prompt runs
    # the training kernels once, every later token one captured step of the decode kernels
    # (csrc/kernels/decode.hip).  CPU: the same steps in stock torch on a cache of plain tensors.

    def _closers(self):
        tr = self.transformer
        return list(zip(tr.h, [blk.ln_1 for blk in tr.h[1:]] + [tr.ln_f]))

    def new_cache(self, B, Lcap, device=None):
        tr = self.transformer
        p = tr.wte.weight
        return KVCache(len(tr.h), B, tr.h[0].attn.heads, Lcap, device or p.device, dtype=p.dtype)

    @torch.no_grad()
    def _prefill(self, ids, attention_mask, cache):
        """Causal forward over the right-padded prompt; appends every layer's K / V; leaves
        ``lens[b] = prompt_len[b] - 1``; returns the logits of each sequence's last prompt token."""
        tr = self.transformer
        B, L = ids.shape
        if B != cache.B or L > cache.Lcap or L > tr.max_pos:
            raise ValueError(f"prompt [{B}, {L}] does not fit the cache ({cache.B} x {cache.Lcap}) / max_pos")
        if attention_mask is None:
            plen = torch.full((B,), L, dtype=torch.int64, device=ids.device)
            bias = None
        else:
            plen = attention_mask.long().sum(1)
            pos = torch.arange(L, device=ids.device)[None]
            if int(plen.min()) < 1 or not bool(((pos < plen[:, None]) == attention_mask.bool()).all()):
                raise ValueError("prefill: the prompt must be right-padded with at least one token per sequence")
            bias = ((1.0 - attention_mask.float()) * -10000.0).reshape(B, L).contiguous()
        gpu = ids.is_cuda
        H = tr.h[0].attn.heads
        if gpu:
            from ..nn.transformer import _AttnFn
            from ..ops import decode as D
            from ..ops import transformer as T
            e = T.embed2_fwd(ids.reshape(-1).contiguous(), shadow_of(tr.wte.weight), shadow_of(tr.wpe.weight), L)
        else:
            from ..nn.transformer import attention_reference
            e = (tr.wte(ids) + tr.wpe(torch.arange(L))[None]).reshape(B * L, -1)
            if bias is not None:
                bias = bias.to(e.dtype)
        x, s = tr.h[0].ln_1.add_norm(e)
        for i, (blk, ln) in enumerate(self._closers()):
            qkv = blk.attn.qkv(x).contiguous()
            if gpu:
                D.kv_append(qkv, cache.k[i], cache.v[i], L)
                ctx = _AttnFn.apply(qkv, B, H, L, bias, None, True)
            else:
                cache.append_cpu(i, qkv, L, decode=False)
                ctx = attention_reference(qkv, B, H, L, bias, causal=True)
            x2, s = blk.ln_2.add_norm(blk.attn.out(ctx), residual=s)
            x, s = ln.add_norm(blk.mlp(x2), residual=s)
        rows = torch.arange(B, device=ids.device) * L + plen - 1
        z = gather_rows(x, rows)
        cache.lens.copy_((plen - 1).to(torch.int32))
        cache.tokens.zero_()
        cache.tokens[:, :L] = ids * (torch.arange(L, device=ids.device)[None] < plen[:, None])
        cache.finished.zero_()
        return self.lm_head(z, keep_pad=True)

    @torch.no_grad()
    def _step(self, cache, advance):
        """One decode step from ``cache.next_ids`` at position ``lens[b]``: returns the logits
        ``[B, vocab (padded to 8 on the GPU)]``; ``advance`` also picks the next token."""
        tr = self.transformer
        if not cache.lens.is_cuda:
            e = tr.wte(cache.next_ids) + tr.wpe(cache.lens.long().clamp(max=tr.max_pos - 1))
            x, s = tr.h[0].ln_1.add_norm(e)
            for i, (blk, ln) in enumerate(self._closers()):
                qkv = blk.attn.qkv(x)
                cache.append_cpu(i, qkv, 1, decode=True)
                x2, s = blk.ln_2.add_norm(blk.attn.out(cache.attend_cpu(i, qkv)), residual=s)
                x, s = ln.add_norm(blk.mlp(x2), residual=s)
            logits = self.lm_head(x)
            if advance:
                _advance_cpu(cache, logits, cache.gen)
            return logits
        from ..ops import decode as D
        e = D.embed2_at(cache.next_ids, cache.lens, shadow_of(tr.wte.weight), shadow_of(tr.wpe.weight))
        x, s = tr.h[0].ln_1.add_norm(e)
        for i, (blk, ln) in enumerate(self._closers()):
            qkv = blk.attn.qkv.forward_small(x)
            D.kv_append(qkv, cache.k[i], cache.v[i], 1, lens=cache.lens)
            ctx = D.attn_decode(qkv, cache.k[i], cache.v[i], cache.lens, ws=cache.ws)
            x2, s = blk.ln_2.add_norm(blk.attn.out.forward_small(ctx), residual=s)
            m = blk.mlp.c_proj.forward_small(blk.mlp.c_fc.forward_small(x2, act=self.activation))
            x, s = ln.add_norm(m, residual=s)
        logits = self.lm_head.forward_small(x, keep_pad=True)
        if advance:
            self._pick(cache, logits)
        return logits

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

    def _replay(self, cache, advance):
        """The GPU step as one captured graph per (cache, advance, sampling, filtered); captured
        on first use after an eager warm-up whose effect on the decode state is rolled back.  The
        filter parameters live in device memory: other values replay the same graph."""
        key = (bool(advance), bool(cache.sample), bool(cache.filtered))
        ent = cache._graphs.get(key)
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
            _advance_cpu(cache, logits, cache.gen)
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
        option of that name): an n-gram lookup in each sequence's own history (n-grams of up to
        ``max_matching_ngram_size`` tokens) drafts ``k`` tokens and one round of ``k + 1`` rows per
        sequence verifies them (:meth:`draft_lookup`, :meth:`verify_step`), so a round emits 1 to
        ``k + 1`` tokens per sequence.  The result is, element for element, what the same call
        returns with ``k = 0``, greedy or sampled; ``last_generate_stats`` then holds ``rounds``,
        ``accepted`` (draft tokens accepted) and ``tokens`` (tokens the rounds committed), both
        summed over the sequences.  Limits: ``B <= 4``, ``B * (k + 1) <= 16``, no ``top_k`` /
        ``top_p`` / ``repetition_penalty``."""
        tr = self.transformer
        B, L = ids.shape
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if B > 16:
            raise ValueError(f"generate: batch {B} > 16 (the decode GEMMs take at most 16 rows)")
        plen = torch.full((B,), L, dtype=torch.int64) if attention_mask is None else attention_mask.long().sum(1).cpu()
        if int(plen.max()) + max_new_tokens > tr.max_pos:
            raise ValueError(f"generate: prompt {int(plen.max())} + {max_new_tokens} new tokens exceeds max_pos "
                             f"{tr.max_pos}")
        k = _draft_count(prompt_lookup_num_tokens, max_matching_ngram_size)
        if k:
            return self._generate_lookup(ids, attention_mask, plen, max_new_tokens, temperature, eos_token_id, seed,
                                         top_k, top_p, repetition_penalty, k, int(max_matching_ngram_size))
        Lcap = -(-(L + max_new_tokens) // 64) * 64
        sample = temperature > 0
        caches = self.__dict__.setdefault("_kml_decode_caches", {})
        # the captured step holds the addresses of the bf16 shadows: a model moved or flattened
        # again gets a new cache (and capture)
        stamp = shadow_of(tr.wte.weight).data_ptr() if ids.is_cuda else 0
        key = (B, Lcap, sample, ids.device, tr.wte.weight.dtype, stamp)
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

    # ------------------------------------------------------------------ speculative decoding
    # A verify round feeds q = k + 1 rows per sequence — next_ids[b] and k draft tokens at positions
    # lens[b] .. lens[b] + k — and commits the longest prefix the model itself would have picked.
    # Row j is computed exactly as the plain step at length lens[b] + j computes it (skinny GEMMs
    # whose rows do not depend on the row count, attention with k_attn_decode's order of sums, the
    # noise step of that position), so the tokens are plain decoding's, bit for bit.  K / V rows of
    # rejected drafts stay in the cache: the next round overwrites them before a query reads them.

    def draft_lookup(self, cache, k, max_ngram=2):
        """Prompt-lookup drafts for the next verify round: int64 ``[B, k]`` on the cache's device,
        an n-gram lookup in ``cache.tokens[b, 0 .. lens[b]]`` (``nn.lookup_draft_reference`` is the
        rule).  With ``k == cache.draft_tokens`` the result is the cache's own draft buffer."""
        own = cache.draft if cache.draft is not None and k == cache.draft_tokens else None
        if cache.lens.is_cuda:
            from ..ops import decode as D
            return D.draft_lookup(cache.tokens, cache.lens, k, max_ngram, out=own)
        d = lookup_draft_reference(cache.tokens, cache.lens, k, max_ngram)
        return d if own is None else own.copy_(d)

    @torch.no_grad()
    def verify_step(self, cache, draft_ids):
        """One verify round on a cache prepared with ``reset(draft_tokens=k)`` and prefilled:
        feeds ``next_ids[b], draft_ids[b, 0], ..., draft_ids[b, k-1]`` at positions ``lens[b] ..
        lens[b] + k``, then accepts and commits on the device (``ops.decode.verify_pick`` has the
        rule): ``tokens``, ``next_ids``, ``lens``, ``finished`` and ``cache.stats`` advance.  Any
        drafter may supply ``draft_ids`` (int64 ``[B, k]``).  Returns the logits ``[B * (k + 1),
        vocab (padded to 8 on the GPU)]``, row ``b * (k + 1) + j`` for position ``lens[b] + j``."""
        k = cache.draft_tokens
        if k < 1:
            raise ValueError("verify_step: the cache was not reset with draft_tokens >= 1")
        if draft_ids.dtype != torch.int64 or tuple(draft_ids.shape) != (cache.B, k):
            raise ValueError(f"verify_step: draft_ids must be int64 [{cache.B}, {k}], got {draft_ids.dtype} "
                             f"{tuple(draft_ids.shape)}")
        if draft_ids.data_ptr() != cache.draft.data_ptr():
            cache.draft.copy_(draft_ids)
        if cache.lens.is_cuda:
            return self._replay_round(cache)
        return self._round_cpu(cache)

    def _round(self, cache):
        """The launches of a GPU verify round, :meth:`_step` on ``B * q`` rows."""
        from ..ops import decode as D
        tr = self.transformer
        q = cache.draft_tokens + 1
        e = D.embed2_multi(cache.next_ids, cache.draft, cache.lens, shadow_of(tr.wte.weight), shadow_of(tr.wpe.weight))
        x, s = tr.h[0].ln_1.add_norm(e)
        for i, (blk, ln) in enumerate(self._closers()):
            qkv = blk.attn.qkv.forward_small(x, skinny=True)
            # append BEFORE attention: query j reads the rows lens[b] .. lens[b] + j this round wrote
            # (and nothing past them: what a rejected draft of an earlier round left there is dead)
            D.kv_append(qkv, cache.k[i], cache.v[i], q, lens=cache.lens)
            ctx = D.attn_decode_multi(qkv, cache.k[i], cache.v[i], cache.lens, q, ws=cache.ws_multi)
            x2, s = blk.ln_2.add_norm(blk.attn.out.forward_small(ctx, skinny=True), residual=s)
            m = blk.mlp.c_proj.forward_small(blk.mlp.c_fc.forward_small(x2, act=self.activation, skinny=True), skinny=True)
            x, s = ln.add_norm(m, residual=s)
        # skinny at every row count: above 4 rows forward_small would send the tied decoder elsewhere
        logits = self.lm_head.forward_small(x, keep_pad=True, skinny=True)
        D.verify_pick(logits, self.vocab, cache.ctl, cache.temp, cache.start, cache.limit, cache.draft, cache.pick,
                      cache.next_ids, cache.tokens, cache.lens, cache.finished, cache.stats, sample=cache.sample)
        return logits

    def _replay_round(self, cache):
        """The GPU verify round as one captured graph per (cache, sampling, q), as :meth:`_replay`
        keeps the plain step: drafts, start, limit, seed, temperature and eos are device memory."""
        key = ("verify", bool(cache.sample), cache.draft_tokens + 1)
        ent = cache._graphs.get(key)
        if ent is None:
            from ..engine.step import capture_graph
            state = [cache.lens, cache.tokens, cache.next_ids, cache.finished, cache.stats]
            keep = [t.clone() for t in state]
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._round(cache)   # the replay re-appends the same K / V rows: idempotent
            cur.wait_stream(side)
            for t, kept in zip(state, keep):
                t.copy_(kept)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with capture_graph(g, capture_error_mode="thread_local"):
                logits = self._round(cache)
            ent = cache._graphs[key] = (g, logits)
        ent[0].replay()
        return ent[1]

    def _round_cpu(self, cache):
        """The CPU twin of a verify round.  The rows of a sequence go through :meth:`_step` one
        position at a time, with the shapes of plain decoding, so that row j has the bits of the
        plain step at that position whatever the BLAS does with another row count."""
        B, q = cache.B, cache.draft_tokens + 1
        feed = torch.cat([cache.next_ids[:, None], cache.draft], 1)
        base, nxt = cache.lens.clone(), cache.next_ids.clone()
        rows = []
        for j in range(q):
            cache.lens.copy_(base + j)
            cache.next_ids.copy_(feed[:, j])
            rows.append(self._step(cache, False))   # appends at lens[b] + j, then attends up to it
        cache.lens.copy_(base)
        cache.next_ids.copy_(nxt)
        logits = torch.stack(rows, 1)   # [B, q, vocab]
        if cache.sample:
            T = float(cache.temp[0])
            pick = torch.empty((B, q), dtype=torch.int64)
            for b in range(B):
                for j in range(q):
                    # the draw plain decoding consumes for this sequence's new token of that index
                    u = cache.uniforms_cpu(int(base[b]) + j - int(cache.start[b]), logits[:, 0].shape)[b]
                    pick[b, j] = (logits[b, j].double() / T - torch.log(-torch.log(u))).argmax(-1)
        else:
            pick = logits.argmax(-1)
        cache.pick.copy_(pick.reshape(-1).to(torch.int32))
        _verify_commit_cpu(cache)
        cache.forget_uniforms_cpu(int((cache.lens - cache.start).min()))
        return logits.reshape(B * q, -1)

    def _generate_lookup(self, ids, attention_mask, plen, max_new_tokens, temperature, eos_token_id, seed, top_k,
                         top_p, repetition_penalty, k, max_ngram):
        tr = self.transformer
        B, L = ids.shape
        q = k + 1
        if B > 4:
            raise ValueError(f"generate: prompt lookup takes batches up to 4, got {B} (above that plain decoding "
                             "sends the tied decoder to another GEMM and identity with it cannot be promised)")
        if B * q > 16:
            raise ValueError(f"generate: {B} sequences x ({k} draft tokens + 1) = {B * q} rows; a verify round "
                             "takes at most 16")
        if top_k != 0 or top_p != 1.0 or repetition_penalty != 1.0:
            raise ValueError("generate: prompt lookup does not run behind top_k, top_p or repetition_penalty "
                             "(the filtered sampler takes one row per sequence)")
        Lcap = -(-(L + max_new_tokens + q) // 64) * 64
        sample = temperature > 0
        caches = self.__dict__.setdefault("_kml_decode_caches", {})
        stamp = shadow_of(tr.wte.weight).data_ptr() if ids.is_cuda else 0
        key = (B, Lcap, sample, ids.device, tr.wte.weight.dtype, stamp, q)
        cache = caches.get(key)
        if cache is None:
            cache = caches[key] = self.new_cache(B, Lcap, ids.device)
        cache.reset(seed=seed, temperature=temperature, eos_token_id=eos_token_id, start=plen - 1,
                    limit=plen - 1 + max_new_tokens, draft_tokens=k)
        if ids.is_cuda:
            for p in self.parameters():
                shadow_of(p)
        self.prefill(ids, attention_mask, cache)
        # How the host learns that every sequence is at its limit: the commit leaves max over b of
        # limit[b] - lens[b] in cache.stats[2].  A round moves a sequence by at most q, so
        # ceil(remaining / q) rounds are needed whatever is accepted; only then is stats read
        # again (16 bytes) — at most one read per round, far fewer when little is accepted.
        rounds, remaining, st = 0, max_new_tokens - 1, [0, 0, 0, 0]
        while remaining > 0:
            n = -(-remaining // q)
            for _ in range(n):
                self.verify_step(cache, self.draft_lookup(cache, k, max_ngram))
            rounds += n
            st = cache.stats.tolist()
            remaining = st[2]
        self.last_generate_stats = {"rounds": rounds, "accepted": st[0], "tokens": st[1]}
        W = L + max_new_tokens
        out = cache.tokens[:, :W].clone()
        fill = 0 if eos_token_id is None else int(eos_token_id)
        end = (plen + max_new_tokens).to(out.device)
        out.masked_fill_(torch.arange(W, device=out.device)[None] >= end[:, None], fill)
        return out


def _draft_count(k, max_ngram):
    """``prompt_lookup_num_tokens`` as an int (None: 0), both options checked."""
    k = 0 if k is None else k
    if isinstance(k, bool) or not isinstance(k, (int, float)) or int(k) != k or k < 0:
        raise ValueError(f"prompt_lookup_num_tokens must be an integer >= 0, got {k!r}")
    if isinstance(max_ngram, bool) or not isinstance(max_ngram, (int, float)) or int(max_ngram) != max_ngram \
            or max_ngram < 1:
        raise ValueError(f"max_matching_ngram_size must be an integer >= 1, got {max_ngram!r}")
    return int(k)


def _verify_commit_cpu(cache):
    """Stock-torch twin of the commit of ``kml_verify_pick`` on a CPU cache whose ``pick`` holds
    the rows' choices: per sequence, pick j lands at ``tokens[b, lens[b] + j + 1]`` while that index
    is ``<= limit[b]`` and every earlier draft equalled its pick without being eos; a sequence
    finished before the round commits eos in every slot; one at its limit is frozen."""
    eos = int(cache.ctl[2])
    B, q, Lcap = cache.B, cache.draft_tokens + 1, cache.Lcap
    pick, draft = cache.pick.reshape(B, q).tolist(), cache.draft.tolist()
    acc = com = rem = 0
    for b in range(B):
        p, lim = int(cache.lens[b]), int(cache.limit[b])
        m = 0
        if p < lim:
            fin = int(cache.finished[b])
            was = eos >= 0 and fin != 0
            last = 0
            for j in range(q):
                at = p + j + 1
                if at > lim:
                    break
                tok = eos if was else pick[b][j]
                if 0 <= at < Lcap:
                    cache.tokens[b, at] = tok
                last, m = tok, j + 1
                if was:
                    continue
                if eos >= 0 and tok == eos:
                    fin = 1
                    break
                if j == q - 1 or draft[b][j] != tok:
                    break
            cache.finished[b] = fin
            cache.next_ids[b] = last
            cache.lens[b] = p + m
            com += m
            acc += 0 if was else m - 1
        rem = max(rem, lim - (p + m))
    cache.stats[0] += acc
    cache.stats[1] += com
    cache.stats[2] = rem


def _advance_cpu(cache, logits, gen):
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


def gpt2_small(**kw) -> GPT2LMHeadModel:
    return GPT2LMHeadModel(**kw)


def gpt2_tiny(**kw) -> GPT2LMHeadModel:
    """2-layer, 128-hidden variant for tests."""
    cfg = dict(vocab=1000, hidden=128, layers=2, heads=2, inter=512, max_pos=256)
    cfg.update(kw)
    return GPT2LMHeadModel(**cfg)
