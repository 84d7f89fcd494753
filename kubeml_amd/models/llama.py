"""Llama-style decoder-only language model (HuggingFace ``LlamaForCausalLM`` architecture and
``state_dict`` names: ``model.embed_tokens.weight``, ``model.layers.{i}.self_attn.q_proj.weight``,
..., ``lm_head.weight``) on the MI355X layers, head dim 64 or 128:

* RMSNorm with the pre-norm residual stream carried inside its launches — a chain of
  :meth:`RMSNorm.add_norm`, as ``GPT2Model`` chains ``LayerNorm.add_norm`` (csrc/kernels/llama.hip);
* one fused ``qkv`` projection ``[(H + 2 Hkv) * d, hidden]`` without bias (head dim d = 64 or 128,
  whatever ``hidden / heads`` is), rotary position embedding in place on its output (``kml_rope``
  / ``kml_rope128``), grouped-query causal flash attention (``kml_attn_gqa_fwd / _bwd``, at head dim
  128 ``kml_attn128_fwd / _bwd`` of csrc/kernels/attention_d128.hip: ``Hkv`` K/V heads shared by
  groups of ``H / Hkv`` query heads);
* gated SiLU MLP: one fused ``gate_up`` projection ``[2 I, hidden]``, ``kml_swiglu_fwd / _bwd``,
  ``down_proj``;
* one token table (no position table), optionally tied to ``lm_head``; shifted labels and the
  fused cross entropy as in ``GPT2LMHeadModel``;
* packed rows: ``forward(..., doc_ids=...)`` (``nn.transformer.pack_documents``) keeps attention
  inside each document — the band variants of the attention kernels, ``kml_attn_gqa_band_fwd / _bwd``
  and ``kml_attn128_band_fwd / _bwd``, which also skip the key tiles of earlier documents — and
  scores no token against the next document.  Training and evaluation only: ``generate`` and the
  decode path take one document a row.

``state_dict`` / ``load_state_dict`` split and concatenate the fused ``qkv`` / ``gate_up``
parameters, so HF checkpoints of the family load directly.  Build from a checkpoint's
``config.json`` with :meth:`LlamaForCausalLM.from_hf_config`.

Inference: ``generate`` / ``prefill`` / ``decode_step`` / ``prefill_logits`` / ``decode_logits``
(:class:`~kubeml_amd.nn.decode.DecodeMixin`, GPT-2's) on a :class:`~kubeml_amd.nn.KVCache` of
``Hkv`` heads.  The prompt runs the training kernels once and appends its rotated keys; every later
token is one captured step of eight launches a layer (csrc/kernels/decode.hip): ``qkv`` skinny GEMM,
``kml_kv_append_rope`` (Q rotated in place, K rotated into and V copied to the cache at row
``lens[b]``), ``kml_attn_decode_gqa`` (a chunk of a K/V head loaded once for its group of query
heads), ``o_proj``, add + RMSNorm, ``kml_gemm_skinny_glu`` (gate and up GEMM with the SwiGLU in the
epilogue), ``down_proj``, add + RMSNorm.  Not implemented: speculative decoding
(``prompt_lookup_num_tokens > 0`` raises ``ValueError``), KV-cache decoding at head dim 128 (such
a model trains and evaluates full sequences; ``new_cache`` / ``prefill`` / ``decode_step`` /
``generate`` raise ``NotImplementedError``), ``rope_scaling``, paged caches.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as tnn
from torch.autograd import Function

from ..nn.decode import DecodeMixin, KVCache, advance_cpu
from ..nn.flat import grad_storage_of, shadow_of
from ..nn.modules import Linear, _pad_nograd, cross_entropy
from ..nn.transformer import (RMSNorm, _AttnFn, _bf, attention_reference, doc_key_start, gather_rows, rope,
                              rope_reference, rope_table, swiglu)


class _TokEmbFn(Function):
    """Token embedding: the row-gather kernel; backward = the word-table scatter-add."""

    @staticmethod
    def forward(ctx, ids, wte, L):
        from ..ops import transformer as T
        ctx.save = (ids, wte)
        ctx.L = L
        return T.gather_rows(shadow_of(wte), ids)

    @staticmethod
    def backward(ctx, dsum):
        from ..ops import transformer as T
        ids, wte = ctx.save
        T.embed_bwd(ids, None, _bf(dsum).contiguous(), grad_storage_of(wte), None, None, ctx.L)
        ctx.save = None
        return None, None, None


class LlamaAttention(tnn.Module):
    """Fused ``qkv`` Linear (rows: H query heads | Hkv key heads | Hkv value heads) + RoPE +
    grouped-query causal attention + ``o_proj``; HF's ``q_proj`` / ``k_proj`` / ``v_proj`` through
    the state-dict hooks."""

    def __init__(self, hidden, heads, kv_heads, head_dim=64):
        super().__init__()
        if kv_heads < 1 or heads % kv_heads:
            raise ValueError(f"kv_heads {kv_heads} must divide heads {heads}")
        if head_dim not in (64, 128):
            raise ValueError(f"head_dim {head_dim}: the attention kernels are written for 64 and 128")
        self.hidden, self.heads, self.kv_heads, self.head_dim = hidden, heads, kv_heads, head_dim
        self.qkv = Linear(hidden, (heads + 2 * kv_heads) * head_dim, bias=False)
        self.o_proj = Linear(heads * head_dim, hidden, bias=False)   # whatever hidden / heads is
        self._register_state_dict_hook(LlamaAttention._sd_hook)
        self._register_load_state_dict_pre_hook(LlamaAttention._load_hook, with_module=True)

    @staticmethod
    def _sd_hook(mod, sd, prefix, local_metadata):
        w = sd.pop(prefix + "qkv.weight")
        D, E = mod.heads * mod.head_dim, mod.kv_heads * mod.head_dim
        sd[prefix + "q_proj.weight"], sd[prefix + "k_proj.weight"], sd[prefix + "v_proj.weight"] = \
            w[:D], w[D:D + E], w[D + E:]
        sd[prefix + "o_proj.weight"] = sd.pop(prefix + "o_proj.weight")   # HF order: q, k, v, o
        return sd

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        names = [prefix + n + "_proj.weight" for n in ("q", "k", "v")]
        if all(n in sd for n in names):
            sd[prefix + "qkv.weight"] = torch.cat([sd.pop(n) for n in names], 0)

    def forward(self, x, B, L, table, bias=None, key_start=None):
        """key_start: int32 ``[B, L]`` of packed rows (``doc_key_start``) — a token attends its own
        document only.  RoPE keeps the row position: its scores depend on position differences alone."""
        H, Hkv, d = self.heads, self.kv_heads, self.head_dim
        qkv = rope(self.qkv(x), table, L, H, Hkv, head_dim=d)
        if not x.is_cuda:
            ctx = attention_reference(qkv, B, H, L, bias, causal=True, kv_heads=Hkv, head_dim=d, key_start=key_start)
        else:
            ctx = _AttnFn.apply(qkv, B, H, L, bias, None, True, Hkv, d, key_start)
        return self.o_proj(ctx)


class LlamaMLP(tnn.Module):
    """``down_proj(silu(gate_proj(x)) * up_proj(x))`` with gate and up as one ``gate_up`` Linear
    (gate rows first); HF's ``gate_proj`` / ``up_proj`` through the state-dict hooks."""

    def __init__(self, hidden, inter):
        super().__init__()
        if inter % 8:
            raise ValueError("the SwiGLU kernel needs inter % 8 == 0")
        self.inter = inter
        self.gate_up = Linear(hidden, 2 * inter, bias=False)
        self.down_proj = Linear(inter, hidden, bias=False)
        self._register_state_dict_hook(LlamaMLP._sd_hook)
        self._register_load_state_dict_pre_hook(LlamaMLP._load_hook, with_module=True)

    @staticmethod
    def _sd_hook(mod, sd, prefix, local_metadata):
        w = sd.pop(prefix + "gate_up.weight")
        sd[prefix + "gate_proj.weight"], sd[prefix + "up_proj.weight"] = w[:mod.inter], w[mod.inter:]
        sd[prefix + "down_proj.weight"] = sd.pop(prefix + "down_proj.weight")   # HF order: gate, up, down
        return sd

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        names = [prefix + n + "_proj.weight" for n in ("gate", "up")]
        if all(n in sd for n in names):
            sd[prefix + "gate_up.weight"] = torch.cat([sd.pop(n) for n in names], 0)

    def forward(self, x):
        return self.down_proj(swiglu(self.gate_up(x)))

    def forward_small(self, x):
        """Inference-only forward for M <= 16 rows (a decode step): the gate / up GEMM with the
        SwiGLU in its epilogue (``kml_gemm_skinny_glu``; ``kml_gemm_skinny_glu_w8`` once ``gate_up``
        holds an int8 copy, ``Linear.quantize_small``), then ``down_proj.forward_small``.  On the
        CPU the plain forward."""
        if not x.is_cuda:
            return self.forward(x)
        with torch.no_grad():
            from ..ops import decode as D
            gu = self.gate_up
            x = _bf(x)
            if x.shape[1] != gu.in_pad:
                x = _pad_nograd(x, gu.in_pad)
            if gu._buffers.get("w8") is not None:   # Linear.quantize_small("int8")
                h = D.gemm_skinny_glu_w8(x.contiguous(), gu.w8, gu.w8_scale)
            else:
                h = D.gemm_skinny_glu(x.contiguous(), shadow_of(gu.weight).view(gu.out_pad, gu.in_pad))
            return self.down_proj.forward_small(h)


class LlamaDecoderLayer(tnn.Module):
    """``h += attn(input_layernorm(h))``, ``h += mlp(post_attention_layernorm(h))``.  The layer
    receives ``input_layernorm(h)`` already computed (by the previous layer's closing add-and-
    normalise) and returns its MLP branch and the stream; the caller's next ``add_norm`` closes it."""

    def __init__(self, hidden, heads, kv_heads, inter, eps, head_dim=64):
        super().__init__()
        self.self_attn = LlamaAttention(hidden, heads, kv_heads, head_dim)
        self.mlp = LlamaMLP(hidden, inter)
        self.input_layernorm = RMSNorm(hidden, eps)
        self.post_attention_layernorm = RMSNorm(hidden, eps)

    def forward(self, x, s, B, L, table, bias=None, key_start=None):
        a = self.self_attn(x, B, L, table, bias, key_start)
        x2, s2 = self.post_attention_layernorm.add_norm(a, residual=s)
        return self.mlp(x2), s2


class LlamaModel(tnn.Module):
    def __init__(self, vocab, hidden, layers, heads, kv_heads, inter, max_pos, eps, rope_theta, head_dim=64):
        super().__init__()
        self.embed_tokens = tnn.Embedding(vocab, hidden)
        self.layers = tnn.ModuleList([LlamaDecoderLayer(hidden, heads, kv_heads, inter, eps, head_dim)
                                      for _ in range(layers)])
        self.norm = RMSNorm(hidden, eps)
        self.max_pos = max_pos
        # cos | sin of every position: built in fp64, rounded to fp32 once; a buffer, not a parameter
        self.register_buffer("rope_table", rope_table(max_pos, rope_theta, head_dim=head_dim), persistent=False)
        # storage rows padded to 8 so a tied lm_head Linear can share the token table
        vp = -(-vocab // 8) * 8
        self.embed_tokens.weight._kml_storage_shape = (vp, hidden)
        self.embed_tokens.weight._kml_view = lambda st: st[:vocab, :hidden]

    def forward(self, ids, attention_mask=None, doc_ids=None):
        B, L = ids.shape
        if L > self.max_pos:
            raise ValueError(f"sequence length {L} exceeds max_pos {self.max_pos}")
        key_start = None
        if doc_ids is not None:   # packed rows: every layer's attention stays inside a document
            if doc_ids.shape != ids.shape:
                raise ValueError(f"doc_ids {tuple(doc_ids.shape)} must have the shape of ids {tuple(ids.shape)}")
            key_start = doc_key_start(doc_ids)
        bias = None
        if attention_mask is not None:
            bias = ((1.0 - attention_mask.float()) * -10000.0).reshape(B, L).contiguous()
        if not ids.is_cuda:
            e = self.embed_tokens(ids).reshape(B * L, -1)
            if bias is not None:
                bias = bias.to(e.dtype)
        else:
            e = _TokEmbFn.apply(ids.reshape(-1).contiguous(), self.embed_tokens.weight, L)
        # from here on (x, s) = (RMSNorm(s), stream)
        x, s = self.layers[0].input_layernorm.add_norm(e)
        closers = [lay.input_layernorm for lay in self.layers[1:]] + [self.norm]
        for lay, norm in zip(self.layers, closers):
            m, s = lay(x, s, B, L, self.rope_table, bias, key_start)
            x, s = norm.add_norm(m, residual=s)
        return x


class LlamaForCausalLM(DecodeMixin, tnn.Module):
    def __init__(self, vocab=32000, hidden=576, layers=30, heads=9, kv_heads=3, inter=1536, max_pos=2048, eps=1e-5,
                 rope_theta=10000.0, tie_word_embeddings=False, seed: int = 0, head_dim: int = 64):
        super().__init__()
        self.vocab = vocab
        self.tie_word_embeddings = bool(tie_word_embeddings)
        self.seed = seed
        self.head_dim = head_dim
        self.model = LlamaModel(vocab, hidden, layers, heads, kv_heads, inter, max_pos, eps, rope_theta, head_dim)
        self.lm_head = Linear(hidden, vocab, bias=False)
        if self.tie_word_embeddings:   # lm_head.weight IS the token table
            self.lm_head.weight = self.model.embed_tokens.weight
        self._init_weights()
        self._register_load_state_dict_pre_hook(LlamaForCausalLM._load_hook, with_module=True)

    @classmethod
    def from_hf_config(cls, config, **overrides):
        """Build the model a HuggingFace Llama ``config`` describes: a ``LlamaConfig``, a dict, or
        the path of a ``config.json``.  Maps the sizes, ``rms_norm_eps``, ``rope_theta`` and
        ``tie_word_embeddings``.  Raises ``ValueError`` for what this model does not implement:
        a head dim (``head_dim``, or ``hidden_size // num_attention_heads`` without one) other than
        64 or 128, ``hidden_act`` other than ``silu``, a ``rope_scaling``,
        ``attention_bias`` / ``mlp_bias``, a non-zero ``attention_dropout``.  ``overrides`` replace
        constructor arguments.  Follow with ``load_state_dict(hf_model.state_dict())``.  A head-dim-128
        model trains and evaluates full sequences; its KV-cache decoding is not implemented yet."""
        if isinstance(config, (str, os.PathLike)):
            with open(config) as f:
                config = json.load(f)
        elif hasattr(config, "to_dict"):
            config = config.to_dict()
        if not isinstance(config, dict):
            raise TypeError(f"from_hf_config: a LlamaConfig, a dict or a path, got {type(config).__name__}")
        c = config
        hidden, heads = c.get("hidden_size", 4096), c.get("num_attention_heads", 32)
        head_dim = c.get("head_dim") or hidden // heads
        if head_dim not in (64, 128):
            raise ValueError(f"from_hf_config: head dim {head_dim} (hidden {hidden}, {heads} heads); only 64 and "
                             "128 are implemented")
        if c.get("hidden_act", "silu") != "silu":
            raise ValueError(f"from_hf_config: hidden_act {c.get('hidden_act')!r} (supported: 'silu')")
        if c.get("rope_scaling") is not None:
            raise ValueError("from_hf_config: rope_scaling is not implemented")
        for k in ("attention_bias", "mlp_bias"):
            if c.get(k, False):
                raise ValueError(f"from_hf_config: {k} is not implemented")
        if c.get("attention_dropout", 0.0) != 0.0:
            raise ValueError("from_hf_config: attention_dropout is not implemented")
        kvh = c.get("num_key_value_heads")
        kw = dict(vocab=c.get("vocab_size", 32000), hidden=hidden, layers=c.get("num_hidden_layers", 32), heads=heads,
                  kv_heads=heads if kvh is None else kvh, inter=c.get("intermediate_size", 11008),
                  max_pos=c.get("max_position_embeddings", 2048), eps=c.get("rms_norm_eps", 1e-6),
                  rope_theta=c.get("rope_theta", 10000.0), tie_word_embeddings=c.get("tie_word_embeddings", False),
                  head_dim=head_dim)
        kw.update(overrides)
        return cls(**kw)

    def _init_weights(self):
        g = torch.Generator().manual_seed(self.seed)
        for m in self.modules():
            if isinstance(m, (Linear, tnn.Embedding)):
                if m is self.lm_head and self.tie_word_embeddings:
                    continue
                with torch.no_grad():
                    m.weight.normal_(0.0, 0.02, generator=g)
            elif isinstance(m, RMSNorm):
                tnn.init.ones_(m.weight)

    @staticmethod
    def _load_hook(mod, sd, prefix, local_metadata, strict, missing, unexpected, errors):
        if mod.tie_word_embeddings and prefix + "lm_head.weight" not in sd \
                and prefix + "model.embed_tokens.weight" in sd:
            sd[prefix + "lm_head.weight"] = sd[prefix + "model.embed_tokens.weight"]

    def forward(self, ids, attention_mask=None, labels=None, return_correct=False, doc_ids=None):
        """ids [B, L]; labels [B, L] (may be ``ids`` itself): position t is scored against
        labels[:, t + 1], the last position of every sequence is ignored.  Returns logits
        ``[B*L, vocab]``, or the mean loss (and the correct count) when labels are given.

        doc_ids int [B, L]: rows packed from several documents (``nn.transformer.pack_documents``),
        constant within a document and changing at each boundary.  A token then attends its own
        document only (the band attention kernels, ``key_start`` = the row at which its document
        starts; rotary positions stay the row's, which gives the scores of positions restarted at 0),
        and the last token of a document is not scored against the first token of the next."""
        z = self.model(ids, attention_mask, doc_ids)
        if labels is None:
            return self.lm_head(z)
        if doc_ids is not None:   # a document's first token is nobody's target
            first = torch.zeros_like(doc_ids, dtype=torch.bool)
            first[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
            labels = labels.masked_fill(first, -100)
        if ids.is_cuda:
            from ..ops import transformer as T
            tgt = T.lm_shift_labels(labels, -100)
        else:
            tgt = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], 1)
        logits = self.lm_head(z, keep_pad=True)   # vocab-padded logits used in place
        return cross_entropy(logits, tgt.reshape(-1), ignore_index=-100, return_correct=return_correct,
                             classes=self.vocab)

    # ------------------------------------------------------------------ KV-cache decoding
    # generate / prefill / decode_step / prefill_logits / decode_logits and the captured replay of
    # _step are nn.decode.DecodeMixin's; this model supplies the cache, _prefill and _step.

    @property
    def _decode_table(self):
        return self.model.embed_tokens.weight

    @property
    def _decode_max_pos(self):
        return self.model.max_pos

    def _closers(self):
        m = self.model
        return list(zip(m.layers, [lay.input_layernorm for lay in m.layers[1:]] + [m.norm]))

    def _decode_check(self):
        if self.head_dim != 64:
            raise NotImplementedError(f"KV-cache decoding at head dim {self.head_dim} is not implemented: head dim 128 "
                                      "decodes with the follow-up to the head-dim-128 training kernels")

    def prefill(self, ids, attention_mask, cache):
        self._decode_check()
        return super().prefill(ids, attention_mask, cache)

    def decode_step(self, cache):
        self._decode_check()
        return super().decode_step(cache)

    def generate(self, *args, **kw):
        self._decode_check()
        return super().generate(*args, **kw)

    def new_cache(self, B, Lcap, device=None):
        self._decode_check()
        m = self.model
        at = m.layers[0].self_attn
        p = m.embed_tokens.weight
        return KVCache(len(m.layers), B, at.heads, Lcap, device or p.device, dtype=p.dtype, kv_heads=at.kv_heads)

    @torch.no_grad()
    def _prefill(self, ids, attention_mask, cache):
        """Causal forward over the right-padded prompt; appends every layer's rotated K and its V;
        leaves ``lens[b] = prompt_len[b] - 1``; returns the logits of each sequence's last prompt
        token."""
        m = self.model
        B, L = ids.shape
        if B != cache.B or L > cache.Lcap or L > m.max_pos:
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
        at0 = m.layers[0].self_attn
        H, Hkv = at0.heads, at0.kv_heads
        if gpu:
            from ..ops import decode as D
            from ..ops import transformer as T
            e = T.gather_rows(shadow_of(m.embed_tokens.weight), ids.reshape(-1).contiguous())
        else:
            e = m.embed_tokens(ids).reshape(B * L, -1)
            if bias is not None:
                bias = bias.to(e.dtype)
        x, s = m.layers[0].input_layernorm.add_norm(e)
        for i, (lay, norm) in enumerate(self._closers()):
            at = lay.self_attn
            qkv = rope(at.qkv(x), m.rope_table, L, H, Hkv)   # the flash kernel reads rotated Q and K
            if gpu:
                D.kv_append_rope(qkv, cache.k[i], cache.v[i], L, H, m.rope_table, rotate=False)   # append only
                ctx = _AttnFn.apply(qkv, B, H, L, bias, None, True, Hkv)
            else:
                cache.append_cpu(i, qkv, L, decode=False)
                ctx = attention_reference(qkv, B, H, L, bias, causal=True, kv_heads=Hkv)
            x2, s = lay.post_attention_layernorm.add_norm(at.o_proj(ctx), residual=s)
            x, s = norm.add_norm(lay.mlp(x2), residual=s)
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
        m = self.model
        at0 = m.layers[0].self_attn
        H, Hkv = at0.heads, at0.kv_heads
        if not cache.lens.is_cuda:
            pos = cache.lens.long().clamp(0, m.max_pos - 1)
            x, s = m.layers[0].input_layernorm.add_norm(m.embed_tokens(cache.next_ids))
            for i, (lay, norm) in enumerate(self._closers()):
                at = lay.self_attn
                qkv = rope_reference(at.qkv(x), m.rope_table, 1, H, Hkv, pos=pos)
                cache.append_cpu(i, qkv, 1, decode=True)
                x2, s = lay.post_attention_layernorm.add_norm(at.o_proj(cache.attend_cpu(i, qkv)), residual=s)
                x, s = norm.add_norm(lay.mlp(x2), residual=s)
            logits = self.lm_head(x)
            if advance:
                advance_cpu(cache, logits, cache.gen)
            return logits
        from ..ops import decode as D
        from ..ops import transformer as T
        e = T.gather_rows(shadow_of(m.embed_tokens.weight), cache.next_ids)
        x, s = m.layers[0].input_layernorm.add_norm(e)
        for i, (lay, norm) in enumerate(self._closers()):
            at = lay.self_attn
            qkv = at.qkv.forward_small(x)
            D.kv_append_rope(qkv, cache.k[i], cache.v[i], 1, H, m.rope_table, lens=cache.lens)
            ctx = D.attn_decode_gqa(qkv, cache.k[i], cache.v[i], cache.lens, H, ws=cache.ws)
            x2, s = lay.post_attention_layernorm.add_norm(at.o_proj.forward_small(ctx), residual=s)
            x, s = norm.add_norm(lay.mlp.forward_small(x2), residual=s)
        logits = self.lm_head.forward_small(x, keep_pad=True)
        if advance:
            self._pick(cache, logits)
        return logits


def llama_tiny(**kw) -> LlamaForCausalLM:
    """2-layer, 128-hidden, 4-head / 2-KV-head variant for tests (gpt2_tiny's scale)."""
    cfg = dict(vocab=1000, hidden=128, layers=2, heads=4, kv_heads=2, inter=352, max_pos=256)
    cfg.update(kw)
    return LlamaForCausalLM(**cfg)
