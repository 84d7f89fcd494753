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
  cross-entropy kernels in place.

FFN activation: the erf GELU of the GEMM epilogue (HF ``activation_function="gelu"``); GPT-2's
tanh approximation (``gelu_new``) has no epilogue yet.
"""
from __future__ import annotations

import torch
import torch.nn as tnn
from torch.autograd import Function

from ..nn.flat import grad_storage_of, shadow_of
from ..nn.modules import Linear, cross_entropy
from ..nn.transformer import Dropout, LayerNorm, RNGState, SelfAttention, _bf


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


class GPT2MLP(tnn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
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
        return self.c_proj(self.c_fc(x, act="gelu"))   # erf-GELU in the GEMM epilogue


class GPT2Block(tnn.Module):
    """``h += drop(attn(ln_1(h)))``, ``h += drop(mlp(ln_2(h)))``.  The block receives
    ``ln_1(h)`` already computed (by the previous block's closing add-and-normalise) and
    returns its MLP branch and the stream; the caller's next ``add_norm`` closes it."""

    def __init__(self, hidden, heads, inter, eps, dropout, rng):
        super().__init__()
        self.ln_1 = LayerNorm(hidden, eps=eps)
        self.attn = GPT2Attention(hidden, heads, dropout, rng)
        self.ln_2 = LayerNorm(hidden, eps=eps)
        self.mlp = GPT2MLP(hidden, inter)
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
    def __init__(self, vocab, hidden, layers, heads, inter, max_pos, eps, dropout, rng):
        super().__init__()
        self.wte = tnn.Embedding(vocab, hidden)
        self.wpe = tnn.Embedding(max_pos, hidden)
        self.drop = Dropout(dropout, rng)   # embd_pdrop
        self.h = tnn.ModuleList([GPT2Block(hidden, heads, inter, eps, dropout, rng) for _ in range(layers)])
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
        if activation != "gelu":
            raise ValueError(f"activation {activation!r}: only the erf GELU (\"gelu\") has a GEMM epilogue; "
                             "GPT-2's tanh approximation (gelu_new) is not implemented")
        self.rng = RNGState(seed)
        self.vocab = vocab
        self.transformer = GPT2Model(vocab, hidden, layers, heads, inter, max_pos, eps, dropout, self.rng)
        self.lm_head = Linear(hidden, vocab, bias=False)
        # weight tying (HF tie_word_embeddings): lm_head.weight IS the token table
        self.lm_head.weight = self.transformer.wte.weight
        self._init_weights(layers)
        self._register_load_state_dict_pre_hook(GPT2LMHeadModel._load_hook, with_module=True)

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


def gpt2_small(**kw) -> GPT2LMHeadModel:
    return GPT2LMHeadModel(**kw)


def gpt2_tiny(**kw) -> GPT2LMHeadModel:
    """2-layer, 128-hidden variant for tests."""
    cfg = dict(vocab=1000, hidden=128, layers=2, heads=2, inter=512, max_pos=256)
    cfg.update(kw)
    return GPT2LMHeadModel(**cfg)
