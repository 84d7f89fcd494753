"""Launchers for the decode kernels (csrc/kernels/decode.hip): KV-cache append, one-query
attention over the cache, the skinny (M <= 16) GEMM, the embedding at the device lengths and
the next-token choice (plain, or behind a repetition penalty, top-k and top-p); and the verify
round of speculative decoding: multi-row embedding and append, multi-query attention, the n-gram
drafter, pick and commit.

Everything a step needs that changes per token — sequence lengths, seed / step, temperature,
eos, the sampling filters — is read from device memory, so one captured step replays for every token.  All launches
go on the current HIP stream and are hipGraph-capturable (no host sync, no memset nodes).
"""
from __future__ import annotations

import math

import torch

from .._native import HIP
from .kernels import BF16, F32, _COUNTERS, _chk, _p, _s
from .transformer import _chk_view

I32 = torch.int32
I64 = torch.int64


def attn_decode_chunk() -> int:
    """Keys per chunk of :func:`attn_decode` (a constant of the kernel)."""
    return int(HIP.raw("kml_attn_decode_chunk"))


def attn_decode_workspace(B, H, Lcap, device):
    """fp32 workspace for the chunk partials of a (B, H, Lcap) cache."""
    return torch.empty(int(HIP.raw("kml_attn_decode_ws_floats", B, H, Lcap)), dtype=F32, device=device)


def _chk_cache(kc, vc, name="cache"):
    for n, t in (("K", kc), ("V", vc)):
        _chk(t, BF16, f"{name} {n}", ndim=4)
    if kc.shape != vc.shape or kc.shape[3] != 64 or kc.shape[2] % 64 or kc.shape[2] < 64:
        raise ValueError(f"{name}: K and V must be [B, H, Lcap, 64] with Lcap a multiple of 64, got "
                         f"{tuple(kc.shape)} / {tuple(vc.shape)}")
    return kc.shape[0], kc.shape[1], kc.shape[2]


def _chk_lens(lens, B):
    _chk(lens, I32, "lens", ndim=1)
    if lens.numel() != B:
        raise ValueError(f"lens: expected [{B}] int32, got {tuple(lens.shape)}")


def kv_append(qkv, kc, vc, Lq, lens=None):
    """Copy the K and V columns of a fused ``[B*Lq, 3*H*64]`` QKV buffer into the cache
    ``kc, vc [B, H, Lcap, 64]``.  ``lens`` None: prefill, row t of sequence b goes to cache row
    t.  ``lens`` given (``Lq <= 16``: 1 in a plain step, the rows of a verify round otherwise):
    row t of sequence b goes to cache row ``lens[b] + t``.  Rows at or past Lcap are dropped."""
    B, H, Lcap = _chk_cache(kc, vc)
    _chk_view(qkv, "qkv")
    if qkv.shape[0] != B * Lq or qkv.shape[1] != 3 * H * 64:
        raise ValueError(f"qkv: expected [{B * Lq}, {3 * H * 64}], got {tuple(qkv.shape)}")
    if lens is not None:
        if not 1 <= Lq <= 16:
            raise ValueError("kv_append: decode mode appends 1..16 rows per sequence")
        _chk_lens(lens, B)
    elif Lq > Lcap:
        raise ValueError(f"kv_append: {Lq} prompt rows do not fit a cache of {Lcap}")
    HIP.call("kml_kv_append", "p i p p p i i i i i s", _p(qkv), qkv.stride(0), _p(kc), _p(vc), _p(lens), B, H, Lq,
             Lcap, int(lens is not None), _s())


def attn_decode(q, kc, vc, lens, ws=None, out=None, scale=None, chunk=None):
    """softmax(q Kᵀ * scale) V over cache rows ``0..lens[b]`` for one query per (b, h).
    q: ``[B, >= H*64]`` bf16 view, head h at columns 64h (the first third of a fused QKV row).
    Cache rows past ``lens[b]`` are never read.  Returns ``[B, H*64]`` bf16.  ``chunk``: another
    keys-per-chunk than the kernel's constant (64 / 128 / 256 / 512; the tuning sweep only)."""
    B, H, Lcap = _chk_cache(kc, vc)
    _chk_view(q, "q")
    if q.shape[0] != B or q.shape[1] < H * 64:
        raise ValueError(f"q: expected a [{B}, >= {H * 64}] view, got {tuple(q.shape)}")
    _chk_lens(lens, B)
    need = int(HIP.raw("kml_attn_decode_ws_floats", B, H, Lcap))
    if ws is None:
        ws = torch.empty(need, dtype=F32, device=q.device)
    _chk(ws, F32, "ws")
    if ws.numel() < need:
        raise ValueError(f"ws: {ws.numel()} floats, the cache needs {need}")
    if out is None:
        out = torch.empty((B, H * 64), dtype=BF16, device=q.device)
    _chk_view(out, "out")
    if out.shape != (B, H * 64):
        raise ValueError(f"out: expected [{B}, {H * 64}], got {tuple(out.shape)}")
    scale = 1.0 / math.sqrt(64) if scale is None else scale
    cnt = _COUNTERS.take(q.device, B * H)
    if chunk is None:
        HIP.call("kml_attn_decode", "p i p p p p p p i i i i f s", _p(q), q.stride(0), _p(kc), _p(vc), _p(lens), _p(ws),
                 _p(cnt), _p(out), out.stride(0), B, H, Lcap, float(scale), _s())
    else:
        if chunk not in (64, 128, 256, 512):
            raise ValueError("chunk must be 64, 128, 256 or 512")
        HIP.call("kml_attn_decode_sweep", "i p i p p p p p p i i i i f s", int(chunk), _p(q), q.stride(0), _p(kc),
                 _p(vc), _p(lens), _p(ws), _p(cnt), _p(out), out.stride(0), B, H, Lcap, float(scale), _s())
    return out


_SKINNY_ACT = {None: 0, "gelu": 1, "gelu_tanh": 2}   # kml_gemm_skinny's act codes


def gemm_skinny(x, w, bias=None, act=None, out=None, splits=None):
    """y[M, N] = act(x[M, K] @ w[N, K]ᵀ + bias) for M <= 16: bf16 in / out, fp32 accumulate, fp32
    bias, ``act`` None, "gelu" (erf) or "gelu_tanh" (the tanh approximation).  x, w and out may be row-major views with a row stride
    that is a multiple of 8.  Row m of the result does not depend on M or on the other rows.
    ``splits``: another K split than the kernel's plan for (N, K) (the tuning sweep only)."""
    _chk_view(x, "x")
    _chk_view(w, "w")
    M, K = x.shape
    N = w.shape[0]
    if not 1 <= M <= 16:
        raise ValueError(f"gemm_skinny: M = {M} rows; the skinny kernel takes 1..16")
    if w.shape[1] != K or K % 8 or K < 8:
        raise ValueError(f"gemm_skinny: x {tuple(x.shape)} vs w {tuple(w.shape)} (K a multiple of 8)")
    if act not in _SKINNY_ACT:
        raise ValueError(f"gemm_skinny: act {act!r}")
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() < N:
            raise ValueError("bias shorter than N")
    if out is None:
        out = torch.empty((M, N), dtype=BF16, device=x.device)
    if out.dtype != BF16 or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1 or out.shape != (M, N):
        raise ValueError(f"out: expected a row-major bf16 [{M}, {N}] GPU view")
    S = int(HIP.raw("kml_gemm_skinny_splits", N, K)) if splits is None else int(splits)
    if S < 1:
        raise ValueError(f"gemm_skinny: no plan for N = {N}, K = {K}" if splits is None else "splits must be >= 1")
    ws = cnt = None
    if S > 1:
        groups = -(-N // 16)
        ws = torch.empty(groups * S * 256, dtype=F32, device=x.device)
        cnt = _COUNTERS.take(x.device, groups)
    HIP.call("kml_gemm_skinny", "p i p i p p i i i i i i p p s", _p(x), x.stride(0), _p(w), w.stride(0), _p(bias),
             _p(out), out.stride(0), M, N, K, _SKINNY_ACT[act], 0 if splits is None else S, _p(ws), _p(cnt),
             _s())
    return out


def embed2_at(ids, lens, word, pos, out=None):
    """out[b] = word[ids[b]] + pos[lens[b]] (bf16 tables; ids int64 [B], lens int32 [B])."""
    _chk(ids, I64, "ids", ndim=1)
    B = ids.numel()
    _chk_lens(lens, B)
    _chk(word, BF16, "word", ndim=2)
    _chk(pos, BF16, "pos", ndim=2)
    N = word.shape[1]
    if pos.shape[1] != N or N % 4:
        raise ValueError(f"embed2_at: tables {tuple(word.shape)} / {tuple(pos.shape)}")
    if out is None:
        out = torch.empty((B, N), dtype=BF16, device=ids.device)
    _chk(out, BF16, "out", ndim=2)
    if out.shape != (B, N):
        raise ValueError(f"out: expected [{B}, {N}]")
    HIP.call("kml_embed2_at", "p p p p p i i l i s", _p(ids), _p(lens), _p(word), _p(pos), _p(out), B, N,
             word.shape[0], pos.shape[0], _s())
    return out


def decode_advance(logits, classes, ctl, temp, next_ids, tokens, lens, finished, sample):
    """Pick the next token of every sequence from its bf16 logits row and advance the decode
    state.  ctl int32 ``[seed, step, eos (-1: none), 0]``; temp fp32 ``[temperature]``.
    ``sample`` False: argmax, lowest index on ties; True: Gumbel-max at ``temp[0]``.  Writes
    ``next_ids[b]`` and ``tokens[b, lens[b] + 1]``, forces / records eos, increments ``lens[b]``
    (saturating at Lcap - 1) and the step."""
    _chk_view(logits, "logits")
    B, ldw = logits.shape
    if not 1 <= classes <= ldw:
        raise ValueError(f"decode_advance: {classes} classes in rows of {ldw}")
    _chk(ctl, I32, "ctl", ndim=1)
    _chk(temp, F32, "temp", ndim=1)
    _chk(next_ids, I64, "next_ids", ndim=1)
    _chk(tokens, I64, "tokens", ndim=2)
    _chk(finished, I32, "finished", ndim=1)
    _chk_lens(lens, B)
    if ctl.numel() < 4 or temp.numel() < 1 or next_ids.numel() != B or finished.numel() != B or tokens.shape[0] != B:
        raise ValueError("decode_advance: state tensors do not match the batch")
    # a row of `ldw` columns must be readable in 16-byte groups up to `classes`
    if logits.stride(0) < -(-classes // 8) * 8:
        raise ValueError("decode_advance: logits rows shorter than the classes padded to 8")
    ticket = _COUNTERS.take(logits.device, 1)
    HIP.call("kml_decode_advance", "p i i i p p p p p p i i p s", _p(logits), logits.stride(0), int(classes),
             int(bool(sample)), _p(temp), _p(ctl), _p(next_ids), _p(tokens), _p(lens), _p(finished), B,
             tokens.shape[1], _p(ticket), _s())


def sample_max_classes() -> int:
    """The widest row :func:`decode_sample` takes: it counts every bf16 value of the row in 16 bits
    and keeps the penalised ids in a 65536-bit bitmap (both constants of the kernel)."""
    return int(HIP.raw("kml_decode_sample_max_classes"))


def sampling_params(temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, sample=True):
    """Check the sampling parameters and return what the kernel reads: ``(fpar, ipar)`` =
    ``([temperature, top_p, penalty, 1 / penalty], [top_k])``.  Limits: ``penalty > 0``,
    ``0 < top_p <= 1``, ``top_k >= 0`` (0: off), ``temperature > 0`` when sampling (greedy: the
    nucleus is measured at temperature 1).  ``1 / penalty`` is stored, in fp32, because the kernel
    multiplies and never divides."""
    if not penalty > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {penalty}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k}")
    if sample and not temperature > 0:
        raise ValueError(f"temperature must be > 0 when sampling, got {temperature}")
    T = float(temperature) if sample else 1.0
    return [T, float(top_p), float(penalty), 1.0 / float(penalty)], [min(int(top_k), 0x7FFFFFFF)]


def decode_sample(logits, classes, ctl, fpar, ipar, next_ids, tokens, lens, finished, sample, info=None):
    """:func:`decode_advance` behind HF's processor chain, in the same single launch: the
    repetition penalty over the distinct ids of ``tokens[b, 0 .. lens[b]]`` (each logit rounded to
    bf16 again), top-k with ties at the k-th value kept, top-p over whole classes of equal value at
    temperature ``fpar[0]``, then the argmax (``sample`` False) or the Gumbel-max draw among the
    kept columns.  ``fpar`` fp32 ``[temperature, top_p, penalty, 1 / penalty]`` and ``ipar`` int32
    ``[top_k]`` as :func:`sampling_params` gives them, on the device.  At most
    :func:`sample_max_classes` classes.  Returns ``info`` fp32 ``[B, 4]``: the smallest kept value,
    the kept column count, kept mass / mass of all non-NaN columns, the row maximum after the
    penalty."""
    _chk_view(logits, "logits")
    B, ldw = logits.shape
    if not 1 <= classes <= ldw:
        raise ValueError(f"decode_sample: {classes} classes in rows of {ldw}")
    if classes > sample_max_classes():
        raise ValueError(f"decode_sample: {classes} classes; the kernel counts at most {sample_max_classes()}")
    _chk(ctl, I32, "ctl", ndim=1)
    _chk(fpar, F32, "fpar", ndim=1)
    _chk(ipar, I32, "ipar", ndim=1)
    _chk(next_ids, I64, "next_ids", ndim=1)
    _chk(tokens, I64, "tokens", ndim=2)
    _chk(finished, I32, "finished", ndim=1)
    _chk_lens(lens, B)
    if (ctl.numel() < 4 or fpar.numel() < 4 or ipar.numel() < 1 or next_ids.numel() != B or finished.numel() != B or
            tokens.shape[0] != B):
        raise ValueError("decode_sample: state tensors do not match the batch")
    if logits.stride(0) < -(-classes // 8) * 8:
        raise ValueError("decode_sample: logits rows shorter than the classes padded to 8")
    if info is None:
        info = torch.empty((B, 4), dtype=F32, device=logits.device)
    _chk(info, F32, "info", ndim=2)
    if info.shape != (B, 4):
        raise ValueError(f"info: expected [{B}, 4]")
    ticket = _COUNTERS.take(logits.device, 1)
    HIP.call("kml_decode_sample", "p i i i p p p p p p p p i i p s", _p(logits), logits.stride(0), int(classes),
             int(bool(sample)), _p(fpar), _p(ipar), _p(info), _p(ctl), _p(next_ids), _p(tokens), _p(lens),
             _p(finished), B, tokens.shape[1], _p(ticket), _s())
    return info


# ------------------------------------------------------------------ verify rounds (speculative decoding)
def attn_decode_multi_workspace(B, H, Lcap, Q, device):
    """fp32 workspace for the chunk partials of ``Q`` queries per (sequence, head)."""
    return torch.empty(int(HIP.raw("kml_attn_decode_multi_ws_floats", B, H, Lcap, Q)), dtype=F32, device=device)


def _chk_draft(draft, B, K, name="draft"):
    _chk(draft, I64, name, ndim=2)
    if draft.shape != (B, K) or not draft.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous [{B}, {K}] int64 tensor, got {tuple(draft.shape)}")


def attn_decode_multi(q, kc, vc, lens, Q, ws=None, out=None, scale=None):
    """:func:`attn_decode` for ``Q <= 16`` queries per (b, h) in one pass over the cache: row
    ``b * Q + j`` of ``q [B*Q, >= H*64]`` sees cache rows ``0 .. lens[b] + j`` and its output row is
    bit-identical to :func:`attn_decode` called with ``lens[b] + j``.  Returns ``[B*Q, H*64]`` bf16."""
    B, H, Lcap = _chk_cache(kc, vc)
    _chk_view(q, "q")
    if not 1 <= Q <= 16:
        raise ValueError(f"attn_decode_multi: Q = {Q} queries; the kernel takes 1..16")
    if q.shape[0] != B * Q or q.shape[1] < H * 64:
        raise ValueError(f"q: expected a [{B * Q}, >= {H * 64}] view, got {tuple(q.shape)}")
    _chk_lens(lens, B)
    need = int(HIP.raw("kml_attn_decode_multi_ws_floats", B, H, Lcap, Q))
    if ws is None:
        ws = torch.empty(need, dtype=F32, device=q.device)
    _chk(ws, F32, "ws")
    if ws.numel() < need:
        raise ValueError(f"ws: {ws.numel()} floats, {Q} queries on this cache need {need}")
    if out is None:
        out = torch.empty((B * Q, H * 64), dtype=BF16, device=q.device)
    _chk_view(out, "out")
    if out.shape != (B * Q, H * 64):
        raise ValueError(f"out: expected [{B * Q}, {H * 64}], got {tuple(out.shape)}")
    scale = 1.0 / math.sqrt(64) if scale is None else scale
    cnt = _COUNTERS.take(q.device, B * H * Q)
    HIP.call("kml_attn_decode_multi", "p i p p p p p p i i i i i f s", _p(q), q.stride(0), _p(kc), _p(vc), _p(lens),
             _p(ws), _p(cnt), _p(out), out.stride(0), B, H, Lcap, int(Q), float(scale), _s())
    return out


def embed2_multi(next_ids, draft, lens, word, pos, out=None):
    """The embedding of a verify round: ``out[b*Q + j] = word[x_j] + pos[lens[b] + j]`` with
    ``x_0 = next_ids[b]`` and ``x_j = draft[b, j - 1]`` (``draft`` int64 ``[B, Q - 1]``); the
    position is clamped to the table as :func:`embed2_at` clamps it."""
    _chk(next_ids, I64, "next_ids", ndim=1)
    B = next_ids.numel()
    _chk(draft, I64, "draft", ndim=2)
    K = draft.shape[1]
    _chk_draft(draft, B, K)
    if not 1 <= K <= 15:
        raise ValueError(f"embed2_multi: {K} draft tokens; a round takes 1..15")
    _chk_lens(lens, B)
    _chk(word, BF16, "word", ndim=2)
    _chk(pos, BF16, "pos", ndim=2)
    N = word.shape[1]
    if pos.shape[1] != N or N % 4:
        raise ValueError(f"embed2_multi: tables {tuple(word.shape)} / {tuple(pos.shape)}")
    Q = K + 1
    if out is None:
        out = torch.empty((B * Q, N), dtype=BF16, device=next_ids.device)
    _chk(out, BF16, "out", ndim=2)
    if out.shape != (B * Q, N):
        raise ValueError(f"out: expected [{B * Q}, {N}]")
    HIP.call("kml_embed2_multi", "p p p p p p i i i l i s", _p(next_ids), _p(draft), _p(lens), _p(word), _p(pos),
             _p(out), B, Q, N, word.shape[0], pos.shape[0], _s())
    return out


def draft_lookup(tokens, lens, k, max_ngram=2, out=None):
    """Prompt-lookup drafter: ``k`` draft tokens per sequence from its own history ``tokens[b, 0 ..
    lens[b]]`` (:func:`kubeml_amd.nn.lookup_draft_reference` is the rule, in stock torch).
    Returns int64 ``[B, k]``."""
    _chk(tokens, I64, "tokens", ndim=2)
    B, Lcap = tokens.shape
    _chk_lens(lens, B)
    if int(k) != k or k < 1 or int(max_ngram) != max_ngram or max_ngram < 1:
        raise ValueError(f"draft_lookup: k = {k}, max_ngram = {max_ngram} (integers >= 1)")
    if not tokens.is_contiguous():
        raise ValueError("draft_lookup: tokens must be contiguous")
    if out is None:
        out = torch.empty((B, int(k)), dtype=I64, device=tokens.device)
    _chk_draft(out, B, int(k), "out")
    HIP.call("kml_draft_lookup", "p p p i i i i s", _p(tokens), _p(lens), _p(out), B, Lcap, int(k), int(max_ngram),
             _s())
    return out


def verify_pick(logits, classes, ctl, temp, start, limit, draft, pick, next_ids, tokens, lens, finished, stats,
                sample):
    """The last launch of a verify round.  ``logits [B*Q, >= classes]`` bf16: row ``b*Q + j`` is
    the model's output for position ``lens[b] + j``.  Every row is picked as
    :func:`decode_advance` picks (argmax, or Gumbel-max at ``temp[0]``) with the noise step
    ``lens[b] + j - start[b]``; then, per sequence, pick j is committed to ``tokens[b, lens[b] + j
    + 1]`` while that index is ``<= limit[b]`` and every earlier draft matched its pick
    (``draft[b, j-1] == pick[b, j-1]``) without being eos; ``next_ids``, ``lens`` and ``finished``
    advance accordingly.  ``pick`` int32 ``[B*Q]`` receives every row's choice; ``stats`` int32
    ``[4]`` accumulates ``[accepted drafts, committed tokens]`` and holds ``max(limit - lens)``."""
    _chk_view(logits, "logits")
    R, ldw = logits.shape
    B = lens.numel()
    if B < 1 or R % B or not 2 <= R // B <= 16:
        raise ValueError(f"verify_pick: {R} rows for {B} sequences (2..16 rows each)")
    Q = R // B
    if not 1 <= classes <= ldw:
        raise ValueError(f"verify_pick: {classes} classes in rows of {ldw}")
    _chk(ctl, I32, "ctl", ndim=1)
    _chk(temp, F32, "temp", ndim=1)
    _chk(next_ids, I64, "next_ids", ndim=1)
    _chk(tokens, I64, "tokens", ndim=2)
    _chk(finished, I32, "finished", ndim=1)
    _chk(pick, I32, "pick", ndim=1)
    _chk(stats, I32, "stats", ndim=1)
    _chk_lens(lens, B)
    _chk_lens(start, B)
    _chk_lens(limit, B)
    _chk_draft(draft, B, Q - 1)
    if (ctl.numel() < 4 or temp.numel() < 1 or next_ids.numel() != B or finished.numel() != B or
            tokens.shape[0] != B or not tokens.is_contiguous() or pick.numel() < R or stats.numel() < 4):
        raise ValueError("verify_pick: state tensors do not match the batch")
    if logits.stride(0) < -(-classes // 8) * 8:
        raise ValueError("verify_pick: logits rows shorter than the classes padded to 8")
    ticket = _COUNTERS.take(logits.device, 1)
    HIP.call("kml_verify_pick", "p i i i p p p p p p p p p p p i i i p s", _p(logits), logits.stride(0), int(classes),
             int(bool(sample)), _p(temp), _p(ctl), _p(start), _p(limit), _p(draft), _p(pick), _p(next_ids),
             _p(tokens), _p(lens), _p(finished), _p(stats), B, Q, tokens.shape[1], _p(ticket), _s())
