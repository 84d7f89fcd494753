"""Launchers for the transformer kernels (csrc/kernels/attention.hip, transformer.hip).

All take/return token-major bf16 tensors ``[T, N]`` (T = batch x seq), fp32 statistics
and fp32 gradient accumulators; every launch goes on the current HIP stream and is
hipGraph-capturable (no host sync, no memset nodes).
"""
from __future__ import annotations

import math

import os

import torch

from .._native import HIP
from .kernels import BF16, F32, _COUNTERS, _chk, _p, _s

I64 = torch.int64


def _chk_view(t, name):
    """bf16 GPU row-major 2-d view (column slices of a wider buffer allowed)."""
    if t.dtype != BF16:
        raise TypeError(f"{name}: expected bfloat16, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor")
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16:
        raise ValueError(f"{name}: expected a 16-byte aligned row-major 2-d view, got stride {t.stride()}")


def _drop_args(drop):
    """drop = (ctr [seed, step] device tensor, salt, p) or None."""
    if drop is None or drop[2] <= 0.0:
        return 0, 0, 0.0
    ctr, salt, p = drop
    _chk(ctr, F32, "ctr")
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must be in [0, 1)")
    return ctr.data_ptr(), int(salt) & 0x7FFFFFFF, float(p)


def attn_keep_buffer(B, H, L, device):
    """Buffer for the attention-dropout keep bits the forward writes and the backward reads
    (attention.hip ``Drop``): one u64 word per (b*h, key tile, query), queries padded to
    whole 64-row tiles — B*H*L^2/8 bytes, 12.6 MB per BERT-base layer at L = 512."""
    nkb = (L + 63) // 64
    return torch.empty(B * H * nkb * nkb * 64 * 8, dtype=torch.uint8, device=device)


def _keep_arg(keep, B, H, L, drop):
    if keep is None or drop is None or drop[2] <= 0.0:
        return 0
    nkb = (L + 63) // 64
    if keep.dtype != torch.uint8 or not keep.is_cuda or keep.numel() < B * H * nkb * nkb * 512:
        raise ValueError("keep must be a GPU uint8 buffer from attn_keep_buffer(B, H, L)")
    return keep.data_ptr()


def _kv_heads(H, kv_heads):
    """Hkv of a grouped-query call (None: H, the one-K/V-head-per-query-head entry points)."""
    Hkv = H if kv_heads is None else int(kv_heads)
    if Hkv < 1 or H % Hkv:
        raise ValueError(f"kv_heads {kv_heads} must divide heads {H}")
    return Hkv


def _head_dim(head_dim, drop):
    """64 (attention.hip) or 128 (attention_d128.hip, which has no attention dropout)."""
    if head_dim not in (64, 128):
        raise ValueError(f"head_dim {head_dim}: the attention kernels are written for 64 and 128")
    if head_dim == 128 and drop is not None and drop[2] > 0.0:
        raise ValueError("attention dropout is not implemented at head_dim 128")
    return head_dim


def _key_start(key_start, B, L, causal, kv_heads, drop):
    """The ``key_start`` operand of the band kernels: int32 ``[B, L]`` contiguous on the GPU, with
    ``causal=True``, ``kv_heads`` given (``kv_heads=H`` for plain multi-head) and no dropout."""
    if not causal or kv_heads is None:
        raise ValueError("key_start needs causal=True and kv_heads (kv_heads=H for one K/V head per query head)")
    if drop is not None and drop[2] > 0.0:
        raise ValueError("key_start with attention dropout is not implemented")
    if not torch.is_tensor(key_start) or key_start.dtype != torch.int32:
        raise ValueError(f"key_start: expected an int32 tensor, got {getattr(key_start, 'dtype', type(key_start))}")
    if not key_start.is_cuda or tuple(key_start.shape) != (B, L) or not key_start.is_contiguous():
        raise ValueError(f"key_start: expected a contiguous GPU [{B}, {L}] tensor, got {tuple(key_start.shape)}")
    return key_start.data_ptr()


def attn_fwd(q, k, v, B, H, L, bias=None, out=None, scale=None, drop=None, keep=None, causal=False, kv_heads=None,
             head_dim=64, key_start=None):
    """q/k/v: [B*L, ld] bf16 views with head h at columns 64h..64h+63 (may be column
    slices of one fused QKV buffer).  kv_heads: grouped-query attention — k / v hold ``kv_heads``
    heads and query head h reads K/V head ``h // (H // kv_heads)`` (None: H heads, the plain entry
    points).  drop: (ctr, salt, p) attention-probability dropout;
    keep: optional :func:`attn_keep_buffer` that receives the dropout keep bits, so
    :func:`attn_bwd` reads them instead of re-hashing.  causal: query t attends keys <= t only
    (the key tiles above the diagonal are skipped).  head_dim: 64, or 128 (head h at columns
    128h..128h+127; ``kml_attn128_fwd``, no dropout).  key_start: int32 ``[B, L]`` on the GPU —
    query t attends keys ``key_start[b, t] .. t`` only (``0 <= key_start[b, t] <= t``, non-decreasing
    in t: the row at which t's document starts in a packed batch, ``nn.transformer.doc_key_start``,
    or ``max(0, t - W + 1)`` for a window); the key tiles before it are skipped.  Needs ``causal``,
    ``kv_heads`` and no dropout.  Returns (out [B*L, H*head_dim], lse [B*H, L])."""
    Hkv = _kv_heads(H, kv_heads)
    D = _head_dim(head_dim, drop)
    ks = None if key_start is None else _key_start(key_start, B, L, causal, kv_heads, drop)
    for n, t, hh in (("q", q, H), ("k", k, Hkv), ("v", v, Hkv)):
        _chk_view(t, n)
        if t.shape[0] != B * L or t.shape[1] < hh * D:
            raise ValueError(f"{n}: expected a row-major [B*L, >= {hh * D}] view, got {tuple(t.shape)}")
    if bias is not None:
        _chk(bias, F32, "bias")
        if bias.numel() != B * L:
            raise ValueError("bias must be [B, L]")
    if out is None:
        out = torch.empty((B * L, H * D), dtype=BF16, device=q.device)
    lse = torch.empty((B * H, L), dtype=F32, device=q.device)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    c, salt, pd = _drop_args(drop)
    if ks is not None:
        HIP.call("kml_attn128_band_fwd" if D == 128 else "kml_attn_gqa_band_fwd", "p p p p p p p i i i i i i i i f s",
                 _p(q), _p(k), _p(v), _p(out), _p(lse), _p(bias), ks, q.stride(0), k.stride(0), v.stride(0),
                 out.stride(0), B, H, Hkv, L, float(scale), _s())
        return out, lse
    if D == 128:
        HIP.call("kml_attn128_fwd", "p p p p p p i i i i i i i i f p i f p i s",
                 _p(q), _p(k), _p(v), _p(out), _p(lse), _p(bias), q.stride(0), k.stride(0), v.stride(0),
                 out.stride(0), B, H, Hkv, L, float(scale), 0, 0, 0.0, 0, int(bool(causal)), _s())
        return out, lse
    if kv_heads is not None:
        HIP.call("kml_attn_gqa_fwd", "p p p p p p i i i i i i i i f p i f p i s",
                 _p(q), _p(k), _p(v), _p(out), _p(lse), _p(bias), q.stride(0), k.stride(0), v.stride(0),
                 out.stride(0), B, H, Hkv, L, float(scale), c, salt, pd, _keep_arg(keep, B, H, L, drop),
                 int(bool(causal)), _s())
        return out, lse
    HIP.call("kml_attn_causal_fwd" if causal else "kml_attn_fwd", "p p p p p p i i i i i i i f p i f p s",
             _p(q), _p(k), _p(v), _p(out), _p(lse), _p(bias), q.stride(0), k.stride(0), v.stride(0), out.stride(0),
             B, H, L, float(scale), c, salt, pd, _keep_arg(keep, B, H, L, drop), _s())
    return out, lse


def attn_bwd(q, k, v, o, dout, lse, B, H, L, bias=None, dq=None, dk=None, dv=None, scale=None, drop=None,
             keep=None, causal=False, kv_heads=None, head_dim=64, key_start=None):
    """Gradients of attention; dq/dk/dv may be column views of one [B*L, 3*H*64] buffer.
    keep: the keep-bit buffer the forward filled (same drop), or None to re-hash the mask;
    causal, kv_heads, head_dim, key_start: as given to :func:`attn_fwd`.  Grouped-query: dk / dv have
    ``kv_heads * head_dim`` columns, each head the sum over its group of query heads (fp32
    accumulators, fixed order)."""
    dev = q.device
    Hkv = _kv_heads(H, kv_heads)
    D = _head_dim(head_dim, drop)
    if dq is None:
        dq = torch.empty((B * L, H * D), dtype=BF16, device=dev)
    if dk is None:
        dk = torch.empty((B * L, Hkv * D), dtype=BF16, device=dev)
    if dv is None:
        dv = torch.empty((B * L, Hkv * D), dtype=BF16, device=dev)
    for n, t, hh in (("q", q, H), ("k", k, Hkv), ("v", v, Hkv), ("o", o, H), ("dout", dout, H), ("dq", dq, H),
                     ("dk", dk, Hkv), ("dv", dv, Hkv)):
        _chk_view(t, n)
        if t.shape[0] != B * L or t.shape[1] < hh * D:
            raise ValueError(f"{n}: expected [B*L, >= {hh * D}], got {tuple(t.shape)}")
    if lse.shape != (B * H, L) or lse.dtype != F32:
        raise ValueError("lse must be fp32 [B*H, L] from attn_fwd")
    dsum = torch.empty((B * H, L), dtype=F32, device=dev)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    c, salt, pd = _drop_args(drop)
    if key_start is not None:
        ks = _key_start(key_start, B, L, causal, kv_heads, drop)
        HIP.call("kml_attn128_band_bwd" if D == 128 else "kml_attn_gqa_band_bwd",
                 "p p p p p p p p p p p p i i i i i i i i i i i i f s",
                 _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dsum), _p(bias), ks, _p(dq), _p(dk), _p(dv),
                 q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0), dk.stride(0),
                 dv.stride(0), B, H, Hkv, L, float(scale), _s())
        return dq, dk, dv
    if D == 128:
        HIP.call("kml_attn128_bwd", "p p p p p p p p p p p i i i i i i i i i i i i f p i f p i s",
                 _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dsum), _p(bias), _p(dq), _p(dk), _p(dv),
                 q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0), dk.stride(0),
                 dv.stride(0), B, H, Hkv, L, float(scale), 0, 0, 0.0, 0, int(bool(causal)), _s())
        return dq, dk, dv
    if kv_heads is not None:
        HIP.call("kml_attn_gqa_bwd", "p p p p p p p p p p p i i i i i i i i i i i i f p i f p i s",
                 _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dsum), _p(bias), _p(dq), _p(dk), _p(dv),
                 q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0), dk.stride(0),
                 dv.stride(0), B, H, Hkv, L, float(scale), c, salt, pd, _keep_arg(keep, B, H, L, drop),
                 int(bool(causal)), _s())
        return dq, dk, dv
    HIP.call("kml_attn_causal_bwd" if causal else "kml_attn_bwd",
             "p p p p p p p p p p p i i i i i i i i i i i f p i f p s",
             _p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(dsum), _p(bias), _p(dq), _p(dk), _p(dv),
             q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0), dk.stride(0),
             dv.stride(0), B, H, L, float(scale), c, salt, pd, _keep_arg(keep, B, H, L, drop), _s())
    return dq, dk, dv


def ln_fwd(x, gamma, beta, res=None, eps=1e-12, keep_sum=True, drop=None):
    """LayerNorm over the last dim of a [T, N] bf16 tensor (optionally of x + res).
    Returns (y, ln_input, mean, rstd) — ln_input is x + res (or x).  drop = (ctr, salt, p):
    x goes through :func:`dropout` (same mask) as it is loaded — LN(dropout(x) + res) in one
    pass; ln_input is then dropout(x) + res."""
    _chk(x, BF16, "x")
    N = x.shape[-1]
    M = x.numel() // N
    y = torch.empty_like(x)
    s = torch.empty_like(x) if ((res is not None or drop is not None) and keep_sum) else None
    mean = torch.empty(M, dtype=F32, device=x.device)
    rstd = torch.empty(M, dtype=F32, device=x.device)
    ctr, salt, p = drop if drop is not None else (None, 0, 0.0)
    HIP.call("kml_ln_fwd", "p p p p p p p p l i f p i f s", _p(x), _p(res), _p(gamma), _p(beta), _p(y), _p(s),
             _p(mean), _p(rstd), M, N, float(eps), _p(ctr), int(salt) & 0x7FFFFFFF, float(p), _s())
    return y, (s if s is not None else x), mean, rstd


def ln_bwd(dy, xin, mean, rstd, gamma, dgamma, dbeta, dx_add=None, drop=None, dbias_in=None):
    """dx (+ dx_add) ; dgamma/dbeta += (deterministic two-level reduce).  drop = (ctr, salt,
    p) of a forward :func:`ln_fwd` dropout: returns (dx, dropout(dx)) — the gradients of the
    residual input and of the pre-dropout input — from one pass.  dbias_in (fp32 [N]) +=
    column sums of the input gradient: the bias gradient of the Linear feeding the LN."""
    _chk(dy, BF16, "dy")
    N = dy.shape[-1]
    M = dy.numel() // N
    dx = torch.empty_like(dy)
    dxd = torch.empty_like(dy) if drop is not None else None
    ctr, salt, p = drop if drop is not None else (None, 0, 0.0)
    nws = HIP.raw("kml_ln_bwd_ws_floats", M, N)
    ws = torch.empty(nws, dtype=F32, device=dy.device)
    cnt = _COUNTERS.take(dy.device, 1)
    if dbias_in is not None:
        _chk(dbias_in, F32, "dbias_in")
        if dbias_in.numel() < N:
            raise ValueError("dbias_in shorter than N")
    HIP.call("kml_ln_bwd", "p p p p p p p p p p p l i p p i f p s", _p(dy), _p(xin), _p(mean), _p(rstd), _p(gamma),
             _p(dx), _p(dx_add), _p(dgamma), _p(dbeta), _p(ws), _p(cnt), M, N, _p(dxd), _p(ctr),
             int(salt) & 0x7FFFFFFF, float(p), _p(dbias_in), _s())
    return (dx, dxd) if drop is not None else dx


def rmsnorm_fwd(x, gamma, res=None, eps=1e-5, keep_sum=True):
    """RMSNorm over the last dim of a [T, N] bf16 tensor (optionally of x + res).  Returns
    (y, norm_input, rstd) — norm_input is x + res (or x itself without a residual)."""
    _chk(x, BF16, "x")
    N = x.shape[-1]
    M = x.numel() // N
    if res is not None:
        _chk(res, BF16, "res")
        if res.shape != x.shape:
            raise ValueError("res must have x's shape")
    if gamma.numel() < N:
        raise ValueError("gamma shorter than N")
    y = torch.empty_like(x)
    s = torch.empty_like(x) if (res is not None and keep_sum) else None
    rstd = torch.empty(M, dtype=F32, device=x.device)
    HIP.call("kml_rmsnorm_fwd", "p p p p p p l i f s", _p(x), _p(res), _p(gamma), _p(y), _p(s), _p(rstd), M, N,
             float(eps), _s())
    return y, (s if s is not None else x), rstd


def rmsnorm_bwd(dy, xin, rstd, gamma, dgamma, dx_add=None):
    """dx (+ dx_add); dgamma += column sums of dy * xin * rstd — per-block partial rows folded in
    block order by the last block of the same launch (deterministic, no float atomics)."""
    _chk(dy, BF16, "dy")
    _chk(xin, BF16, "xin")
    _chk(dgamma, F32, "dgamma")
    N = dy.shape[-1]
    M = dy.numel() // N
    if xin.shape != dy.shape or rstd.numel() != M or dgamma.numel() < N or gamma.numel() < N:
        raise ValueError("rmsnorm_bwd: shapes of xin / rstd / gamma / dgamma do not match dy")
    if dx_add is not None:
        _chk(dx_add, BF16, "dx_add")
        if dx_add.shape != dy.shape:
            raise ValueError("dx_add must have dy's shape")
    dx = torch.empty_like(dy)
    ws = torch.empty(HIP.raw("kml_rmsnorm_bwd_ws_floats", M, N), dtype=F32, device=dy.device)
    cnt = _COUNTERS.take(dy.device, 1)
    HIP.call("kml_rmsnorm_bwd", "p p p p p p p p p l i s", _p(dy), _p(xin), _p(rstd), _p(gamma), _p(dx), _p(dx_add),
             _p(dgamma), _p(ws), _p(cnt), M, N, _s())
    return dx


def rope_(qkv, table, L, H, kv_heads, backward=False):
    """Rotary embedding in place on the fused ``[B*L, (H + 2 kv_heads) * D]`` projection buffer (or
    its gradient with ``backward``: the transpose rotation): the H query and kv_heads key heads are
    rotated by the position ``row % L``, V is left alone.  table: ``nn.transformer.rope_table``; its
    width is the head dim D, 64 or 128."""
    _chk_view(qkv, "qkv")
    _chk(table, F32, "table")
    if table.dim() != 2 or table.shape[1] not in (64, 128) or L > table.shape[0]:
        raise ValueError(f"rope_: table must be [max_pos >= {L}, 64 or 128], got {tuple(table.shape)}")
    D = table.shape[1]
    if qkv.shape[1] != (H + 2 * kv_heads) * D or qkv.shape[0] % L:
        raise ValueError(f"rope_: expected [B*{L}, {(H + 2 * kv_heads) * D}], got {tuple(qkv.shape)}")
    HIP.call("kml_rope128" if D == 128 else "kml_rope", "p i p l i i i i i s", _p(qkv), qkv.stride(0), _p(table), qkv.shape[0], L, H, kv_heads,
             table.shape[0], int(bool(backward)), _s())
    return qkv


def _chk_gu(gu, name):
    _chk_view(gu, name)
    if gu.shape[1] % 16:
        raise ValueError(f"{name}: expected [T, 2*I] with I % 8 == 0, got {tuple(gu.shape)}")
    return gu.shape[0], gu.shape[1] // 2


def swiglu_fwd(gu):
    """h = silu(gu[:, :I]) * gu[:, I:] of the fused gate/up projection ``[T, 2*I]``."""
    T_, I = _chk_gu(gu, "gu")
    h = torch.empty((T_, I), dtype=BF16, device=gu.device)
    HIP.call("kml_swiglu_fwd", "p i p l i s", _p(gu), gu.stride(0), _p(h), T_, I, _s())
    return h


def swiglu_bwd(dh, gu):
    """dgu ``[T, 2*I]`` = [dh u sig(g) (1 + g (1 - sig(g))) | dh silu(g)] from dh ``[T, I]``."""
    T_, I = _chk_gu(gu, "gu")
    _chk(dh, BF16, "dh")
    if tuple(dh.shape) != (T_, I) or not dh.is_contiguous() or gu.stride(0) != 2 * I:
        raise ValueError(f"swiglu_bwd: dh must be contiguous [{T_}, {I}] and gu contiguous")
    dgu = torch.empty_like(gu)
    HIP.call("kml_swiglu_bwd", "p p i p l i s", _p(dh), _p(gu), gu.stride(0), _p(dgu), T_, I, _s())
    return dgu


def _tanh(approximate, who):
    if approximate not in ("none", "tanh"):
        raise ValueError(f"{who}: approximate {approximate!r} (\"none\" or \"tanh\")")
    return approximate == "tanh"


def gelu_fwd(x, approximate="none"):
    """y = gelu(x): the erf form, or with approximate="tanh" the tanh approximation
    (torch's ``F.gelu`` argument; HF ``gelu_new``)."""
    tanh = _tanh(approximate, "gelu_fwd")
    y = torch.empty_like(x)
    if tanh:
        HIP.call("kml_gelu_tanh_fwd", "p p l s", _p(x), _p(y), x.numel(), _s())
    else:
        HIP.call("kml_gelu_fwd", "p p l s", _p(x), _p(y), x.numel(), _s())
    return y


def gelu_bwd(dy, x, dbias=None, approximate="none"):
    """dx = dy * gelu'(x).  dbias (fp32 [N]) += column sums of dx over the rows of the
    [M, N] map, from the same pass (the bias gradient of the Linear whose pre-activation x is).
    approximate: as :func:`gelu_fwd`."""
    tanh = _tanh(approximate, "gelu_bwd")
    dx = torch.empty_like(dy)
    if dbias is not None:
        _chk(dbias, F32, "dbias")
        N = dy.shape[-1]
        M = dy.numel() // N
        if dbias.numel() < N:
            raise ValueError("dbias shorter than N")
        ws = torch.empty(HIP.raw("kml_gelu_bwd_colsum_ws_floats", M, N), dtype=F32, device=dy.device)
        if tanh:
            HIP.call("kml_gelu_tanh_bwd_colsum", "p p p p p l i s", _p(dy), _p(x), _p(dx), _p(dbias), _p(ws), M, N,
                     _s())
        else:
            HIP.call("kml_gelu_bwd_colsum", "p p p p p l i s", _p(dy), _p(x), _p(dx), _p(dbias), _p(ws), M, N, _s())
        return dx
    if tanh:
        HIP.call("kml_gelu_tanh_bwd", "p p p l s", _p(dy), _p(x), _p(dx), dy.numel(), _s())
    else:
        HIP.call("kml_gelu_bwd", "p p p l s", _p(dy), _p(x), _p(dx), dy.numel(), _s())
    return dx


def dropout(x, ctr, salt, p):
    """Counter-based dropout: mask is a hash of (ctr[0] seed, ctr[1] step, salt, index)."""
    y = torch.empty_like(x)
    HIP.call("kml_dropout", "p p p i f l s", _p(x), _p(y), _p(ctr), int(salt) & 0x7FFFFFFF, float(p), x.numel(), _s())
    return y


def embed_fwd(ids, tt, word, pos, type_, L):
    T = ids.numel()
    N = word.shape[-1]
    out = torch.empty((T, N), dtype=BF16, device=ids.device)
    HIP.call("kml_embed_fwd", "p p p p p p l i i s", _p(ids), _p(tt), _p(word), _p(pos), _p(type_), _p(out), T, L, N,
             _s())
    return out


def embed_bwd(ids, tt, dsum, dword, dpos, dtype, L):
    """Word / position / token-type table gradients (+=).  With all three tables: one pass over
    dsum (k_embed_bwd_fused)."""
    T = ids.numel()
    N = dsum.shape[-1]
    HIP.call("kml_embed_bwd", "p p p p p p l i i s", _p(ids), _p(tt), _p(dsum), _p(dword), _p(dpos), _p(dtype), T, L,
             N, _s())


def embed2_fwd(ids, word, pos, L):
    """Two-table embedding (decoder LMs): word[ids] + pos[t % L].  Its backward is
    :func:`embed_bwd` with ``tt`` and ``dtype`` None."""
    T = ids.numel()
    N = word.shape[-1]
    out = torch.empty((T, N), dtype=BF16, device=ids.device)
    HIP.call("kml_embed2_fwd", "p p p p l i i s", _p(ids), _p(word), _p(pos), _p(out), T, L, N, _s())
    return out


def lm_shift_labels(ids, ignore_index=-100):
    """Next-token labels of int64 ``[B, L]`` ids: out[b, t] = ids[b, t + 1], out[b, L - 1] = ignore."""
    if ids.dtype != I64 or ids.dim() != 2 or not ids.is_cuda:
        raise TypeError("lm_shift_labels: int64 [B, L] GPU ids")
    ids = ids.contiguous()
    B, L = ids.shape
    out = torch.empty_like(ids)
    HIP.call("kml_lm_shift_labels", "p p i i l s", _p(ids), _p(out), B, L, int(ignore_index), _s())
    return out


def gather_rows(src, idx):
    N = src.shape[-1]
    out = torch.empty((idx.numel(), N), dtype=src.dtype, device=src.device)
    HIP.call("kml_gather_rows", "p p p l i s", _p(src), _p(idx), _p(out), idx.numel(), N, _s())
    return out


def scatter_rows(src, idx, dst, accumulate=False):
    N = src.shape[-1]
    HIP.call("kml_scatter_rows", "p p p l i i s", _p(src), _p(idx), _p(dst), idx.numel(), N, int(accumulate), _s())
    return dst
