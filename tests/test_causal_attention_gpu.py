"""Causal mode of the flash-attention kernels (attention.hip CAUSAL) against fp32 torch with a
lower-triangular mask, per 64-row tile as well as over the whole tensor; exact masking
properties; dropout on both backward modes; graph capture; the non-causal path unchanged."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

# L: 7 a single partial tile; 64 one tile, diagonal only; 100 the diagonal tile is also the tail
# tile; 128 one skipped + one full off-diagonal tile; 192 dKV starts at an odd query tile for key
# tile 1 (two iterations), the forward prefetch ends early; 300 five tiles with a tail
LS = [7, 64, 100, 128, 192, 300]
BH = [(2, 2), (1, 3)]

# whole-tensor norm-relative bounds: those of test_transformer_gpu.py::test_attention_fwd_bwd
WHOLE = {"out": 1e-2, "dq": 3e-2, "dk": 3e-2, "dv": 2e-2}
# per-(b, h, 64-row tile) norm-relative bounds: 2x the largest per-tile error of the NON-causal
# kernels against their fp32 reference on the same inputs (every L / (B, H) / bias case
# below), measured on an MI355X: out 0.00260, dq 0.00291, dk 0.00279, dv 0.00291 (the
# causal kernels' own worst tiles: 0.00259, 0.00392, 0.00441, 0.00254).
# The factor 2: a causal row averages fewer terms, so less rounding error cancels.
TILE_MEASURED = {"out": 0.00260, "dq": 0.00291, "dk": 0.00279, "dv": 0.00291}
TILE = {k: 2.0 * v for k, v in TILE_MEASURED.items()}


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _tile_rel(a, ref, B, H, L):
    """largest norm-relative error over the (b, h, 64-row tile) blocks of a [B*L, H*64] tensor"""
    worst = 0.0
    a, ref = a.float().view(B, L, H, 64), ref.float().view(B, L, H, 64)
    for r0 in range(0, L, 64):
        d = (a[:, r0:r0 + 64] - ref[:, r0:r0 + 64]).pow(2).sum(dim=(1, 3)).sqrt()
        n = ref[:, r0:r0 + 64].pow(2).sum(dim=(1, 3)).sqrt()
        worst = max(worst, float((d / (n + 1e-12)).max()))
    return worst


def _inputs(B, H, L, use_bias, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    D = H * 64
    qkv = (torch.randn(B * L, 3 * D, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dout = torch.randn(B * L, D, device=dev, generator=g).to(torch.bfloat16)
    bias = None
    if use_bias:
        keep = torch.rand(B, L, device=dev, generator=g) > 0.2
        keep[:, 0] = True
        bias = torch.where(keep, 0.0, -10000.0).float().contiguous()
    return qkv, dout, bias


def _run(qkv, dout, bias, B, H, L, causal, drop=None, keep="auto"):
    """kernel forward + backward; returns out, lse, dq, dk, dv"""
    from kubeml_amd.ops import transformer as T
    D = H * 64
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    kw = {"causal": True} if causal else {}
    kb = T.attn_keep_buffer(B, H, L, qkv.device) if drop is not None else None
    out, lse = T.attn_fwd(q, k, v, B, H, L, bias=bias, drop=drop, keep=kb, **kw)
    dqkv = torch.empty_like(qkv)
    T.attn_bwd(q, k, v, out, dout, lse, B, H, L, bias=bias, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:],
               drop=drop, keep=kb if keep == "auto" else None, **kw)
    return out, lse, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:]


def _reference(qkv, dout, bias, B, H, L, causal, keep=None):
    """fp32 torch (nn.transformer.attention_reference) forward + autograd backward"""
    from kubeml_amd.nn.transformer import attention_reference
    D = H * 64
    x = qkv.float().clone().requires_grad_(True)
    ref = attention_reference(x, B, H, L, bias, keep=keep, causal=causal)
    ref.backward(dout.float())
    g = x.grad
    return ref.detach(), g[:, :D], g[:, D:2 * D], g[:, 2 * D:]


def measure(B, H, L, use_bias, causal):
    """{tensor: (whole-tensor error, worst per-tile error)} of one case (also used to measure
    the non-causal per-tile baseline the TILE bounds come from)"""
    qkv, dout, bias = _inputs(B, H, L, use_bias)
    out, _, dq, dk, dv = _run(qkv, dout, bias, B, H, L, causal)
    ro, rq, rk, rv = _reference(qkv, dout, bias, B, H, L, causal)
    return {n: (_rel(a, r), _tile_rel(a, r, B, H, L))
            for n, a, r in (("out", out, ro), ("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv))}


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("L", LS)
def test_causal_matches_fp32_reference(L, B, H, use_bias):
    errs = measure(B, H, L, use_bias, causal=True)
    print("causal", L, B, H, use_bias, {k: (round(w, 5), round(t, 5)) for k, (w, t) in errs.items()})
    for name, (whole, tile) in errs.items():
        assert whole < WHOLE[name], (name, "whole", whole)
        assert tile < TILE[name], (name, "tile", tile)


@functools.lru_cache(maxsize=None)
def _prefix_runs():
    """L = 192: a run, and a run with rows >= 100 of q, k, v and dout replaced"""
    B, H, L, cut = 2, 2, 192, 100
    qkv, dout, _ = _inputs(B, H, L, False, seed=1)
    qkv2, dout2, _ = _inputs(B, H, L, False, seed=2)
    rows = (torch.arange(B * L, device=dev) % L) >= cut
    qkv2 = torch.where(rows[:, None], qkv2 * 3.0, qkv)
    dout2 = torch.where(rows[:, None], dout2, dout)
    a = _run(qkv, dout, None, B, H, L, True)
    b = _run(qkv2.contiguous(), dout2.contiguous(), None, B, H, L, True)
    return (B, H, L, cut, rows), qkv, a, b


def test_query0_output_is_value_row0():
    """query 0 sees key 0 alone: its probability is exactly 1, the output row is V's row 0"""
    for L in (7, 192):
        for B, H in BH:
            qkv, dout, _ = _inputs(B, H, L, False, seed=3)
            out = _run(qkv, dout, None, B, H, L, True)[0]
            D = H * 64
            assert torch.equal(out.view(B, L, D)[:, 0], qkv[:, 2 * D:].view(B, L, D)[:, 0])


def test_prefix_invariance_is_exact():
    """rows < 100 of out, LSE and dQ do not depend on rows >= 100 of q, k, v, dout: bit for bit
    (the mask is applied before the running max, and a row's rescale decisions are its own)"""
    (B, H, L, cut, rows), _, a, b = _prefix_runs()
    head = ~rows
    assert torch.equal(a[0][head], b[0][head])
    assert torch.equal(a[1].view(B * H, L)[:, :cut], b[1].view(B * H, L)[:, :cut])
    assert torch.equal(a[2][head], b[2][head])
    assert not torch.equal(a[0][rows], b[0][rows])


def test_suffix_keys_get_zero_gradient_from_zero_dout():
    """dout rows >= 100 zero: no query that sees keys >= 100 carries a gradient, so rows >= 100
    of dK and dV are exactly 0"""
    B, H, L, cut = 2, 2, 192, 100
    qkv, dout, _ = _inputs(B, H, L, False, seed=4)
    rows = (torch.arange(B * L, device=dev) % L) >= cut
    dout = torch.where(rows[:, None], torch.zeros_like(dout), dout).contiguous()
    _, _, dq, dk, dv = _run(qkv, dout, None, B, H, L, True)
    assert dk[rows].float().abs().max().item() == 0.0
    assert dv[rows].float().abs().max().item() == 0.0
    assert dk[~rows].float().abs().max().item() > 0.0 and dv[~rows].float().abs().max().item() > 0.0


def _attn_keep(seed, step, salt, B, H, L, p):
    """Python replica of the kernel's dropout mask (attention.hip Drop::keep): the helper of
    test_transformer_gpu.py"""
    import numpy as np
    M = np.uint64(0xFFFFFFFF)

    def mul(a, b):
        return (a.astype(np.uint64) * np.uint64(b)) & M

    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    k0 = np.uint64((int(seed) ^ salt) & 0xFFFFFFFF)
    keep = np.zeros((B, H, L, L), dtype=np.float32)
    q = np.arange(L, dtype=np.uint64).reshape(L, 1)
    key = np.arange(L, dtype=np.uint64).reshape(1, L)
    kbase = (key & ~np.uint64(63)) + np.uint64(4) * ((key & np.uint64(15)) >> np.uint64(2))
    c = (q * np.uint64((L + 1) // 2) + (kbase >> np.uint64(1))) & M
    off = (key >> np.uint64(1)) - (kbase >> np.uint64(1))
    for b in range(B):
        for h in range(H):
            bh = np.uint64(b * H + h)
            k1 = ((np.uint64(int(step)) * np.uint64(0x632BE5AB)) & M) ^ ((bh * np.uint64(0x5851F42D)) & M)
            hh = mul(np.full_like(c, k0), 0x9E3779B1) ^ mul((np.full_like(c, k1) + np.uint64(0x7F4A7C15)) & M,
                                                            0x85EBCA77) ^ mul(c, 0xC2B2AE3D)
            hh ^= hh >> np.uint64(15)
            hh = mul(hh, 0x2C1B3C6D)
            hh ^= hh >> np.uint64(12)
            hh = mul(hh, 0x297A2D39)
            hh ^= hh >> np.uint64(15)
            hh = (hh + mul(off, 0x9E3779B9)) & M
            hh ^= hh >> np.uint64(16)
            hh = mul(hh, 0x7FEB352D)
            hh ^= hh >> np.uint64(15)
            half = np.where((key & np.uint64(1)) == 1, hh >> np.uint64(16), hh & np.uint64(0xFFFF))
            keep[b, h] = np.where(half >= thr, 1.0 / (1.0 - p), 0.0)
    return torch.from_numpy(keep)


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("L", [100, 192])
def test_causal_dropout_matches_masked_reference(L, use_bias):
    """p = 0.25 on the keep-bit path and on the re-hash path (keep=None in the backward) against
    fp32 autograd under the same mask (bounds of test_attention_dropout_matches_masked_reference);
    the two backward modes agree bit for bit"""
    B, H, p = 2, 2, 0.25
    qkv, dout, bias = _inputs(B, H, L, use_bias, seed=5)
    ctr = torch.tensor([11.0, 3.0], device=dev)
    salt = 7919 * 3
    keep = _attn_keep(11, 3, salt, B, H, L, p).to(dev)
    drop = (ctr, salt, p)
    bits = _run(qkv, dout, bias, B, H, L, True, drop=drop)
    rehash = _run(qkv, dout, bias, B, H, L, True, drop=drop, keep=None)
    ro, rq, rk, rv = _reference(qkv, dout, bias, B, H, L, True, keep=keep)
    assert _rel(bits[0], ro) < 2e-2
    assert _rel(torch.cat(bits[2:], 1), torch.cat((rq, rk, rv), 1)) < 3e-2
    for a, b in zip(bits, rehash):
        assert torch.equal(a, b)


def test_causal_graph_capture_replays_bit_identical():
    B, H, L = 2, 2, 192
    qkv, dout, bias = _inputs(B, H, L, True, seed=6)
    ctr = torch.tensor([5.0, 1.0], device=dev)
    drop = (ctr, 7919, 0.25)
    eager = [t.clone() for t in _run(qkv, dout, bias, B, H, L, True, drop=drop)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(qkv, dout, bias, B, H, L, True, drop=drop)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = _run(qkv, dout, bias, B, H, L, True, drop=drop)
    for _ in range(2):
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a, b)


@pytest.mark.parametrize("L,use_bias", [(100, True), (192, False)])
def test_non_causal_unchanged_by_keyword(L, use_bias):
    """causal=False through the new keyword == the call without the keyword, bit for bit"""
    from kubeml_amd.ops import transformer as T
    B, H = 2, 2
    D = H * 64
    qkv, dout, bias = _inputs(B, H, L, use_bias, seed=7)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    drop = (torch.tensor([3.0, 2.0], device=dev), 7919, 0.25)
    res = []
    for kw in ({}, {"causal": False}):
        kb = T.attn_keep_buffer(B, H, L, qkv.device)
        out, lse = T.attn_fwd(q, k, v, B, H, L, bias=bias, drop=drop, keep=kb, **kw)
        dq, dk, dv = T.attn_bwd(q, k, v, out, dout, lse, B, H, L, bias=bias, drop=drop, keep=kb, **kw)
        res.append((out, lse, dq, dk, dv))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    causal = T.attn_fwd(q, k, v, B, H, L, bias=bias, drop=drop, causal=True)[0]
    assert not torch.equal(causal, res[0][0])
