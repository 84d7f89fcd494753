"""The Llama block's kernels (csrc/kernels/llama.hip: RMSNorm, RoPE, SwiGLU; attention.hip:
grouped-query flash attention) against plain torch in fp32 / fp64 on the same bf16 inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
# tests/test_causal_attention_gpu.py's whole-tensor bounds
WHOLE = {"out": 1e-2, "dq": 3e-2, "dk": 3e-2, "dv": 2e-2}
# one bf16 store (2^-9 per element), a factor 2 for the cancellation in a*c - b*s and the fp32 table
ONE_ROUNDING = 2.0 ** -8


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(BF)


# (5, ...) and (7, ...): a partial last block in the dgamma fold; 576: lanes not evenly filled
@pytest.mark.parametrize("M,N,res", [(300, 768, True), (64, 1024, False), (5, 128, True), (7, 576, True)])
def test_rmsnorm_fwd_bwd(M, N, res):
    from kubeml_amd.ops import transformer as T
    g = torch.Generator(device=dev).manual_seed(M + N)
    x, r, dy, da = (_randn(g, M, N) for _ in range(4))
    gamma = torch.rand(N, device=dev, generator=g) + 0.5
    y, s, rstd = T.rmsnorm_fwd(x, gamma, res=r if res else None, eps=1e-5)
    dgam = [torch.zeros(N, device=dev) for _ in range(2)]
    dx = [T.rmsnorm_bwd(dy, s, rstd, gamma, d, dx_add=da if res else None) for d in dgam]
    sr = (x.float() + r.float()).to(BF) if res else x
    assert torch.equal(s, sr)
    # reference on the bf16 stream the kernel normalises in fp32 before its one rounding
    sd = (x.double() + r.double() if res else x.double()).requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    yr = sd * torch.rsqrt(sd.pow(2).mean(-1, keepdim=True) + 1e-5) * gd
    yr.backward(dy.double())
    dxr = sd.grad + (da.double() if res else 0)
    print("y", _rel(y, yr), "dx", _rel(dx[0], dxr), "dgamma", _rel(dgam[0], gd.grad))
    assert _rel(y, yr) < 1e-2
    assert _rel(dx[0], dxr) < 2e-2
    assert _rel(dgam[0], gd.grad) < 1e-2
    assert torch.equal(dgam[0], dgam[1]) and torch.equal(dx[0], dx[1])


@pytest.mark.parametrize("B,L,H,Hkv,theta", [(2, 7, 2, 1, 1e4), (1, 300, 3, 3, 5e5)])
def test_rope_fwd_bwd(B, L, H, Hkv, theta):
    from kubeml_amd.nn.transformer import rope_reference, rope_table
    from kubeml_amd.ops import transformer as T
    g = torch.Generator(device=dev).manual_seed(L)
    table = rope_table(L + 3, theta, device=dev)
    n = (H + Hkv) * 64
    x, dy = _randn(g, B * L, n + Hkv * 64), _randn(g, B * L, n + Hkv * 64)
    xd = x.double().requires_grad_(True)
    ref = rope_reference(xd, table.double(), L, H, Hkv)
    ref.backward(dy.double())
    y = T.rope_(x.clone(), table, L, H, Hkv)
    dx = T.rope_(dy.clone(), table, L, H, Hkv, backward=True)
    print("fwd", _rel(y[:, :n], ref[:, :n]), "bwd", _rel(dx[:, :n], xd.grad[:, :n]))
    assert torch.equal(y[:, n:], x[:, n:]) and torch.equal(dx[:, n:], dy[:, n:])   # V untouched
    assert torch.equal(y[::L], x[::L]) and torch.equal(dx[::L], dy[::L])           # position 0
    assert not torch.equal(y[1::L, :n], x[1::L, :n])
    assert _rel(y[:, :n], ref[:, :n]) <= ONE_ROUNDING
    assert _rel(dx[:, :n], xd.grad[:, :n]) <= ONE_ROUNDING


@pytest.mark.parametrize("T_,I", [(5, 8), (33, 520), (300, 1536)])
def test_swiglu_fwd_bwd(T_, I):
    from kubeml_amd.ops import transformer as T
    g = torch.Generator(device=dev).manual_seed(I)
    gu, dh = _randn(g, T_, 2 * I, scale=8.0), _randn(g, T_, I)
    if T_ * I > 100000:
        assert gu[:, :I].float().abs().max() > 30   # the tails of both signs are in the input
    h = T.swiglu_fwd(gu)
    dgu = T.swiglu_bwd(dh, gu)
    x = gu.double().requires_grad_(True)
    ref = torch.nn.functional.silu(x[:, :I]) * x[:, I:]
    ref.backward(dh.double())
    assert torch.isfinite(h.float()).all() and torch.isfinite(dgu.float()).all()
    errs = (_rel(h, ref), _rel(dgu[:, :I], x.grad[:, :I]), _rel(dgu[:, I:], x.grad[:, I:]))
    print("h, dgate, dup", errs)
    assert max(errs) <= ONE_ROUNDING


def _gqa_inputs(B, H, Hkv, L, use_bias, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = _randn(g, B * L, (H + 2 * Hkv) * 64, scale=0.5)
    dout = _randn(g, B * L, H * 64)
    bias = None
    if use_bias:
        keep = torch.rand(B, L, device=dev, generator=g) > 0.2
        keep[:, 0] = True
        bias = torch.where(keep, 0.0, -10000.0).float().contiguous()
    return qkv, dout, bias


def _run(qkv, dout, bias, B, H, Hkv, L, causal, drop=None, kv_heads="same", keep_bits=True):
    """kernel forward + backward on a fused [B*L, (H + 2 Hkv)*64] buffer: out, lse, dq, dk, dv
    (keep_bits False: no keep buffer, the backward re-hashes the dropout mask)"""
    from kubeml_amd.nn.transformer import _split_qkv
    from kubeml_amd.ops import transformer as T
    kvh = Hkv if kv_heads == "same" else kv_heads
    q, k, v = _split_qkv(qkv, H, Hkv)
    kb = T.attn_keep_buffer(B, H, L, qkv.device) if drop is not None and keep_bits else None
    out, lse = T.attn_fwd(q, k, v, B, H, L, bias=bias, drop=drop, keep=kb, causal=causal, kv_heads=kvh)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = _split_qkv(dqkv, H, Hkv)
    T.attn_bwd(q, k, v, out, dout, lse, B, H, L, bias=bias, dq=dq, dk=dk, dv=dv, drop=drop, keep=kb, causal=causal,
               kv_heads=kvh)
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv", [(2, 4, 2), (1, 3, 1)])
@pytest.mark.parametrize("L", [7, 64, 100, 192, 300])
def test_gqa_attention_vs_fp32(L, B, H, Hkv, causal):
    from kubeml_amd.nn.transformer import _split_qkv, attention_reference
    qkv, dout, bias = _gqa_inputs(B, H, Hkv, L, use_bias=(B, H, Hkv) == (2, 4, 2), seed=L)
    out, _, dq, dk, dv = _run(qkv, dout, bias, B, H, Hkv, L, causal)
    x = qkv.float().clone().requires_grad_(True)
    ref = attention_reference(x, B, H, L, bias, causal=causal, kv_heads=Hkv)   # repeat_interleave of K/V heads
    ref.backward(dout.float())
    rq, rk, rv = _split_qkv(x.grad, H, Hkv)   # autograd sums each group's gradient into its K/V head
    assert dk.shape[1] == Hkv * 64 and dv.shape[1] == Hkv * 64
    errs = {"out": _rel(out, ref), "dq": _rel(dq, rq), "dk": _rel(dk, rk), "dv": _rel(dv, rv)}
    print(errs)
    for n, e in errs.items():
        assert e < WHOLE[n], (n, e)


@pytest.mark.parametrize("keep_bits", [True, False])
def test_gqa_matches_expanded_mha_with_dropout(keep_bits):
    """the twin: the existing MHA kernels on K/V columns repeated per query head, same dropout
    (the forward's keep bits, or the backward re-hashing the mask per query head)"""
    B, H, Hkv, L, G = 2, 4, 2, 192, 2
    qkv, dout, bias = _gqa_inputs(B, H, Hkv, L, True, seed=11)
    ctr = torch.tensor([3.0, 5.0], device=dev)
    drop = (ctr, 77, 0.1)
    out, lse, dq, dk, dv = _run(qkv, dout, bias, B, H, Hkv, L, True, drop=drop, keep_bits=keep_bits)
    out2, lse2, dq2, dk2, dv2 = _run(qkv, dout, bias, B, H, Hkv, L, True, drop=drop, keep_bits=keep_bits)
    assert all(torch.equal(a, b) for a, b in ((dq, dq2), (dk, dk2), (dv, dv2)))
    D, E = H * 64, Hkv * 64
    rep = lambda t: t.reshape(B * L, Hkv, 64).repeat_interleave(G, dim=1).reshape(B * L, D)
    wide = torch.cat([qkv[:, :D], rep(qkv[:, D:D + E]), rep(qkv[:, D + E:])], 1).contiguous()
    to, tl, tq, tk, tv = _run(wide, dout, bias, B, H, H, L, True, drop=drop, kv_heads=None, keep_bits=keep_bits)
    assert torch.equal(out, to) and torch.equal(lse, tl) and torch.equal(dq, tq)
    fold = lambda t: t.float().reshape(B * L, Hkv, G, 64).sum(2).reshape(B * L, E)
    print("dk", _rel(dk, fold(tk)), "dv", _rel(dv, fold(tv)))
    assert _rel(dk, fold(tk)) < WHOLE["dk"] and _rel(dv, fold(tv)) < WHOLE["dv"]


@pytest.mark.parametrize("causal", [True, False])
def test_gqa_with_one_head_per_group_is_the_old_kernel(causal):
    B, H, L = 2, 2, 100
    qkv, dout, bias = _gqa_inputs(B, H, H, L, True, seed=5)
    new = _run(qkv, dout, bias, B, H, H, L, causal, kv_heads=H)
    old = _run(qkv, dout, bias, B, H, H, L, causal, kv_heads=None)
    assert all(torch.equal(a, b) for a, b in zip(new, old))


def test_gqa_refuses_heads_not_divisible():
    from kubeml_amd.ops import transformer as T
    qkv, _, _ = _gqa_inputs(1, 3, 2, 64, False)
    with pytest.raises(ValueError):
        T.attn_fwd(qkv[:, :192], qkv[:, 192:320], qkv[:, 320:], 1, 3, 64, kv_heads=2)
