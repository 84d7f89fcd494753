"""Head dim 128 (csrc/kernels/attention_d128.hip, kml_rope128): the flash attention forward, dQ and
dKV kernels and the rotary embedding against plain torch in fp64 on the same bf16 inputs."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
D = 128
# the project's whole-tensor bounds for this comparison (tests/test_llama_kernels_gpu.py)
WHOLE = {"out": 1e-2, "dq": 3e-2, "dk": 3e-2, "dv": 2e-2}
ONE_ROUNDING = 2.0 ** -8   # one bf16 store (2^-9 per element), a factor 2 for the cancellation in a*c - b*s


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=dev, generator=g) * scale).to(BF)


def _inputs(B, H, Hkv, L, use_bias, seed, qk_std=0.5):
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = _randn(g, B * L, (H + 2 * Hkv) * D, scale=0.5)
    qkv[:, :(H + Hkv) * D] = _randn(g, B * L, (H + Hkv) * D, scale=qk_std)
    dout = _randn(g, B * L, H * D)
    bias = None
    if use_bias:
        keep = torch.rand(B, L, device=dev, generator=g) > 0.2
        keep[:, 0] = True
        bias = torch.where(keep, 0.0, -10000.0).float().contiguous()
    return qkv, dout, bias


def _run(qkv, dout, bias, B, H, Hkv, L, causal):
    """kernel forward + backward in place on the fused buffer and a fused gradient buffer"""
    from kubeml_amd.nn.transformer import _split_qkv
    from kubeml_amd.ops import transformer as T
    q, k, v = _split_qkv(qkv, H, Hkv, D)
    out, lse = T.attn_fwd(q, k, v, B, H, L, bias=bias, causal=causal, kv_heads=Hkv, head_dim=D)
    dq, dk, dv = _split_qkv(torch.empty_like(qkv), H, Hkv, D)
    T.attn_bwd(q, k, v, out, dout, lse, B, H, L, bias=bias, dq=dq, dk=dk, dv=dv, causal=causal, kv_heads=Hkv,
               head_dim=D)
    return {"out": out, "dq": dq, "dk": dk, "dv": dv}


def _reference(x, dout, bias, B, H, Hkv, L, causal, cast=lambda t: t):
    """attention_reference and its autograd gradients with every input through ``cast`` (to fp64:
    the reference; to bf16: torch's own bf16 attention)"""
    from kubeml_amd.nn.transformer import _split_qkv, attention_reference
    x = cast(x).clone().requires_grad_(True)
    ref = attention_reference(x, B, H, L, None if bias is None else cast(bias), causal=causal, kv_heads=Hkv,
                              head_dim=D)
    ref.backward(cast(dout))
    rq, rk, rv = _split_qkv(x.grad, H, Hkv, D)
    return {"out": ref.detach(), "dq": rq, "dk": rk, "dv": rv}


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv", [(2, 4, 2), (1, 3, 1), (1, 2, 2)])
@pytest.mark.parametrize("L", [7, 64, 100, 300])
def test_attention_d128_vs_fp64(L, B, H, Hkv, causal):
    qkv, dout, bias = _inputs(B, H, Hkv, L, use_bias=(B, H, Hkv) == (2, 4, 2), seed=L)
    got = _run(qkv, dout, bias, B, H, Hkv, L, causal)
    ref = _reference(qkv, dout, bias, B, H, Hkv, L, causal, cast=lambda t: t.double())
    assert got["dk"].shape[1] == Hkv * D and got["dv"].shape[1] == Hkv * D
    errs = {n: _rel(got[n], ref[n]) for n in WHOLE}
    print(errs)
    for n, e in errs.items():
        assert e < WHOLE[n], (n, e)
    again = _run(qkv, dout, bias, B, H, Hkv, L, causal)
    assert all(torch.equal(got[n], again[n]) for n in WHOLE)


def test_attention_d128_peaked_softmax():
    """q, k at std 1.5 (scores of std ~2.2 after the scale): at most twice the error of torch's own
    bf16 attention (bf16 matmul inputs, fp32 accumulation), which also rounds P and dS to bf16 once.
    Measured (profiles/r22/attn_d128.md): kernel out / dq / dk / dv 2.1e-3 / 2.9e-3 / 2.8e-3 /
    2.3e-3, torch bf16 8.9e-3 / 8.7e-3 / 8.8e-3 / 9.0e-3."""
    B, H, Hkv, L = 1, 3, 1, 300
    qkv, dout, _ = _inputs(B, H, Hkv, L, False, seed=17, qk_std=1.5)
    got = _run(qkv, dout, None, B, H, Hkv, L, True)
    ref = _reference(qkv, dout, None, B, H, Hkv, L, True, cast=lambda t: t.double())
    low = _reference(qkv, dout, None, B, H, Hkv, L, True, cast=lambda t: t.to(BF))
    for n in WHOLE:
        e, e_bf = _rel(got[n], ref[n]), _rel(low[n], ref[n])
        print(n, "kernel", e, "torch bf16", e_bf)
        assert e <= 2 * e_bf, (n, e, e_bf)


@pytest.mark.parametrize("B,L,H,Hkv,theta", [(2, 7, 2, 1, 1e4), (1, 300, 3, 3, 5e5)])
def test_rope128_fwd_bwd(B, L, H, Hkv, theta):
    from kubeml_amd.nn.transformer import rope_reference, rope_table
    from kubeml_amd.ops import transformer as T
    g = torch.Generator(device=dev).manual_seed(L)
    table = rope_table(L + 3, theta, device=dev, head_dim=D)
    n = (H + Hkv) * D
    x, dy = _randn(g, B * L, n + Hkv * D), _randn(g, B * L, n + Hkv * D)
    xd = x.double().requires_grad_(True)
    ref = rope_reference(xd, table.double(), L, H, Hkv, head_dim=D)
    ref.backward(dy.double())
    y = T.rope_(x.clone(), table, L, H, Hkv)
    dx = T.rope_(dy.clone(), table, L, H, Hkv, backward=True)
    print("fwd", _rel(y[:, :n], ref[:, :n]), "bwd", _rel(dx[:, :n], xd.grad[:, :n]))
    assert torch.equal(y[:, n:], x[:, n:]) and torch.equal(dx[:, n:], dy[:, n:])   # V untouched
    assert torch.equal(y[::L], x[::L]) and torch.equal(dx[::L], dy[::L])           # position 0
    assert not torch.equal(y[1::L, :n], x[1::L, :n])
    assert _rel(y[:, :n], ref[:, :n]) <= ONE_ROUNDING
    assert _rel(dx[:, :n], xd.grad[:, :n]) <= ONE_ROUNDING


def test_d128_refusals():
    from kubeml_amd.nn.transformer import _split_qkv
    from kubeml_amd.ops import transformer as T
    qkv, _, _ = _inputs(1, 2, 2, 64, False, seed=1)
    q, k, v = _split_qkv(qkv, 2, 2, D)
    ctr = torch.tensor([3.0, 5.0], device=dev)
    with pytest.raises(ValueError):
        T.attn_fwd(q, k, v, 1, 2, 64, drop=(ctr, 77, 0.1), kv_heads=2, head_dim=D)
    with pytest.raises(ValueError):
        T.attn_fwd(q, k, v, 1, 2, 64, kv_heads=2, head_dim=96)
