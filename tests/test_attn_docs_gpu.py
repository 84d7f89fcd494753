"""The band attention kernels (key_start: packed documents, windows) at head dim 64 and 128 against
attention_reference(key_start=...) in fp64 on the same bf16 inputs, per document / 64-row block."""
import pytest
import torch

from test_attn_d128_gpu import WHOLE, _randn

pytestmark = pytest.mark.gpu
dev = "cuda"
DOCS = [1, 37, 64, 95, 3, 100]   # L = 300: a one-token document, a boundary on a tile edge, one over 3 blocks
CASES = [(2, 4, 2), (1, 3, 1), (1, 2, 2)]


def _layout(name):
    """(key_start [L], the row segments errors are measured on)"""
    if name == "window":   # of 40 keys: leading tiles skipped, nearly every row cut inside a tile
        return (torch.arange(300) - 39).clamp(min=0).int(), [(a, min(a + 64, 300)) for a in range(0, 300, 64)]
    lens = {"docs": DOCS, "tiny": [3, 4], "tiny2": [5, 2]}[name]
    s = torch.tensor([0] + lens[:-1]).cumsum(0)
    return torch.repeat_interleave(s, torch.tensor(lens)).int(), [(int(a), int(a) + n) for a, n in zip(s, lens)]


def _seg_err(got, ref, lo, hi):
    """relative norm of the error on rows lo..hi.  The reference dq / dk of a one-token document are
    exactly 0 (softmax of one score); there the error is set against the tensor's norm per row."""
    den = ref[lo:hi].norm() or ref.norm() * ((hi - lo) / ref.shape[0]) ** 0.5
    return ((got[lo:hi].double() - ref[lo:hi]).norm() / den).item()


def _setup(D, B, H, Hkv, name):
    """inputs; the second sequence of B = 2 takes another layout and a key bias with a padded tail"""
    lay = [_layout(name)] + [_layout({"docs": "window", "window": "docs", "tiny": "tiny2"}[name])] * (B - 1)
    L = lay[0][0].numel()
    g = torch.Generator(device=dev).manual_seed(L + D)
    qkv, dout = _randn(g, B * L, (H + 2 * Hkv) * D, scale=0.5), _randn(g, B * L, H * D)
    bias = None
    if B == 2:
        bias = torch.zeros(B, L, device=dev)
        bias[1, L - max(2, L // 10):] = -10000.0
    return qkv, dout, bias, torch.stack([k for k, _ in lay]).to(dev).contiguous(), [s for _, s in lay], L


def _run(D, qkv, dout, bias, ks, B, H, Hkv, L, ref=False):
    from kubeml_amd.nn.transformer import _split_qkv, attention_reference
    from kubeml_amd.ops import transformer as T
    if ref:   # fp64 autograd on the same bf16 values
        x = qkv.double().requires_grad_(True)
        out = attention_reference(x, B, H, L, None if bias is None else bias.double(), causal=True, kv_heads=Hkv,
                                  head_dim=D, key_start=ks)
        out.backward(dout.double())
        return dict(zip(("out", "dq", "dk", "dv"), (out.detach(), *_split_qkv(x.grad, H, Hkv, D))))
    q, k, v = _split_qkv(qkv, H, Hkv, D)
    out, lse = T.attn_fwd(q, k, v, B, H, L, bias=bias, causal=True, kv_heads=Hkv, head_dim=D, key_start=ks)
    dq, dk, dv = _split_qkv(torch.empty_like(qkv), H, Hkv, D)
    T.attn_bwd(q, k, v, out, dout, lse, B, H, L, bias=bias, dq=dq, dk=dk, dv=dv, causal=True, kv_heads=Hkv,
               head_dim=D, key_start=ks)
    return {"out": out, "dq": dq, "dk": dk, "dv": dv}


@pytest.mark.parametrize("name", ["docs", "window", "tiny"])
@pytest.mark.parametrize("B,H,Hkv", CASES)
@pytest.mark.parametrize("D", [64, 128])
def test_band_attention_vs_fp64(D, B, H, Hkv, name):
    qkv, dout, bias, ks, segs, L = _setup(D, B, H, Hkv, name)
    got, ref = _run(D, qkv, dout, bias, ks, B, H, Hkv, L), _run(D, qkv, dout, bias, ks, B, H, Hkv, L, ref=True)
    worst = {n: max(_seg_err(got[n], ref[n], b * L + lo, b * L + hi) for b in range(B) for lo, hi in segs[b])
             for n in WHOLE}
    print(worst)
    for n, e in worst.items():
        assert e < WHOLE[n], (n, e)
    again = _run(D, qkv, dout, bias, ks, B, H, Hkv, L)
    assert all(torch.equal(got[n], again[n]) for n in WHOLE)


@pytest.mark.parametrize("B,H,Hkv", CASES)
@pytest.mark.parametrize("D", [64, 128])
def test_documents_are_isolated_bit_for_bit(D, B, H, Hkv):
    """new Q, K, V and dout rows in document 3 (rows 102..196) change no bit of any other document"""
    qkv, dout, bias, ks, _, L = _setup(D, B, H, Hkv, "docs")
    ks = ks[:1].repeat(B, 1)
    a = _run(D, qkv, dout, bias, ks, B, H, Hkv, L)
    t = torch.arange(B * L, device=dev) % L
    rows = (t >= 102) & (t < 197)
    g = torch.Generator(device=dev).manual_seed(9)
    qkv[rows], dout[rows] = _randn(g, B * 95, qkv.shape[1], scale=0.5), _randn(g, B * 95, dout.shape[1])
    b = _run(D, qkv, dout, bias, ks, B, H, Hkv, L)
    for n in WHOLE:
        assert torch.equal(a[n][~rows], b[n][~rows]) and not torch.equal(a[n][rows], b[n][rows]), n


@pytest.mark.parametrize("B,H,Hkv", CASES)
@pytest.mark.parametrize("D", [64, 128])
def test_zero_key_start_changes_nothing(D, B, H, Hkv):
    qkv, dout, bias, ks, _, L = _setup(D, B, H, Hkv, "docs")
    a = _run(D, qkv, dout, bias, torch.zeros_like(ks), B, H, Hkv, L)
    b = _run(D, qkv, dout, bias, None, B, H, Hkv, L)
    assert all(torch.equal(a[n], b[n]) for n in WHOLE)


def test_key_start_refusals():
    from kubeml_amd.nn.transformer import _split_qkv
    from kubeml_amd.ops import transformer as T
    qkv, _, _, ks, _, L = _setup(64, 1, 2, 2, "tiny")
    q, k, v = _split_qkv(qkv, 2, 2, 64)
    ctr = torch.tensor([3.0, 5.0], device=dev)
    for kw in (dict(causal=False, key_start=ks), dict(causal=True, key_start=ks, drop=(ctr, 7, 0.1)),
               dict(causal=True, key_start=ks[:, :6].contiguous()), dict(causal=True, key_start=ks.long())):
        with pytest.raises(ValueError):
            T.attn_fwd(q, k, v, 1, 2, L, kv_heads=2, **kw)
