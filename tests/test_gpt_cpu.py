"""GPT-2 decoder LM on the CPU path: causal attention reference, label shift, HuggingFace
state-dict names and logits.  Runs without a device."""
import pytest
import torch
import torch.nn.functional as F


def _tiny(**kw):
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    return gpt2_tiny(**kw)


@pytest.mark.parametrize("use_bias", [False, True])
def test_causal_reference_matches_sdpa(use_bias):
    from kubeml_amd.nn.transformer import attention_reference
    torch.manual_seed(0)
    B, H, L = 2, 3, 37
    D = H * 64
    qkv = torch.randn(B * L, 3 * D, dtype=torch.float64)
    bias = None
    mask = torch.ones(L, L, dtype=torch.bool).tril()[None, None]
    if use_bias:
        keep = torch.rand(B, L) > 0.3
        keep[:, 0] = True
        bias = torch.where(keep, 0.0, -10000.0).double()
        mask = mask & keep.view(B, 1, 1, L)
    out = attention_reference(qkv, B, H, L, bias, causal=True)
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, L, H, 64).permute(0, 2, 1, 3) for i in range(3))
    if use_bias:
        ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    else:
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=True)
    ref = ref.permute(0, 2, 1, 3).reshape(B * L, D)
    assert (out - ref).abs().max().item() < 1e-10
    # the non-causal reference is untouched by the new keyword
    assert torch.equal(attention_reference(qkv, B, H, L, bias), attention_reference(qkv, B, H, L, bias, causal=False))
    assert not torch.equal(out, attention_reference(qkv, B, H, L, bias))


def test_shifted_loss_and_state_dict_round_trip():
    m = _tiny(dropout=0.0).double().eval()
    B, L, V = 3, 19, 1000
    ids = torch.randint(0, V, (B, L))
    with torch.no_grad():
        logits = m(ids)
        loss, correct = m(ids, labels=ids, return_correct=True)
    assert logits.shape == (B * L, V)
    lg = logits.view(B, L, V)
    ref = F.cross_entropy(lg[:, :-1].reshape(-1, V), ids[:, 1:].reshape(-1))
    # the CPU cross-entropy path evaluates the loss in fp32 (nn/modules.py): a few ulps of ~6.9
    assert abs(loss.item() - ref.item()) < 1e-5
    assert int(correct) == int((lg[:, :-1].argmax(-1) == ids[:, 1:]).sum())
    sd = m.state_dict()
    want = {"transformer.wte.weight", "transformer.wpe.weight", "transformer.ln_f.weight", "transformer.ln_f.bias",
            "lm_head.weight"}
    for i in range(2):
        for n in ("ln_1", "ln_2", "attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj"):
            want |= {f"transformer.h.{i}.{n}.weight", f"transformer.h.{i}.{n}.bias"}
    assert set(sd) == want
    # HF Conv1D layout: [in, out]
    assert tuple(sd["transformer.h.0.attn.c_attn.weight"].shape) == (128, 384)
    assert tuple(sd["transformer.h.0.mlp.c_fc.weight"].shape) == (128, 512)
    assert tuple(sd["transformer.h.0.mlp.c_proj.weight"].shape) == (512, 128)
    assert m.lm_head.weight is m.transformer.wte.weight
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(1)
    m2 = gpt2_tiny(dropout=0.0).double().eval()
    m2.load_state_dict({k: v.clone() for k, v in sd.items()})
    sd2 = m2.state_dict()
    for k in sd:
        assert torch.equal(sd[k], sd2[k]), k
    with torch.no_grad():
        assert torch.equal(m2(ids), logits)


def test_logits_match_huggingface():
    tr = pytest.importorskip("transformers")
    from kubeml_amd.models.gpt import GPT2LMHeadModel
    cfg = tr.GPT2Config(vocab_size=211, n_positions=64, n_embd=128, n_layer=2, n_head=2, n_inner=256,
                        activation_function="gelu", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                        layer_norm_epsilon=1e-5)
    torch.manual_seed(0)
    hf = tr.GPT2LMHeadModel(cfg).double().eval()
    for p in hf.parameters():   # the default init leaves biases at 0 and LayerNorm at identity
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn_like(p))
    ours = GPT2LMHeadModel(vocab=211, hidden=128, layers=2, heads=2, inter=256, max_pos=64, eps=1e-5,
                           dropout=0.0).double().eval()
    ours.load_state_dict(hf.state_dict())
    B, L = 2, 33
    ids = torch.randint(0, 211, (B, L))
    mask = torch.ones(B, L, dtype=torch.int64)
    with torch.no_grad():
        ref = hf(ids).logits.reshape(B * L, -1)
        got = ours(ids)
        assert (got - ref).abs().max().item() < 1e-8
        mask[1, L - 6:] = 0   # right padding: the logits of the real positions do not move
        got_m = ours(ids, attention_mask=mask).view(B, L, -1)
        ref_m = hf(ids, attention_mask=mask).logits
        assert (got_m[0] - ref_m[0]).abs().max().item() < 1e-8
        assert (got_m[1, :L - 6] - ref_m[1, :L - 6]).abs().max().item() < 1e-8


def test_activation_other_than_erf_gelu_is_refused():
    from kubeml_amd.models.gpt import GPT2LMHeadModel, gpt2_tiny
    with pytest.raises(ValueError):
        gpt2_tiny(activation="gelu_new")
    with pytest.raises(ValueError):
        GPT2LMHeadModel(vocab=100, hidden=64, layers=1, heads=1, inter=128, max_pos=16, activation="relu")


def test_add_norm_cpu_matches_composition():
    """LayerNorm.add_norm on the CPU path: (LN(x + r), x + r), gradients through both outputs."""
    from kubeml_amd.nn.transformer import LayerNorm
    torch.manual_seed(0)
    ln = LayerNorm(32, eps=1e-5).double()
    x = torch.randn(5, 32, dtype=torch.float64, requires_grad=True)
    r = torch.randn(5, 32, dtype=torch.float64, requires_grad=True)
    y, s = ln.add_norm(x, residual=r)
    assert torch.equal(s, x + r)
    assert torch.allclose(y, F.layer_norm(x + r, (32,), ln.weight, ln.bias, 1e-5))
    y0, s0 = ln.add_norm(x)
    assert s0 is x and torch.allclose(y0, ln(x))
