"""The tanh-approximated GELU (HF ``gelu_new``) on the CPU path: the power of the elementwise
bound the GPU tests use, ``Linear(act="gelu_tanh")`` / ``nn.GELU(approximate="tanh")`` against
``F.gelu(approximate="tanh")`` in fp64, ``GPT2LMHeadModel.from_hf_config`` against HuggingFace's
own model, its refusals, and greedy ``generate`` with prompt lookup on a tanh model.

The bound, for a bf16 result y and the fp64 reference r: ``|y - r| <= 2^-7 |r| + 2^-20`` — bf16
rounding is <= 2^-8 relative, an fp32 evaluation adds ~1e-6, and the absolute term covers the far
negative tail, where the fp64 tanh form saturates to exactly 0."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

BF = torch.bfloat16


def all_finite_bf16():
    """every finite bf16 value (65 280 of them), as a bf16 tensor"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits.to(torch.int16).view(BF)


def violations(y, r):
    """number of elements of y outside |y - r| <= 2^-7 |r| + 2^-20 (r fp64); a NaN counts"""
    err = (y.double() - r).abs()
    return int((~(err <= 2.0 ** -7 * r.abs() + 2.0 ** -20)).sum())


def ref_fwd(x):
    return F.gelu(x.double(), approximate="tanh")


def ref_grad(x):
    xd = x.double().requires_grad_(True)
    F.gelu(xd, approximate="tanh").sum().backward()
    return xd.grad


def test_the_bound_passes_the_fp32_sigmoid_form_and_refuses_erf():
    x = all_finite_bf16()
    assert x.numel() == 65280
    r, rg = ref_fwd(x), ref_grad(x)
    # the sigmoid form in fp32: x s, s = sigmoid(2u); s + x s (1 - s) 2 sqrt(2/pi) (1 + 0.134145 x^2)
    x32 = x.float()
    xc = x32.clamp(-12.0, 12.0)
    k = math.sqrt(2.0 / math.pi)
    s = torch.sigmoid(2.0 * k * (xc + 0.044715 * xc ** 3))
    y32 = x32 * s
    g32 = s + x32 * s * (1.0 - s) * (2.0 * k) * (1.0 + 0.134145 * xc * xc)
    assert torch.isfinite(y32).all() and torch.isfinite(g32).all()
    nf, ng = violations(y32.to(BF), r), violations(g32.to(BF), rg)
    # erf GELU, the wrong function: it must be caught
    xe = x.float().requires_grad_(True)
    ye = F.gelu(xe)
    ye.sum().backward()
    ef, eg = violations(ye.detach().to(BF), r), violations(xe.grad.to(BF), rg)
    print(f"violations: sigmoid form fwd {nf} grad {ng}; erf fwd {ef} grad {eg}")
    assert nf == 0 and ng == 0
    assert ef >= 100 and eg >= 100


def test_linear_and_gelu_module_equal_torch_tanh_gelu_in_fp64():
    from kubeml_amd.nn import Linear
    from kubeml_amd.nn.transformer import GELU
    torch.manual_seed(0)
    lin = Linear(24, 40).double()
    x = (3.0 * torch.randn(7, 24, dtype=torch.float64)).requires_grad_(True)
    y = lin(x, act="gelu_tanh")
    want = F.gelu(F.linear(x, lin.weight, lin.bias), approximate="tanh")
    assert torch.equal(y, want)
    dy = torch.randn_like(y)
    got = torch.autograd.grad(y, [x, lin.weight, lin.bias], dy)
    ref = torch.autograd.grad(want, [x, lin.weight, lin.bias], dy)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # it is not the erf form
    assert (y - lin(x, act="gelu")).abs().max().item() > 1e-4
    z = (3.0 * torch.randn(5, 33, dtype=torch.float64)).requires_grad_(True)
    act = GELU(approximate="tanh")
    out, want = act(z), F.gelu(z, approximate="tanh")
    assert torch.equal(out, want)
    dz = torch.randn_like(out)
    assert torch.equal(torch.autograd.grad(out, z, dz)[0], torch.autograd.grad(want, z, dz)[0])
    assert torch.equal(GELU()(z), F.gelu(z)) and torch.equal(GELU("none")(z), F.gelu(z))
    with pytest.raises(ValueError):
        GELU(approximate="sigmoid")


def _hf_config(tr, **kw):
    cfg = dict(vocab_size=211, n_positions=64, n_embd=128, n_layer=2, n_head=2, n_inner=256,
               activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
               layer_norm_epsilon=1e-5)
    cfg.update(kw)
    return tr.GPT2Config(**cfg)


def test_from_hf_config_reproduces_huggingface_gelu_new_logits():
    tr = pytest.importorskip("transformers")
    from kubeml_amd.models.gpt import GPT2LMHeadModel
    cfg = _hf_config(tr)
    torch.manual_seed(0)
    hf = tr.GPT2LMHeadModel(cfg).double().eval()
    for p in hf.parameters():   # the default init leaves biases at 0 and LayerNorm at identity
        if p.dim() == 1:
            p.data.add_(0.1 * torch.randn_like(p))
    ours = GPT2LMHeadModel.from_hf_config(cfg).double().eval()
    assert ours.activation == "gelu_tanh" and ours.transformer.h[0].mlp.activation == "gelu_tanh"
    ours.load_state_dict(hf.state_dict())
    erf = GPT2LMHeadModel(vocab=211, hidden=128, layers=2, heads=2, inter=256, max_pos=64, eps=1e-5, dropout=0.0,
                          activation="gelu").double().eval()
    erf.load_state_dict(hf.state_dict())
    B, L = 2, 33
    ids = torch.randint(0, 211, (B, L))
    mask = torch.ones(B, L, dtype=torch.int64)
    with torch.no_grad():
        ref = hf(ids).logits.reshape(B * L, -1)
        got = ours(ids)
        assert (got - ref).abs().max().item() < 1e-8
        # the same weights behind the erf GELU are another model: the comparison sees the activation
        assert (erf(ids) - ref).abs().max().item() > 1e-6
        mask[1, L - 6:] = 0   # right padding: the logits of the real positions do not move
        got_m = ours(ids, attention_mask=mask).view(B, L, -1)
        ref_m = hf(ids, attention_mask=mask).logits
        assert (got_m[0] - ref_m[0]).abs().max().item() < 1e-8
        assert (got_m[1, :L - 6] - ref_m[1, :L - 6]).abs().max().item() < 1e-8


BASE = dict(vocab_size=97, n_positions=32, n_embd=64, n_layer=1, n_head=1, n_inner=None,
            activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
            layer_norm_epsilon=1e-6)


def test_from_hf_config_dict_path_and_n_inner(tmp_path):
    from kubeml_amd.models.gpt import GPT2LMHeadModel
    m = GPT2LMHeadModel.from_hf_config(BASE)
    tr = m.transformer
    assert m.activation == "gelu_tanh" and m.vocab == 97 and tr.max_pos == 32 and len(tr.h) == 1
    assert tr.h[0].mlp.c_fc.out_features == 256 and tr.h[0].mlp.c_fc.in_features == 64   # n_inner None: 4 n_embd
    assert tr.h[0].attn.heads == 1 and tr.ln_f.eps == 1e-6 and tr.h[0].drop1.p == 0.0
    # extra keys of a real config.json are ignored; the path form reads the same thing
    path = tmp_path / "config.json"
    path.write_text(json.dumps(dict(BASE, model_type="gpt2", architectures=["GPT2LMHeadModel"], n_inner=128,
                                    activation_function="gelu_pytorch_tanh", resid_pdrop=0.1, embd_pdrop=0.1,
                                    attn_pdrop=0.1)))
    for cfg in (str(path), path):
        m2 = GPT2LMHeadModel.from_hf_config(cfg)
        assert m2.activation == "gelu_tanh" and m2.transformer.h[0].mlp.c_fc.out_features == 128
        assert m2.transformer.h[0].drop1.p == 0.1
    assert GPT2LMHeadModel.from_hf_config(dict(BASE, activation_function="gelu")).activation == "gelu"
    # overrides replace constructor arguments
    m3 = GPT2LMHeadModel.from_hf_config(BASE, activation="gelu", max_pos=16)
    assert m3.activation == "gelu" and m3.transformer.max_pos == 16


@pytest.mark.parametrize("bad", [dict(activation_function="relu"), dict(activation_function="gelu_fast"),
                                 dict(embd_pdrop=0.1), dict(attn_pdrop=0.2),
                                 dict(scale_attn_by_inverse_layer_idx=True), dict(reorder_and_upcast_attn=True)])
def test_from_hf_config_refuses_what_the_model_does_not_implement(bad):
    from kubeml_amd.models.gpt import GPT2LMHeadModel
    with pytest.raises(ValueError):
        GPT2LMHeadModel.from_hf_config(dict(BASE, **bad))


def test_constructor_takes_gelu_tanh_and_names_it_in_the_refusal():
    from kubeml_amd.models.gpt import gpt2_tiny
    assert gpt2_tiny(activation="gelu_tanh").activation == "gelu_tanh"
    assert gpt2_tiny().activation == "gelu"
    with pytest.raises(ValueError, match="gelu_tanh.*from_hf_config"):
        gpt2_tiny(activation="gelu_new")
    with pytest.raises(TypeError):
        type(gpt2_tiny()).from_hf_config(3)


def test_greedy_generate_with_prompt_lookup_on_a_tanh_model():
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    m = gpt2_tiny(dropout=0.0, activation="gelu_tanh").eval()
    g = torch.Generator().manual_seed(5)
    block = torch.randint(1, 1000, (6,), generator=g)
    ids = torch.stack([block.repeat(3), torch.randint(1, 1000, (18,), generator=g)])
    mask = torch.ones_like(ids)
    mask[1, 11:] = 0
    ids = ids * mask
    ref = m.generate(ids, mask, max_new_tokens=12)
    out = m.generate(ids, mask, max_new_tokens=12, prompt_lookup_num_tokens=3)
    assert torch.equal(out, ref)
    torch.manual_seed(0)
    erf = gpt2_tiny(dropout=0.0).eval()   # same weights, erf GELU: other logits
    with torch.no_grad():
        assert (erf(ids[:1]) - m(ids[:1])).abs().max().item() > 0
