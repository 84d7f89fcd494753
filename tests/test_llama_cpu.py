"""Llama model on the CPU path: HF state-dict names and shapes, the fused-parameter round trip,
from_hf_config, and the forward against a plain-torch Llama written from the HF formulas."""
import pytest
import torch
import torch.nn.functional as F

CFG = dict(vocab_size=50, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
           head_dim=64, intermediate_size=96, max_position_embeddings=32, rms_norm_eps=1e-6, rope_theta=5e5,
           tie_word_embeddings=True, hidden_act="silu")


def _model(**kw):
    from kubeml_amd.models import LlamaForCausalLM
    return LlamaForCausalLM.from_hf_config(CFG, **kw)


def _hf_shapes():
    out = {"model.embed_tokens.weight": (50, 128)}
    for i in range(2):
        p = f"model.layers.{i}."
        out.update({p + "self_attn.q_proj.weight": (256, 128), p + "self_attn.k_proj.weight": (128, 128),
                    p + "self_attn.v_proj.weight": (128, 128), p + "self_attn.o_proj.weight": (128, 256),
                    p + "mlp.gate_proj.weight": (96, 128), p + "mlp.up_proj.weight": (96, 128),
                    p + "mlp.down_proj.weight": (128, 96), p + "input_layernorm.weight": (128,),
                    p + "post_attention_layernorm.weight": (128,)})
    out.update({"model.norm.weight": (128,), "lm_head.weight": (50, 128)})
    return out


def test_state_dict_has_hf_names_and_round_trips():
    m = _model()
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == _hf_shapes()
    assert list(sd) == list(_hf_shapes())
    m2 = _model(seed=7)
    assert not torch.equal(m2.model.layers[0].self_attn.qkv.weight, m.model.layers[0].self_attn.qkv.weight)
    m2.load_state_dict(sd)
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
    assert m2.lm_head.weight is m2.model.embed_tokens.weight


def test_from_hf_config_maps_fields():
    m = _model()
    att = m.model.layers[1].self_attn
    assert (att.heads, att.kv_heads, m.model.layers[0].mlp.inter, m.model.max_pos) == (4, 2, 96, 32)
    assert m.model.norm.eps == 1e-6 and m.tie_word_embeddings and len(m.model.layers) == 2
    assert torch.allclose(m.model.rope_table[1, 1], torch.cos(torch.tensor(5e5 ** (-1 / 32))))
    assert not _model(tie_word_embeddings=False).tie_word_embeddings


@pytest.mark.parametrize("field,value", [("head_dim", 32), ("hidden_act", "gelu"), ("rope_scaling", {"type": "linear"}),
                                         ("attention_bias", True), ("mlp_bias", True), ("attention_dropout", 0.1)])
def test_from_hf_config_refuses(field, value):
    from kubeml_amd.models import LlamaForCausalLM
    with pytest.raises(ValueError):
        LlamaForCausalLM.from_hf_config({**CFG, field: value})


def _plain_llama(sd, ids, mask, H=4, Hkv=2, eps=1e-6, theta=5e5):
    """HF's modeling_llama formulas (rotate_half, repeat_kv, silu(gate) * up) on the state dict"""
    B, L = ids.shape
    norm = lambda x, w: w * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    rot = lambda x: torch.cat([-x[..., 32:], x[..., :32]], -1)
    inv = 1.0 / theta ** (torch.arange(0, 64, 2, dtype=torch.float64) / 64)
    emb = torch.cat([torch.outer(torch.arange(L, dtype=torch.float64), inv)] * 2, -1)
    cos, sin = emb.cos(), emb.sin()
    add = torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)[None, None] \
        + ((1.0 - mask.double()) * -10000.0)[:, None, None, :]
    h = sd["model.embed_tokens.weight"][ids]
    for i in range(2):
        p = f"model.layers.{i}."
        x = norm(h, sd[p + "input_layernorm.weight"])
        q, k, v = (F.linear(x, sd[p + f"self_attn.{n}_proj.weight"]).view(B, L, -1, 64).transpose(1, 2) for n in "qkv")
        q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
        k, v = (t[:, :, None].expand(B, Hkv, H // Hkv, L, 64).reshape(B, H, L, 64) for t in (k, v))   # repeat_kv
        a = (q @ k.transpose(2, 3) / 8.0 + add).softmax(-1) @ v
        h = h + F.linear(a.transpose(1, 2).reshape(B, L, H * 64), sd[p + "self_attn.o_proj.weight"])
        x = norm(h, sd[p + "post_attention_layernorm.weight"])
        h = h + F.linear(F.silu(F.linear(x, sd[p + "mlp.gate_proj.weight"])) * F.linear(x, sd[p + "mlp.up_proj.weight"]),
                         sd[p + "mlp.down_proj.weight"])
    return F.linear(norm(h, sd["model.norm.weight"]), sd["lm_head.weight"]).reshape(B * L, -1)


def test_cpu_forward_is_the_hf_block():
    m = _model(tie_word_embeddings=False).double()
    with torch.no_grad():   # norm weights away from 1 so that their placement matters
        for n, p in m.named_parameters():
            if "norm" in n:
                p.uniform_(0.5, 1.5)
    # the table is rounded to fp32 once; the plain model's fp64 angles differ from it by <= 2^-24
    ang = torch.outer(torch.arange(32.0, dtype=torch.float64), 5e5 ** (-torch.arange(32, dtype=torch.float64) / 32))
    m.model.rope_table = torch.cat([ang.cos(), ang.sin()], 1)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 50, (2, 19), generator=g)
    mask = torch.ones(2, 19, dtype=torch.int64)
    mask[1, 15:] = 0
    with torch.no_grad():
        ours = m(ids, mask)
        ref = _plain_llama(m.state_dict(), ids, mask)
    assert ours.shape == ref.shape == (38, 50)
    assert (ours - ref).abs().max() < 1e-10
