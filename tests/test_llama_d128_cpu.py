"""Head-dim-128 Llama on the CPU path: from_hf_config, the HF state-dict round trip, a forward."""
import pytest
import torch

CFG = dict(vocab_size=50, hidden_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
           intermediate_size=96, max_position_embeddings=32, rope_theta=5e5)
H, HKV, D = 2, 1, 128


def _model(cfg=CFG, **kw):
    from kubeml_amd.models import LlamaForCausalLM
    return LlamaForCausalLM.from_hf_config(cfg, **kw)


# explicit head_dim (hidden / heads would be 64), or inferred from hidden 256 / 2 heads
@pytest.mark.parametrize("cfg", [{**CFG, "hidden_size": 128, "head_dim": 128}, CFG])
def test_from_hf_config_accepts_head_dim_128(cfg):
    m = _model(cfg)
    att = m.model.layers[0].self_attn
    assert att.head_dim == D and tuple(att.qkv.weight.shape) == ((H + 2 * HKV) * D, cfg["hidden_size"])
    assert tuple(m.model.rope_table.shape) == (32, D)
    assert torch.allclose(m.model.rope_table[1, 1], torch.cos(torch.tensor(5e5 ** (-1 / 64))))


def test_state_dict_round_trips_through_hf_names():
    m = _model()
    sd = m.state_dict()
    p = "model.layers.1.self_attn."
    assert tuple(sd[p + "q_proj.weight"].shape) == (H * D, 256)
    assert tuple(sd[p + "k_proj.weight"].shape) == tuple(sd[p + "v_proj.weight"].shape) == (HKV * D, 256)
    assert tuple(sd[p + "o_proj.weight"].shape) == (256, H * D)
    m2 = _model(seed=7)
    assert not torch.equal(m2.model.layers[1].self_attn.qkv.weight, m.model.layers[1].self_attn.qkv.weight)
    m2.load_state_dict(sd)
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n


def test_cpu_forward_and_loss_are_finite():
    m = _model()
    ids = torch.randint(0, 50, (2, 19), generator=torch.Generator().manual_seed(2))
    mask = torch.ones(2, 19, dtype=torch.int64)
    mask[1, 15:] = 0
    logits = m(ids, mask)
    assert logits.shape == (38, 50) and torch.isfinite(logits).all()
    loss = m(ids, mask, labels=ids)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(m.model.layers[0].self_attn.qkv.weight.grad).all()
