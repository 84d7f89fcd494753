"""A head-dim-128 Llama (from_hf_config) on the MI355X kernels against the same model's fp64 CPU
path, with tests/test_llama_gpu.py's comparison and bounds; decoding is refused."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
CFG = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=64,
           vocab_size=96, num_hidden_layers=2, max_position_embeddings=128, rms_norm_eps=1e-5)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _models():
    from kubeml_amd.models.llama import LlamaForCausalLM
    from kubeml_amd.nn import flatten_module
    ref = LlamaForCausalLM.from_hf_config(CFG).double()
    gpu = LlamaForCausalLM.from_hf_config(CFG, seed=1)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev)
    flatten_module(gpu)
    return ref, gpu


def test_llama_d128_matches_fp64():
    ref, gpu = _models()
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 96, (2, 70), generator=g)
    mask = torch.ones(2, 70, dtype=torch.int64)
    mask[0, 61:] = 0
    ref.train()
    gpu.train()
    lr = ref(ids, mask, labels=ids)
    lr.backward()
    lg = gpu(ids.to(dev), mask.to(dev), labels=ids.to(dev))
    lg.backward()
    print("loss", lg.item(), lr.item())
    assert abs(lg.item() - lr.item()) < 0.02 * abs(lr.item())
    gr = {n: p.grad for n, p in ref.named_parameters()}
    gg = {n: p.grad.float().cpu() for n, p in gpu.named_parameters()}
    assert set(gg) == set(gr)
    print("worst gradient", max((_rel(gg[n], gr[n]), n) for n in gg))
    for n in gg:   # model.layers.0.self_attn.qkv.weight among them
        assert _rel(gg[n], gr[n]) < 0.08, (n, _rel(gg[n], gr[n]))
    gpu.eval()
    ref.eval()
    with torch.no_grad():
        zo = gpu(ids.to(dev), mask.to(dev)).float().cpu()
        zr = ref(ids, mask)
    assert zo.shape == (2 * 70, 96)
    assert _rel(zo, zr) < 0.02


def test_llama_d128_generate_is_refused():
    _, gpu = _models()
    with pytest.raises(NotImplementedError):
        gpu.generate(torch.zeros(1, 4, dtype=torch.int64, device=dev), max_new_tokens=2)
