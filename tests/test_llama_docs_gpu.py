"""Packed documents through LlamaForCausalLM on the GPU (the band attention kernels, head dim 64 and
128) against the CPU model on the same weights and doc_ids; tests/test_llama_gpu.py's bounds."""
import pytest
import torch

from test_llama_gpu import _rel

pytestmark = pytest.mark.gpu
dev = "cuda"


@pytest.mark.parametrize("kw", [{}, dict(hidden=256, heads=2, kv_heads=1, head_dim=128)])
def test_packed_llama_matches_cpu(kw):
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.nn.transformer import pack_documents
    ref = llama_tiny(**kw).double()
    gpu = llama_tiny(seed=1, **kw)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev)
    flatten_module(gpu)
    g = torch.Generator().manual_seed(0)
    ids, mask, doc = pack_documents([torch.randint(1, 1000, (n,), generator=g) for n in (23, 1, 40, 66)], 70)
    assert ids.shape == (2, 70)   # [23 | 1 | 40 | 6 pad], [66 | 4 pad]
    labels = ids.masked_fill(mask == 0, -100)
    lr = ref(ids, mask, labels=labels, doc_ids=doc)
    lr.backward()
    lg = gpu(ids.to(dev), mask.to(dev), labels=labels.to(dev), doc_ids=doc.to(dev))
    lg.backward()
    print("loss", lg.item(), lr.item())
    assert abs(lg.item() - lr.item()) < 0.02 * abs(lr.item())
    gr = dict(ref.named_parameters())
    for n, p in gpu.named_parameters():
        e = _rel(p.grad.float().cpu(), gr[n].grad)
        assert e < 0.08, (n, e)
    with torch.no_grad():
        zo, zr = gpu.eval()(ids.to(dev), mask.to(dev), doc_ids=doc.to(dev)).float().cpu(), ref.eval()(ids, mask, doc_ids=doc)
    assert zo.shape == (2 * 70, 1000) and _rel(zo, zr) < 0.02
