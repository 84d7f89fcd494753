"""Llama decoder LM on the MI355X kernels vs the same modules' fp64 CPU path (tied and untied
head); model-level causality; a graph-captured AdamW loop."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _fp64_pair(tie):
    """llama_tiny at B = 2, L = 128, the last 5 positions of row 0 masked: (loss, grads, eval
    logits) of the fp64 CPU path and of the GPU kernels, from the same state dict"""
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import flatten_module
    ref = llama_tiny(tie_word_embeddings=tie).double()
    gpu = llama_tiny(tie_word_embeddings=tie, seed=1)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev)
    flatten_module(gpu)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 1000, (2, 128), generator=g)
    mask = torch.ones(2, 128, dtype=torch.int64)
    mask[0, 123:] = 0
    ref.train()
    gpu.train()
    lr = ref(ids, mask, labels=ids)
    lr.backward()
    lg = gpu(ids.to(dev), mask.to(dev), labels=ids.to(dev))
    lg.backward()
    gr = {n: p.grad.clone() for n, p in ref.named_parameters()}
    gg = {n: p.grad.float().cpu().clone() for n, p in gpu.named_parameters()}
    gpu.eval()
    ref.eval()
    with torch.no_grad():
        zo = gpu(ids.to(dev), mask.to(dev)).float().cpu()
        zr = ref(ids, mask)
    return (lr.item(), gr, zr), (lg.item(), gg, zo)


@pytest.mark.parametrize("tie", [False, True])
def test_llama_tiny_matches_fp64(tie):
    (lr, gr, zr), (lg, gg, zo) = _fp64_pair(tie)
    print("loss", lg, lr)
    assert abs(lg - lr) < 0.02 * abs(lr)
    assert set(gg) == set(gr) and ("lm_head.weight" in gg) == (not tie)
    print("worst gradient", max((_rel(gg[n], gr[n]), n) for n in gg), "logits", _rel(zo, zr))
    for n in gg:
        e = _rel(gg[n], gr[n])
        assert e < 0.08, (n, e)
    assert zo.shape == (2 * 128, 1000)
    assert _rel(zo, zr) < 0.02


def test_model_is_causal_bit_for_bit():
    """eval mode, L = 128: changing ids[:, 70:] leaves the logits of positions < 70 bit-identical"""
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import flatten_module
    m = llama_tiny().to(dev)
    flatten_module(m)
    m.eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 1000, (2, 128), generator=g).to(dev)
    ids2 = ids.clone()
    ids2[:, 70:] = torch.randint(0, 1000, (2, 58), generator=g).to(dev)
    with torch.no_grad():
        a = m(ids).view(2, 128, -1)
        b = m(ids2).view(2, 128, -1)
    assert torch.equal(a[:, :70], b[:, :70])
    assert not torch.equal(a[:, 70:], b[:, 70:])


def test_llama_tiny_graphed_adamw_learns():
    """tests/test_gpt_gpu.py's route and bound: the captured step starts at the untrained loss
    and halves it in 60 replays on one batch"""
    from kubeml_amd.engine.step import GraphedTrainStep, train_state_tensors
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    m = llama_tiny().to(dev)
    sp = flatten_module(m)
    m.train()
    opt = AdamW(m.parameters(), lr=2e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, 1000, (4, 128), generator=g).to(dev)

    def fb():
        sp.zero_grad()
        loss = m(ids, labels=ids)
        loss.backward()
        return loss
    step = GraphedTrainStep(fb, opt.step, warmup=2, state_tensors=train_state_tensors(m, sp, opt))
    step.capture()
    first = None
    for i in range(60):
        l = step()
        if i == 0:
            first = float(l.detach())
    last = float(l.detach())
    print("first", first, "last", last)
    assert first > 0.9 * math.log(1000) and last < 0.5 * first, (first, last)
