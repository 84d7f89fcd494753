"""GPT-2 decoder LM on the MI355X kernels vs the same modules' fp64 CPU path; model-level
causality; the tied token table; a graph-captured AdamW loop; the label-shift kernel; the
example function through a server."""
import functools
import math
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _fp64_pair():
    """gpt2_tiny(dropout=0) at B = 2, L = 128: (loss, grads, eval logits) of the fp64 CPU path
    and of the GPU kernels, from the same parameters"""
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    ref = gpt2_tiny(dropout=0.0).double()
    gpu = gpt2_tiny(dropout=0.0)
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
    return (lr.item(), gr, zr), (lg.item(), gg, zo), (ref, gpu)


def test_gpt2_tiny_matches_fp64():
    (lr, gr, zr), (lg, gg, zo), _ = _fp64_pair()
    print("loss", lg, lr)
    assert abs(lg - lr) < 0.02 * abs(lr)
    assert set(gg) == set(gr)
    worst = max((_rel(gg[n], gr[n]), n) for n in gg)
    print("worst gradient", worst, "logits", _rel(zo, zr))
    for n in gg:
        e = _rel(gg[n], gr[n])
        assert e < 0.08, (n, e)
    assert zo.shape == (2 * 128, 1000)
    assert _rel(zo, zr) < 0.02


def test_tied_token_table_gets_both_gradients():
    """lm_head.weight IS the token table; its gradient is the decoder's plus the embedding's
    (the fp64 path sums both through autograd) — either one alone is far off"""
    (_, gr, _), (_, gg, _), (ref, gpu) = _fp64_pair()
    assert gpu.lm_head.weight is gpu.transformer.wte.weight
    assert ref.lm_head.weight is ref.transformer.wte.weight
    names = [n for n, _ in gpu.named_parameters()]
    assert "transformer.wte.weight" in names and "lm_head.weight" not in names
    both = gr["transformer.wte.weight"]
    assert _rel(gg["transformer.wte.weight"], both) < 0.08
    # the embedding's share alone, from the fp64 path with the head's use of the table detached
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 1000, (2, 128), generator=g)
    mask = torch.ones(2, 128, dtype=torch.int64)
    mask[0, 123:] = 0
    ref.train()
    ref.zero_grad()
    z = ref.transformer(ids, mask)
    w = ref.lm_head.weight.detach()
    tgt = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], -100)], 1).reshape(-1)
    torch.nn.functional.cross_entropy((z @ w.t()).float(), tgt, ignore_index=-100).backward()
    emb_only = ref.transformer.wte.weight.grad.clone()
    ref.zero_grad()
    ref.eval()
    dec_only = both - emb_only
    assert _rel(emb_only, both) > 0.2 and _rel(dec_only, both) > 0.2   # both shares matter
    assert _rel(gg["transformer.wte.weight"], emb_only) > 0.2
    assert _rel(gg["transformer.wte.weight"], dec_only) > 0.2


def test_model_is_causal_bit_for_bit():
    """eval mode, L = 192: changing ids[:, 100:] leaves logits[:, :100] bit-identical"""
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    m = gpt2_tiny().to(dev)
    flatten_module(m)
    m.eval()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 1000, (2, 192), generator=g).to(dev)
    ids2 = ids.clone()
    ids2[:, 100:] = torch.randint(0, 1000, (2, 92), generator=g).to(dev)
    with torch.no_grad():
        a = m(ids).view(2, 192, -1)
        b = m(ids2).view(2, 192, -1)
    assert torch.equal(a[:, :100], b[:, :100])
    assert not torch.equal(a[:, 100:], b[:, 100:])


def test_gpt2_tiny_graphed_adamw_learns():
    from kubeml_amd.engine.step import GraphedTrainStep, train_state_tensors
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    torch.manual_seed(0)
    m = gpt2_tiny(dropout=0.1).to(dev)
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
    # the warm-up and capture steps are rolled back (state_tensors), so step 0 below is the
    # first update of the random-init model and its loss the untrained one
    step = GraphedTrainStep(fb, opt.step, warmup=2,
                            state_tensors=train_state_tensors(m, sp, opt, [m.rng.tensor(torch.device(dev, 0))]))
    step.capture()
    first = None
    for i in range(60):
        l = step()
        if i == 0:
            first = float(l.detach())
    last = float(l.detach())
    print("first", first, "last", last)
    assert first > 0.9 * math.log(1000) and last < 0.5 * first, (first, last)


@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (2, 128)])
def test_lm_shift_labels_kernel(B, L):
    from kubeml_amd.ops import transformer as T
    g = torch.Generator().manual_seed(B * 1000 + L)
    ids = torch.randint(0, 50257, (B, L), generator=g).to(dev)
    out = T.lm_shift_labels(ids, -100)
    ref = torch.cat([ids[:, 1:], torch.full_like(ids[:, :1], -100)], 1)
    assert out.dtype == torch.int64 and out.shape == ids.shape
    assert torch.equal(out, ref)
    assert torch.equal(T.lm_shift_labels(ids, -7)[:, -1], torch.full((B,), -7, device=dev))


def _train_function(tmp_path, fn_name, fn_file, ds_name, arrs, batch, epochs, k, lr, workers=1, parallelism=1):
    """Upload ``arrs`` (xtr, ytr, xte, yte) as ``ds_name``, register ``fn_file`` and run
    ``kubeml train`` through the controller; returns (client, job id, history).  The helper of
    tests/test_e2e_gpu.py."""
    from kubeml_amd.api.types import TrainOptions, TrainRequest
    from kubeml_amd.client import KubemlClient
    from kubeml_amd.config import Config
    from kubeml_amd.control.server import KubeMLServer
    cfg = Config()
    cfg.store_dir = str(tmp_path / "store")
    srv = KubeMLServer(cfg, n_workers=workers, use_gpu=True, task_timeout=600).start(
        ports={k_: 0 for k_ in ("controller", "scheduler", "ps", "storage", "metrics")})
    try:
        c = KubemlClient(srv.url())
        paths = {}
        for key, v in arrs.items():
            paths[key] = str(tmp_path / f"{key}.npy")
            np.save(paths[key], v)
        c.datasets.create(ds_name, paths["xtr"], paths["ytr"], paths["xte"], paths["yte"])
        c.functions.create(fn_name, os.path.join(ROOT, "examples", fn_file))
        jid = c.networks.train(TrainRequest(batch_size=batch, epochs=epochs, dataset=ds_name, lr=lr,
                                            function_name=fn_name,
                                            options=TrainOptions(default_parallelism=parallelism,
                                                                 static_parallelism=True, validate_every=1, k=k)))
        t0 = time.time()
        while c.tasks.status(jid)["state"] == "running":
            assert time.time() - t0 < 600
            time.sleep(0.5)
        st = c.tasks.status(jid)
        assert st["state"] == "finished", (st, c.logs(jid).decode()[-3000:])
        return c, jid, c.histories.get(jid).data
    finally:
        srv.stop()


def test_gpt2_function_on_gpu_worker(tmp_path, monkeypatch):
    """examples/function_gpt2.py (tiny preset) through the controller on one GPU worker"""
    monkeypatch.setenv("KUBEML_GPT2_PRESET", "tiny")
    rng = np.random.default_rng(4)
    L = 64
    arrs = {"xtr": rng.integers(0, 1000, (64, L)).astype(np.int64),
            "ytr": np.zeros(64, dtype=np.int64),
            "xte": rng.integers(0, 1000, (32, L)).astype(np.int64),
            "yte": np.zeros(32, dtype=np.int64)}
    _, _, h = _train_function(tmp_path, "gpt2", "function_gpt2.py", "lm_tokens", arrs, batch=16, epochs=2, k=-1,
                              lr=1e-4)
    print("train loss", h.train_loss, "accuracy", h.accuracy)
    assert len(h.train_loss) == 2 and all(np.isfinite(h.train_loss))
    # random init (weights of std 0.02, hidden 128: logits of std ~0.23) puts the loss within a few
    # hundredths of ln(1000) = 6.91, and four AdamW steps at lr 1e-4 barely move it
    assert abs(h.train_loss[0] - math.log(1000)) < 0.3
    assert len(h.accuracy) == 2 and all(0 <= a <= 100 for a in h.accuracy)
