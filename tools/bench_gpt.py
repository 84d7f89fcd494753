"""GPT-2 small causal-LM training throughput on MI355X (not the headline bench — see
bench.py).  Synthetic token batches of the real shape (there is no network for a corpus),
random-init GPT-2 small (124 M params, tied LM head), fused AdamW, bf16 compute, fp32 master
weights, hidden + attention-probability dropout 0.1, every position scored against the next
token (label shift on the device), the whole step captured as one hipGraph.  Attention is the
causal flash-attention kernel (csrc/kernels/attention.hip); every GEMM, the 50257-way tied
decoder included, runs on csrc/kernels/gemm.hip or the tile ops/gemm_tuning.json names.

    python tools/bench_gpt.py [--batch 16] [--seq 1024] [--steps 20] [--warmup 3] [--layers 12]
                              [--activation gelu|gelu_tanh]
Prints one JSON line (tokens/s over all processed tokens).  Single GPU: the model has no
``stages()`` for backward-overlapped gradient exchange yet.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--activation", choices=("gelu", "gelu_tanh"), default="gelu",
                    help="FFN activation: the erf GELU or the tanh approximation of the released checkpoints")
    a = ap.parse_args()

    import torch
    from kubeml_amd.engine.step import GraphedTrainStep
    from kubeml_amd.models.gpt import gpt2_small
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    m = gpt2_small(layers=a.layers, seed=1, activation=a.activation).to(dev)
    sp = flatten_module(m)
    m.train()
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
    B, L, V = a.batch, a.seq, m.vocab
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(0, V, (B, L), device=dev, generator=g)

    def fb():
        sp.zero_grad()
        loss = m(ids, labels=ids)
        loss.backward()
        return loss

    step = GraphedTrainStep(fb, opt.step, use_graph=not a.no_graph, warmup=1)
    step.capture()
    for _ in range(a.warmup):
        loss = step()
    torch.cuda.synchronize()
    first = float(loss.detach())
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "GPT-2 small causal-LM training tokens/s", "value": round(B * L * a.steps / dt, 1),
                      "unit": "tokens/s", "n_gpus": 1, "ms_per_step": round(dt / a.steps * 1e3, 3),
                      "batch_per_gpu": B, "seq": L, "layers": a.layers, "activation": a.activation,
                      "params": sum(p.numel() for p in m.parameters()),
                      "optimizer": "fused AdamW", "dtype": "bf16", "data": "synthetic tokens, random init",
                      "graph": not a.no_graph, "attention": "causal flash attention (attention.hip)",
                      "loss_first_last": [round(first, 4), round(float(loss.detach()), 4)]}), flush=True)


if __name__ == "__main__":
    main()
