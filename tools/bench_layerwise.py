"""Cost of the layer-wise optimizer steps (LAMB / LARS, two launches each) against the one-launch
optimizer of the same recipe family at the same size, alternating in one process.

    python tools/bench_layerwise.py [--rounds 7] [--iters 20] [--out FILE.json]

LAMB against AdamW on the BERT-base flat space, LARS against SGD with momentum on the ResNet-34
flat space: the real layouts (the models are built on the meta device for their parameter shapes,
the buffers hold random values).  Each round times ``iters`` back-to-back launches of every variant
between device events, the variants alternating inside the round; the per-launch time of a variant
is the median over the rounds, its spread the min .. max.  Bytes per parameter (what the algorithm
must move): AdamW 30 (w, g, m, v in; w, m, v and the bf16 shadow out); LAMB 24 in launch 1 (w, g, m,
v in; m, v out) and 18 in launch 2 (w, m, v in; w and the shadow out), 42 together; SGD with
momentum 22; LARS 8 in launch 1 (w, g in) and 22 in launch 2, 30 together.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def space_offsets(module):
    """FlatParamSpace's offsets for ``module`` (reverse registration order, storage shapes, 64-aligned
    regions) without allocating its buffers."""
    from kubeml_amd.nn.flat import ALIGN, _storage_spec
    seen, uniq = set(), []
    for p in module.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            uniq.append(p)
    offsets, dims, off = [], [], 0
    for p in reversed(uniq):
        n = math.prod(_storage_spec(p)[0])
        offsets.append((off, n))
        dims.append(p.ndim)
        off += -(-n // ALIGN) * ALIGN
    return offsets, dims, max(off, ALIGN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from kubeml_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("bench_layerwise: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3          # us per launch

    def layout(make):
        with torch.device("meta"):
            model = make()
        offsets, dims, n = space_offsets(model)
        chunks, ranges = K.layer_tables(offsets, n, dev)
        # the usual recipe: decay and adaptation on the weights, neither on biases / norm weights
        hp = torch.tensor([[1e-4, 0.01, 1.0, 0.0] if d > 1 else [1e-4, 0.0, 0.0, 0.0] for d in dims], device=dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        w = torch.randn(n, device=dev, generator=gen)
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        return dict(n=n, tensors=len(offsets), chunks=chunks, ranges=ranges, hp=hp, w=w, g=g,
                    m=torch.zeros_like(w), v=torch.zeros_like(w), sh=torch.empty(n, dtype=torch.bfloat16, device=dev),
                    part=torch.zeros(2 * chunks.shape[0], device=dev), ratio=torch.ones(len(offsets), device=dev),
                    max_chunks=int(ranges[:, 1].max()))

    def measure(L, variants):
        for fn, _ in variants.values():                      # warm every code object
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):                            # alternate the variants inside a round
            for k, (fn, _) in variants.items():
                times[k].append(timed(fn))
        res = {}
        for k, (_, nbytes) in variants.items():
            med = statistics.median(times[k])
            res[k] = {"us": round(med, 1), "min_us": round(min(times[k]), 1), "max_us": round(max(times[k]), 1),
                      "bytes_per_param": nbytes, "TB_per_s": round(L["n"] * nbytes / (med * 1e-6) / 1e12, 3)}
        return res

    out = {"rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "layer_chunk": K.LAYER_CHUNK}
    lr_dev = torch.full((1,), 1e-4, device=dev)
    step_dev = torch.ones(1, device=dev)
    first_dev = torch.zeros(1, device=dev)

    from kubeml_amd.models.bert import bert_base_mlm
    L = layout(bert_base_mlm)

    def lamb1():
        K.lamb_moments_(L["w"], L["g"], L["m"], L["v"], L["chunks"], L["ranges"], L["hp"], L["part"], L["ratio"], 1.0,
                        step_dev=step_dev)

    def lamb2():
        K.lamb_apply_(L["w"], L["m"], L["v"], L["sh"], L["chunks"], L["hp"], L["ratio"], 1.0, step_dev=step_dev)

    def lamb():
        lamb1()
        lamb2()
    res = measure(L, {
        "adamw": (lambda: K.adam_(L["w"], L["g"], L["m"], L["v"], L["sh"], 1e-4, 1.0, wd=0.01, decoupled=True,
                                  lr_dev=lr_dev, step_dev=step_dev), 30.0),
        "lamb_moments": (lamb1, 24.0), "lamb_apply": (lamb2, 18.0), "lamb_step": (lamb, 42.0)})
    res["lamb_over_adamw"] = round(res["lamb_step"]["us"] / res["adamw"]["us"], 4)
    res.update(numel=L["n"], tensors=L["tensors"], chunks=int(L["chunks"].shape[0]),
               max_chunks_of_a_tensor=L["max_chunks"])
    out["bert_base"] = res
    del L
    torch.cuda.empty_cache()

    from kubeml_amd.models.resnet import resnet34
    L = layout(lambda: resnet34(1000))

    def lars1():
        K.lars_norms_(L["w"], L["g"], L["chunks"], L["ranges"], L["hp"], L["part"], L["ratio"])

    def lars2():
        K.lars_apply_(L["w"], L["g"], L["m"], L["sh"], L["chunks"], L["hp"], L["ratio"], momentum=0.9,
                      first_dev=first_dev)

    def lars():
        lars1()
        lars2()
    res = measure(L, {
        "sgd_momentum": (lambda: K.sgd_(L["w"], L["g"], L["m"], L["sh"], 1e-4, wd=1e-4, momentum=0.9, lr_dev=lr_dev,
                                        first_dev=first_dev), 22.0),
        "lars_norms": (lars1, 8.0), "lars_apply": (lars2, 22.0), "lars_step": (lars, 30.0)})
    res["lars_over_sgd"] = round(res["lars_step"]["us"] / res["sgd_momentum"]["us"], 4)
    res.update(numel=L["n"], tensors=L["tensors"], chunks=int(L["chunks"].shape[0]),
               max_chunks_of_a_tensor=L["max_chunks"])
    out["resnet34"] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
