"""Cost of the soft-target cross-entropy against the hard-label kernels, and of mixup / CutMix
inside the augment launch against the plain augment launch, alternating in one process.

    python tools/bench_soft_targets.py [--rounds 7] [--iters 20] [--eager] [--out FILE.json]

Cross-entropy forward + backward at (256, 1000) bf16 (the ResNet head) and at (2432, 30522 in
30528) bf16 (the MLM head): hard labels, label smoothing over integer labels, packed (y, y2, lam)
targets with smoothing.  All three read the logits twice and write the gradient once, 6 bytes per
logit.  Augmentation at 256 x 32 x 32 x 3 from a 50 000-image resident source and at 128 x 224 x
224 x 3 from a 2048-image one: plain, mixup (a second 3-byte gather per pixel: (16 + 6) / (16 + 3)
= 1.16 of the plain traffic) and CutMix (one gather per pixel: 1.0).  Every augment variant is
followed by the counter advance, so consecutive launches read different samples.

Each round times ``iters`` back-to-back launches of every variant between device events, the
variants alternating inside the round; the time per launch is the median over the rounds, its
spread the min .. max.  The launches are replayed from a captured graph, so the host's issue rate
does not bound the small shapes; ``--eager`` issues them from Python instead.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("bench_soft_targets: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)

    def runner(fn):
        """iters back-to-back launches of fn as one callable (a graph replay unless --eager)."""
        def many():
            for _ in range(a.iters):
                fn()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()                                             # warm the code object and the allocator
        torch.cuda.current_stream().wait_stream(s)
        if a.eager:
            return many
        g = torch.cuda.CUDAGraph()
        with capture_graph(g):
            many()
        return g.replay

    def measure(variants, unit_bytes=None):
        runs = {k: runner(fn) for k, fn in variants.items()}
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):                            # alternate the variants inside a round
            for k, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / a.iters * 1e3)      # us per launch
        res = {}
        for k in variants:
            med = statistics.median(times[k])
            res[k] = {"us": round(med, 2), "min_us": round(min(times[k]), 2), "max_us": round(max(times[k]), 2)}
            if unit_bytes and k in unit_bytes:
                res[k]["TB_per_s"] = round(unit_bytes[k] / (med * 1e-6) / 1e12, 3)
        return res

    out = {"rounds": a.rounds, "iters": a.iters, "graph": not a.eager, "device": torch.cuda.get_device_name(0)}

    # ---- cross-entropy --------------------------------------------------------------------------
    for name, (B, C, ld) in {"ce_256x1000": (256, 1000, 1000), "ce_2432x30522": (2432, 30522, 30528)}.items():
        logits = (torch.randn(B, ld, device=dev, generator=gen) * 3).to(torch.bfloat16)
        y = torch.randint(0, C, (B,), device=dev, generator=gen)
        y2 = torch.randint(0, C, (B,), device=dev, generator=gen)
        packed = torch.stack([y.float(), y2.float(), torch.rand(B, device=dev, generator=gen)], 1).contiguous()
        go = torch.ones(1, device=dev)
        h3, hws, hl = K.ce_fwd(logits, y, classes=C)
        s3, sws, sl = K.ce_soft_fwd(logits, y, classes=C, label_smoothing=0.1)
        p3, pws, pl = K.ce_soft_fwd(logits, packed, classes=C, label_smoothing=0.1)

        def pair(fwd, bwd):
            def f():
                o3, ws, t = fwd()
                bwd(t, ws, o3)
            return f
        hard_f = lambda: K.ce_fwd(logits, y, classes=C)
        hard_b = lambda t=hl, ws=hws, o3=h3: K.ce_bwd(logits, t, ws, o3, grad_out=go, classes=C)
        soft_f = lambda: K.ce_soft_fwd(logits, y, classes=C, label_smoothing=0.1)
        soft_b = lambda t=sl, ws=sws, o3=s3: K.ce_soft_bwd(logits, t, ws, o3, grad_out=go, classes=C,
                                                           label_smoothing=0.1)
        pack_f = lambda: K.ce_soft_fwd(logits, packed, classes=C, label_smoothing=0.1)
        pack_b = lambda t=pl, ws=pws, o3=p3: K.ce_soft_bwd(logits, t, ws, o3, grad_out=go, classes=C,
                                                           label_smoothing=0.1)
        n = B * ld
        res = measure({"hard_fwd": hard_f, "soft_fwd": soft_f, "packed_fwd": pack_f,
                       "hard_bwd": hard_b, "soft_bwd": soft_b, "packed_bwd": pack_b,
                       "hard": pair(hard_f, hard_b), "soft": pair(soft_f, soft_b), "packed": pair(pack_f, pack_b)},
                      {"hard_fwd": 2 * n, "soft_fwd": 2 * n, "packed_fwd": 2 * n, "hard_bwd": 4 * n,
                       "soft_bwd": 4 * n, "packed_bwd": 4 * n, "hard": 6 * n, "soft": 6 * n, "packed": 6 * n})
        res["soft_over_hard"] = round(res["soft"]["us"] / res["hard"]["us"], 4)
        res["packed_over_hard"] = round(res["packed"]["us"] / res["hard"]["us"], 4)
        out[name] = res
        del logits
        torch.cuda.empty_cache()

    # ---- augmentation ---------------------------------------------------------------------------
    for name, (N, B, H, W) in {"augment_256x32x32": (50000, 256, 32, 32), "augment_128x224x224": (2048, 128, 224, 224)}.items():
        src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
        labels = torch.randint(0, 1000, (N,), device=dev, generator=gen)
        x = torch.empty((B, H, W, 8), dtype=torch.bfloat16, device=dev)
        yb = torch.empty((B,), dtype=torch.int64, device=dev)
        tb = torch.empty((B, 3), device=dev)
        ctrs = {k: torch.tensor([1.0, 0.0, 0.0], device=dev) for k in ("plain", "mixup", "cutmix", "advance")}

        def plain():
            K.augment(src, labels, ctrs["plain"], B, out=x, labels_out=yb, train=True)
            K.advance_counter_(ctrs["plain"], B, N)

        def mixed(key, **mix):
            def f():
                K.augment_mix(src, labels, ctrs[key], B, out=x, targets_out=tb, train=True, **mix)
                K.advance_counter_(ctrs[key], B, N)
            return f
        px = B * H * W
        res = measure({"plain": plain, "mixup": mixed("mixup", mixup_alpha=1.0),
                       "cutmix": mixed("cutmix", cutmix_alpha=1.0),
                       "advance": lambda: K.advance_counter_(ctrs["advance"], B, N)},
                      {"plain": 19 * px, "mixup": 22 * px, "cutmix": 19 * px})
        for k in ("mixup", "cutmix"):
            res[k + "_over_plain"] = round(res[k]["us"] / res["plain"]["us"], 4)
            res[k + "_over_plain_less_advance"] = round((res[k]["us"] - res["advance"]["us"]) /
                                                        (res["plain"]["us"] - res["advance"]["us"]), 4)
        out[name] = res
        del src
        torch.cuda.empty_cache()

    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
