"""Cost of the resample launch (RandomResizedCrop / Resize + CenterCrop, ``kml_augment_resample``)
against the plain augment launch of the same output size, alternating in one process.

    python tools/bench_augment.py [--rounds 7] [--iters 20] [--batch 128] [--resnet50] [--out FILE.json]

The plain launch (``kml_augment``, flip + normalise) from a resident 224 x 224 x 3 source, and the
resample launch from a resident 256 x 256 x 3 source to 224 x 224 in four configurations: train
(RandomResizedCrop + flip), eval (Resize(256) + CenterCrop(224)), train with mixup, train with
CutMix.  Every launch is followed by the counter advance, so consecutive launches read other
samples and draw other boxes.

Bytes are computed from shapes: what is written, ``B * 224 * 224 * 16``, plus what has to be read
at least once: ``B * 224 * 224 * 3`` for the plain launch, the boxes' pixels for the resample launch
(the mean box of the timed steps from ``rrc_plan``; twice that for mixup, whose every pixel gathers
from two samples; the whole 256 x 256 image for eval).  ``floor_us`` is those bytes at 6.3 TB/s (the
bandwidth a streaming kernel reaches on this GPU: derived, not measured here), ``floor_share`` the
floor over the measured time.

Each round times ``iters`` back-to-back launches of every variant between device events, replayed
from a captured graph, the variants alternating inside the round; the time per launch is the median
over the rounds, its spread the min .. max.

``--resnet50``: the graphed ResNet-50 train step of ``tools/bench_resnet50.py`` (batch 128, SGD) fed
by the plain launch and by the resample launch (train), one model, two captured steps, alternating.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLOOR_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--resnet50", action="store_true")
    ap.add_argument("--steps", type=int, default=20, help="ResNet-50 steps per round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("bench_augment: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    B, n, S, Ss = a.batch, a.images, 224, 256
    src224 = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, device=dev, generator=gen)
    src256 = torch.randint(0, 256, (n, Ss, Ss, 3), dtype=torch.uint8, device=dev, generator=gen)
    labels = torch.randint(0, 1000, (n,), device=dev, generator=gen)
    x = torch.empty((B, S, S, 8), dtype=torch.bfloat16, device=dev)
    yb = torch.empty((B,), dtype=torch.int64, device=dev)
    tb = torch.empty((B, 3), device=dev)
    names = ("plain", "train", "eval", "mixup", "cutmix", "advance")
    ctrs = {k: torch.tensor([1.0, 0.0, 0.0], device=dev) for k in names}

    def plain():
        K.augment(src224, labels, ctrs["plain"], B, out=x, labels_out=yb, pad=0, flip=True, train=True)
        K.advance_counter_(ctrs["plain"], B, n)

    def resample(key, **kw):
        def f():
            K.augment_resample(src256, labels, ctrs[key], B, S, out=x, labels_out=yb, targets_out=tb, **kw)
            K.advance_counter_(ctrs[key], B, n)
        return f
    variants = {"plain": plain, "train": resample("train"), "eval": resample("eval", train=False, resize=256),
                "mixup": resample("mixup", mixup_alpha=1.0), "cutmix": resample("cutmix", cutmix_alpha=1.0),
                "advance": lambda: K.advance_counter_(ctrs["advance"], B, n)}

    def graphed(fn, reps):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()                                             # warm the code object and the allocator
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with capture_graph(g):
            for _ in range(reps):
                fn()
        return g.replay

    def measure(runs, reps):
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):                            # alternate the variants inside a round
            for k, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps * 1e3)      # us per launch / step
        return {k: {"us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
                for k, t in times.items()}

    out = {"rounds": a.rounds, "iters": a.iters, "batch": B, "device": torch.cuda.get_device_name(0)}
    res = measure({k: graphed(fn, a.iters) for k, fn in variants.items()}, a.iters)
    # mean box of the steps the train variant went through
    steps = int(ctrs["train"][1].item())
    p = K.rrc_plan(torch.tensor([1.0, 0.0, 0.0], device=dev), min(steps, 512), B, Ss, Ss).double()
    box = float((p[..., 2] * p[..., 3]).mean())
    px = B * S * S
    read = {"plain": 3 * px, "train": 3 * B * box, "eval": 3 * B * Ss * Ss, "mixup": 6 * B * box, "cutmix": 3 * B * box}
    for k, rd in read.items():
        byts = rd + 16 * px
        res[k]["bytes"] = int(byts)
        res[k]["floor_us"] = round(byts / (FLOOR_TBS * 1e12) * 1e6, 2)
        res[k]["floor_share"] = round(res[k]["floor_us"] / res[k]["us"], 3)
        res[k]["over_plain"] = round(res[k]["us"] / res["plain"]["us"], 3)
    out["mean_box_pixels"] = round(box, 1)
    out["fallback_share"] = round(float(p[..., 5].mean()), 4)
    out["launch"] = res

    if a.resnet50:
        from kubeml_amd.engine.step import GraphedTrainStep
        from kubeml_amd.models.resnet import resnet50
        from kubeml_amd.nn import backward_loss, cross_entropy, flatten_module
        from kubeml_amd.optim import SGD
        torch.manual_seed(0)
        model = resnet50(1000).to(dev)
        space = flatten_module(model)
        model.train()
        opt = SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        sctr = {k: torch.tensor([11.0, 0.0, 0.0], device=dev) for k in ("plain", "resample")}

        def make(key):
            def fwd_bwd():
                if key == "plain":
                    K.augment(src224, labels, sctr[key], B, out=x, labels_out=yb, pad=0, flip=True, train=True)
                else:
                    K.augment_resample(src256, labels, sctr[key], B, S, out=x, labels_out=yb)
                space.zero_grad()
                loss = cross_entropy(model(x), yb)
                backward_loss(loss)
                return loss

            def opt_step():
                opt.step()
                K.advance_counter_(sctr[key], B, n)
            st = GraphedTrainStep(fwd_bwd, opt_step, warmup=2)
            st.capture()
            return st
        steps = {k: make(k) for k in ("plain", "resample")}

        def many(st):
            def f():
                for _ in range(a.steps):
                    st()
            return f
        r50 = measure({k: many(st) for k, st in steps.items()}, a.steps)
        r50["resample_minus_plain_us"] = round(r50["resample"]["us"] - r50["plain"]["us"], 2)
        r50["steps_per_round"] = a.steps
        out["resnet50_step"] = r50

    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
