"""Cost of the grouped optimizer launch (kml_sgd_groups / kml_adam_groups) against the single-group
launch of the same build at the same size, alternating in one process.

    python tools/bench_param_groups.py [--numel 109760000] [--rounds 7] [--iters 20] [--out FILE.json]

Default size: the BERT-base flat space (about 110 M elements).  Each round times ``iters``
back-to-back launches of the single-group kernel and then of the grouped one between device events;
the per-launch time of a variant is the median over the rounds, its spread the min .. max of the
rounds.  Bytes per parameter (what the algorithm must move): AdamW reads w, g, m, v and writes w, m, v
and the bf16 shadow, 30 bytes; SGD with momentum reads w, g, mom and writes w, mom and the shadow,
22 bytes; the grouped launch adds the granule byte, 1/64 byte.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=64 * 1715000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from kubeml_amd.ops import kernels as K
    if not torch.cuda.is_available():
        print("bench_param_groups: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cuda", 0)
    n = a.numel // 64 * 64
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    # BERT-like assignment: long decay runs (weights) with short no-decay runs (biases, LayerNorm) between
    cpu = torch.Generator().manual_seed(1)
    gid = torch.zeros(n // 64, dtype=torch.uint8)
    marks = torch.randint(0, n // 64, (2000,), generator=cpu)
    for k, s in enumerate(marks.tolist()):
        gid[s:s + 12] = 1 + k % (a.groups - 1) if a.groups > 1 else 0
    gid = gid.to(dev)
    lr_dev = torch.full((1,), 1e-4, device=dev)
    step_dev = torch.ones(1, device=dev)
    first_dev = torch.zeros(1, device=dev)

    def variants(kind):
        rows = [[1e-4, 0.01]] + [[1e-4 / (k + 1), 0.0] for k in range(1, a.groups)]
        hp = torch.tensor(rows, dtype=torch.float32, device=dev)
        if kind == "adamw":
            return (lambda: K.adam_(w, g, m, v, sh, 1e-4, 1.0, wd=0.01, decoupled=True, lr_dev=lr_dev,
                                    step_dev=step_dev),
                    lambda: K.adam_groups_(w, g, m, v, sh, gid, hp, 1.0, 0, decoupled=True, step_dev=step_dev))
        return (lambda: K.sgd_(w, g, m, sh, 1e-4, wd=0.01, momentum=0.9, lr_dev=lr_dev, first_dev=first_dev),
                lambda: K.sgd_groups_(w, g, m, sh, gid, hp, 0, momentum=0.9, first_dev=first_dev))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3          # us per launch

    out = {"numel": n, "groups": a.groups, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    for kind, nbytes in (("adamw", 30.0), ("sgd_momentum", 22.0)):
        single, grouped = variants(kind)
        for fn in (single, grouped):                         # warm both code objects
            fn()
        torch.cuda.synchronize()
        ts, tg = [], []
        for _ in range(a.rounds):                            # alternate: single, grouped, single, ...
            ts.append(timed(single))
            tg.append(timed(grouped))
        res = {}
        for name, t, b in (("single", ts, nbytes), ("grouped", tg, nbytes + 1.0 / 64)):
            med = statistics.median(t)
            res[name] = {"us": round(med, 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1),
                         "bytes_per_param": round(b, 4), "TB_per_s": round(n * b / (med * 1e-6) / 1e12, 3)}
        res["grouped_over_single"] = round(res["grouped"]["us"] / res["single"]["us"], 4)
        out[kind] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
