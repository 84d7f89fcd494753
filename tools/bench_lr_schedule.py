"""Cost of the device LR schedule (csrc/kernels/lr_schedule.hip): the ``kml_lr_schedule`` launch alone and the
ResNet-34 graphed train step without a schedule, with the device schedule, and driven by a host ``set_lr``
before every replay (what a per-step schedule costs without it), alternating in one process.

    python tools/bench_lr_schedule.py [--rounds 7] [--iters 256] [--steps 100] [--out FILE.json]

The launch alone at 1 row (the lr scalar), 8 rows of stride 2 (a full group table) and 200 rows of stride 4
(BERT-base under LAMB: a row per tensor): ``iters`` back-to-back launches issued from the host between
device events, and the same ``iters`` launches as a dependent chain of one captured graph (what a launch
costs inside a captured step).  The step variants run a ``constant`` schedule, so all of them train the same
weights and differ in launches and host work only; ``plain_again`` is a second build of the plain step.
Each variant's time is the median over the rounds, its spread the min .. max.  The launch moves a few hundred
bytes: its time is launch latency, there is no bandwidth floor to compare with.  Prints one JSON line.
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
    ap.add_argument("--iters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true", help="the launch only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_lr_schedule: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    from kubeml_amd.models.resnet import resnet34
    from kubeml_amd.nn import cross_entropy, flatten_module
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.optim import SGD, LRSchedule, lr_factor
    dev = torch.device("cuda", 0)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3          # us per call

    def summary(ts):
        return {"us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}

    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters}
    shape = dict(kind="cosine", warmup=5.0, total=90.0, min_ratio=0.0, warmup_start=0.0)
    layouts = {"rows1_stride1": (1, 1), "rows8_stride2": (8, 2), "rows200_stride4": (200, 4)}
    launches = {}
    for name, (rows, stride) in layouts.items():
        table = torch.zeros(rows * stride, device=dev)
        base = torch.full((rows,), 0.1, device=dev)
        ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        pos = torch.tensor([0.0, 1e-3], device=dev)
        last = torch.zeros(2, device=dev)
        launches[name] = (lambda t=table, r=rows, s=stride, b=base, c=ctl, p=pos, l=last:
                          K.lr_schedule_(t, r, s, b, c, p, l, 1, **shape)), ctl
    for fn, _ in launches.values():
        fn()
    torch.cuda.synchronize()
    # the same launches as nodes of one graph, each depending on the one before it: what a launch costs
    # inside a captured step, where the host does not issue it
    from kubeml_amd.engine.step import capture_graph
    graphs = {}
    for k, (fn, _) in launches.items():
        g = torch.cuda.CUDAGraph()
        with capture_graph(g):
            for _ in range(a.iters):
                fn()
        graphs[k] = g
    ts = {k: [] for k in launches}
    tg = {k: [] for k in launches}
    for _ in range(a.rounds):                     # alternate the layouts inside every round
        for k, (fn, ctl) in launches.items():
            ctl.zero_()
            ts[k].append(timed(fn, a.iters))
            ctl.zero_()
            graphs[k].replay()
            tg[k].append(timed(graphs[k].replay, 4) / a.iters)
    out["launch"] = {k: summary(v) for k, v in ts.items()}              # issued from the host, back to back
    out["launch_in_graph"] = {k: summary(v) for k, v in tg.items()}     # per node of a captured chain

    if not a.no_step:
        from kubeml_amd.engine.dp import make_train_step
        B, n_local = a.batch, 50000
        # a constant schedule: f = 1, so every variant trains the same weights, bit for bit, and the variants
        # differ in their launches and host work only.  plain_again is a second build of plain: what two
        # builds of the same step differ by (buffer placement)
        sched_shape = dict(kind="constant", total=1)
        steps = {}
        for variant in ("plain", "device_schedule", "host_set_lr", "plain_again"):
            torch.manual_seed(1234)
            model = resnet34(num_classes=1000).to(dev)
            space = flatten_module(model)
            model.train()
            g2 = torch.Generator(device=dev).manual_seed(0)
            data = torch.randint(0, 256, (n_local, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g2)
            labels = torch.randint(0, 10, (n_local,), dtype=torch.int64, device=dev, generator=g2)
            ctr = torch.tensor([1000.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            xbuf = torch.empty((B, 32, 32, 8), dtype=torch.bfloat16, device=dev)
            ybuf = torch.empty((B,), dtype=torch.int64, device=dev)
            opt = SGD(model.parameters(), lr=0.01, weight_decay=1e-4)
            sched = LRSchedule(opt, **sched_shape) if variant == "device_schedule" else None
            pre = (lambda data=data, labels=labels, ctr=ctr, xbuf=xbuf, ybuf=ybuf:
                   K.augment(data, labels, ctr, B, out=xbuf, labels_out=ybuf, train=True))
            st = make_train_step(model, space, opt, cross_entropy, xbuf, ybuf, pre=pre, advance=(ctr, B, n_local),
                                 extra_state=[ctr], lr_schedule=sched)
            st.capture()
            if variant == "host_set_lr":
                # what a per-step schedule costs today: the host twin and a fill of the lr scalar before every replay
                count = [0]

                def run(st=st, opt=opt, count=count):
                    opt.set_lr(float(torch.tensor(0.01) * lr_factor(count[0], 0.0, 1.0, **sched_shape)))
                    count[0] += 1
                    return st()
            else:
                run = st
            for _ in range(10):
                run()
            torch.cuda.synchronize()
            steps[variant] = run
        ts = {k: [] for k in steps}
        for _ in range(a.rounds):                 # alternate: plain, device, host, plain again, plain, ...
            for k, run in steps.items():
                ts[k].append(timed(run, a.steps))
        res = {"batch": B, "steps_per_round": a.steps, **{k: summary(v) for k, v in ts.items()}}
        res["device_minus_plain_us"] = round(res["device_schedule"]["us"] - res["plain"]["us"], 2)
        res["host_minus_plain_us"] = round(res["host_set_lr"]["us"] - res["plain"]["us"], 2)
        res["plain_again_minus_plain_us"] = round(res["plain_again"]["us"] - res["plain"]["us"], 2)
        out["resnet34_step"] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
