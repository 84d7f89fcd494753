"""Cost of the weight EMA (csrc/kernels/ema.hip): the update launch, the swap launch and the
ResNet-34 graphed train step with and without an EMA, alternating in one process.

    python tools/bench_ema.py [--rounds 7] [--iters 32] [--steps 100] [--bert-numel N] [--out FILE.json]

Sizes: the ResNet-34 state prefix (parameters in storage layout + BN running statistics, measured
from the flattened bench.py model) and the BERT-base flat space as tools/bench_param_groups.py sizes
it.  Each round times ``iters`` back-to-back launches of every variant between device events; a
variant's time is the median over the rounds, its spread the min .. max.  Bytes the algorithm must
move per element: the applying update reads ema and w and writes ema, 12; a launch that does not
apply, 0; the swap reads and writes both and writes the bf16 shadow, 18; AdamW (same run, same
space) 30.  The floor is bytes over 6.3 TB/s.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bert-numel", type=int, default=64 * 1715000)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_ema: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    from kubeml_amd.models.resnet import resnet34
    from kubeml_amd.nn import cross_entropy, flatten_module
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.optim import EMA, SGD
    from kubeml_amd.optim.ema import UPDATE_BLOCKS
    dev = torch.device("cuda", 0)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3          # us per call

    def summary(ts, n, nbytes):
        med = statistics.median(ts)
        r = {"us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "bytes_per_elem": nbytes}
        if nbytes:
            r["floor_us"] = round(n * nbytes / (HBM_TBS * 1e12) * 1e6, 2)
            r["TB_per_s"] = round(n * nbytes / (med * 1e-6) / 1e12, 3)
        return r

    def build(with_ema):
        torch.manual_seed(1234)
        model = resnet34(num_classes=1000).to(dev)
        space = flatten_module(model)
        model.train()
        return model, space, (EMA(model, decay=0.9999) if with_ema else None)

    out = {"device": torch.cuda.get_device_name(0), "update_blocks": UPDATE_BLOCKS, "rounds": a.rounds,
           "iters": a.iters, "hbm_TB_per_s": HBM_TBS}
    model, space, _ = build(False)
    sizes = {"resnet34_prefix": int(space.i64_off), "bert_base_space": a.bert_numel // 64 * 64}
    del model, space
    gen = torch.Generator(device=dev).manual_seed(0)
    for name, n in sizes.items():
        w = torch.randn(n, device=dev, generator=gen)
        e = w.clone()
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        m, v = torch.zeros_like(w), torch.zeros_like(w)
        sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
        lr_dev, step_dev = torch.full((1,), 1e-4, device=dev), torch.ones(1, device=dev)
        ctl = torch.zeros(4, dtype=torch.int32, device=dev)
        aout = torch.zeros(1, device=dev)
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        def upd(every):
            return lambda: K.ema_update_(e, w, 0.9999, every, True, ctl, aout, ticket, max_blocks=UPDATE_BLOCKS)
        variants = {
            "update_apply": (upd(1), 12),
            "update_skip": (upd(1 << 30), 0),
            "update_every32": (upd(32), 12 / 32),
            "swap": (lambda: K.ema_swap_(w, e, sh, n), 18),
            "adamw": (lambda: K.adam_(w, g, m, v, sh, 1e-4, 1.0, wd=0.01, decoupled=True, lr_dev=lr_dev,
                                      step_dev=step_dev), 30),
        }
        iters = a.iters // 32 * 32 or 32          # whole periods of update_every=32
        for fn, _ in variants.values():
            fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in variants}
        for _ in range(a.rounds):                 # alternate the variants inside every round
            for k, (fn, _) in variants.items():
                ctl.zero_()
                ts[k].append(timed(fn, iters))
        out[name] = {"numel": n, **{k: summary(ts[k], n, variants[k][1]) for k in variants}}
        del w, e, g, m, v, sh
        torch.cuda.empty_cache()

    if not a.no_step:
        from kubeml_amd.engine.dp import make_train_step
        B, n_local = a.batch, 50000
        steps = {}
        for with_ema in (False, True):
            model, space, ema = build(with_ema)
            g2 = torch.Generator(device=dev).manual_seed(0)
            data = torch.randint(0, 256, (n_local, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g2)
            labels = torch.randint(0, 10, (n_local,), dtype=torch.int64, device=dev, generator=g2)
            ctr = torch.tensor([1000.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            xbuf = torch.empty((B, 32, 32, 8), dtype=torch.bfloat16, device=dev)
            ybuf = torch.empty((B,), dtype=torch.int64, device=dev)
            opt = SGD(model.parameters(), lr=0.01, weight_decay=1e-4)
            pre = (lambda data=data, labels=labels, ctr=ctr, xbuf=xbuf, ybuf=ybuf:
                   K.augment(data, labels, ctr, B, out=xbuf, labels_out=ybuf, train=True))
            st = make_train_step(model, space, opt, cross_entropy, xbuf, ybuf, pre=pre, advance=(ctr, B, n_local),
                                 extra_state=[ctr], ema=ema)
            st.capture()
            for _ in range(10):
                st()
            torch.cuda.synchronize()
            steps[with_ema] = st
        ts = {False: [], True: []}
        for _ in range(a.rounds):                 # alternate: without, with, without, ...
            for with_ema in (False, True):
                ts[with_ema].append(timed(steps[with_ema], a.steps))
        res = {"batch": B, "steps_per_round": a.steps,
               "without_ema": summary(ts[False], 0, 0), "with_ema": summary(ts[True], 0, 0)}
        res["delta_us"] = round(res["with_ema"]["us"] - res["without_ema"]["us"], 2)
        out["resnet34_step"] = res
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
