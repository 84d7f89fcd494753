"""KV-cache decoding of GPT-2 small (random weights) on one GPU: the decode step against the
same step on the existing Linear route and against full recompute, the skinny GEMM against the
existing small-M route per shape, and the decode attention over its keys-per-chunk choices.

    python tools/bench_gpt_decode.py [--rounds 5] [--iters 20] [--new 256] [--out FILE.json]
                                     [--top-k K] [--top-p P] [--repetition-penalty R] [--skip-kernels]
                                     [--prompt-lookup K[,K...]]

* decode: B in {1, 4, 16}, prompt 128, ``--new`` tokens.  (a) the captured step of ``generate``
  (``decode_step`` replays, timed between device events after the prefill); (b) the same step
  with every ``forward_small`` sent to ``Linear.forward``; (c) ``model(ids)`` on the whole growing
  sequence per token, B = 1, 32 tokens, host clock ending in a synchronise.  (a) and (b) alternate
  inside every round; the figure is the median over the rounds.  With ``--top-k`` / ``--top-p`` /
  ``--repetition-penalty`` (default: off) a third variant, ``filtered``, is the captured step whose
  last launch is ``kml_decode_sample`` with those filters, sampling at temperature 1.
* sampler: ``kml_decode_advance`` against ``kml_decode_sample`` alone on ``[B, 50264]`` logits, a
  history of 384 tokens, B in {1, 4, 16}; the filters of the flags, or 50 / 0.95 / 1.2 without any.
* GEMM: the five GPT-2 small weight shapes at M in {1, 4, 8, 16}: ``gemm_skinny`` against what
  ``Linear.forward`` launches at that M (the 1x1 implicit-GEMM conv, plus the GELU launch).  Each
  variant walks a ring of weight copies of at least 64 MB, so no launch finds its weights in the
  L2 the previous one filled; ``iters`` launches per captured graph, variants alternating.
* attention: B = 4, H = 12, Lcap = 1024, n in {128, 512, 1023} keys, chunk in {64, 128, 256, 512}.
* floor: the bf16 weight bytes one token reads, over the 6.3 TB/s the microarchitecture notes give
  as the achievable HBM rate — derived, not measured.
* ``--prompt-lookup K[,K...]``: only the speculative-decoding measurements (:func:`prompt_lookup`):
  the verify round of K + 1 rows beside the plain step (``K = 0``: the plain step alone), oracle and
  n-gram drafts, and the multi-query decode attention beside separate one-query launches.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("c_attn", 2304, 768, None, True), ("attn.c_proj", 768, 768, None, True),
          ("c_fc+gelu", 3072, 768, "gelu", True), ("mlp.c_proj", 768, 3072, None, True),
          ("lm_head", 50264, 768, None, False)]


class _Everything:
    """stands in for nn.modules._SMALL_EXISTING: every shape takes the existing route from row 0"""

    def get(self, key, default=None):
        return 0


def prompt_lookup(a, ks, graphed, alternate):
    """``--prompt-lookup K[,K...]``: speculative decoding with k draft tokens per verify round.

    * attention: B = 1, H = 12, ``kml_attn_decode_multi`` at q in {4, 8, 16} queries against q
      separate ``kml_attn_decode`` launches, lens in {256, 1024}; captured, alternating.
    * model (GPT-2 small, random weights, prompt 128, ``--new`` tokens), for B in {1, 4} and every K
      with B (K + 1) <= 16, all variants alternating inside every round of one process:
      ``step`` — the plain captured decode step (what K = 0 runs; the baseline); ``round`` — one
      verify round (replays of the captured round on constant drafts: the launches do not depend
      on what is accepted); ``oracle`` — a whole decode with teacher-forced drafts (the plain run's
      own continuation, gathered by three stock-torch launches per round, which are inside the
      time): every draft accepted, the ceiling; ``break_even`` = round / step, the tokens per
      round and sequence above which speculation wins.
    * realised: ``generate`` with the n-gram drafter against plain ``generate`` (host clock,
      prefill included) on a prompt that repeats a block of 16 tokens and on random token ids.
      K = 0 reports the plain step only."""
    import torch
    from kubeml_amd.ops import decode as D
    dev = torch.device("cuda", 0)
    BF = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    out = {"ks": ks}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def stat(v, nd=2):
        return {"us": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    if not a.skip_kernels:
        B, H, Lcap = 1, 12, 1152
        kc = torch.randn(B, H, Lcap, 64, device=dev, generator=gen).to(BF)
        vc = torch.randn(B, H, Lcap, 64, device=dev, generator=gen).to(BF)
        ws1 = D.attn_decode_workspace(B, H, Lcap, dev)
        o1 = torch.empty(B, H * 64, dtype=BF, device=dev)
        attn = []
        for n in (256, 1024):
            lens = torch.full((B,), n, dtype=torch.int32, device=dev)
            for q in (4, 8, 16):
                rows = torch.randn(B * q, 3 * H * 64, device=dev, generator=gen).to(BF)
                wsm = D.attn_decode_multi_workspace(B, H, Lcap, q, dev)
                om = torch.empty(B * q, H * 64, dtype=BF, device=dev)
                each = [lens + j for j in range(q)]

                def multi():
                    for _ in range(a.iters):
                        D.attn_decode_multi(rows, kc, vc, lens, q, ws=wsm, out=om)

                def separate():
                    for _ in range(a.iters):
                        for j in range(q):
                            D.attn_decode(rows[j:j + 1], kc, vc, each[j], ws=ws1, out=o1)
                r = alternate({"multi": graphed(multi), "separate": graphed(separate)}, a.iters)
                attn.append({"lens": n, "q": q, "B": B, "H": H, **r})
                print(json.dumps(attn[-1]), file=sys.stderr, flush=True)
        out["attention"] = attn
    if a.skip_model:
        return out

    from kubeml_amd.models.gpt import gpt2_small
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    model = gpt2_small(dropout=0.0, activation=a.activation).to(dev).eval()
    flatten_module(model)
    prompt, new = 128, a.new
    W = prompt + new
    cases = []
    for Bm in (1, 4):
        for K in ks:
            if Bm * (K + 1) > 16:
                continue
            q = K + 1
            ids = torch.randint(0, 50257, (Bm, prompt), device=dev, generator=gen)
            plain = model.new_cache(Bm, W + q, dev)

            def arm_plain():
                plain.reset()
                model.prefill(ids, None, plain)
            arm_plain()
            model.decode_step(plain)   # capture

            def steps():
                for _ in range(new - 1):
                    model.decode_step(plain)
            case = {"B": Bm, "K": K, "prompt": prompt, "new": new}
            if K == 0:
                v = []
                for _ in range(a.rounds):
                    arm_plain()
                    v.append(timed(steps) / (new - 1))
                case["step"] = stat(v)
                cases.append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
                continue
            ref = model.generate(ids, max_new_tokens=new)
            spec = model.new_cache(Bm, W + q, dev)
            start = torch.full((Bm,), prompt - 1)
            ar = torch.arange(1, q, device=dev)[None]

            def arm():
                spec.reset(start=start, limit=start + new, draft_tokens=K)
                model.prefill(ids, None, spec)
            arm()
            model.verify_step(spec, spec.draft)   # capture
            nr = max(1, (new - 1) // q)           # constant (zero) drafts: a sequence moves 1 .. q per round

            def rounds():
                for _ in range(nr):
                    model.verify_step(spec, spec.draft)
            no = -(-(new - 1) // q)

            def oracle():
                for _ in range(no):
                    draft = ref.gather(1, (spec.lens[:, None].long() + ar).clamp(max=W - 1))
                    model.verify_step(spec, draft)
            t = {"step": [], "round": [], "oracle": []}
            for _ in range(a.rounds):
                arm_plain()
                t["step"].append(timed(steps) / (new - 1))
                arm()
                t["round"].append(timed(rounds) / nr)
                arm()
                t["oracle"].append(timed(oracle))
            st = spec.stats.tolist()
            case["step"], case["round"] = stat(t["step"]), stat(t["round"])
            case["break_even_tokens_per_round"] = round(case["round"]["us"] / case["step"]["us"], 3)
            us = statistics.median(t["oracle"])
            case["oracle"] = {"rounds": no, "accepted": st[0], "tokens": st[1],
                              "exact": bool(torch.equal(spec.tokens[:, :W], ref)), "decode_us": round(us, 1),
                              "tokens_per_s": round(Bm * (new - 1) / us * 1e6, 1),
                              "plain_tokens_per_s": round(Bm / case["step"]["us"] * 1e6, 1)}
            block = torch.randint(0, 50257, (Bm, 16), device=dev, generator=gen).repeat(1, prompt // 16)
            for name, p in (("repeated_block", block), ("random_ids", ids)):
                want = model.generate(p, max_new_tokens=new)
                got = model.generate(p, max_new_tokens=new, prompt_lookup_num_tokens=K)
                tp, tl = [], []
                for _ in range(a.rounds):
                    for v, kw in ((tp, {}), (tl, {"prompt_lookup_num_tokens": K})):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        model.generate(p, max_new_tokens=new, **kw)
                        torch.cuda.synchronize()
                        v.append(time.perf_counter() - t0)
                s = model.last_generate_stats
                case[name] = {"exact": bool(torch.equal(want, got)), **s,
                              "accepted_per_round": round(s["accepted"] / s["rounds"], 3),
                              "tokens_per_round_and_sequence": round(s["tokens"] / s["rounds"] / Bm, 3),
                              "plain_call_s": round(statistics.median(tp), 4),
                              "lookup_call_s": round(statistics.median(tl), 4),
                              "plain_tokens_per_s": round(Bm * new / statistics.median(tp), 1),
                              "lookup_tokens_per_s": round(Bm * new / statistics.median(tl), 1)}
            cases.append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del plain, spec
            model.__dict__.pop("_kml_decode_caches", None)
    out["model"] = cases
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true", help="no GEMM / attention sweeps")
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--prompt-lookup", default=None, metavar="K[,K...]",
                    help="only the prompt-lookup (speculative decoding) measurements, for these draft counts")
    ap.add_argument("--activation", choices=("gelu", "gelu_tanh"), default="gelu",
                    help="the model's FFN activation (the kernel sweeps keep their own)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_gpt_decode: needs a GPU (no fall-back)", file=sys.stderr)
        sys.exit(2)
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.nn import modules as NM
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    BF = torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)

    def graphed(fn):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with capture_graph(g):
            fn()
        return g.replay

    def alternate(runs, per_run):
        """median (min, max) microseconds per launch of every variant, alternating inside a round"""
        times = {k: [] for k in runs}
        for k, run in runs.items():
            run()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / per_run)
        return {k: {"us": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                for k, v in times.items()}

    res = {"device": torch.cuda.get_device_name(0), "chunk": D.attn_decode_chunk(), "rounds": a.rounds,
           "iters": a.iters, "activation": a.activation}
    if a.prompt_lookup is not None:
        res["prompt_lookup"] = prompt_lookup(a, [int(k) for k in a.prompt_lookup.split(",")], graphed, alternate)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    filt = dict(top_k=a.top_k, top_p=a.top_p, repetition_penalty=a.repetition_penalty)
    filtered = a.top_k != 0 or a.top_p != 1.0 or a.repetition_penalty != 1.0
    res["filters"] = filt if filtered else None

    # ------------------------------------------------------------------ skinny GEMM vs existing
    def existing(x, w, bias, act):
        M, Kd = x.shape
        N = w.shape[0]
        y = K.conv_fwd(x.view(M, 1, 1, Kd), w.view(N, 1, 1, Kd), 1, 1, (1, 1), (0, 0), bias=bias).view(M, N)
        return T.gelu_fwd(y) if act == "gelu" else y

    if not a.skip_kernels:
        gemm = []
        for name, N, Kd, act, has_bias in SHAPES:
            copies = max(2, min(48, -(-(64 << 20) // (N * Kd * 2))))
            ws = [(torch.randn(N, Kd, device=dev, generator=gen) * 0.02).to(BF) for _ in range(copies)]
            bias = torch.randn(N, device=dev, generator=gen) if has_bias else None
            for M in (1, 4, 8, 16):
                x = torch.randn(M, Kd, device=dev, generator=gen).to(BF)
                out = torch.empty(M, N, dtype=BF, device=dev)
                ring = [ws[i % copies] for i in range(a.iters)]

                def sk():
                    for w in ring:
                        D.gemm_skinny(x, w, bias, act=act, out=out)

                def ex():
                    for w in ring:
                        existing(x, w, bias, act)
                runs = {"skinny": graphed(sk), "existing": graphed(ex)}
                if M == 4 and N == 768:       # the K-split sweep behind the plan of the two narrow shapes
                    for S in (1, 2, 4, 8):
                        def sks(S=S):
                            for w in ring:
                                D.gemm_skinny(x, w, bias, act=act, out=out, splits=S)
                        runs[f"skinny_splits_{S}"] = graphed(sks)
                r = alternate(runs, a.iters)
                floor = N * Kd * 2 / 6.3e12 * 1e6
                gemm.append({"shape": name, "N": N, "K": Kd, "M": M, "splits": int(D.HIP.raw("kml_gemm_skinny_splits", N, Kd)),
                             **r, "weight_floor_us_derived": round(floor, 3)})
                print(json.dumps(gemm[-1]), file=sys.stderr, flush=True)
            del ws
        res["gemm"] = gemm

        # ------------------------------------------------------------------ decode attention, chunk sweep
        B, H, Lcap = 4, 12, 1024
        kc = torch.randn(B, H, Lcap, 64, device=dev, generator=gen).to(BF)
        vc = torch.randn(B, H, Lcap, 64, device=dev, generator=gen).to(BF)
        q = torch.randn(B, 3 * H * 64, device=dev, generator=gen).to(BF)
        wsb = D.attn_decode_workspace(B, H, Lcap, dev)
        o = torch.empty(B, H * 64, dtype=BF, device=dev)
        attn = []
        for n in (128, 512, 1023):
            lens = torch.full((B,), n - 1, dtype=torch.int32, device=dev)
            runs = {}
            for c in (64, 128, 256, 512):
                def f(c=c):
                    for _ in range(a.iters):
                        D.attn_decode(q, kc, vc, lens, ws=wsb, out=o, chunk=c)
                runs[str(c)] = graphed(f)
            r = alternate(runs, a.iters)
            attn.append({"keys": n, "B": B, "H": H, "Lcap": Lcap, "chunk_us": r})
            print(json.dumps(attn[-1]), file=sys.stderr, flush=True)
        res["attention"] = attn

    # ------------------------------------------------------------------ the sampler alone
    fk = filt if filtered else dict(top_k=50, top_p=0.95, repetition_penalty=1.2)
    fpar, ipar = D.sampling_params(1.0, fk["top_k"], fk["top_p"], fk["repetition_penalty"])
    sampler = []
    for Bm in (1, 4, 16):
        logits = (torch.randn(Bm, 50264, device=dev, generator=gen) * 3.0).to(BF)

        def state():
            st = dict(ctl=torch.tensor([1, 0, -1, 0], dtype=torch.int32, device=dev),
                      next_ids=torch.zeros(Bm, dtype=torch.int64, device=dev),
                      tokens=torch.randint(0, 50257, (Bm, 1024), device=dev, generator=gen),
                      lens=torch.full((Bm,), 383, dtype=torch.int32, device=dev),
                      finished=torch.zeros(Bm, dtype=torch.int32, device=dev))
            return st
        sa, ss = state(), state()
        temp = torch.ones(1, device=dev)
        fp, ip = torch.tensor(fpar, device=dev), torch.tensor(ipar, dtype=torch.int32, device=dev)
        info = torch.empty(Bm, 4, device=dev)

        def adv():
            for _ in range(a.iters):
                D.decode_advance(logits, 50257, temp=temp, sample=True, **sa)

        def smp():
            for _ in range(a.iters):
                D.decode_sample(logits, 50257, fpar=fp, ipar=ip, sample=True, info=info, **ss)
        r = alternate({"kml_decode_advance": graphed(adv), "kml_decode_sample": graphed(smp)}, a.iters)
        sampler.append({"B": Bm, "classes": 50257, "history": 384, **fk, **r})
        print(json.dumps(sampler[-1]), file=sys.stderr, flush=True)
    res["sampler"] = sampler

    # ------------------------------------------------------------------ the model
    if not a.skip_model:
        from kubeml_amd.models.gpt import gpt2_small
        from kubeml_amd.nn import flatten_module
        torch.manual_seed(0)
        model = gpt2_small(dropout=0.0, activation=a.activation).to(dev).eval()
        flatten_module(model)
        tr = model.transformer
        wbytes = 2 * (sum(l.out_pad * l.in_pad for blk in tr.h
                          for l in (blk.attn.qkv, blk.attn.out, blk.mlp.c_fc, blk.mlp.c_proj)) +
                      model.lm_head.out_pad * model.lm_head.in_pad)
        res["weight_bytes_per_token"] = wbytes
        res["weight_stream_floor_us_derived"] = round(wbytes / 6.3e12 * 1e6, 2)
        prompt, new = 128, a.new
        routes = NM._SMALL_EXISTING
        res["small_existing_routes"] = {f"{n}x{k}": m for (n, k), m in routes.items()}
        decode = []
        for Bm in (1, 4, 16):
            ids = torch.randint(0, 50257, (Bm, prompt), device=dev, generator=gen)
            per = {}
            caches = {}
            kws = {"generate": {}, "existing_linears": {}}
            if filtered:
                kws["filtered"] = dict(temperature=1.0, seed=1, **filt)
            for variant in kws:
                NM._SMALL_EXISTING = _Everything() if variant == "existing_linears" else routes
                caches[variant] = model.new_cache(Bm, prompt + new, dev)
                caches[variant].reset(**kws[variant])
                model.prefill(ids, None, caches[variant])
                model.decode_step(caches[variant])       # capture under this variant's routing
            NM._SMALL_EXISTING = routes
            times = {v: [] for v in caches}
            for _ in range(a.rounds):
                for variant, cache in caches.items():
                    cache.reset(**kws[variant])
                    model.prefill(ids, None, cache)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(new - 1):
                        model.decode_step(cache)
                    e1.record()
                    e1.synchronize()
                    times[variant].append(e0.elapsed_time(e1) * 1e3 / (new - 1))
            for variant, v in times.items():
                us = statistics.median(v)
                per[variant] = {"us_per_token_step": round(us, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                                "tokens_per_s": round(Bm / us * 1e6, 1)}
            # whole generate() call, prefill and host loop included
            t0 = time.perf_counter()
            model.generate(ids, max_new_tokens=new)
            torch.cuda.synchronize()
            per["generate_call_s"] = round(time.perf_counter() - t0, 4)
            if Bm == 1:
                seq = ids.clone()
                with torch.no_grad():
                    model(seq)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(32):
                        z = model(seq)
                        seq = torch.cat([seq, z[-1:, :50257].float().argmax(-1, keepdim=True)], 1)
                    torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / 32 * 1e6
                per["recompute"] = {"us_per_token_step": round(us, 2), "tokens_per_s": round(1e6 / us, 1), "tokens": 32}
            decode.append({"B": Bm, "prompt": prompt, "new": new, **per})
            print(json.dumps(decode[-1]), file=sys.stderr, flush=True)
            del caches
            model.__dict__.pop("_kml_decode_caches", None)
        res["decode"] = decode

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
