"""KV-cache decoding of the 576 / 9 / 3 / 1536 x 30-layer Llama model of tools/bench_llama.py
(random weights) on one GPU: the captured decode step, and each of its three new kernels beside the
launches it replaces.

    python tools/bench_llama_decode.py [--rounds 7] [--iters 20] [--new 256] [--skip-model] [--out FILE.json]
                                       [--preset {576,tinyllama}] [--weights {bf16,int8}]

``--preset tinyllama``: the TinyLlama-1.1B shape (hidden 2048, 32 heads / 4 K/V heads, inter 5632, 22
layers, vocab 32000), random weights.  ``--weights int8``: only the weight-only int8 comparison —
* w8: ``gemm_skinny_w8`` / ``gemm_skinny_glu_w8`` against the bf16 kernels on the preset's five weight
  shapes, M in {1, 4, 16}, alternating; every launch reads the next of a ring of weight copies of more
  than 320 MB per variant (past the 256 MB last-level cache).  ``floor_us``: the variant's weight bytes
  over 6.3 TB/s — derived, not measured.
* step: the captured step in bf16 and after ``quantize_decode_weights("int8")``, alternating, B in
  {1, 4, 16}; ``floor_us`` / ``floor_us_int8``: the weight bytes a token reads, derived the same way.
  Layers whose shape is in ``nn.modules._SMALL_W8_SLOWER`` (all of the 576 preset's) stay bf16 in the
  step; the w8 section calls the kernels directly and measures them whatever the table says.

* step: B in {1, 4, 16}, prompt 128, ``--new`` tokens: the captured step of ``generate``
  (``decode_step`` replays, timed between device events after the prefill) and the same step with
  the MLP as ``gemm_skinny`` + ``swiglu_fwd`` (``mlp_unfused``), alternating inside every round;
  tokens/s = B / step.  ``floor_us``: the bf16 weight bytes one token reads over the 6.3 TB/s the
  microarchitecture notes give as the achievable HBM rate — derived, not measured.
* glu: ``gemm_skinny_glu`` against ``gemm_skinny`` + ``swiglu_fwd`` on the [2 x 1536, 576] weight,
  M in {1, 4, 16}, every launch on the next of a ring of weight copies (> 64 MB: no L2 hits).
* attention: ``attn_decode_gqa`` (its own choice of heads per block, then 1 and 4 forced) against
  ``attn_decode`` on the repeat-interleaved cache, B in {4, 16}, (H, Hkv) in {(9, 3), (8, 1), (32, 4)},
  Lcap 4096, 384 and 4096 keys.
* append: ``kv_append_rope`` against ``rope_`` + the append-only launch, B in {1, 16}, H = 9, Hkv = 3.
Kernel figures: ``iters`` launches per captured graph, variants alternating, median (min, max) us.

Prints one JSON line.
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
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--preset", choices=("576", "tinyllama"), default="576")
    ap.add_argument("--weights", choices=("bf16", "int8"), default="bf16")
    a = ap.parse_args()
    cfg = {"576": dict(hidden=576, heads=9, kv_heads=3, inter=1536, layers=30, vocab=32000),
           "tinyllama": dict(hidden=2048, heads=32, kv_heads=4, inter=5632, layers=22, vocab=32000)}[a.preset]
    import torch
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.nn.transformer import rope_table
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import transformer as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_llama_decode: no GPU")
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
        for run in runs.values():
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

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=gen).to(BF)

    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "preset": a.preset,
           "weights": a.weights}
    if a.weights == "int8":
        return w8_bench(a, cfg, res, torch, D, dev, graphed, alternate, rnd)

    # ---- the gated GEMM alone
    I, K, ring = 1536, 576, 20
    ws = [rnd(2 * I, K) * 0.05 for _ in range(ring)]
    res["glu"] = []
    for M in (1, 4, 16):
        x, h, gu = rnd(M, K), torch.empty(M, I, dtype=BF, device=dev), torch.empty(M, 2 * I, dtype=BF, device=dev)

        def fused():
            for i in range(a.iters):
                D.gemm_skinny_glu(x, ws[i % ring], out=h)

        def pair():
            for i in range(a.iters):
                T.swiglu_fwd(D.gemm_skinny(x, ws[i % ring], out=gu))
        res["glu"].append({"M": M, **alternate({"fused": graphed(fused), "gemm+swiglu": graphed(pair)}, a.iters)})

    # ---- grouped-query decode attention alone
    res["attention"] = []
    Lcap = 4096
    for B, H, Hkv in ((4, 9, 3), (4, 8, 1), (16, 32, 4)):
        kc, vc, q = rnd(B, Hkv, Lcap, 64), rnd(B, Hkv, Lcap, 64), rnd(B, H * 64)
        kr, vr = (t.repeat_interleave(H // Hkv, 1).contiguous() for t in (kc, vc))
        wsa, o = D.attn_decode_gqa_workspace(B, H, Lcap, dev), torch.empty(B, H * 64, dtype=BF, device=dev)
        for n in (384, 4096):
            lens = torch.full((B,), n - 1, dtype=torch.int32, device=dev)

            def gqa(hpb):
                def f():
                    for _ in range(a.iters):
                        D.attn_decode_gqa(q, kc, vc, lens, H, ws=wsa, out=o, heads_per_block=hpb)
                return f

            def repeated():
                for _ in range(a.iters):
                    D.attn_decode(q, kr, vr, lens, ws=wsa, out=o)
            res["attention"].append({"H": H, "Hkv": Hkv, "keys": n, "B": B,
                                     **alternate({"gqa": graphed(gqa(None)), "gqa_1_head": graphed(gqa(1)),
                                                  "gqa_4_heads": graphed(gqa(4)), "repeated": graphed(repeated)},
                                                 a.iters)})

    # ---- the append alone
    res["append"] = []
    H, Hkv, table = 9, 3, rope_table(2048).to(dev)
    for B in (1, 16):
        qkv, kc, vc = rnd(B, (H + 2 * Hkv) * 64), rnd(B, Hkv, 512, 64), rnd(B, Hkv, 512, 64)
        lens = torch.full((B,), 300, dtype=torch.int32, device=dev)

        def fused():
            for _ in range(a.iters):
                D.kv_append_rope(qkv, kc, vc, 1, H, table, lens=lens)

        def pair():
            for _ in range(a.iters):
                T.rope_(qkv, table, 1, H, Hkv)
                D.kv_append_rope(qkv, kc, vc, 1, H, table, lens=lens, rotate=False)
        res["append"].append({"B": B, **alternate({"fused": graphed(fused), "rope+append": graphed(pair)}, a.iters)})

    # ---- the captured step
    if not a.skip_model:
        from kubeml_amd.models.llama import LlamaForCausalLM, LlamaMLP
        from kubeml_amd.nn import flatten_module
        from kubeml_amd.nn.flat import shadow_of
        torch.manual_seed(0)
        model = LlamaForCausalLM(**cfg).to(dev).eval()
        flatten_module(model)
        wbytes = 2 * sum(p.numel() for n, p in model.named_parameters() if "embed_tokens" not in n)
        res["floor_us"] = round(wbytes / 6.3e12 * 1e6, 2)
        fused_small = LlamaMLP.forward_small

        def unfused_small(self, x):
            gu = self.gate_up
            w = shadow_of(gu.weight).view(gu.out_pad, gu.in_pad)
            return self.down_proj.forward_small(T.swiglu_fwd(D.gemm_skinny(x.contiguous(), w)))
        prompt, new = 128, a.new
        res["step"] = []
        for B in (1, 4, 16):
            ids = torch.randint(0, cfg["vocab"], (B, prompt), device=dev, generator=gen)
            caches = {}
            for name, fs in (("step", fused_small), ("mlp_unfused", unfused_small)):
                LlamaMLP.forward_small = fs
                c = caches[name] = model.new_cache(B, prompt + new, dev)
                c.reset()
                model.prefill(ids, None, c)
                model.decode_step(c)   # capture, with this variant's launches
            LlamaMLP.forward_small = fused_small

            def run(c):
                def go():
                    c.reset()
                    model.prefill(ids, None, c)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(new - 1):
                        model.decode_step(c)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / (new - 1)
                return go
            times = {k: [] for k in caches}
            for _ in range(a.rounds):
                for k, c in caches.items():
                    times[k].append(run(c)())
            row = {"B": B}
            for k, v in times.items():
                us = statistics.median(v)
                row[k] = {"us": round(us, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                          "tokens_per_s": round(B / us * 1e6, 1)}
            res["step"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)

    finish(a, res)


def finish(a, res):
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def w8_bench(a, cfg, res, torch, D, dev, graphed, alternate, rnd):
    """``--weights int8``: bf16 against int8, single GEMMs and the captured step."""
    BF = torch.bfloat16
    hid, inter, hd = cfg["hidden"], cfg["inter"], 64
    shapes = [("qkv", (cfg["heads"] + 2 * cfg["kv_heads"]) * hd, hid, False), ("o_proj", hid, hid, False),
              ("gate_up", 2 * inter, hid, True), ("down_proj", hid, inter, False), ("lm_head", cfg["vocab"], hid, False)]
    res["w8"] = []
    for name, N, K, glu in shapes:
        ring = max(a.iters, -(-320 * 2 ** 20 // (N * K)))   # int8 copies of N*K bytes: > 320 MB; bf16: twice that
        wb = [rnd(N, K) * 0.05 for _ in range(ring)]
        wq = [D.quant_rows_i8(w) for w in wb]
        for M in (1, 4, 16):
            x = rnd(M, K)
            o = torch.empty(M, N // 2 if glu else N, dtype=BF, device=dev)

            def bf16():
                for w in wb:
                    (D.gemm_skinny_glu if glu else D.gemm_skinny)(x, w, out=o)

            def int8():
                for q, sc in wq:
                    (D.gemm_skinny_glu_w8(x, q, sc, out=o) if glu else D.gemm_skinny_w8(x, q, sc, out=o))
            row = {"layer": name, "N": N, "K": K, "M": M, "ring": ring,
                   "floor_us": {"bf16": round(2 * N * K / 6.3e6, 3), "int8": round(N * K / 6.3e6, 3)},
                   **alternate({"bf16": graphed(bf16), "int8": graphed(int8)}, ring)}
            res["w8"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del wb, wq
        torch.cuda.empty_cache()
    if not a.skip_model:
        from kubeml_amd.models.llama import LlamaForCausalLM
        from kubeml_amd.nn import flatten_module
        torch.manual_seed(0)
        model = LlamaForCausalLM(**cfg).to(dev).eval()
        flatten_module(model)
        wbytes = sum(p.numel() for n, p in model.named_parameters() if "embed_tokens" not in n)
        res["floor_us"], res["floor_us_int8"] = round(2 * wbytes / 6.3e6, 2), round(wbytes / 6.3e6, 2)
        prompt, new = 128, a.new
        res["step"] = []
        for B in (1, 4, 16):
            ids = torch.randint(0, cfg["vocab"], (B, prompt), device=dev)
            c = model.new_cache(B, prompt + new, dev)
            times = {"bf16": [], "int8": []}
            for _ in range(a.rounds + 1):   # the first round is a warm-up and is dropped
                for k in times:
                    # switching retires the captured step: the untimed decode_step below captures this variant's
                    model.quantize_decode_weights(None if k == "bf16" else "int8")
                    c.reset()
                    model.prefill(ids, None, c)
                    model.decode_step(c)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(new - 2):
                        model.decode_step(c)
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / (new - 2))
            row = {"B": B}
            for k, v in times.items():
                us = statistics.median(v[1:])
                row[k] = {"us": round(us, 2), "min": round(min(v[1:]), 2), "max": round(max(v[1:]), 2),
                          "tokens_per_s": round(B / us * 1e6, 1)}
            res["step"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    finish(a, res)


if __name__ == "__main__":
    main()
