"""Llama-style causal-LM training throughput on MI355X, and the four Llama kernels alone at that
model's shapes (not the headline bench — see bench.py).  Synthetic token batches, random init:
30 layers, hidden 576, 9 heads / 3 K/V heads, inter 1536, vocab 49152, tied head; fused AdamW, bf16
compute, fp32 master weights, the whole step captured as one hipGraph.

    python tools/bench_llama.py [--batch 16] [--seq 1024] [--steps 10] [--warmup 2] [--layers 30]
                                [--no-step] [--no-kernels] [--reps 20] [--head-dim 128]
Prints one JSON line per part: the kernels, then the step (tokens/s over all processed tokens).
The kernel part gives call times: device events around one launcher call on an idle queue, so each
includes the launcher's host path (output allocation, the ctypes call) — RMSNorm, RoPE and SwiGLU
forward / backward beside their HBM floors (bytes moved over 6.3 TB/s), and the grouped-query
attention (H = 9, Hkv = 3) forward and backward beside the existing causal kernels at H = 9,
Hkv = 9, the compared calls alternating inside one timing loop.  Kernel times (and the split of an
attention backward into dQ and dKV) come from a kernel trace of ``--no-step`` in a run of its own:

    rocprofv3 --kernel-trace -d out -o run -- python tools/bench_llama.py --no-step
    python tools/rocpd_summary.py out/*/run_results.db

``--head-dim 128`` switches both parts to a head-dim-128 model (hidden 2048, 16 heads / 4 K/V heads,
inter 5632, vocab 32000, untied) and the kernel part to csrc/kernels/attention_d128.hip: the forward
call and the backward call (dQ and dKV launches; their split again from the kernel trace) at H = 16,
Hkv = 4, D = 128, taking turns in one loop with the D = 64 kernels at H = 32, Hkv = 8 (the same
FLOPs and bytes) and with ``torch.nn.functional.scaled_dot_product_attention`` on the D = 128
operands (K/V heads repeated beforehand), and RoPE at 128 forward / backward; median and range.

``--docs N [N ...]`` times only the attention forward and backward calls with ``key_start`` (rows
packed from N equal documents; the band kernels) beside the plain causal calls on the same operands,
at the head dim of ``--head-dim``: ``python tools/bench_llama.py --docs 1 4 16 [--head-dim 128]``.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12
CFG = dict(vocab=49152, hidden=576, heads=9, kv_heads=3, inter=1536, max_pos=2048, tie_word_embeddings=True)
CFG128 = dict(vocab=32000, hidden=2048, heads=16, kv_heads=4, inter=5632, max_pos=2048, head_dim=128)


def bench_step(a, torch):
    from kubeml_amd.engine.step import GraphedTrainStep
    from kubeml_amd.models.llama import LlamaForCausalLM
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    dev = torch.device("cuda", 0)
    cfg = CFG128 if a.head_dim == 128 else CFG
    m = LlamaForCausalLM(layers=a.layers, seed=1, **cfg).to(dev)
    sp = flatten_module(m)
    m.train()
    opt = AdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
    B, L = a.batch, a.seq
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(0, m.vocab, (B, L), device=dev, generator=g)

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
    name = "/".join(str(cfg[k]) for k in ("hidden", "heads", "kv_heads", "inter"))
    print(json.dumps({"metric": f"Llama {name} (head dim {a.head_dim}) causal-LM training tokens/s",
                      "value": round(B * L * a.steps / dt, 1), "unit": "tokens/s", "n_gpus": 1,
                      "ms_per_step": round(dt / a.steps * 1e3, 3), "batch_per_gpu": B, "seq": L, "layers": a.layers,
                      "params": sum(p.numel() for p in m.parameters()), "optimizer": "fused AdamW", "dtype": "bf16",
                      "data": "synthetic tokens, random init", "graph": not a.no_graph,
                      "loss_first_last": [round(first, 4), round(float(loss.detach()), 4)]}), flush=True)


def _time_alternating(torch, fns, reps, spread=False):
    """device-event ms around one call of each fn on an idle queue (host path included), the fns
    taking turns inside one loop (after a warm-up round); returns the median of ``reps`` rounds per fn
    (spread: (median, min, max))"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    if spread:
        return [(sorted(v)[len(v) // 2], min(v), max(v)) for v in ms]
    return [sorted(v)[len(v) // 2] for v in ms]


def bench_kernels128(a, torch):
    """the head-dim-128 attention calls beside D = 64 at twice the heads and torch SDPA; RoPE at 128"""
    import torch.nn.functional as F
    from kubeml_amd.nn.transformer import _split_qkv, rope_table
    from kubeml_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    B, L, H, Hkv = a.batch, a.seq, CFG128["heads"], CFG128["kv_heads"]
    Tn = B * L
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    dout = rnd(Tn, H * 128)
    runs = {}
    for name, D, h, hkv in (("d128", 128, H, Hkv), ("d64", 64, 2 * H, 2 * Hkv)):
        buf = rnd(Tn, (h + 2 * hkv) * D) * 0.5
        q, k, v = _split_qkv(buf, h, hkv, D)
        o, lse = T.attn_fwd(q, k, v, B, h, L, causal=True, kv_heads=hkv, head_dim=D)
        dq, dk, dv = _split_qkv(torch.empty_like(buf), h, hkv, D)
        runs[name + "_fwd"] = lambda q=q, k=k, v=v, h=h, hkv=hkv, D=D: T.attn_fwd(
            q, k, v, B, h, L, causal=True, kv_heads=hkv, head_dim=D)
        runs[name + "_bwd"] = lambda q=q, k=k, v=v, o=o, lse=lse, dq=dq, dk=dk, dv=dv, h=h, hkv=hkv, D=D: T.attn_bwd(
            q, k, v, o, dout, lse, B, h, L, dq=dq, dk=dk, dv=dv, causal=True, kv_heads=hkv, head_dim=D)
        if D == 128:   # torch SDPA on the same operands, [B, H, L, 128], K/V heads repeated once outside the timing
            sq, sk, sv = (t.reshape(B, L, -1, D).transpose(1, 2) for t in (q, k, v))
            sk, sv = (t.repeat_interleave(H // Hkv, dim=1) for t in (sk, sv))
            sq, sk, sv = (t.contiguous().requires_grad_(True) for t in (sq, sk, sv))
            so = F.scaled_dot_product_attention(sq, sk, sv, is_causal=True)
            sdo = dout.reshape(B, L, H, D).transpose(1, 2).contiguous()
            runs["sdpa_fwd"] = lambda sq=sq, sk=sk, sv=sv: F.scaled_dot_product_attention(sq, sk, sv, is_causal=True)
            runs["sdpa_bwd"] = lambda so=so, sq=sq, sk=sk, sv=sv: torch.autograd.grad(so, (sq, sk, sv), sdo,
                                                                                      retain_graph=True)
    qkv = rnd(Tn, (H + 2 * Hkv) * 128) * 0.5
    table = rope_table(L, 10000.0, device=dev, head_dim=128)
    runs["rope128_fwd"] = lambda: T.rope_(qkv, table, L, H, Hkv)
    runs["rope128_bwd"] = lambda: T.rope_(qkv, table, L, H, Hkv, backward=True)
    names = ["d128_fwd", "d64_fwd", "sdpa_fwd", "d128_bwd", "d64_bwd", "sdpa_bwd", "rope128_fwd", "rope128_bwd"]
    out = {"batch": B, "seq": L, "reps": a.reps, "heads_d128": [H, Hkv], "heads_d64": [2 * H, 2 * Hkv]}
    for n, (med, lo, hi) in zip(names, _time_alternating(torch, [runs[n] for n in names], a.reps, spread=True)):
        out[n] = {"call_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
    # causal attention: 2 GEMMs forward, 5 backward, half of the L x L tiles
    flops = 0.5 * 4.0 * B * H * L * L * 128
    out["causal_fwd_flops"] = flops
    out["rope_hbm_floor_ms"] = round(2 * Tn * (H + Hkv) * 128 * 2 / HBM_BYTES_PER_S * 1e3, 4)
    print(json.dumps({"metric": "head-dim-128 attention calls (device events around one call; median, range)",
                      **out}), flush=True)


def bench_docs(a, torch):
    """the band attention calls (key_start of N equal documents a row, for every N of --docs) beside
    the plain causal calls on the same operands, all taking turns in one loop; median and range"""
    from kubeml_amd.nn.transformer import _split_qkv, doc_key_start
    from kubeml_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    D, cfg = a.head_dim, CFG128 if a.head_dim == 128 else CFG
    B, L, H, Hkv = a.batch, a.seq, cfg["heads"], cfg["kv_heads"]
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    buf, dout = rnd(B * L, (H + 2 * Hkv) * D) * 0.5, rnd(B * L, H * D)
    q, k, v = _split_qkv(buf, H, Hkv, D)
    dq, dk, dv = _split_qkv(torch.empty_like(buf), H, Hkv, D)
    kw = dict(causal=True, kv_heads=Hkv, head_dim=D)
    runs = {}
    for n in [0] + a.docs:   # 0: no key_start, the plain causal kernels
        ks = None
        if n:
            ks = doc_key_start((torch.arange(L, device=dev) * n // L).expand(B, L))
        o, lse = T.attn_fwd(q, k, v, B, H, L, key_start=ks, **kw)
        name = f"docs{n}" if n else "causal"
        runs[name + "_fwd"] = lambda ks=ks: T.attn_fwd(q, k, v, B, H, L, key_start=ks, **kw)
        runs[name + "_bwd"] = lambda ks=ks, o=o, lse=lse: T.attn_bwd(q, k, v, o, dout, lse, B, H, L, dq=dq, dk=dk,
                                                                     dv=dv, key_start=ks, **kw)
    out = {"batch": B, "seq": L, "reps": a.reps, "head_dim": D, "heads": [H, Hkv]}
    for n, (med, lo, hi) in zip(runs, _time_alternating(torch, list(runs.values()), a.reps, spread=True)):
        out[n] = {"call_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
    print(json.dumps({"metric": "band attention calls, N equal documents a row (device events around one call; "
                                "median, range)", **out}), flush=True)


def bench_kernels(a, torch):
    from kubeml_amd.nn.transformer import _split_qkv, rope_table
    from kubeml_amd.ops import transformer as T
    dev = torch.device("cuda", 0)
    B, L, H, Hkv, N, I = a.batch, a.seq, CFG["heads"], CFG["kv_heads"], CFG["hidden"], CFG["inter"]
    Tn = B * L
    g = torch.Generator(device=dev).manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)
    out = {"batch": B, "seq": L, "reps": a.reps, "hbm_bytes_per_s": HBM_BYTES_PER_S}

    def put(name, ms, nbytes):
        out[name] = {"call_ms": round(ms, 4), "hbm_floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4)}

    # RMSNorm with the residual stream: reads x, res, writes y, sum; backward reads dy, s, dx_add, writes dx
    x, r, dy, da = rnd(Tn, N), rnd(Tn, N), rnd(Tn, N), rnd(Tn, N)
    gam, dgam = torch.ones(N, device=dev), torch.zeros(N, device=dev)
    y, s, rstd = T.rmsnorm_fwd(x, gam, res=r)
    f, b = _time_alternating(torch, [lambda: T.rmsnorm_fwd(x, gam, res=r),
                                     lambda: T.rmsnorm_bwd(dy, s, rstd, gam, dgam, dx_add=da)], a.reps)
    put("rmsnorm_fwd", f, 4 * Tn * N * 2)
    put("rmsnorm_bwd", b, 4 * Tn * N * 2)
    # RoPE in place: reads and writes the Q and K columns
    qkv = rnd(Tn, (H + 2 * Hkv) * 64) * 0.5
    table = rope_table(L, 10000.0, device=dev)
    f, b = _time_alternating(torch, [lambda: T.rope_(qkv, table, L, H, Hkv),
                                     lambda: T.rope_(qkv, table, L, H, Hkv, backward=True)], a.reps)
    put("rope_fwd", f, 2 * Tn * (H + Hkv) * 64 * 2)
    put("rope_bwd", b, 2 * Tn * (H + Hkv) * 64 * 2)
    # SwiGLU: reads gu (2 I), writes h (I); backward reads dh (I), gu (2 I), writes dgu (2 I)
    gu, dh = rnd(Tn, 2 * I), rnd(Tn, I)
    f, b = _time_alternating(torch, [lambda: T.swiglu_fwd(gu), lambda: T.swiglu_bwd(dh, gu)], a.reps)
    put("swiglu_fwd", f, 3 * Tn * I * 2)
    put("swiglu_bwd", b, 5 * Tn * I * 2)
    # attention: GQA (H, Hkv) beside the existing causal kernels at (H, H), alternating
    dout = rnd(Tn, H * 64)
    wide = rnd(Tn, 3 * H * 64) * 0.5
    runs = {}
    for name, buf, kvh, kw in (("gqa", qkv, Hkv, Hkv), ("mha", wide, H, None)):
        q, k, v = _split_qkv(buf, H, kvh)
        o, lse = T.attn_fwd(q, k, v, B, H, L, causal=True, kv_heads=kw)
        dbuf = torch.empty_like(buf)
        dq, dk, dv = _split_qkv(dbuf, H, kvh)
        runs[name + "_fwd"] = lambda q=q, k=k, v=v, kw=kw: T.attn_fwd(q, k, v, B, H, L, causal=True, kv_heads=kw)
        runs[name + "_bwd"] = lambda q=q, k=k, v=v, o=o, lse=lse, dq=dq, dk=dk, dv=dv, kw=kw: T.attn_bwd(
            q, k, v, o, dout, lse, B, H, L, dq=dq, dk=dk, dv=dv, causal=True, kv_heads=kw)
    names = ["gqa_fwd", "mha_fwd", "gqa_bwd", "mha_bwd"]
    for n, ms in zip(names, _time_alternating(torch, [runs[n] for n in names], a.reps)):
        out["attn_" + n] = {"call_ms": round(ms, 4)}
    print(json.dumps({"metric": "Llama kernel calls at the model's shapes (device events around one call, median)",
                      **out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--head-dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--docs", type=int, nargs="+", default=[], metavar="N")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_llama.py needs a GPU")
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    if a.docs:   # the packed-document attention calls alone
        return bench_docs(a, torch)
    if not a.no_kernels:
        (bench_kernels128 if a.head_dim == 128 else bench_kernels)(a, torch)
    if not a.no_step:
        bench_step(a, torch)


if __name__ == "__main__":
    main()
