"""KV-cache decoding of the Llama-style model on the GPU: the append that rotates (RoPE) into an
Hkv-head cache, grouped-query decode attention and the gated skinny GEMM, each bit-compared with
the kernels it replaces and measured against fp64 with those kernels as the yardstick (an error of
at most twice theirs); then teacher-forced logits against the fp64 CPU model and ``generate``."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _guarded(B, H, Lcap, guard=512):
    """K and V as views inside ONE allocation with `guard` elements of 7.0 before, between and after"""
    n = B * H * Lcap * 64
    buf = torch.full((3 * guard + 2 * n,), 7.0, dtype=BF, device=dev)
    return buf, buf[guard:guard + n].view(B, H, Lcap, 64), buf[2 * guard + n:2 * guard + 2 * n].view(B, H, Lcap, 64)


@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 1)])
@pytest.mark.parametrize("lens", [(0, 63), (64, 127), (5, 130)])   # 130 >= Lcap: that sequence is dropped
def test_append_rope_decode_is_kml_rope_then_placement(H, Hkv, lens):
    from kubeml_amd.nn.transformer import rope_reference, rope_table
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import transformer as T
    B, Lcap, max_pos = 2, 128, 256
    nq, nk = H * 64, Hkv * 64
    table = rope_table(max_pos).to(dev)
    qkv = torch.randn(B, nq + 2 * nk, generator=torch.Generator().manual_seed(H)).to(BF).to(dev)
    # kml_rope rotates row p of an L-row sequence at position p: put each row at its own position
    seq = torch.zeros(max_pos, nq + 2 * nk, dtype=BF, device=dev)
    seq[list(lens)] = qkv
    rot = T.rope_(seq, table, max_pos, H, Hkv)[list(lens)]
    buf, kc, vc = _guarded(B, Hkv, Lcap)
    expect = buf.clone()
    n = kc.numel()
    ek, ev = expect[512:512 + n].view_as(kc), expect[1024 + n:1024 + 2 * n].view_as(vc)
    for b, r in enumerate(lens):
        if r < Lcap:
            ek[b, :, r] = rot[b, nq:nq + nk].view(Hkv, 64)
            ev[b, :, r] = qkv[b, nq + nk:].view(Hkv, 64)
    got = qkv.clone()
    D.kv_append_rope(got, kc, vc, 1, H, table, lens=torch.tensor(lens, dtype=torch.int32, device=dev))
    assert torch.equal(buf, expect)                       # the rotated key and the value at lens[b], nothing else
    assert torch.equal(got[:, :nq], rot[:, :nq])          # Q rotated in place, the bits of kml_rope
    assert torch.equal(got[:, nq + nk:], qkv[:, nq + nk:])
    # accuracy against the fp64 rotation from the same table, kml_rope as the yardstick
    ref = rope_reference(qkv.double().cpu(), table.cpu(), 1, H, Hkv, pos=torch.tensor(lens))
    keep = [b for b, r in enumerate(lens) if r < Lcap]
    mine = torch.cat([got[keep, :nq], torch.stack([kc[b, :, lens[b]].reshape(nk) for b in keep])], 1)
    e, ey = _rel(mine, ref[keep, :nq + nk]), _rel(rot[keep, :nq + nk], ref[keep, :nq + nk])
    print(f"H {H} Hkv {Hkv} lens {lens}: append+rope {e:.3e}, kml_rope {ey:.3e}")
    assert e <= 2.0 * ey


@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 1)])
def test_append_rope_prefill_appends_without_rotating(H, Hkv):
    from kubeml_amd.nn.transformer import rope_table
    from kubeml_amd.ops import decode as D
    B, Lq, Lcap = 2, 5, 128
    nq, nk = H * 64, Hkv * 64
    qkv = torch.randn(B * Lq, nq + 2 * nk, generator=torch.Generator().manual_seed(9)).to(BF).to(dev)
    buf, kc, vc = _guarded(B, Hkv, Lcap)
    expect = buf.clone()
    n = kc.numel()
    expect[512:512 + n].view_as(kc)[:, :, :Lq] = qkv[:, nq:nq + nk].view(B, Lq, Hkv, 64).permute(0, 2, 1, 3)
    expect[1024 + n:1024 + 2 * n].view_as(vc)[:, :, :Lq] = qkv[:, nq + nk:].view(B, Lq, Hkv, 64).permute(0, 2, 1, 3)
    got = qkv.clone()
    D.kv_append_rope(got, kc, vc, Lq, H, rope_table(256).to(dev), rotate=False)
    assert torch.equal(buf, expect) and torch.equal(got, qkv)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (3, 1), (8, 1)])   # G = 1, 2, 3 (remainder), 8 (second z-group)
@pytest.mark.parametrize("hpb", [4, 1])   # both block shapes, whichever the grid size would pick
def test_gqa_decode_attention_is_attn_decode_on_the_repeated_cache(H, Hkv, hpb):
    from kubeml_amd.ops import decode as D
    C = D.attn_decode_chunk()
    G, Lcap = H // Hkv, -(-(2 * C + 8) // 64) * 64
    g = torch.Generator().manual_seed(10 * H + Hkv)
    for ns in ((1, C), (64, C + 1), (C - 1, 2 * C + 7)):   # keys per sequence; lens = n - 1
        B = len(ns)
        q = torch.randn(B, H * 64, generator=g).to(BF).to(dev)
        kc = torch.randn(B, Hkv, Lcap, 64, generator=g).to(BF).to(dev)
        vc = torch.randn(B, Hkv, Lcap, 64, generator=g).to(BF).to(dev)
        lens = torch.tensor([n - 1 for n in ns], dtype=torch.int32, device=dev)
        out = D.attn_decode_gqa(q, kc, vc, lens, H, heads_per_block=hpb)
        yard = D.attn_decode(q, kc.repeat_interleave(G, 1).contiguous(), vc.repeat_interleave(G, 1).contiguous(), lens)
        assert torch.equal(_bits(out), _bits(yard))
        ref = torch.empty(B, H, 64, dtype=torch.float64)
        for b, n in enumerate(ns):
            k = kc[b, :, :n].double().cpu().repeat_interleave(G, 0)
            v = vc[b, :, :n].double().cpu().repeat_interleave(G, 0)
            p = (q[b].double().cpu().view(H, 1, 64) @ k.transpose(1, 2) / math.sqrt(64)).softmax(-1)
            ref[b] = (p @ v).view(H, 64)
        e, ey = _rel(out, ref.view(B, -1)), _rel(yard, ref.view(B, -1))
        print(f"H {H} Hkv {Hkv} heads/block {hpb} keys {ns}: gqa {e:.3e}, attn_decode on the repeated cache {ey:.3e}")
        assert e <= 2.0 * ey
        # NaN in every cache row past lens: never read
        past = torch.arange(Lcap, device=dev)[None, None, :, None] > lens[:, None, None, None]
        dirty = D.attn_decode_gqa(q, kc.masked_fill(past, float("nan")), vc.masked_fill(past, float("nan")), lens, H,
                                  heads_per_block=hpb)
        assert torch.isfinite(out.float()).all() and torch.equal(_bits(out), _bits(dirty))


# (128, 512): the plan of that shape keeps K in one block, so the split the case is there for is asked for
@pytest.mark.parametrize("I,K,splits", [(352, 128, None), (344, 128, None), (128, 512, 4), (1536, 576, None)])
def test_glu_gemm_against_fp64_and_the_unfused_pair(I, K, splits):
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import transformer as T
    g = torch.Generator().manual_seed(I * 7 + K)
    w = (torch.randn(2 * I, K, generator=g) * 0.1).to(BF)
    x16 = torch.randn(16, K, generator=g).to(BF)
    wg = w.to(dev)
    full = None
    for M in (16, 3, 1):
        x = x16[:M]
        xg = x.to(dev).contiguous()
        gu = x.double() @ w.double().t()
        ref = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        y = D.gemm_skinny_glu(xg, wg, splits=splits)
        yard = T.swiglu_fwd(D.gemm_skinny(xg, wg))
        e, ey = _rel(y, ref), _rel(yard, ref)
        print(f"I {I} K {K} M {M}: fused {e:.3e}, gemm_skinny + swiglu_fwd {ey:.3e}")
        assert y.shape == (M, I) and e <= 2.0 * ey
        if M == 16:
            full = y
        else:   # a row's result does not depend on M or on the other rows
            assert torch.equal(_bits(y), _bits(full[:M]))
    for m in (5, 15):
        one = D.gemm_skinny_glu(x16[m:m + 1].to(dev).contiguous(), wg, splits=splits)
        assert torch.equal(_bits(one), _bits(full[m:m + 1]))


@functools.lru_cache(maxsize=None)
def _models():
    from kubeml_amd.models.llama import llama_tiny
    from kubeml_amd.nn import flatten_module
    ref = llama_tiny().double().eval()
    gpu = llama_tiny(seed=1)
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev).eval()
    flatten_module(gpu)
    return ref, gpu


def test_teacher_forced_logits_match_fp64_and_replay_is_bitwise():
    ref, gpu = _models()
    plens, steps = (100, 37), 40
    g = torch.Generator().manual_seed(21)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    ids = torch.randint(1, 1000, (2, L), generator=g) * mask
    forced = torch.randint(0, 1000, (2, steps), generator=g)
    want, full_err = [], 0.0
    with torch.no_grad():
        for b, n in enumerate(plens):
            seq = torch.cat([ids[b, :n], forced[b]])
            z = ref(seq[None])
            want.append(z[n - 1:])                         # [1 + steps, vocab]
            zg = gpu(seq[None].to(dev)).float().cpu()
            full_err = max(full_err, _rel(zg[n - 1:], z[n - 1:]))
    want = torch.stack(want)                               # [2, 1 + steps, vocab]
    cache = gpu.new_cache(2, L + steps, dev)
    assert cache.k[0].shape == (2, 2, 192, 64)             # Hkv heads
    got = [gpu.prefill_logits(ids.to(dev), mask.to(dev), cache).float().cpu()]
    fg = forced.to(dev)
    for t in range(steps):
        got.append(gpu.decode_logits(cache, fg[:, t]).float().cpu())
    errs = [_rel(got[t], want[:, t]) for t in range(1 + steps)]
    print(f"cached decode vs fp64: worst step {max(errs):.4f} (prefill {errs[0]:.4f}); "
          f"training forward on the same tokens {full_err:.4f}")
    assert got[0].shape == (2, 1000)
    assert max(errs) <= 2.0 * full_err, errs
    assert cache.lens.tolist() == [n - 1 + steps for n in plens]
    # the captured step replayed from the same cache state: bit-identical logits
    lens = cache.lens.clone()
    a = gpu.decode_logits(cache, fg[:, 0])
    cache.lens.copy_(lens)
    b = gpu.decode_logits(cache, fg[:, 0])
    assert torch.equal(_bits(a), _bits(b))
    assert len(cache._graphs) == 1


def test_generate_greedy_eos_filters_and_refusal():
    _, gpu = _models()
    plens, new = (17, 3, 40, 1), 48
    g = torch.Generator().manual_seed(31)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long().to(dev)
    ids = (torch.randint(1, 1000, (4, L), generator=g) * mask.cpu()).to(dev)
    free = gpu.generate(ids, mask, max_new_tokens=new).cpu()
    assert free.dtype == torch.int64 and free.shape == (4, L + new)
    assert torch.equal(free, gpu.generate(ids, mask, max_new_tokens=new).cpu())
    for b, n in enumerate(plens):
        assert torch.equal(free[b, :n], ids[b, :n].cpu())
        assert (free[b, n + new:] == 0).all() and int(free[b].max()) < 1000
    eos = int(free[0, plens[0] + 5])
    out = gpu.generate(ids, mask, max_new_tokens=new, eos_token_id=eos).cpu()
    for b, n in enumerate(plens):
        gen, ref = out[b, n:n + new].tolist(), free[b, n:n + new].tolist()
        cut = gen.index(eos) if eos in gen else new
        assert gen[:cut] == ref[:cut] and all(t == eos for t in gen[cut:])
        assert torch.equal(out[b, :n], ids[b, :n].cpu()) and (out[b, n + new:] == eos).all()
    assert out[0, plens[0]:].tolist().index(eos) <= 5
    kw = dict(max_new_tokens=new, top_k=5, temperature=0.8, seed=1)
    hot = gpu.generate(ids, mask, **kw).cpu()
    assert torch.equal(hot, gpu.generate(ids, mask, **kw).cpu()) and not torch.equal(hot, free)
    with pytest.raises(ValueError):
        gpu.generate(ids, mask, max_new_tokens=new, prompt_lookup_num_tokens=3)
