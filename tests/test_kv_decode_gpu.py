"""The decode kernels (csrc/kernels/decode.hip) and the KV-cache path of the GPT-2 model on the
GPU: decode attention and the skinny GEMM against references with the existing kernels as the
yardstick, what the attention must never read, the cache append and its bounds, the sampler,
teacher-forced logits against the fp64 CPU model and greedy ``generate``."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _row_rel(o, ref, H):
    """worst norm-relative error over the (b, h) rows of [B, H*64] outputs"""
    o, ref = o.double().cpu().view(-1, H, 64), ref.double().cpu().view(-1, H, 64)
    return ((o - ref).norm(dim=-1) / ref.norm(dim=-1)).max().item()


def _chunk():
    from kubeml_amd.ops import decode as D
    return D.attn_decode_chunk()


def _seq(n, H, seed):
    """fused bf16 QKV [n, 3*H*64] of one sequence of n tokens (CPU)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3 * H * 64, generator=g).to(BF)


def _last_row_fp32(qkv, H):
    """fp32 torch: attention output of the LAST token of the sequence over all its keys, [H*64]"""
    n, D = qkv.shape[0], H * 64
    q = qkv[-1, :D].float().view(H, 1, 64)
    k = qkv[:, D:2 * D].float().view(n, H, 64).permute(1, 0, 2)
    v = qkv[:, 2 * D:].float().view(n, H, 64).permute(1, 0, 2)
    p = (q @ k.transpose(1, 2) / math.sqrt(64)).softmax(-1)
    return (p @ v).reshape(D)


def _fill_cache(seqs, H, Lcap, fill=0.0):
    """K, V [B, H, Lcap, 64] holding each sequence's keys / values in rows 0..n-1, `fill` elsewhere;
    q [B, 3*H*64] = each sequence's last fused row; lens = n - 1"""
    B, D = len(seqs), H * 64
    kc = torch.full((B, H, Lcap, 64), fill, dtype=BF)
    vc = torch.full((B, H, Lcap, 64), fill, dtype=BF)
    for b, s in enumerate(seqs):
        n = s.shape[0]
        kc[b, :, :n] = s[:, D:2 * D].view(n, H, 64).permute(1, 0, 2)
        vc[b, :, :n] = s[:, 2 * D:].view(n, H, 64).permute(1, 0, 2)
    q = torch.stack([s[-1] for s in seqs])
    lens = torch.tensor([s.shape[0] - 1 for s in seqs], dtype=torch.int32)
    return q.to(dev), kc.to(dev), vc.to(dev), lens.to(dev)


@functools.lru_cache(maxsize=None)
def _attention_errors():
    """worst (b, h)-row error of the decode kernel and of attn_fwd(causal=True)'s last row over
    the same case list, both against fp32 torch"""
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import transformer as T
    C = _chunk()
    counts = [1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 7]
    Lcap = -(-(2 * C + 8) // 64) * 64
    cases = [(2, [counts[i], counts[(i + 4) % 9]]) for i in range(9)] + [(3, [n]) for n in counts]
    worst_dec = worst_yard = 0.0
    for ci, (H, ns) in enumerate(cases):
        seqs = [_seq(n, H, 100 * ci + b) for b, n in enumerate(ns)]
        ref = torch.stack([_last_row_fp32(s, H) for s in seqs])
        q, kc, vc, lens = _fill_cache(seqs, H, Lcap)
        o = D.attn_decode(q, kc, vc, lens)
        worst_dec = max(worst_dec, _row_rel(o, ref, H))
        Dm = H * 64
        for b, s in enumerate(seqs):
            sg = s.to(dev)
            n = s.shape[0]
            y, _ = T.attn_fwd(sg[:, :Dm], sg[:, Dm:2 * Dm], sg[:, 2 * Dm:], 1, H, n, causal=True)
            worst_yard = max(worst_yard, _row_rel(y[n - 1:n], ref[b:b + 1], H))
    return worst_dec, worst_yard


def test_decode_attention_within_twice_the_flash_kernel_error():
    dec, yard = _attention_errors()
    print(f"decode attention worst row error {dec:.3e}; attn_fwd(causal) last row {yard:.3e}; chunk {_chunk()}")
    assert dec <= 2.0 * yard


@pytest.mark.parametrize("poison", [float("nan"), 1e30])
def test_decode_attention_never_reads_past_lens(poison):
    from kubeml_amd.ops import decode as D
    C = _chunk()
    H, Lcap = 2, -(-(2 * C + 8) // 64) * 64
    seqs = [_seq(5, H, 1), _seq(C + 2, H, 2)]
    q, kc, vc, lens = _fill_cache(seqs, H, Lcap, fill=0.0)
    clean = D.attn_decode(q, kc, vc, lens)
    q2, kp, vp, _ = _fill_cache(seqs, H, Lcap, fill=poison)
    assert not (kp[0, 0, 5:].float().abs() < 1e29).any()   # every row past lens[0] is poisoned
    dirty = D.attn_decode(q2, kp, vp, lens)
    assert torch.isfinite(clean.float()).all()
    assert torch.equal(clean.view(torch.int16), dirty.view(torch.int16))


def test_decode_attention_independent_of_capacity_and_batch():
    from kubeml_amd.ops import decode as D
    H = 2
    s = _seq(100, H, 7)
    outs = []
    for Lcap in (128, 320):
        q, kc, vc, lens = _fill_cache([s], H, Lcap)
        outs.append(D.attn_decode(q, kc, vc, lens))
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    q, kc, vc, lens = _fill_cache([s, _seq(3, H, 8), _seq(300, H, 9), _seq(64, H, 10)], H, 320)
    four = D.attn_decode(q, kc, vc, lens)
    assert torch.equal(four[:1].view(torch.int16), outs[1].view(torch.int16))
    # one key: the probability is 1 and the output V's row 0, exactly
    one = _seq(1, H, 11)
    q, kc, vc, lens = _fill_cache([one], H, 128)
    o = D.attn_decode(q, kc, vc, lens)
    assert torch.equal(o.cpu().view(torch.int16), one[:, 2 * H * 64:].view(torch.int16))


def test_kv_append_prefill_round_trips():
    from kubeml_amd.ops import decode as D
    B, H, Lq, Lcap = 2, 2, 70, 128
    D_ = H * 64
    qkv = torch.randn(B * Lq, 3 * D_, generator=torch.Generator().manual_seed(0)).to(BF).to(dev)
    kc = torch.full((B, H, Lcap, 64), 7.0, dtype=BF, device=dev)
    vc = torch.full((B, H, Lcap, 64), 7.0, dtype=BF, device=dev)
    D.kv_append(qkv, kc, vc, Lq)
    k = qkv[:, D_:2 * D_].view(B, Lq, H, 64).permute(0, 2, 1, 3)
    v = qkv[:, 2 * D_:].view(B, Lq, H, 64).permute(0, 2, 1, 3)
    assert torch.equal(kc[:, :, :Lq], k) and torch.equal(vc[:, :, :Lq], v)
    assert (kc[:, :, Lq:] == 7.0).all() and (vc[:, :, Lq:] == 7.0).all()


def _guarded(B, H, Lcap, guard=512):
    """K and V as views inside ONE allocation with `guard` elements of 7.0 before, between and after"""
    n = B * H * Lcap * 64
    buf = torch.full((3 * guard + 2 * n,), 7.0, dtype=BF, device=dev)
    kc = buf[guard:guard + n].view(B, H, Lcap, 64)
    vc = buf[2 * guard + n:2 * guard + 2 * n].view(B, H, Lcap, 64)
    return buf, kc, vc


def test_kv_append_decode_lands_at_lens_and_nowhere_else():
    from kubeml_amd.ops import decode as D
    B, H, Lcap = 3, 2, 128
    D_ = H * 64
    qkv = torch.randn(B, 3 * D_, generator=torch.Generator().manual_seed(1)).to(BF).to(dev)
    buf, kc, vc = _guarded(B, H, Lcap)
    lens = torch.tensor([3, 100, Lcap - 1], dtype=torch.int32, device=dev)
    D.kv_append(qkv, kc, vc, 1, lens=lens)
    expect = torch.full_like(buf, 7.0)
    n = kc.numel()
    ek, ev = expect[512:512 + n].view_as(kc), expect[1024 + n:1024 + 2 * n].view_as(vc)
    for b, r in enumerate(lens.tolist()):
        ek[b, :, r] = qkv[b, D_:2 * D_].view(H, 64)
        ev[b, :, r] = qkv[b, 2 * D_:].view(H, 64)
    assert torch.equal(buf, expect)
    # the saturated sequence steps once more: the row is rewritten in place, nothing moves
    qkv2 = (qkv.float() + 1.0).to(BF)
    D.kv_append(qkv2, kc, vc, 1, lens=lens)
    for b, r in enumerate(lens.tolist()):
        ek[b, :, r] = qkv2[b, D_:2 * D_].view(H, 64)
        ev[b, :, r] = qkv2[b, 2 * D_:].view(H, 64)
    assert torch.equal(buf, expect)
    # rows outside [0, Lcap) are dropped: the guards and the cache stay as they are
    before = buf.clone()
    D.kv_append(qkv, kc, vc, 1, lens=torch.tensor([Lcap, -1, Lcap + 5], dtype=torch.int32, device=dev))
    assert torch.equal(buf, before)


@pytest.mark.parametrize("N,K,act", [(384, 128, None), (128, 128, None), (512, 128, "gelu"), (128, 512, None),
                                     (1000, 128, None), (3072, 768, "gelu"), (768, 3072, None),
                                     (32776, 128, None)])   # the last: the 4-wave blocks of a vocabulary-sized N
def test_skinny_gemm_against_fp64_and_the_large_gemm(N, K, act):
    from kubeml_amd.ops import decode as D
    from kubeml_amd.ops import gemm as G
    g = torch.Generator().manual_seed(N * 7 + K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
    x16 = torch.randn(16, K, generator=g).to(BF)
    bias = torch.randn(N, generator=g)
    wg, bg = w.to(dev), bias.to(dev)
    full = None
    for M in (16, 3, 1):
        x = x16[:M]
        xg = x.to(dev).contiguous()
        for b in (bias, None):
            ref = x.double() @ w.double().t()
            if b is not None:
                ref = ref + b.double()
            if act == "gelu":
                ref = torch.nn.functional.gelu(ref)
            y = D.gemm_skinny(xg, wg, None if b is None else bg, act=act)
            yard = G.linear_fwd(xg, wg, None if b is None else bg, act=1 if act == "gelu" else 0)
            e, ey = _rel(y.cpu(), ref), _rel(yard.cpu(), ref)
            print(f"N {N} K {K} act {act} M {M} bias {b is not None}: skinny {e:.3e} linear_fwd {ey:.3e}")
            assert y.shape == (M, N) and e <= 2.0 * ey
            if b is not None:
                if M == 16:
                    full = y
                else:   # a row's result does not depend on M or on the other rows
                    assert torch.equal(y.view(torch.int16), full[:M].view(torch.int16))
    for m in (5, 15):
        one = D.gemm_skinny(x16[m:m + 1].to(dev).contiguous(), wg, bg, act=act)
        assert torch.equal(one.view(torch.int16), full[m:m + 1].view(torch.int16))


def test_embed2_at_reads_the_position_from_lens():
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(2)
    word = torch.randn(40, 128, generator=g).to(BF).to(dev)
    pos = torch.randn(64, 128, generator=g).to(BF).to(dev)
    ids = torch.tensor([3, 39, 0], device=dev)
    lens = torch.tensor([0, 63, 17], dtype=torch.int32, device=dev)
    out = D.embed2_at(ids, lens, word, pos)
    assert torch.equal(out, (word[ids].float() + pos[lens.long()].float()).to(BF))


def _sampler_state(B, Lcap, eos=-1, seed=5, temperature=1.0):
    ctl = torch.tensor([seed, 0, eos, 0], dtype=torch.int32, device=dev)
    temp = torch.tensor([temperature], dtype=torch.float32, device=dev)
    return dict(ctl=ctl, temp=temp, next_ids=torch.zeros(B, dtype=torch.int64, device=dev),
                tokens=torch.zeros(B, Lcap, dtype=torch.int64, device=dev),
                lens=torch.zeros(B, dtype=torch.int32, device=dev),
                finished=torch.zeros(B, dtype=torch.int32, device=dev))


def test_greedy_advance_is_argmax_lowest_index_on_ties():
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(5, 5000, generator=g).to(BF)
    plant = [0, 4999, 2047, 2048, 777]
    for b, c in enumerate(plant[:4]):
        logits[b, c] = 9.0
    logits[4, 4100] = 9.0    # a tie across waves and strides: the lower column wins
    logits[4, 777] = 9.0
    logits[4, 3000] = 9.0
    pad = torch.full((5, 5008), 50.0, dtype=BF)   # columns past `classes` hold larger values
    pad[:, :5000] = logits
    st = _sampler_state(5, 64, eos=777)
    st["lens"].copy_(torch.tensor([0, 5, 62, 63, 9], dtype=torch.int32))
    D.decode_advance(pad.to(dev), 5000, sample=False, **st)
    assert st["next_ids"].tolist() == plant
    assert torch.equal(st["next_ids"][:4].cpu(), logits[:4].float().argmax(-1))
    assert st["lens"].tolist() == [1, 6, 63, 63, 10]          # saturates at Lcap - 1
    assert st["finished"].tolist() == [0, 0, 0, 0, 1]         # row 4 drew eos
    assert st["ctl"].tolist() == [5, 1, 777, 0]
    tok = st["tokens"].cpu()
    assert tok[0, 1] == 0 and tok[1, 6] == 4999 and tok[2, 63] == 2047 and tok[4, 10] == 777
    assert int((tok != 0).sum()) == 3                          # row 3's write at Lcap is dropped
    # a finished sequence emits eos whatever its logits say
    D.decode_advance(pad.to(dev), 5000, sample=False, **st)
    assert st["next_ids"].tolist() == [0, 4999, 2047, 2048, 777] and st["finished"].tolist() == [0, 0, 0, 0, 1]
    st["finished"][0] = 1
    D.decode_advance(pad.to(dev), 5000, sample=False, **st)
    assert st["next_ids"].tolist()[0] == 777 and st["ctl"].tolist()[1] == 3


def test_advance_writes_stay_inside_tokens_when_saturated():
    from kubeml_amd.ops import decode as D
    B, Lcap = 2, 64
    buf = torch.full((B * Lcap + 128,), -7, dtype=torch.int64, device=dev)
    st = _sampler_state(B, Lcap)
    st["tokens"] = buf[64:64 + B * Lcap].view(B, Lcap)
    st["lens"].fill_(Lcap - 1)
    logits = torch.zeros(B, 8, dtype=BF, device=dev)
    for _ in range(2):
        D.decode_advance(logits, 8, sample=True, **st)
    assert (buf == -7).all() and st["lens"].tolist() == [Lcap - 1] * B


def test_gumbel_max_frequencies_follow_the_softmax():
    """8 classes, 16 rows x 256 steps = 4096 draws at T = 1: every class frequency within
    5 sqrt(p (1 - p) / 4096) of its softmax probability (a sound generator fails with
    probability under 1e-5)"""
    from kubeml_amd.ops import decode as D
    row = torch.tensor([1.5, 0.0, -1.0, 0.5, 2.0, -2.0, 1.0, 0.25]).to(BF)
    logits = row[None].repeat(16, 1).contiguous().to(dev)
    st = _sampler_state(16, 64, seed=1234)
    draws = []
    for _ in range(256):
        D.decode_advance(logits, 8, sample=True, **st)
        draws.append(st["next_ids"].clone())
    draws = torch.stack(draws).cpu().reshape(-1)
    assert draws.numel() == 4096 and st["ctl"].tolist()[1] == 256
    p = row.double().softmax(-1)
    f = torch.bincount(draws, minlength=8).double() / 4096
    print("softmax", [round(v, 4) for v in p.tolist()], "frequency", [round(v, 4) for v in f.tolist()])
    tol = 5.0 * (p * (1 - p) / 4096).sqrt()
    assert ((f - p).abs() <= tol).all(), ((f - p).abs() / tol).tolist()
    # another temperature is another distribution: T = 0.5 sharpens it
    st = _sampler_state(16, 64, seed=99, temperature=0.5)
    hot = []
    for _ in range(64):
        D.decode_advance(logits, 8, sample=True, **st)
        hot.append(st["next_ids"].clone())
    f2 = torch.bincount(torch.stack(hot).cpu().reshape(-1), minlength=8).double() / 1024
    p2 = (row.double() / 0.5).softmax(-1)
    assert ((f2 - p2).abs() <= 5.0 * (p2 * (1 - p2) / 1024).sqrt()).all()


@functools.lru_cache(maxsize=None)
def _models():
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    ref = gpt2_tiny(dropout=0.0).double().eval()
    gpu = gpt2_tiny(dropout=0.0)
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
    got = [gpu.prefill_logits(ids.to(dev), mask.to(dev), cache).float().cpu()]
    fg = forced.to(dev)
    for t in range(steps):
        got.append(gpu.decode_logits(cache, fg[:, t]).float().cpu())
    errs = [_rel(got[t], want[:, t]) for t in range(1 + steps)]
    print(f"cached decode vs fp64: worst step {max(errs):.4f} (prefill {errs[0]:.4f}); "
          f"full forward on the same tokens {full_err:.4f}")
    assert got[0].shape == (2, 1000)
    assert max(errs) < 0.02, errs
    assert cache.lens.tolist() == [n - 1 + steps for n in plens]
    # the captured step replayed from the same cache state: bit-identical logits
    lens = cache.lens.clone()
    a = gpu.decode_logits(cache, fg[:, 0])
    cache.lens.copy_(lens)
    b = gpu.decode_logits(cache, fg[:, 0])
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert len(cache._graphs) == 1


def test_greedy_generate_on_the_gpu():
    _, gpu = _models()
    plens, new = (17, 3, 40, 1), 64
    g = torch.Generator().manual_seed(31)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    ids = (torch.randint(1, 1000, (4, L), generator=g) * mask).to(dev)
    free = gpu.generate(ids, mask.to(dev), max_new_tokens=new).cpu()
    assert free.dtype == torch.int64 and free.shape == (4, L + new)
    for b, n in enumerate(plens):
        assert torch.equal(free[b, :n], ids[b, :n].cpu())
        assert (free[b, n + new:] == 0).all() and int(free[b].max()) < 1000
    eos = int(free[0, plens[0] + 5])
    out = gpu.generate(ids, mask.to(dev), max_new_tokens=new, eos_token_id=eos).cpu()
    again = gpu.generate(ids, mask.to(dev), max_new_tokens=new, eos_token_id=eos).cpu()
    assert torch.equal(out, again)
    stopped = 0
    for b, n in enumerate(plens):
        gen, ref = out[b, n:n + new].tolist(), free[b, n:n + new].tolist()
        cut = gen.index(eos) if eos in gen else new
        stopped += cut < new
        assert gen[:cut] == ref[:cut] and all(t == eos for t in gen[cut:])
        assert torch.equal(out[b, :n], ids[b, :n].cpu()) and (out[b, n + new:] == eos).all()
    assert stopped >= 1 and out[0, plens[0]:].tolist().index(eos) <= 5
    with pytest.raises(ValueError):
        gpu.generate(ids, mask.to(dev), max_new_tokens=256 - L + 1)
