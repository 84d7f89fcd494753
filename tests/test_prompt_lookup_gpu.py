"""Prompt-lookup speculative decoding on the GPU: the kernels of a verify round (multi-query decode
attention, multi-row cache append and embedding, the n-gram drafter, pick / commit) against the
one-row kernels and the CPU twins, the round's logits against one-token-at-a-time decoding, and
``generate(prompt_lookup_num_tokens=k)`` against plain ``generate``.  Every comparison is exact."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
NEW = 20
BLOCK = (11, 57, 402, 7, 950, 33)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _tickets_are_zero():
    from kubeml_amd.ops.kernels import _COUNTERS
    torch.cuda.synchronize()
    return all(int(buf.abs().sum()) == 0 for buf in _COUNTERS.bufs.values())


# ------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("B,q,lens", [(2, 4, [254, 3]),     # sequence 0's queries straddle the chunk boundary at 256
                                      (2, 4, [509, 0]),     # the last queries reach Lcap - 1 and the clamp
                                      (1, 16, [250])])
def test_multi_query_attention_rows_are_the_one_query_kernel_bit_for_bit(B, q, lens):
    from kubeml_amd.ops import decode as D
    H, Lcap = 2, 512
    assert D.attn_decode_chunk() == 256
    g = torch.Generator().manual_seed(100 + q + lens[0])
    kc = torch.randn(B, H, Lcap, 64, generator=g).to(BF).to(dev)
    vc = torch.randn(B, H, Lcap, 64, generator=g).to(BF).to(dev)
    rows = (torch.randn(B * q, 3 * H * 64, generator=g) * 2.0).to(BF).to(dev)
    lens = torch.tensor(lens, dtype=torch.int32, device=dev)
    ws = D.attn_decode_multi_workspace(B, H, Lcap, q, dev)
    ws.fill_(float("nan"))   # a partial that is read without having been written shows
    out = D.attn_decode_multi(rows, kc, vc, lens, q, ws=ws)
    assert out.shape == (B * q, H * 64) and torch.isfinite(out.float()).all()
    assert _tickets_are_zero()
    again = D.attn_decode_multi(rows, kc, vc, lens, q, ws=ws)   # the same workspace and tickets
    assert torch.equal(_bits(out), _bits(again)) and _tickets_are_zero()
    by_q = rows.view(B, q, -1)
    for j in range(q):
        one = D.attn_decode(by_q[:, j], kc, vc, (lens + j).clamp(max=Lcap - 1))
        assert torch.equal(_bits(out.view(B, q, -1)[:, j]), _bits(one)), j


def test_multi_query_attention_never_reads_past_a_query_s_length():
    from kubeml_amd.ops import decode as D
    B, H, Lcap, q = 1, 2, 512, 4
    g = torch.Generator().manual_seed(7)
    kc = torch.randn(B, H, Lcap, 64, generator=g).to(BF).to(dev)
    vc = torch.randn(B, H, Lcap, 64, generator=g).to(BF).to(dev)
    rows = torch.randn(B * q, 3 * H * 64, generator=g).to(BF).to(dev)
    lens = torch.tensor([254], dtype=torch.int32, device=dev)
    clean = D.attn_decode_multi(rows, kc, vc, lens, q)
    kc[:, :, 254 + q:] = float("nan")
    vc[:, :, 254 + q:] = float("nan")
    assert torch.equal(_bits(clean), _bits(D.attn_decode_multi(rows, kc, vc, lens, q)))
    # query 0 must not see rows 255 .. 257 either, which the later queries do read
    kc[:, :, 255:] = float("nan")
    vc[:, :, 255:] = float("nan")
    dirty = D.attn_decode_multi(rows, kc, vc, lens, q)
    assert torch.equal(_bits(clean[:1]), _bits(dirty[:1])) and torch.isnan(dirty[1:].float()).any()


# ------------------------------------------------------------------------- append and embedding
def test_multi_row_append_lands_at_lens_plus_t_and_drops_what_passes_the_cache():
    from kubeml_amd.ops import decode as D
    B, H, Lcap, Lq, guard = 2, 2, 128, 4, 512
    D_ = H * 64
    n = B * H * Lcap * 64
    buf = torch.full((3 * guard + 2 * n,), 7.0, dtype=BF, device=dev)   # sentinel, guards around K and V
    kc = buf[guard:guard + n].view(B, H, Lcap, 64)
    vc = buf[2 * guard + n:2 * guard + 2 * n].view(B, H, Lcap, 64)
    qkv = torch.randn(B * Lq, 3 * D_, generator=torch.Generator().manual_seed(1)).to(BF).to(dev)
    lens = torch.tensor([3, Lcap - 2], dtype=torch.int32, device=dev)
    D.kv_append(qkv, kc, vc, Lq, lens=lens)
    expect = torch.full_like(buf, 7.0)
    ek, ev = expect[guard:guard + n].view_as(kc), expect[2 * guard + n:2 * guard + 2 * n].view_as(vc)
    for b, r in enumerate(lens.tolist()):
        for t in range(Lq):
            if r + t < Lcap:
                ek[b, :, r + t] = qkv[b * Lq + t, D_:2 * D_].view(H, 64)
                ev[b, :, r + t] = qkv[b * Lq + t, 2 * D_:].view(H, 64)
    assert torch.equal(buf, expect)
    before = buf.clone()
    D.kv_append(qkv, kc, vc, Lq, lens=torch.tensor([Lcap, -Lq], dtype=torch.int32, device=dev))
    assert torch.equal(buf, before)


def test_multi_row_embedding_takes_ids_from_next_ids_and_the_drafts():
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(2)
    word = torch.randn(40, 128, generator=g).to(BF).to(dev)
    pos = torch.randn(64, 128, generator=g).to(BF).to(dev)
    nxt = torch.tensor([3, 39], device=dev)
    draft = torch.tensor([[5, 6, 7], [0, 1, 2]], device=dev)
    lens = torch.tensor([0, 62], dtype=torch.int32, device=dev)   # sequence 1: positions 62, 63, 63, 63 (clamped)
    out = D.embed2_multi(nxt, draft, lens, word, pos)
    ids = torch.cat([nxt[:, None], draft], 1).reshape(-1)
    at = (lens[:, None].long() + torch.arange(4, device=dev)[None]).clamp(max=63).reshape(-1)
    assert torch.equal(out, (word[ids].float() + pos[at].float()).to(BF))
    for j in range(4):   # row j is the one-row kernel at lens + j
        one = D.embed2_at(ids.view(2, 4)[:, j].contiguous(), lens + j, word, pos)
        assert torch.equal(out.view(2, 4, -1)[:, j], one)


# -------------------------------------------------------------------------------------- drafter
def _hist(rows, Lcap, pad=999):
    t = torch.full((len(rows), Lcap), pad, dtype=torch.int64)
    for b, r in enumerate(rows):
        t[b, :len(r)] = torch.tensor(r)
    return t, torch.tensor([len(r) - 1 for r in rows], dtype=torch.int32)


# (history, k, max_ngram, expected draft): the hand-made cases of tests/test_prompt_lookup_cpu.py
DRAFT_CASES = [
    ([1, 2, 3, 4], 3, 2, [4, 4, 4]),
    ([5, 6, 7, 8, 6], 3, 2, [7, 8, 6]),
    ([1, 2, 9, 1, 2, 8, 1, 2], 3, 2, [8, 1, 2]),
    ([3, 4, 5, 3, 4], 5, 2, [5, 3, 4, 4, 4]),
    ([9], 3, 2, [9, 9, 9]),
    ([4, 4, 4, 4], 2, 3, [4, 4]),
    ([1, 2, 3, 1, 2, 3, 1], 4, 1, [2, 3, 1, 1]),
]


def test_drafter_kernel_matches_the_twin():
    from kubeml_amd.nn import lookup_draft_reference
    from kubeml_amd.ops import decode as D
    for hist, k, g, want in DRAFT_CASES:
        tokens, lens = _hist([hist], 16)
        got = D.draft_lookup(tokens.to(dev), lens.to(dev), k, g)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and got.tolist() == [want], (hist, k, g)
    # 64 random histories over 5 symbols, lengths 1 .. 200: many matches at every g
    gen = torch.Generator().manual_seed(9)
    lengths = torch.randint(1, 201, (64,), generator=gen).tolist()
    lengths[:3] = [1, 2, 200]
    rows = [torch.randint(0, 5, (n,), generator=gen).tolist() for n in lengths]
    tokens, lens = _hist(rows, 256)
    for k, g in ((5, 3), (15, 1), (1, 4)):
        ref = lookup_draft_reference(tokens, lens, k, g)
        assert torch.equal(D.draft_lookup(tokens.to(dev), lens.to(dev), k, g).cpu(), ref), (k, g)
    assert (ref != 999).all()
    # one history of 1000 tokens: several strides per thread
    long = torch.randint(0, 30, (1000,), generator=gen).tolist()
    tokens, lens = _hist([long], 1024)
    for g in (1, 2, 3):
        ref = lookup_draft_reference(tokens, lens, 7, g)
        assert torch.equal(D.draft_lookup(tokens.to(dev), lens.to(dev), 7, g).cpu(), ref), g


# ---------------------------------------------------------------------------------- pick / commit
EOS = 7


def _round_state(lens, start, limit, finished, draft, Lcap=64, eos=EOS, seed=5, temperature=1.0):
    """a CPU cache (no layers) in the state a round starts from, and its copy on the GPU"""
    from kubeml_amd.nn import KVCache
    B, k = len(lens), len(draft[0])
    cpu = KVCache(0, B, 1, Lcap, "cpu")
    cpu.reset(seed=seed, temperature=temperature, eos_token_id=eos, start=torch.tensor(start),
              limit=torch.tensor(limit), draft_tokens=k)
    cpu.lens.copy_(torch.tensor(lens))
    cpu.finished.copy_(torch.tensor(finished))
    cpu.draft.copy_(torch.tensor(draft))
    cpu.tokens.fill_(-1)
    cpu.next_ids.fill_(-5)
    names = ("ctl", "temp", "start", "limit", "draft", "pick", "next_ids", "tokens", "lens", "finished", "stats")
    return cpu, {n: getattr(cpu, n).clone().to(dev) for n in names}


def _rows(picks, classes=1000, ld=1000):
    """bf16 logits with one dominant column per row (None: an all-NaN row)"""
    g = torch.Generator().manual_seed(4)
    z = torch.randn(len(picks), ld, generator=g).to(BF)
    for r, c in enumerate(picks):
        if c is None:
            z[r] = float("nan")
        else:
            for cc in (c if isinstance(c, tuple) else (c,)):
                z[r, cc] = 9.0
    return z


def _check_round(picks, want_picks, **state):
    from kubeml_amd.models.gpt import _verify_commit_cpu
    from kubeml_amd.ops import decode as D
    cpu, gpu = _round_state(**state)
    D.verify_pick(_rows(picks).to(dev), 1000, sample=False, **gpu)
    assert gpu["pick"].tolist() == want_picks
    assert _tickets_are_zero()
    cpu.pick.copy_(torch.tensor(want_picks, dtype=torch.int32))
    _verify_commit_cpu(cpu)
    for n in ("tokens", "lens", "next_ids", "finished", "stats"):
        assert torch.equal(gpu[n].cpu(), getattr(cpu, n)), n
    return cpu


def test_pick_and_commit_zero_partial_full_acceptance_and_eos_as_a_draft():
    picks = [(10, 900), 1, 2, 3,     # zero acceptance; row 0 has tied maxima: the lowest column
             20, 21, 99, 4,          # partial: two drafts accepted, the third corrected
             30, 31, 32, 33,         # full: three drafts and the bonus token
             40, EOS, 41, 42]        # eos as an accepted draft: the walk ends there
    want = [c[0] if isinstance(c, tuple) else c for c in picks]
    cpu = _check_round(picks, want, lens=[5, 9, 0, 20], start=[2, 9, 0, 3], limit=[63, 63, 63, 63],
                       finished=[0, 0, 0, 0], draft=[[5, 6, 8], [20, 21, 22], [30, 31, 32], [40, EOS, 41]])
    assert cpu.lens.tolist() == [6, 12, 4, 22] and cpu.next_ids.tolist() == [10, 99, 33, EOS]
    assert cpu.finished.tolist() == [0, 0, 0, 1] and cpu.stats.tolist() == [0 + 2 + 3 + 1, 1 + 3 + 4 + 2, 63 - 4, 0]
    assert cpu.tokens[1, 9:14].tolist() == [-1, 20, 21, 99, -1]


def test_pick_and_commit_bonus_eos_finished_frozen_limit_and_nan_rows():
    picks = [50, 51, 52, EOS,        # eos as the bonus token
             1, 2, 3, 4,             # finished before the round: eos in every slot, up to its limit
             60, 61, 62, 63,         # frozen at its limit: nothing moves
             None, 70, 71, 72]       # an all-NaN row picks 0 (which its draft guessed); limit inside the round
    want = [50, 51, 52, EOS, 1, 2, 3, 4, 60, 61, 62, 63, 0, 70, 71, 72]
    cpu = _check_round(picks, want, lens=[5, 9, 30, 20], start=[2, 1, 0, 3], limit=[63, 12, 30, 22],
                       finished=[0, 1, 0, 0], draft=[[50, 51, 52], [1, 2, 3], [60, 61, 62], [0, 70, 71]])
    assert cpu.lens.tolist() == [9, 12, 30, 22] and cpu.next_ids.tolist() == [EOS, EOS, -5, 70]
    assert cpu.finished.tolist() == [1, 1, 0, 0] and cpu.stats.tolist() == [3 + 0 + 0 + 1, 4 + 3 + 0 + 2, 63 - 9, 0]
    assert cpu.tokens[1, 9:14].tolist() == [-1, EOS, EOS, EOS, -1] and (cpu.tokens[2] == -1).all()
    assert cpu.tokens[3, 20:24].tolist() == [-1, 0, 70, -1]


def test_sampled_picks_are_decode_advance_at_the_step_of_each_position():
    from kubeml_amd.ops import decode as D
    B, q, ld = 4, 4, 1000
    lens, start = [5, 9, 0, 20], [2, 9, 0, 3]
    cpu, gpu = _round_state(lens=lens, start=start, limit=[63] * B, finished=[0] * B,
                            draft=[[1, 2, 3]] * B, eos=-1, seed=77, temperature=0.8)
    z = torch.randn(B * q, ld, generator=torch.Generator().manual_seed(6)).to(BF).to(dev)
    D.verify_pick(z, 1000, sample=True, **gpu)
    got = gpu["pick"].view(B, q).tolist()
    for b in range(B):
        for j in range(q):
            st = dict(ctl=torch.tensor([77, lens[b] + j - start[b], -1, 0], dtype=torch.int32, device=dev),
                      temp=gpu["temp"], next_ids=torch.zeros(B, dtype=torch.int64, device=dev),
                      tokens=torch.zeros(B, 64, dtype=torch.int64, device=dev),
                      lens=torch.zeros(B, dtype=torch.int32, device=dev),
                      finished=torch.zeros(B, dtype=torch.int32, device=dev))
            D.decode_advance(z.view(B, q, ld)[:, j], 1000, sample=True, **st)   # row b of the batch: its own noise
            assert got[b][j] == int(st["next_ids"][b]), (b, j)
    assert len({p for row in got for p in row}) > 8   # draws, not one column


# ------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _gpu_model():
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    gpu = gpt2_tiny(dropout=0.0).to(dev).eval()
    flatten_module(gpu)
    return gpu


@functools.lru_cache(maxsize=None)
def _prompts(B, plens=(18, 5, 9, 1)):
    plens = plens[:B]
    L = max(plens)
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(1, 1000, (B, L), generator=g)
    if plens[0] == 18:
        ids[0] = torch.tensor(BLOCK * 3)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    return plens, (ids * mask).to(dev), mask.to(dev)


@functools.lru_cache(maxsize=None)
def _plain(B, sampled, eos=None):
    _, ids, mask = _prompts(B)
    kw = dict(temperature=0.8, seed=3) if sampled else {}
    return _gpu_model().generate(ids, mask, max_new_tokens=NEW, eos_token_id=eos, **kw)


@pytest.mark.parametrize("B,k", [(1, 15), (4, 3)])
def test_verify_round_logits_are_one_token_at_a_time_decoding_bit_for_bit(B, k):
    """pins the embedding, the append, the attention, the skinny routing and LayerNorm at B * q rows"""
    m = _gpu_model()
    plens, ids, mask = _prompts(B, (37, 3, 100, 1))
    pl = torch.tensor(plens)
    q = k + 1
    a = m.new_cache(B, 192, dev)
    a.reset(start=pl - 1, limit=pl - 1 + 64, draft_tokens=k)
    m.prefill(ids, mask, a)
    drafts = torch.randint(0, 1000, (B, k), generator=torch.Generator().manual_seed(8)).to(dev)
    feed = torch.cat([a.next_ids[:, None], drafts], 1)
    got = m.verify_step(a, drafts)[:, :1000].clone().view(B, q, 1000)
    b = m.new_cache(B, 192, dev)
    b.reset()
    m.prefill_logits(ids, mask, b)
    for j in range(q):
        one = m.decode_logits(b, feed[:, j])
        assert torch.equal(_bits(got[:, j]), _bits(one)), j
    for i in range(len(a.k)):   # the caches agree on every row the round wrote
        for s, n in enumerate(plens):
            assert torch.equal(_bits(a.k[i][s, :, :n + q]), _bits(b.k[i][s, :, :n + q]))
            assert torch.equal(_bits(a.v[i][s, :, :n + q]), _bits(b.v[i][s, :, :n + q]))


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B,k", [(1, 1), (1, 3), (1, 7), (1, 15), (4, 3)])
def test_generate_with_prompt_lookup_equals_plain_generate_on_the_gpu(B, k, sampled):
    m = _gpu_model()
    plens, ids, mask = _prompts(B)
    kw = dict(temperature=0.8, seed=3) if sampled else {}
    ref = _plain(B, sampled)
    out = m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=k, **kw)
    assert torch.equal(out, ref)
    st = m.last_generate_stats
    print(f"B {B} k {k} sampled {sampled}: {st}")
    assert st["tokens"] == B * (NEW - 1) and -(-(NEW - 1) // (k + 1)) <= st["rounds"] <= NEW - 1
    eos = int(ref[0, plens[0] + 5])
    ref_e = _plain(B, sampled, eos)
    assert ref_e[0, plens[0]:].tolist().index(eos) <= 5
    out_e = m.generate(ids, mask, max_new_tokens=NEW, eos_token_id=eos, prompt_lookup_num_tokens=k, **kw)
    assert torch.equal(out_e, ref_e)


@pytest.mark.parametrize("sampled", [False, True])
def test_verify_step_with_oracle_drafts_on_the_gpu(sampled):
    m = _gpu_model()
    B, k = 4, 3
    plens, ids, mask = _prompts(B)
    pl = torch.tensor(plens)
    ref = _plain(B, sampled).cpu()
    oracle = torch.stack([ref[b, pl[b] + 1:pl[b] + 1 + k] for b in range(B)]).to(dev)
    cache = m.new_cache(B, max(plens) + NEW + k + 1, dev)
    for i in (None, 1):   # every draft right; then sequence 2's draft 1 wrong
        cache.reset(seed=3, temperature=0.8 if sampled else 0.0, start=pl - 1, limit=pl - 1 + NEW, draft_tokens=k)
        m.prefill(ids, mask, cache)
        drafts = oracle.clone()
        want = [k + 1] * B
        if i is not None:
            drafts[2, i] = (drafts[2, i] + 1) % 1000
            want[2] = i + 1
        m.verify_step(cache, drafts)
        assert (cache.lens.cpu() - pl.to(torch.int32)).tolist() == want
        assert cache.stats.tolist()[:2] == [sum(want) - B, sum(want)]
        for b in range(B):
            n = int(pl[b]) + want[b] + 1
            assert torch.equal(cache.tokens[b, :n].cpu(), ref[b, :n]) and int(cache.next_ids[b]) == int(ref[b, n - 1])


def test_one_captured_round_serves_other_seeds_and_temperatures_and_another_k_captures_its_own():
    m = _gpu_model()
    _, ids, mask = _prompts(4)
    m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=3, temperature=0.8, seed=3)
    caches = m.__dict__["_kml_decode_caches"]
    count = lambda: (len(caches), sum(len(c._graphs) for c in caches.values()))
    n0 = count()
    hot = m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=3, temperature=1.3, seed=11)
    assert count() == n0
    assert torch.equal(hot, m.generate(ids, mask, max_new_tokens=NEW, temperature=1.3, seed=11))
    mine = [c for c in caches.values() if c.draft_tokens == 3 and c.sample and c.B == 4]
    assert len(mine) == 1 and list(mine[0]._graphs) == [("verify", True, 4)]
    n1 = count()
    m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=2, temperature=0.8, seed=3)
    assert count() == (n1[0] + 1, n1[1] + 1)
