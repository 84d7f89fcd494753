"""Prompt-lookup speculative decoding on the CPU path (stock torch, fp32 ``gpt2_tiny``): the n-gram
drafter's rule on hand-made histories, ``generate(prompt_lookup_num_tokens=k)`` against plain
``generate`` element for element (greedy, sampled, with eos, ragged batches), the argument checks,
``verify_step`` fed the plain run's own continuation, and the inert default.  Every comparison is
exact."""
import functools

import pytest
import torch

NEW = 20
BLOCK = (11, 57, 402, 7, 950, 33)


@functools.lru_cache(maxsize=None)
def _model():
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    return gpt2_tiny(dropout=0.0).eval()


@functools.lru_cache(maxsize=None)
def _prompts(B):
    """right-padded prompts; sequence 0 is a repeated block, so that lookups match"""
    plens = (18, 5, 9, 1)[:B]
    L = max(plens)
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(1, 1000, (B, L), generator=g)
    ids[0] = torch.tensor(BLOCK * 3)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    return plens, ids * mask, mask


@functools.lru_cache(maxsize=None)
def _plain(B, sampled, eos=None):
    _, ids, mask = _prompts(B)
    kw = dict(temperature=0.8, seed=3) if sampled else {}
    return _model().generate(ids, mask, max_new_tokens=NEW, eos_token_id=eos, **kw)


def _hist(rows, Lcap=16, pad=999):
    """tokens [B, Lcap] and lens from lists; everything past a history is `pad` (never to be read)"""
    t = torch.full((len(rows), Lcap), pad, dtype=torch.int64)
    for b, r in enumerate(rows):
        t[b, :len(r)] = torch.tensor(r)
    return t, torch.tensor([len(r) - 1 for r in rows], dtype=torch.int32)


# (history, k, max_ngram, expected draft)
DRAFT_CASES = [
    ([1, 2, 3, 4], 3, 2, [4, 4, 4]),                       # no match at g = 2 or 1: the newest token
    ([5, 6, 7, 8, 6], 3, 2, [7, 8, 6]),                    # (8, 6) nowhere; 6 at 1: what follows it
    ([1, 2, 9, 1, 2, 8, 1, 2], 3, 2, [8, 1, 2]),           # (1, 2) at 0 and 3: the most recent wins
    ([3, 4, 5, 3, 4], 5, 2, [5, 3, 4, 4, 4]),              # three tokens follow, the last one pads
    ([9], 3, 2, [9, 9, 9]),                                # lens = 0: nothing to look up
    ([4, 4, 4, 4], 2, 3, [4, 4]),                          # overlapping occurrences, g = 3 at start 0
    ([1, 2, 3, 1, 2, 3, 1], 4, 1, [2, 3, 1, 1]),           # max_ngram 1: the 1 at 3, never past lens
]


def test_drafter_twin_on_hand_made_histories():
    from kubeml_amd.nn import lookup_draft_reference
    for hist, k, g, want in DRAFT_CASES:
        tokens, lens = _hist([hist])
        got = lookup_draft_reference(tokens, lens, k, g)
        assert got.dtype == torch.int64 and got.shape == (1, k)
        assert got[0].tolist() == want, (hist, k, g)
    # a batch: every row by its own history
    same_k = [c for c in DRAFT_CASES if c[1] == 3 and c[2] == 2]
    tokens, lens = _hist([c[0] for c in same_k])
    assert lookup_draft_reference(tokens, lens, 3, 2).tolist() == [c[3] for c in same_k]


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B,k", [(1, 1), (1, 3), (1, 7), (1, 15), (4, 3)])
def test_generate_with_prompt_lookup_equals_plain_generate(B, k, sampled):
    m = _model()
    plens, ids, mask = _prompts(B)
    kw = dict(temperature=0.8, seed=3) if sampled else {}
    ref = _plain(B, sampled)
    out = m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=k, **kw)
    assert torch.equal(out, ref)
    st = m.last_generate_stats
    assert st["tokens"] == B * (NEW - 1) and 0 <= st["accepted"] < st["tokens"]
    assert -(-(NEW - 1) // (k + 1)) <= st["rounds"] <= NEW - 1
    # an eos that sequence 0 draws part-way (taken from the plain run): it stops there, the others go on
    eos = int(ref[0, plens[0] + 5])
    ref_e = _plain(B, sampled, eos)
    first = ref_e[0, plens[0]:].tolist().index(eos)
    assert first <= 5 and (ref_e[0, plens[0] + first:] == eos).all()
    out_e = m.generate(ids, mask, max_new_tokens=NEW, eos_token_id=eos, prompt_lookup_num_tokens=k, **kw)
    assert torch.equal(out_e, ref_e)


def test_lookups_are_accepted_on_the_repeated_prompt():
    """greedy on the repeated block: the drafter must hit sometimes, or the tests above show little"""
    m = _model()
    _, ids, mask = _prompts(1)
    m.generate(ids, mask, max_new_tokens=NEW, prompt_lookup_num_tokens=3)
    st = m.last_generate_stats
    print("prompt lookup on the repeated prompt:", st)
    assert st["accepted"] > 0 and st["rounds"] < NEW - 1


def test_argument_checks():
    m = _model()
    _, ids, mask = _prompts(4)
    for bad in (dict(prompt_lookup_num_tokens=-1), dict(prompt_lookup_num_tokens=1.5),
                dict(prompt_lookup_num_tokens=2, max_matching_ngram_size=0),
                dict(prompt_lookup_num_tokens=4),                       # 4 x 5 = 20 rows
                dict(prompt_lookup_num_tokens=2, top_k=5), dict(prompt_lookup_num_tokens=2, top_p=0.9),
                dict(prompt_lookup_num_tokens=2, repetition_penalty=1.2)):
        with pytest.raises(ValueError):
            m.generate(ids, mask, max_new_tokens=2, **bad)
    five = torch.ones(5, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        m.generate(five, max_new_tokens=2, prompt_lookup_num_tokens=1)   # B > 4 (10 rows would fit)
    # B * (k + 1) = 16 is taken, 17 is not
    m.generate(ids, mask, max_new_tokens=2, prompt_lookup_num_tokens=3)
    m.generate(ids[:1], mask[:1], max_new_tokens=2, prompt_lookup_num_tokens=15)
    with pytest.raises(ValueError):
        m.generate(ids[:1], mask[:1], max_new_tokens=2, prompt_lookup_num_tokens=16)
    # the existing checks stay
    with pytest.raises(ValueError):
        m.generate(ids, mask, max_new_tokens=256 - 18 + 1, prompt_lookup_num_tokens=2)   # max_pos = 256
    with pytest.raises(ValueError):
        m.generate(ids, mask, max_new_tokens=0, prompt_lookup_num_tokens=2)
    with pytest.raises(ValueError):
        m.generate(ids, mask.flip(1), max_new_tokens=2, prompt_lookup_num_tokens=2)      # left-padded


def _prefilled(B, k, sampled, limit_new=NEW):
    m = _model()
    plens, ids, mask = _prompts(B)
    pl = torch.tensor(plens)
    cache = m.new_cache(B, max(plens) + NEW + k + 1)
    cache.reset(seed=3, temperature=0.8 if sampled else 0.0, start=pl - 1, limit=pl - 1 + limit_new, draft_tokens=k)
    m.prefill(ids, mask, cache)
    return m, cache, pl


@pytest.mark.parametrize("sampled", [False, True])
def test_verify_step_with_oracle_drafts(sampled):
    B, k = 4, 3
    ref = _plain(B, sampled)
    m, cache, pl = _prefilled(B, k, sampled)
    assert cache.lens.tolist() == pl.tolist() and cache.next_ids.tolist() == [int(ref[b, pl[b]]) for b in range(B)]
    oracle = torch.stack([ref[b, pl[b] + 1:pl[b] + 1 + k] for b in range(B)])
    logits = m.verify_step(cache, oracle)
    assert logits.shape == (B * (k + 1), 1000)
    assert cache.lens.tolist() == (pl + k + 1).tolist()
    assert cache.stats.tolist()[:2] == [B * k, B * (k + 1)]
    for b in range(B):
        n = int(pl[b])
        assert torch.equal(cache.tokens[b, :n + k + 2], ref[b, :n + k + 2])
        assert int(cache.next_ids[b]) == int(ref[b, n + k + 1])
    # a second round from there, one draft of sequence 2 corrupted at index i
    for i in range(k):
        m, cache, pl = _prefilled(B, k, sampled)
        bad = oracle.clone()
        bad[2, i] = (bad[2, i] + 1) % 1000
        m.verify_step(cache, bad)
        want = [k + 1] * B
        want[2] = i + 1
        assert (cache.lens - pl.to(torch.int32)).tolist() == want
        at = int(pl[2]) + i + 1
        assert int(cache.tokens[2, at]) == int(ref[2, at]) == int(cache.next_ids[2])   # the plain run's token
        assert cache.stats.tolist()[:2] == [B * k - (k - i), B * (k + 1) - (k - i)]


def test_verify_step_commits_nothing_past_the_limit():
    B, k = 4, 3
    ref = _plain(B, False)
    m, cache, pl = _prefilled(B, k, False, limit_new=3)   # lens = start + 1, limit = start + 3
    oracle = torch.stack([ref[b, pl[b] + 1:pl[b] + 1 + k] for b in range(B)])
    m.verify_step(cache, oracle)
    assert cache.lens.tolist() == cache.limit.tolist() == (pl + 2).tolist()
    for b in range(B):
        n = int(pl[b])
        assert torch.equal(cache.tokens[b, :n + 3], ref[b, :n + 3]) and (cache.tokens[b, n + 3:] == 0).all()
    assert cache.stats.tolist()[:3] == [B, 2 * B, 0]
    before = (cache.lens.clone(), cache.tokens.clone(), cache.next_ids.clone())
    m.verify_step(cache, oracle)   # frozen: a further round changes nothing
    assert all(torch.equal(a, b) for a, b in zip(before, (cache.lens, cache.tokens, cache.next_ids)))
    assert cache.stats.tolist()[:3] == [B, 2 * B, 0]


def test_multi_row_cache_twins_match_the_one_row_calls():
    """append_cpu / attend_cpu with several rows per sequence: row t is the one-row call at lens + t"""
    from kubeml_amd.nn import KVCache
    B, H, Lq = 2, 2, 3
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * Lq, 3 * H * 64, generator=g)
    a, b = KVCache(1, B, H, 64, "cpu"), KVCache(1, B, H, 64, "cpu")
    for c in (a, b):
        c.k[0].copy_(torch.randn(c.k[0].shape, generator=torch.Generator().manual_seed(6)))
        c.v[0].copy_(torch.randn(c.v[0].shape, generator=torch.Generator().manual_seed(7)))
        c.lens.copy_(torch.tensor([4, 62]))   # sequence 1: the last row falls off the cache
    a.append_cpu(0, qkv, Lq, decode=True)
    many = a.attend_cpu(0, qkv, Lq).reshape(B, Lq, -1)
    for t in range(Lq):
        one = qkv.reshape(B, Lq, -1)[:, t]
        b.append_cpu(0, one, 1, decode=True)
        assert torch.equal(b.attend_cpu(0, one), many[:, t])
        b.lens.add_(1)
    assert torch.equal(a.k[0], b.k[0]) and torch.equal(a.v[0], b.v[0])


def test_the_default_is_inert():
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    m = gpt2_tiny(dropout=0.0).eval()
    _, ids, mask = _prompts(4)
    out = m.generate(ids, mask, max_new_tokens=4, prompt_lookup_num_tokens=0)
    assert torch.equal(out, m.generate(ids, mask, max_new_tokens=4))
    assert getattr(m, "last_generate_stats", None) is None
    keys = list(m.__dict__["_kml_decode_caches"])
    assert keys == [(4, 64, False, ids.device, torch.float32, 0)]
    cache = m.__dict__["_kml_decode_caches"][keys[0]]
    assert cache.draft_tokens == 0 and cache.draft is None and cache.start is None and cache.stats is None
