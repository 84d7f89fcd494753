"""KV-cache decoding of the GPT-2 model on the CPU path (stock torch, fp64): teacher-forced
logits against the full forward on each sequence alone, and ``generate`` against the greedy
recompute loop."""
import functools

import pytest
import torch

B = 3
PLENS = (5, 9, 1)
STEPS = 12


@functools.lru_cache(maxsize=None)
def _model():
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    return gpt2_tiny(dropout=0.0).double().eval()


@functools.lru_cache(maxsize=None)
def _prompts():
    g = torch.Generator().manual_seed(11)
    L = max(PLENS)
    ids = torch.randint(1, 1000, (B, L), generator=g)
    mask = (torch.arange(L)[None] < torch.tensor(PLENS)[:, None]).long()
    return ids * mask, mask


def _alone(m, seq):
    """logits [len, vocab] of one unpadded sequence through the full forward"""
    with torch.no_grad():
        return m(seq[None])


def test_teacher_forced_logits_match_the_full_forward():
    m = _model()
    ids, mask = _prompts()
    g = torch.Generator().manual_seed(12)
    forced = torch.randint(0, 1000, (B, STEPS), generator=g)
    cache = m.new_cache(B, max(PLENS) + STEPS)
    got = [m.prefill_logits(ids, mask, cache)]
    for t in range(STEPS):
        got.append(m.decode_logits(cache, forced[:, t]))
    got = torch.stack(got, 1)   # [B, 1 + STEPS, vocab]
    assert got.shape == (B, 1 + STEPS, 1000)
    worst = 0.0
    for b, n in enumerate(PLENS):
        full = _alone(m, torch.cat([ids[b, :n], forced[b]]))   # [n + STEPS, vocab]
        worst = max(worst, (got[b] - full[n - 1:]).abs().max().item())
    print("max abs difference, cached vs full forward (fp64):", worst)
    assert worst < 1e-9
    assert cache.lens.tolist() == [n - 1 + STEPS for n in PLENS]


def _greedy_recompute(m, ids, mask, new, eos=None):
    out = []
    for b in range(ids.shape[0]):
        n = int(mask[b].sum())
        seq = ids[b, :n]
        done = False
        for _ in range(new):
            tok = eos if done else int(_alone(m, seq)[-1].argmax())
            done = done or (eos is not None and tok == eos)
            seq = torch.cat([seq, torch.tensor([tok])])
        out.append(seq)
    return out


def test_greedy_generate_equals_recompute_and_eos_fills():
    m = _model()
    ids, mask = _prompts()
    new = 10
    out = m.generate(ids, mask, max_new_tokens=new)
    assert out.dtype == torch.int64 and out.shape == (B, max(PLENS) + new)
    ref = _greedy_recompute(m, ids, mask, new)
    for b, n in enumerate(PLENS):
        assert torch.equal(out[b, :n + new], ref[b]), b
        assert torch.equal(out[b, n + new:], torch.zeros(max(PLENS) - n, dtype=torch.int64))
    # eos = the first token sequence 0 generates: that sequence alone is eos from there on
    eos = int(ref[0][PLENS[0]])
    assert all(eos not in ref[b][PLENS[b]:].tolist() for b in (1, 2)), "pick another seed: eos drawn elsewhere"
    out2 = m.generate(ids, mask, max_new_tokens=new, eos_token_id=eos)
    assert torch.equal(out2[0, :PLENS[0]], ids[0, :PLENS[0]])
    assert torch.equal(out2[0, PLENS[0]:], torch.full((out2.shape[1] - PLENS[0],), eos))
    for b in (1, 2):
        n = PLENS[b]
        assert torch.equal(out2[b, :n + new], ref[b])
        assert torch.equal(out2[b, n + new:], torch.full((max(PLENS) - n,), eos))
    # no mask: every prompt is full length
    full = torch.randint(1, 1000, (2, 4), generator=torch.Generator().manual_seed(5))
    o3 = m.generate(full, max_new_tokens=3)
    r3 = _greedy_recompute(m, full, torch.ones_like(full), 3)
    assert torch.equal(o3, torch.stack(r3))


def test_generate_rejects_what_it_cannot_do():
    m = _model()
    ids, mask = _prompts()
    with pytest.raises(ValueError):
        m.generate(ids, mask, max_new_tokens=256 - max(PLENS) + 1)   # max_pos = 256
    m.generate(ids[:1, :1], max_new_tokens=2)
    with pytest.raises(ValueError):
        m.generate(torch.zeros(17, 2, dtype=torch.int64), max_new_tokens=2)
    left = mask.flip(1)
    with pytest.raises(ValueError):
        m.generate(ids, left, max_new_tokens=2)   # left-padded


def test_sampling_is_repeatable_per_seed():
    m = _model()
    ids, mask = _prompts()
    a = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=3)
    b = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=3)
    c = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=4)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert int(a.min()) >= 0 and int(a.max()) < 1000
