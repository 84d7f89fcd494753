"""Repetition penalty, top-k and top-p of ``generate`` without a GPU: the stock-torch twin
``filter_logits`` against HuggingFace's logits processors, its tie / signed-zero / NaN semantics,
and the CPU ``generate`` with the filters on."""
import functools
import itertools

import pytest
import torch

from kubeml_amd.nn import filter_logits

C = 257
T = 0.7
KS = (1, 5, 256, 257, 1000)
PS = (0.3, 0.9, 1.0)
PENS = (1.0, 1.3)


def _rows():
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(3, C, generator=g) * 3.0
    tokens = torch.randint(0, C, (3, 24), generator=g)
    lens = torch.tensor([23, 9, 0], dtype=torch.int32)
    return logits, tokens, lens


def _penalised(logits, tokens, lens, pen):
    """the penalty written out the slow way, independent of the twin"""
    z = logits.clone()
    for b in range(z.shape[0]):
        for c in set(tokens[b, :int(lens[b]) + 1].tolist()):
            z[b, c] = z[b, c] / pen if z[b, c] > 0 else z[b, c] * pen
    return z


@pytest.mark.parametrize("pen", PENS)
def test_twin_equals_the_hf_processor_chain(pen):
    tf = pytest.importorskip("transformers")
    logits, tokens, lens = _rows()
    # the inputs themselves: no two values tie, and no class boundary's cumulative mass comes
    # within 1e-6 (of Z) of p Z — so keeping whole tied classes cannot differ from HF
    z = _penalised(logits, tokens, lens, pen).double()
    for b in range(3):
        assert torch.unique(z[b]).numel() == C
        v = z[b].sort(descending=True).values
        for k in KS:
            s = v[:k] if k < C else v
            cum = torch.exp((s - s[0]) / T).cumsum(0)
            for p in PS:
                if p < 1.0:
                    assert ((cum - p * cum[-1]).abs() >= 1e-6 * cum[-1]).all(), (b, k, p)
    for k, p in itertools.product(KS, PS):
        zt, keep = filter_logits(logits, tokens, lens, T, k, p, pen)
        for b in range(3):
            hist = tokens[b:b + 1, :int(lens[b]) + 1]
            s = tf.RepetitionPenaltyLogitsProcessor(penalty=pen)(hist, logits[b:b + 1].clone())
            assert torch.equal(s, zt[b:b + 1])
            s = tf.TemperatureLogitsWarper(T)(hist, s)
            s = tf.TopKLogitsWarper(top_k=k)(hist, s)
            s = tf.TopPLogitsWarper(top_p=p)(hist, s)
            assert torch.equal(torch.isfinite(s)[0], keep[b]), (k, p, b)
    assert int(filter_logits(logits, tokens, lens, T, 5, 1.0, pen)[1].sum()) == 15


def test_ties_at_the_kth_value_are_all_kept():
    x = torch.tensor([[1.0, 3.0, 2.0, 2.0, 0.5, 2.0, -1.0]])
    tok, lens = torch.zeros(1, 1, dtype=torch.int64), torch.tensor([-1], dtype=torch.int32)
    _, keep = filter_logits(x, tok, lens, 1.0, 2, 1.0, 1.0)
    assert keep.tolist() == [[False, True, True, True, False, True, False]]
    _, keep = filter_logits(x, tok, lens, 1.0, 1, 1.0, 1.0)
    assert keep.tolist() == [[False, True, False, False, False, False, False]]
    # top-p walks whole classes: 3.0 alone is 0.43 of the mass, with the class of 2.0 0.90, then 0.96, 0.99
    for p, n in ((0.3, 1), (0.5, 4), (0.93, 5), (0.97, 6), (0.999, 7)):
        assert int(filter_logits(x, tok, lens, 1.0, 0, p, 1.0)[1].sum()) == n, p
    # k >= classes and k == 0 are off
    for k in (0, 7, 8):
        assert filter_logits(x, tok, lens, 1.0, k, 1.0, 1.0)[1].all()


def test_signed_zeros_are_one_class_and_nan_is_never_kept():
    nan = float("nan")
    x = torch.tensor([[-1.0, 0.0, -0.0, nan, -2.0, 0.0, nan, -0.0]]).to(torch.bfloat16)
    tok, lens = torch.zeros(1, 1, dtype=torch.int64), torch.tensor([-1], dtype=torch.int32)
    _, keep = filter_logits(x, tok, lens, 1.0, 1, 1.0, 1.0)
    assert keep.tolist() == [[False, True, True, False, False, True, False, True]]
    _, keep = filter_logits(x, tok, lens, 1.0, 0, 1.0, 1.0)
    assert keep.tolist() == [[True, True, True, False, True, True, False, True]]
    _, keep = filter_logits(x, tok, lens, 1.0, 0, 0.5, 1.0)   # the four zeros: 4 / (4 + e^-1 + e^-2) = 0.89
    assert int(keep.sum()) == 4
    z, keep = filter_logits(torch.full((2, 5), nan), torch.zeros(2, 1, dtype=torch.int64),
                            torch.tensor([-1, -1], dtype=torch.int32), 1.0, 2, 0.5, 1.0)
    assert not keep.any() and torch.isnan(z).all()


def test_penalty_once_per_distinct_id_and_ids_outside_the_classes_ignored():
    x = torch.tensor([[2.0, -2.0, 4.0, 1.0], [2.0, -2.0, 4.0, 1.0]])
    tokens = torch.tensor([[2, 2, 2, 9, -3, 1, 0], [3, 0, 0, 0, 0, 0, 0]])
    lens = torch.tensor([5, 0], dtype=torch.int32)   # row 0: column 0 lies past lens; row 1: only id 3
    z, keep = filter_logits(x, tokens, lens, 1.0, 0, 1.0, 2.0)
    assert z.tolist() == [[2.0, -4.0, 2.0, 1.0], [2.0, -2.0, 4.0, 0.5]] and keep.all()
    # bf16 input takes the kernel's arithmetic: bf16(fp32(v) * fp32(1 / penalty)), once
    xb = torch.tensor([[1.7109375, -0.3125, 3.0]]).to(torch.bfloat16)
    zb, _ = filter_logits(xb, torch.tensor([[0, 0, 1]]), torch.tensor([2], dtype=torch.int32), 1.0, 0, 1.0, 1.3)
    inv, pen = torch.tensor(1.0 / 1.3, dtype=torch.float32), torch.tensor(1.3, dtype=torch.float32)
    want = torch.stack([(xb[0, 0].float() * inv).to(torch.bfloat16), (xb[0, 1].float() * pen).to(torch.bfloat16),
                        xb[0, 2]])
    assert zb.dtype == torch.bfloat16 and torch.equal(zb[0], want)


# ------------------------------------------------------------------------------ CPU generate
@functools.lru_cache(maxsize=None)
def _model():
    from kubeml_amd.models.gpt import gpt2_tiny
    torch.manual_seed(0)
    return gpt2_tiny(dropout=0.0).double().eval()


def _prompts():
    g = torch.Generator().manual_seed(11)
    plens = (5, 9, 1)
    ids = torch.randint(1, 1000, (3, 9), generator=g)
    mask = (torch.arange(9)[None] < torch.tensor(plens)[:, None]).long()
    return ids * mask, mask


def test_top_k_1_is_greedy_and_an_all_nan_row_gives_token_0():
    m = _model()
    ids, mask = _prompts()
    new = 10
    # the greedy run by hand: every step's maximum is unique
    cache = m.new_cache(3, 9 + new)
    cache.reset()
    z = [m.prefill(ids, mask, cache)] + [m.decode_step(cache) for _ in range(new - 1)]
    for s in z:
        top = s.topk(2, dim=-1).values
        assert (top[:, 0] > top[:, 1]).all()
    greedy = m.generate(ids, mask, max_new_tokens=new)
    assert torch.equal(greedy[:, :cache.tokens.shape[1]], cache.tokens[:, :greedy.shape[1]])
    for T_, seed in ((0.9, 5), (3.0, 6)):
        assert torch.equal(m.generate(ids, mask, max_new_tokens=new, temperature=T_, seed=seed, top_k=1), greedy)
    assert torch.equal(m.generate(ids, mask, max_new_tokens=new, top_k=1, top_p=0.5), greedy)
    # a filtered pick over a row without one comparable value
    from kubeml_amd.models.gpt import _advance_cpu
    cache.reset(temperature=1.0, top_k=3)
    _advance_cpu(cache, torch.full((3, 1000), float("nan"), dtype=torch.float64), cache.gen)
    assert cache.next_ids.tolist() == [0, 0, 0]


def test_neutral_filters_change_nothing_and_filters_do():
    m = _model()
    ids, mask = _prompts()
    for kw in (dict(), dict(temperature=1.0, seed=3)):
        a = m.generate(ids, mask, max_new_tokens=16, **kw)
        b = m.generate(ids, mask, max_new_tokens=16, top_k=0, top_p=1.0, repetition_penalty=1.0, **kw)
        assert torch.equal(a, b)
    free = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=3)
    cut = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=3, top_k=4, top_p=0.9)
    again = m.generate(ids, mask, max_new_tokens=16, temperature=1.0, seed=3, top_k=4, top_p=0.9)
    assert torch.equal(cut, again) and not torch.equal(cut, free)
    # a strong penalty: greedy decoding no longer repeats what a positive logit once chose
    pen = m.generate(ids, mask, max_new_tokens=16, repetition_penalty=50.0)
    assert not torch.equal(pen, m.generate(ids, mask, max_new_tokens=16))


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(top_p=0.0),
                                dict(top_p=1.5), dict(top_k=-1), dict(top_k=2.5)])
def test_invalid_parameters_raise(kw):
    m = _model()
    ids, mask = _prompts()
    with pytest.raises(ValueError):
        m.generate(ids, mask, max_new_tokens=2, **kw)
    from kubeml_amd.ops.decode import sampling_params
    with pytest.raises(ValueError):
        sampling_params(temperature=0.0, sample=True)
    assert sampling_params(0.0, 3, 0.5, 2.0, sample=False) == ([1.0, 0.5, 2.0, 0.5], [3])
