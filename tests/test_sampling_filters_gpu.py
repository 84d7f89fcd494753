"""``kml_decode_sample`` (csrc/kernels/decode.hip) on the GPU: the kept set against the stock-torch
twin ``filter_logits`` exactly, draws inside it and following it, neutral filters against
``kml_decode_advance`` bit for bit, the repetition penalty, the shared bookkeeping, and the
filters through ``prefill`` / ``decode_step`` / ``generate`` of the GPT-2 model."""
import functools
import itertools

import pytest
import torch

from kubeml_amd.nn import filter_logits

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16

CLASSES, WIDTH = 5000, 5008
T_SET = 0.8
KS = (0, 1, 7, 4999, 5000, 6000)
PS = (1.0, 0.9, 0.5)
# |kernel share - fp64 share| <= 2^-25 (info is fp32, share <= 1) + 2 * 65535 * 2^-47 (a class
# weight is rounded to a multiple of 2^-46, once per column, in numerator and denominator) + 3e-14
# (fp64 exp2 and its argument): profiles/r13/sampling_filters.md
SHARE_BOUND = 2.0 ** -25 + 2.0 ** -30 + 3e-14


def _state(B, Lcap, eos=-1, seed=5, temperature=1.0, top_k=0, top_p=1.0, penalty=1.0, sample=True):
    from kubeml_amd.ops.decode import sampling_params
    fpar, ipar = sampling_params(temperature, top_k, top_p, penalty, sample=sample)
    return dict(ctl=torch.tensor([seed, 0, eos, 0], dtype=torch.int32, device=dev),
                fpar=torch.tensor(fpar, dtype=torch.float32, device=dev),
                ipar=torch.tensor(ipar, dtype=torch.int32, device=dev),
                next_ids=torch.zeros(B, dtype=torch.int64, device=dev),
                tokens=torch.zeros(B, Lcap, dtype=torch.int64, device=dev),
                lens=torch.zeros(B, dtype=torch.int32, device=dev),
                finished=torch.zeros(B, dtype=torch.int32, device=dev))


def _planted():
    """five bf16 rows of 5000 classes in a 5008-wide buffer whose last 8 columns hold 50.0"""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(5, CLASSES, generator=g) * 1.2   # below 6 everywhere
    # 0: six distinct leaders, then a tie at the 7th value across lanes, waves and strides
    for c, v in zip(range(100, 106), (9.0, 8.5, 8.0, 7.5, 7.0, 6.5)):
        x[0, c] = v
    for c in (0, 2047, 2048, 4999):
        x[0, c] = 6.0
    # 1: negative but for three leaders; +0.0 and -0.0 mixed are the 4th value
    x[1] = -x[1].abs() - 0.5
    x[1, 300], x[1, 2500], x[1, 4097] = 2.0, 1.5, 1.0
    for c in (5, 1000, 4095):
        x[1, c] = 0.0
    for c in (6, 2048, 4998):
        x[1, c] = -0.0
    # 2: NaN in the top region
    x[2, 2], x[2, 4000] = 8.0, 7.0
    for c in (1, 2047, 3000):
        x[2, c] = float("nan")
    # 3: all negative
    x[3] = -x[3].abs() * 1.5 - 1.0
    # 4: two values only
    x[4] = torch.where(torch.rand(CLASSES, generator=g) < 0.5, torch.tensor(1.0), torch.tensor(-2.0))
    pad = torch.full((5, WIDTH), 50.0, dtype=BF)
    pad[:, :CLASSES] = x.to(BF)
    assert torch.signbit(pad[1, 6].float()) and not torch.signbit(pad[1, 5].float())
    return pad


def _facts(z, keep, T):
    """what info reports, from the twin's output in fp64: threshold, count, mass share, vmax"""
    x = z.double().cpu() + 0.0
    keep = keep.cpu()
    valid = ~torch.isnan(x)
    xs = torch.where(valid, x, torch.full_like(x, float("-inf")))
    vmax = xs.max(-1).values
    w = torch.exp((xs - vmax[:, None]) / float(torch.tensor(T, dtype=torch.float32)))
    thr = torch.where(keep, x, torch.full_like(x, float("inf"))).min(-1).values
    return thr, keep.sum(-1), (w * keep).sum(-1) / w.sum(-1), vmax


@functools.lru_cache(maxsize=None)
def _reference():
    """the twin on the planted rows for every (k, p), computed once; asserts on the way that no
    class boundary's cumulative mass lies within ten times the share bound of p Z"""
    pad = _planted()
    rows = pad[:, :CLASSES]
    tok, lens = torch.zeros(5, 64, dtype=torch.int64), torch.full((5,), -1, dtype=torch.int32)
    T = float(torch.tensor(T_SET, dtype=torch.float32))
    ref = {}
    for k, p in itertools.product(KS, PS):
        z, keep = filter_logits(rows, tok, lens, T_SET, k, p, 1.0)
        ref[k, p] = _facts(z, keep, T_SET)
        if p < 1.0:
            _, kk = filter_logits(rows, tok, lens, T_SET, k, 1.0, 1.0)   # the top-k survivors
            pf = float(torch.tensor(p, dtype=torch.float32))
            for b in range(5):
                v = (rows[b].double() + 0.0)[kk[b]]
                vals, inv = torch.unique(v, return_inverse=True)
                mass = torch.zeros_like(vals).index_add_(0, inv, torch.exp((v - vals[-1]) / T)).flip(0)
                cum = mass.cumsum(0)
                gap = ((cum - pf * cum[-1]).abs() / cum[-1]).min().item()
                assert gap >= 10.0 * SHARE_BOUND, (k, p, b, gap)
    return pad, ref


@pytest.mark.parametrize("sample", [True, False])
def test_kept_set_is_the_twins_exactly(sample):
    from kubeml_amd.ops import decode as D
    pad, ref = _reference()
    logits = pad.to(dev)
    worst = 0.0
    for k, p in itertools.product(KS, PS):
        st = _state(5, 64, temperature=T_SET, top_k=k, top_p=p, sample=True)
        st["lens"].fill_(-1)
        info = D.decode_sample(logits, CLASSES, sample=sample, **st).cpu()
        thr, cnt, share, vmax = ref[k, p]
        assert torch.equal(info[:, 0].double(), thr), (k, p, info[:, 0].tolist(), thr.tolist())
        assert torch.equal(info[:, 1].long(), cnt), (k, p, info[:, 1].tolist(), cnt.tolist())
        assert torch.equal(info[:, 3].double(), vmax)
        err = (info[:, 2].double() - share).abs().max().item()
        worst = max(worst, err)
        assert err <= SHARE_BOUND, (k, p, info[:, 2].tolist(), share.tolist())
        z, keep = filter_logits(pad[:, :CLASSES], st["tokens"].cpu(), torch.full((5,), -1), T_SET, k, p, 1.0)
        tok = st["next_ids"].cpu()
        assert keep[torch.arange(5), tok].all()
        best = torch.nan_to_num(z.float(), nan=float("-inf")).argmax(-1)
        if not sample:
            assert torch.equal(tok, best)
        else:   # a kept set of one column leaves the draw no choice
            assert torch.equal(tok[cnt == 1], best[cnt == 1])
    print(f"worst mass-share error {worst:.3e} (bound {SHARE_BOUND:.3e})")
    # the planted structure is what the test meant it to be
    assert ref[7, 1.0][1].tolist()[:2] == [10, 9] and ref[7, 1.0][0].tolist()[:2] == [6.0, 0.0]
    assert ref[0, 1.0][1].tolist() == [5000, 5000, 4997, 5000, 5000]


def test_an_all_nan_row_gives_token_0():
    from kubeml_amd.ops import decode as D
    logits = torch.full((2, 16), float("nan"), dtype=BF, device=dev)
    logits[1, 3] = 1.0
    st = _state(2, 64, top_k=2, top_p=0.5)
    st["next_ids"].fill_(9)
    info = D.decode_sample(logits, 16, sample=True, **st).cpu()
    assert st["next_ids"].tolist() == [0, 3] and st["lens"].tolist() == [1, 1] and st["ctl"].tolist()[1] == 1
    assert info[0, 1] == 0 and info[1].tolist() == [1.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("kw", [dict(top_k=3), dict(top_p=0.8)])
def test_draws_stay_inside_the_kept_set_and_follow_it(kw):
    """the 8-class row of the plain sampler's frequency test: 16 rows x 256 steps = 4096 draws"""
    from kubeml_amd.ops import decode as D
    row = torch.tensor([1.5, 0.0, -1.0, 0.5, 2.0, -2.0, 1.0, 0.25]).to(BF)
    logits = row[None].repeat(16, 1).contiguous().to(dev)
    st = _state(16, 512, seed=1234, **kw)
    draws = []
    for _ in range(256):
        D.decode_sample(logits, 8, sample=True, **st)
        draws.append(st["next_ids"].clone())
    draws = torch.stack(draws).cpu().reshape(-1)
    assert draws.numel() == 4096 and st["ctl"].tolist()[1] == 256
    _, keep = filter_logits(row[None], torch.zeros(1, 1, dtype=torch.int64), torch.tensor([-1]), 1.0,
                            kw.get("top_k", 0), kw.get("top_p", 1.0), 1.0)
    keep = keep[0]
    assert keep.tolist() == ([True, False, False, False, True, False, True, False] if "top_k" in kw else
                             [True, False, False, True, True, False, True, False])
    f = torch.bincount(draws, minlength=8).double() / 4096
    assert (f[~keep] == 0).all()
    q = (row.double().exp() * keep).div((row.double().exp() * keep).sum())
    print("renormalised", [round(v, 4) for v in q.tolist()], "frequency", [round(v, 4) for v in f.tolist()])
    tol = 5.0 * (q * (1 - q) / 4096).sqrt()
    assert ((f - q).abs() <= tol)[keep].all(), ((f - q).abs() / tol).tolist()


def test_neutral_filters_are_the_plain_sampler():
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(17)
    pad = torch.full((16, WIDTH), 50.0, dtype=BF)
    pad[:, :CLASSES] = (torch.randn(16, CLASSES, generator=g) * 2.0).to(BF)
    logits = pad.to(dev)
    old = _state(16, 128, eos=777, seed=91, temperature=0.7)
    new = _state(16, 128, eos=777, seed=91, temperature=0.7)
    temp = torch.tensor([0.7], dtype=torch.float32, device=dev)
    plain = {k: v for k, v in old.items() if k not in ("fpar", "ipar")}
    a, b = [], []
    for _ in range(64):
        D.decode_advance(logits, CLASSES, temp=temp, sample=True, **plain)
        D.decode_sample(logits, CLASSES, sample=True, **new)
        a.append(old["next_ids"].clone())
        b.append(new["next_ids"].clone())
    assert torch.equal(torch.stack(a), torch.stack(b))
    assert len(set(torch.stack(a).reshape(-1).tolist())) > 100
    for k in ("tokens", "lens", "finished", "ctl"):
        assert torch.equal(old[k], new[k]), k
    assert new["ctl"].tolist() == [91, 64, 777, 0]


def test_repetition_penalty_moves_the_greedy_pick():
    from kubeml_amd.ops import decode as D
    g = torch.Generator().manual_seed(23)
    x = torch.randn(3, CLASSES, generator=g) * 1.2
    x[1] = -x[1].abs() - 1.0
    lead, runner = 1234, 4321
    x[0, lead], x[0, runner] = 9.0, 8.0          # 9 / 1.5 = 6 < 8
    x[1, lead], x[1, runner] = -0.5, -0.625      # -0.5 * 1.5 = -0.75 < -0.625
    x[2, lead], x[2, runner] = 9.0, 8.0          # the leader is not in this row's history
    pad = torch.full((3, WIDTH), 50.0, dtype=BF)
    pad[:, :CLASSES] = x.to(BF)
    st = _state(3, 64, penalty=1.5, sample=False)
    tokens = torch.full((3, 64), runner, dtype=torch.int64)   # past lens: must not be penalised
    tokens[0, :5] = torch.tensor([lead, 17, lead, 7000, lead])
    tokens[1, :5] = torch.tensor([lead, lead, 5001, lead, 4999])
    tokens[2, :1] = torch.tensor([17])
    lens = torch.tensor([4, 4, 0], dtype=torch.int32)
    st["tokens"].copy_(tokens)
    st["lens"].copy_(lens)
    info = D.decode_sample(pad.to(dev), CLASSES, sample=False, **st).cpu()
    z, keep = filter_logits(pad[:, :CLASSES], tokens, lens, 1.0, 0, 1.0, 1.5)
    assert not torch.equal(z, pad[:, :CLASSES]) and keep.all()
    assert z[0, lead] == 6.0 and z[0, runner] == 8.0 and z[0, 17] != pad[0, 17] and z[1, 4999] != pad[1, 4999]
    want = z.float().argmax(-1)
    assert want.tolist() == [runner, runner, lead]
    assert st["next_ids"].tolist() == want.tolist()
    thr, cnt, share, vmax = _facts(z, keep, 1.0)
    assert torch.equal(info[:, 3].double(), vmax) and vmax.tolist() == [8.0, -0.625, 9.0]
    assert torch.equal(info[:, 0].double(), thr) and info[:, 1].tolist() == [5000.0] * 3
    # top-k over the penalised row: the columns not in the history are untouched, so the count of
    # columns at or above the 50th value and that value are the twin's
    st2 = _state(3, 64, penalty=1.5, top_k=50, sample=False)
    st2["tokens"].copy_(tokens)
    st2["lens"].copy_(lens)
    info = D.decode_sample(pad.to(dev), CLASSES, sample=False, **st2).cpu()
    z, keep = filter_logits(pad[:, :CLASSES], tokens, lens, 1.0, 50, 1.0, 1.5)
    thr, cnt, share, vmax = _facts(z, keep, 1.0)
    assert torch.equal(info[:, 0].double(), thr) and torch.equal(info[:, 1].long(), cnt)
    assert (info[:, 2].double() - share).abs().max() <= SHARE_BOUND


def test_bookkeeping_eos_saturation_and_guard_bands():
    from kubeml_amd.ops import decode as D
    # the greedy test of the plain sampler through the filtered one
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(5, CLASSES, generator=g).to(BF)
    plant = [0, 4999, 2047, 2048, 777]
    for b, c in enumerate(plant[:4]):
        logits[b, c] = 9.0
    logits[4, 4100] = logits[4, 777] = logits[4, 3000] = 9.0   # the lower column wins
    pad = torch.full((5, WIDTH), 50.0, dtype=BF)
    pad[:, :CLASSES] = logits
    st = _state(5, 64, eos=777, top_k=5, top_p=0.9, sample=False)
    st["lens"].copy_(torch.tensor([0, 5, 62, 63, 9], dtype=torch.int32))
    D.decode_sample(pad.to(dev), CLASSES, sample=False, **st)
    assert st["next_ids"].tolist() == plant
    assert st["lens"].tolist() == [1, 6, 63, 63, 10]          # saturates at Lcap - 1
    assert st["finished"].tolist() == [0, 0, 0, 0, 1]         # row 4 drew eos
    assert st["ctl"].tolist() == [5, 1, 777, 0]
    tok = st["tokens"].cpu()
    assert tok[0, 1] == 0 and tok[1, 6] == 4999 and tok[2, 63] == 2047 and tok[4, 10] == 777
    assert int((tok != 0).sum()) == 3                          # row 3's write at Lcap is dropped
    D.decode_sample(pad.to(dev), CLASSES, sample=False, **st)
    assert st["next_ids"].tolist() == plant and st["finished"].tolist() == [0, 0, 0, 0, 1]
    st["finished"][0] = 1
    D.decode_sample(pad.to(dev), CLASSES, sample=False, **st)
    assert st["next_ids"].tolist()[0] == 777 and st["ctl"].tolist()[1] == 3
    # saturated sequences: nothing is written outside tokens, lens stays
    B, Lcap = 2, 64
    buf = torch.full((B * Lcap + 128,), -7, dtype=torch.int64, device=dev)
    st = _state(B, Lcap, top_k=3, penalty=1.2)
    st["tokens"] = buf[64:64 + B * Lcap].view(B, Lcap)
    st["lens"].fill_(Lcap - 1)
    small = torch.zeros(B, 8, dtype=BF, device=dev)
    for _ in range(2):
        D.decode_sample(small, 8, sample=True, **st)
    assert (buf == -7).all() and st["lens"].tolist() == [Lcap - 1] * B
    with pytest.raises(ValueError):
        D.decode_sample(torch.zeros(1, 65536, dtype=BF, device=dev), 65536, sample=True, **_state(1, 64))


# ------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def _model():
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    gpu = gpt2_tiny(dropout=0.0).to(dev).eval()
    flatten_module(gpu)
    return gpu


def _prompts():
    plens = (17, 3, 40)
    g = torch.Generator().manual_seed(31)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    ids = torch.randint(1, 1000, (3, L), generator=g) * mask
    return plens, ids.to(dev), mask.to(dev)


def _drive(gpu, ids, mask, new, **kw):
    """prefill + decode_step by hand: per step (bf16 logits, tokens and lens before the pick, pick)"""
    from kubeml_amd.nn.flat import shadow_of
    for p in gpu.parameters():   # bf16 shadows current, as generate makes them
        shadow_of(p)
    plens = mask.sum(1)
    cache = gpu.new_cache(ids.shape[0], ids.shape[1] + new, dev)
    cache.reset(**kw)
    steps = []
    before = torch.zeros_like(cache.tokens)
    before[:, :ids.shape[1]] = ids
    z = gpu.prefill(ids, mask, cache)
    steps.append((z[:, :1000].clone().cpu(), before.cpu(), (plens - 1).int().cpu(), cache.next_ids.clone().cpu()))
    for _ in range(new - 1):
        tb, lb = cache.tokens.clone().cpu(), cache.lens.clone().cpu()
        z = gpu.decode_step(cache)
        steps.append((z[:, :1000].clone().cpu(), tb, lb, cache.next_ids.clone().cpu()))
    return cache, steps


def test_every_token_of_the_filtered_model_step_lies_in_the_twins_kept_set():
    gpu = _model()
    plens, ids, mask = _prompts()
    kw = dict(top_k=5, top_p=0.9, repetition_penalty=1.2, temperature=0.8)
    cache, steps = _drive(gpu, ids, mask, 12, seed=7, **kw)
    assert cache.filtered and list(cache._graphs) == [(True, True, True)]
    sizes = []
    for z, tb, lb, tok in steps:
        zt, keep = filter_logits(z, tb, lb, 0.8, 5, 0.9, 1.2)
        assert keep[torch.arange(3), tok].all()
        sizes += keep.sum(-1).tolist()
    assert min(sizes) >= 1 and cache.lens.tolist() == [n - 1 + 12 for n in plens]
    # top_k = 1 is greedy wherever the step's maximum is unique
    _, steps = _drive(gpu, ids, mask, 12, seed=7, top_k=1, temperature=0.8)
    unique = 0
    for z, tb, lb, tok in steps:
        zf = z.float()
        one = (zf == zf.max(-1, keepdim=True).values).sum(-1) == 1
        unique += int(one.sum())
        assert torch.equal(tok[one], zf.argmax(-1)[one])
    assert unique >= 30


def test_generate_with_filters_replays_one_graph_and_leaves_plain_generate_alone():
    gpu = _model()
    plens, ids, mask = _prompts()
    new = 12
    gpu.__dict__.pop("_kml_decode_caches", None)
    plain0 = gpu.generate(ids, mask, max_new_tokens=new)
    hot0 = gpu.generate(ids, mask, max_new_tokens=new, temperature=0.8, seed=7)
    kw = dict(top_k=5, top_p=0.9, repetition_penalty=1.2, temperature=0.8)
    a = gpu.generate(ids, mask, max_new_tokens=new, seed=7, **kw)
    b = gpu.generate(ids, mask, max_new_tokens=new, seed=7, **kw)
    c = gpu.generate(ids, mask, max_new_tokens=new, seed=8, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, hot0)
    for r, n in enumerate(plens):
        assert torch.equal(a[r, :n], ids[r, :n]) and int(a[r].max()) < 1000
    caches = gpu.__dict__["_kml_decode_caches"]
    count = lambda: (len(caches), sum(len(cc._graphs) for cc in caches.values()))
    n0 = count()
    k1 = gpu.generate(ids, mask, max_new_tokens=new, seed=7, top_k=1, temperature=0.8)
    gpu.generate(ids, mask, max_new_tokens=new, seed=7, top_p=0.5, temperature=1.3)
    gpu.generate(ids, mask, max_new_tokens=new, seed=7, repetition_penalty=1.7, top_k=40, temperature=0.8)
    assert count() == n0
    # greedy with a filter is its own graph (sample off, filtered on), captured once
    g1 = gpu.generate(ids, mask, max_new_tokens=new, top_k=1)
    g2 = gpu.generate(ids, mask, max_new_tokens=new, top_k=3, top_p=0.7)
    assert torch.equal(g1, plain0) and torch.equal(g2, plain0)
    assert count()[1] == n0[1] + 1
    # top_k = 1 while sampling: greedy too, as long as no step's maximum ties (checked by hand above)
    assert k1.shape == plain0.shape
    # the plain paths after the filtered calls, and from fresh caches
    assert torch.equal(gpu.generate(ids, mask, max_new_tokens=new), plain0)
    assert torch.equal(gpu.generate(ids, mask, max_new_tokens=new, temperature=0.8, seed=7), hot0)
    gpu.__dict__.pop("_kml_decode_caches", None)
    assert torch.equal(gpu.generate(ids, mask, max_new_tokens=new), plain0)
    assert torch.equal(gpu.generate(ids, mask, max_new_tokens=new, temperature=0.8, seed=7), hot0)
