"""The tanh-approximated GELU (HF ``gelu_new``) on the GPU: the stand-alone kernels over every
finite bf16 input, the GEMM forward epilogues of every tile, FFN2's dgrad epilogue, the skinny
decode GEMM, the model's fused training route and the captured decode step.

The kernel tests cannot use a rel-Frobenius check: over randn inputs the tanh and the erf GELU
differ by 2e-4, far inside 1e-2.  They feed exact products (one-hot operands, so that every
accumulator is exactly one bf16 value) and check every element against fp64:
``|y - r| <= 2^-7 |r| + 2^-20`` (bf16 rounding <= 2^-8 relative, fp32 evaluation ~1e-6, the
absolute term for the far negative tail).  tests/test_gelu_tanh_cpu.py shows that the erf GELU
breaks this bound at >= 100 inputs, forward and gradient."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gelu_tanh_cpu import all_finite_bf16, ref_fwd, ref_grad, violations

pytestmark = pytest.mark.gpu
dev = "cuda"
BF = torch.bfloat16
DYS = (1.0, -2.0, 0.5)
TILES = [(256, 256), (256, 256, 4), (256, 256, 8), (256, 192, 8), (256, 128), (128, 256), (128, 128), (128, 128, 2),
         (128, 128, 3, "mf32"), (128, 128, 2, "mf32")]   # the list of test_gemm_gpu.py::test_forward_bias_gelu


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(y, r, what):
    """every element of the bf16 result y within the bound of the fp64 reference r, none NaN"""
    y = y.detach().cpu()
    assert not torch.isnan(y.float()).any(), what
    n = violations(y, r)
    err = ((y.double() - r).abs() / (2.0 ** -7 * r.abs() + 2.0 ** -20)).max().item()
    print(f"{what}: {y.numel()} elements, worst error {err:.3f} of the bound, {n} violations")
    assert n == 0, (what, n)


@functools.lru_cache(maxsize=None)
def vals(limit):
    """every bf16 value with |v| <= limit (both zeros included), on the CPU"""
    x = all_finite_bf16()
    return x[x.float().abs() <= limit].contiguous()


def _tiled(v, n):
    return v[torch.arange(n) % v.numel()]


# ------------------------------------------------------------------------- stand-alone kernels
@functools.lru_cache(maxsize=None)
def _all_refs():
    x = all_finite_bf16()
    return x, ref_fwd(x), ref_grad(x)


def test_gelu_fwd_every_finite_bf16_input_both_kernels():
    from kubeml_amd.ops import transformer as T
    x, r, _ = _all_refs()
    assert vals(8.0).numel() == 33282
    y8 = T.gelu_fwd(x.to(dev), approximate="tanh")              # n % 16 == 0: k_gelu_fwd8
    _check(y8, r, "gelu_fwd tanh, 8-wide kernel")
    tail = torch.tensor([0.5, -0.5, 3.0, -3.0]).to(BF)
    x4 = torch.cat([x, tail])                                   # n = 65280 + 4: the 4-wide kernel
    assert x4.numel() % 8 == 4
    y4 = T.gelu_fwd(x4.to(dev), approximate="tanh")
    _check(y4, ref_fwd(x4), "gelu_fwd tanh, 4-wide kernel")
    assert torch.equal(_bits(y4[:x.numel()]), _bits(y8))
    # saturation: y rounds to x from 8 up, vanishes from -8 down
    yf, xf = y8.float().cpu(), x.float()
    assert torch.equal(yf[xf >= 8], xf[xf >= 8])
    assert (yf[xf <= -8].abs() <= 2.0 ** -20).all()
    # NaN propagates; the erf kernel behind the default argument is another function
    nan = torch.full((8,), float("nan")).to(BF).to(dev)
    assert torch.isnan(T.gelu_fwd(nan, approximate="tanh").float()).all()
    assert violations(T.gelu_fwd(x.to(dev)).cpu(), r) >= 100
    assert torch.equal(_bits(T.gelu_fwd(x.to(dev), approximate="none")), _bits(T.gelu_fwd(x.to(dev))))
    with pytest.raises(ValueError):
        T.gelu_fwd(x.to(dev), approximate="sigmoid")


@pytest.mark.parametrize("dy", DYS)
def test_gelu_bwd_every_finite_bf16_input(dy):
    from kubeml_amd.ops import transformer as T
    x, _, rg = _all_refs()
    d = torch.full(x.shape, dy).to(BF).to(dev)
    dx = T.gelu_bwd(d, x.to(dev), approximate="tanh")
    _check(dx, rg * dy, f"gelu_bwd tanh, dy {dy}")
    g, xf = dx.float().cpu() / dy, x.float()
    assert (g[xf >= 8] == 1).all()
    assert (g[xf <= -8].abs() <= 2.0 ** -20).all()
    nan = torch.full((8,), float("nan")).to(BF).to(dev)
    assert torch.isnan(T.gelu_bwd(d[:8].contiguous(), nan, approximate="tanh").float()).all()
    assert violations(T.gelu_bwd(d, x.to(dev)).cpu(), rg * dy) >= 100   # erf: caught


@pytest.mark.parametrize("M,N", [(300, 72), (7, 1028)])
def test_gelu_bwd_tanh_with_bias_colsum(M, N):
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.ops import transformer as T
    torch.manual_seed(6)
    dy = torch.randn(M, N, device=dev).to(BF)
    x = (2.5 * torch.randn(M, N, device=dev)).to(BF)
    ref = T.gelu_bwd(dy, x, approximate="tanh")
    assert not torch.equal(_bits(ref), _bits(T.gelu_bwd(dy, x)))
    db = torch.full((N,), 0.5, device=dev)
    dx = T.gelu_bwd(dy, x, dbias=db, approximate="tanh")
    assert torch.equal(_bits(dx), _bits(ref))
    want = torch.full((N,), 0.5, device=dev)
    K.colsum_(ref, want)
    assert _rel(db, want) < 1e-5


# ------------------------------------------------------------------------- GEMM forward epilogues
@functools.lru_cache(maxsize=None)
def _fwd_case(with_bias):
    """T = ip = 256, op = 136, x the identity: the accumulator of y[m, n] is exactly w[n, m]"""
    T, ip, op = 256, 256, 136
    v = vals(4.0 if with_bias else 8.0)
    assert v.numel() <= op * ip
    w = _tiled(v, op * ip).view(op, ip).contiguous()
    b = torch.full((op,), 0.5 if with_bias else 0.0)
    x = torch.eye(T, ip).to(BF)
    pre = (w.float().t() + b).to(BF).contiguous()                     # the fp32 sum, rounded once
    ref = F.gelu(w.double().t() + b.double(), approximate="tanh")
    return x.to(dev), w.to(dev), b.to(dev), pre, ref


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("tile", TILES)
def test_gemm_forward_epilogue_tanh(tile, with_bias):
    from kubeml_amd.ops import gemm as G
    from kubeml_amd.ops import transformer as TT
    T, ip, op = 256, 256, 136
    x, w, b, pre_want, ref = _fwd_case(with_bias)

    def run(act):
        y = torch.empty(T, op, dtype=BF, device=dev)
        pre = torch.empty_like(y)
        G.gemm(x, ip, w, ip, y, op, T, op, ip, 0, 0, bias=b, act=act, c2=pre, tile=tile, splits=1)
        return y, pre
    y, pre = run(G.GELU_TANH)
    assert torch.equal(_bits(pre.cpu()), _bits(pre_want))
    _check(y, ref, f"gemm tile {tile} bias {with_bias}")
    # the erf code is the function it was: not the tanh form, and (where the accumulator is a
    # bf16 value) bit for bit what the stand-alone erf kernel makes of it
    ye, pre_e = run(G.GELU)
    assert torch.equal(_bits(pre_e), _bits(pre))
    assert violations(ye.cpu(), ref) >= 50
    if not with_bias:
        assert torch.equal(_bits(ye), _bits(TT.gelu_fwd(pre)))
        assert torch.equal(_bits(y), _bits(TT.gelu_fwd(pre, approximate="tanh")))
    y0 = torch.empty(T, op, dtype=BF, device=dev)
    G.gemm(x, ip, w, ip, y0, op, T, op, ip, 0, 0, bias=b, act=0, tile=tile, splits=1)
    assert torch.equal(_bits(y0), _bits(pre))
    with pytest.raises(ValueError):
        G.gemm(x, ip, w, ip, y0, op, T, op, ip, 0, 0, bias=b, act=9, tile=tile, splits=1)


def _force_phase_tile(monkeypatch):
    """the phase tile on a small FFN2 dgrad, as tests/test_bert_gpu.py forces it"""
    from kubeml_amd.ops import gemm as G
    orig = G.plan

    def plan(layout, M, N, K):
        if layout == 1 and N % 256 == 0 and N > K:
            return (256, 256, 8), 1
        return orig(layout, M, N, K)
    monkeypatch.setattr(G, "plan", plan)


# ------------------------------------------------------------------------- dgrad epilogue
def test_dgrad_epilogue_tanh(monkeypatch):
    from kubeml_amd.ops import gemm as G
    _force_phase_tile(monkeypatch)
    T, ip, op = 300, 256, 64                     # a ragged second M-tile
    dy = torch.zeros(T, op)
    dy[torch.arange(T), torch.arange(T) % op] = 1.0
    c = torch.tensor(DYS)[torch.arange(op) % 3]   # row k of w is the constant c[k]
    w = c[:, None].expand(op, ip).contiguous()
    pre = _tiled(vals(8.0), T * ip).view(T, ip).contiguous()
    assert T * ip >= 2 * vals(8.0).numel()
    scale = c[torch.arange(T) % op].double()[:, None]            # (dy w)[m, n] = c[m % op], exactly
    ref = ref_grad(pre) * scale
    db = torch.zeros(ip, device=dev)
    dx = G.linear_dgrad_gelu(dy.to(BF).to(dev), w.to(BF).to(dev), pre.to(dev), dbias=db, approximate="tanh")
    assert dx is not None and dx.shape == (T, ip)
    _check(dx, ref, "dgrad epilogue tanh")
    assert _rel(db.cpu(), dx.double().sum(0).cpu()) < 1e-5
    erf = G.linear_dgrad_gelu(dy.to(BF).to(dev), w.to(BF).to(dev), pre.to(dev))
    assert erf is not None and violations(erf.cpu(), ref) >= 100
    assert torch.equal(_bits(erf), _bits(G.linear_dgrad_gelu(dy.to(BF).to(dev), w.to(BF).to(dev), pre.to(dev),
                                                             approximate="none")))
    with pytest.raises(ValueError):
        G.linear_dgrad_gelu(dy.to(BF).to(dev), w.to(BF).to(dev), pre.to(dev), approximate="new")


# ------------------------------------------------------------------------- skinny decode GEMM
# (512, 128) is gpt2_tiny's c_fc; the plan does not split it (two K chunks), so it also runs with an
# explicit split of 2, and (768, 3072) is a shape the plan itself splits over blocks
@pytest.mark.parametrize("N,K,splits", [(3072, 768, None), (512, 128, None), (512, 128, 2), (768, 3072, None)])
@pytest.mark.parametrize("with_bias", [False, True])
def test_skinny_gemm_tanh(N, K, splits, with_bias):
    from kubeml_amd.ops import decode as D
    v = vals(4.0 if with_bias else 8.0)
    if N == 3072:
        assert 16 * N >= v.numel()               # every value somewhere in the 16 rows
    else:
        v = v[::-(-v.numel() // (16 * N))]       # an even subset of the range
    S = int(D.HIP.raw("kml_gemm_skinny_splits", N, K)) if splits is None else splits
    if (N, K) == (768, 3072) or splits:
        assert S > 1
    w = torch.ones(N, K, dtype=BF)
    w[:, :16] = _tiled(v, 16 * N).view(16, N).t()           # x row m is one-hot at column m
    x = torch.eye(16, K).to(BF)
    b = torch.full((N,), 0.5) if with_bias else None
    acc = w[:, :16].double().t() + (0.5 if with_bias else 0.0)
    ref = F.gelu(acc, approximate="tanh")
    wg, bg = w.to(dev), None if b is None else b.to(dev)
    full = D.gemm_skinny(x.to(dev), wg, bg, act="gelu_tanh", splits=splits)
    _check(full, ref, f"skinny N {N} K {K} splits {S} bias {with_bias}")
    for M in (1, 4):   # a row's result does not depend on M
        part = D.gemm_skinny(x[:M].contiguous().to(dev), wg, bg, act="gelu_tanh", splits=splits)
        assert torch.equal(_bits(part), _bits(full[:M]))
    erf = D.gemm_skinny(x.to(dev), wg, bg, act="gelu", splits=splits)
    assert violations(erf.cpu(), ref) >= 10   # the erf form is caught (18 .. 152 on these inputs in torch)
    with pytest.raises(ValueError):
        D.gemm_skinny(x.to(dev), wg, bg, act="gelu_new")


# ------------------------------------------------------------------------- model, fused route
def test_gpt_ffn_tanh_backward_in_dgrad_epilogue_matches_unfused(monkeypatch):
    """2048 tokens, 256 features: every Linear on the gemm.hip route, c_fc's tanh GELU in the forward
    epilogue and its backward in c_proj's dgrad epilogue (modules._GELU_FUSE) == the separate pass"""
    from kubeml_amd.models.gpt import GPT2LMHeadModel
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.nn import modules as MO
    from kubeml_amd.nn import transformer as TR
    from kubeml_amd.ops import gemm as G
    from kubeml_amd.ops import transformer as OT
    _force_phase_tile(monkeypatch)
    calls, passes = [], []
    real, real_bwd = G.linear_dgrad_gelu, OT.gelu_bwd

    def spy(*a, **k):
        r = real(*a, **k)
        calls.append((k.get("approximate"), r is not None))
        return r

    def spy_bwd(*a, **k):
        passes.append(k.get("approximate"))
        return real_bwd(*a, **k)
    monkeypatch.setattr(G, "linear_dgrad_gelu", spy)
    monkeypatch.setattr(OT, "gelu_bwd", spy_bwd)
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, 1000, (16, 128), generator=g).to(dev)
    out = []
    old = MO._GELU_FUSE
    try:
        for fuse in (False, True):
            MO._GELU_FUSE = fuse
            torch.manual_seed(0)
            TR.Dropout._salt = 0
            m = GPT2LMHeadModel(vocab=1000, hidden=256, layers=1, heads=4, inter=1024, max_pos=128,
                                activation="gelu_tanh", dropout=0.1).to(dev)
            flatten_module(m)
            m.train()
            loss = m(ids, labels=ids)
            loss.backward()
            torch.cuda.synchronize()
            assert m.transformer.h[0].mlp.c_fc._kml_route == "gemm"
            out.append((float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()}))
    finally:
        MO._GELU_FUSE = old
    assert calls == [("tanh", True)], calls          # the fused run: the tanh dgrad epilogue ran
    assert passes == ["tanh"], passes                # the unfused run: the tanh backward pass
    (l0, p0), (l1, p1) = out
    assert l1 == l0
    for n in p0:
        e = _rel(p1[n], p0[n])
        assert e < (1e-2 if n.endswith("bias") else 1e-3), (n, e)


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    """a tanh gpt2_tiny: the fp64 CPU model and its GPU twin with the same parameters"""
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    ref = gpt2_tiny(dropout=0.0, activation="gelu_tanh").double()
    gpu = gpt2_tiny(dropout=0.0, activation="gelu_tanh")
    gpu.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    gpu = gpu.to(dev)
    flatten_module(gpu)
    return ref, gpu


def test_tanh_gpt2_tiny_matches_fp64():
    """the tolerances of tests/test_gpt_gpu.py::test_gpt2_tiny_matches_fp64"""
    ref, gpu = _tiny_pair()
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 1000, (2, 128), generator=g)
    mask = torch.ones(2, 128, dtype=torch.int64)
    mask[0, 123:] = 0
    ref.train()
    gpu.train()
    ref.zero_grad()
    lr = ref(ids, mask, labels=ids)
    lr.backward()
    lg = gpu(ids.to(dev), mask.to(dev), labels=ids.to(dev))
    lg.backward()
    assert abs(lg.item() - lr.item()) < 0.02 * abs(lr.item())
    gr = {n: p.grad for n, p in ref.named_parameters()}
    for n, p in gpu.named_parameters():
        e = _rel(p.grad.float().cpu(), gr[n])
        assert e < 0.08, (n, e)
    ref.eval()
    gpu.eval()
    with torch.no_grad():
        assert _rel(gpu(ids.to(dev), mask.to(dev)).float().cpu(), ref(ids, mask)) < 0.02


# ------------------------------------------------------------------------- decode
def _prompts():
    plens = (100, 37)
    g = torch.Generator().manual_seed(21)
    L = max(plens)
    mask = (torch.arange(L)[None] < torch.tensor(plens)[:, None]).long()
    ids = torch.randint(1, 1000, (2, L), generator=g) * mask
    return plens, ids, mask, g


def test_tanh_teacher_forced_logits_match_fp64_and_the_step_runs_the_tanh_skinny_gemm(monkeypatch):
    """the tolerance of tests/test_kv_decode_gpu.py; every c_fc call of the captured step and of a
    verify round (gpt2_tiny: the skinny GEMM with N = 512) carries act="gelu_tanh" """
    from kubeml_amd.ops import decode as D
    ref, gpu = _tiny_pair()
    ref.eval()
    gpu.eval()
    seen = []
    real = D.gemm_skinny

    def spy(x, w, bias=None, act=None, **k):
        seen.append((w.shape[0], act))
        return real(x, w, bias, act=act, **k)
    monkeypatch.setattr(D, "gemm_skinny", spy)
    plens, ids, mask, g = _prompts()
    steps = 12
    forced = torch.randint(0, 1000, (2, steps), generator=g)
    want = []
    with torch.no_grad():
        for b, n in enumerate(plens):
            want.append(ref(torch.cat([ids[b, :n], forced[b]])[None])[n - 1:])
    want = torch.stack(want)                               # [2, 1 + steps, vocab]
    cache = gpu.new_cache(2, max(plens) + steps, dev)
    got = [gpu.prefill_logits(ids.to(dev), mask.to(dev), cache).float().cpu()]
    assert not seen
    for t in range(steps):
        got.append(gpu.decode_logits(cache, forced[:, t].to(dev)).float().cpu())
    errs = [_rel(got[t], want[:, t]) for t in range(1 + steps)]
    print(f"tanh cached decode vs fp64: worst step {max(errs):.4f} (prefill {errs[0]:.4f})")
    assert max(errs) < 0.02, errs

    def fc_calls():
        fc = [a for n, a in seen if n == 512]
        rest = [a for n, a in seen if n != 512]
        assert fc and set(fc) == {"gelu_tanh"} and set(rest) == {None}, seen
        return len(fc)
    layers = len(gpu.transformer.h)
    assert fc_calls() == 2 * layers                        # warm-up and capture; replays call nothing
    del seen[:]
    spec = gpu.new_cache(2, max(plens) + steps, dev)
    spec.reset(draft_tokens=3)
    gpu.prefill(ids.to(dev), mask.to(dev), spec)
    gpu.verify_step(spec, gpu.draft_lookup(spec, 3))
    assert fc_calls() == 2 * layers


@pytest.mark.parametrize("sampled", [False, True])
def test_tanh_generate_with_prompt_lookup_equals_plain(sampled):
    _, gpu = _tiny_pair()
    gpu.eval()
    g = torch.Generator().manual_seed(5)
    block = torch.randint(1, 1000, (6,), generator=g)
    ids = torch.stack([block.repeat(3), torch.randint(1, 1000, (18,), generator=g)])
    mask = torch.ones_like(ids)
    mask[1, 11:] = 0
    ids = (ids * mask).to(dev)
    kw = dict(temperature=0.8, seed=3) if sampled else {}
    ref = gpu.generate(ids, mask.to(dev), max_new_tokens=24, **kw)
    out = gpu.generate(ids, mask.to(dev), max_new_tokens=24, prompt_lookup_num_tokens=3, **kw)
    assert torch.equal(out, ref)


def test_erf_and_tanh_models_decode_different_logits():
    """the same constructor call but for the activation: each model captures its own step"""
    from kubeml_amd.models.gpt import gpt2_tiny
    from kubeml_amd.nn import flatten_module
    plens, ids, mask, g = _prompts()
    nxt = torch.randint(0, 1000, (2,), generator=g).to(dev)
    outs = []
    for act in ("gelu", "gelu_tanh", "gelu"):
        torch.manual_seed(0)
        m = gpt2_tiny(dropout=0.0, activation=act).to(dev).eval()
        for p in m.transformer.h.parameters():   # pre-activations of a few units: where the two forms differ
            if p.dim() == 2:
                p.data.mul_(8.0)
        flatten_module(m)
        cache = m.new_cache(2, 128, dev)
        a = m.prefill_logits(ids.to(dev), mask.to(dev), cache).clone()
        outs.append((a, m.decode_logits(cache, nxt)))
    (pe, de), (pt, dt), (pe2, de2) = outs
    assert torch.equal(_bits(pe), _bits(pe2)) and torch.equal(_bits(de), _bits(de2))
    assert not torch.equal(_bits(pe), _bits(pt)) and not torch.equal(_bits(de), _bits(dt))
