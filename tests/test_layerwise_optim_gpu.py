"""Fused LAMB and LARS on the MI355X: the two-launch layer-wise step (segmented, deterministic
per-tensor norms over the chunk table, then the update), the optimizer classes, the graph-captured
step and ``KubeModel.step``.

The yardstick is ``Ref`` below: a per-tensor fp64 torch implementation of the formulas in
``kubeml_amd/optim/layerwise.py``'s docstring, independent of the package's own CPU path.

Tolerances
----------
* trust ratios, rtol 1e-5.  A sum of squares is blocked fp32 summation of non-negative terms:
  ``_sumsq_bound`` counts the additions on the longest path (32 per thread of a chunk, the block
  fold, the per-lane share of the tensor's partials, the butterfly); a norm has half that error
  plus its square root's rounding, a ratio two norms and a few more roundings.  For the layouts
  here that is below 3e-6; the rest of 1e-5 covers the fp32 inputs of the sums (weights and u after
  earlier steps, a few units of 2^-24 each and not systematic).
* weights, atol 1e-5: the project's bound for fused Adam against torch at these magnitudes.  The
  same reference run in fp32 against fp64 on the CPU deviates by at most 3.2e-7 (LAMB) and 4.1e-7
  (LARS) on this layout (profiles/r9/layerwise_optim.md); four times that is below 1e-5, so 1e-5
  stands.
* moments: every step adds at most five roundings relative to the largest term, so 16 * 2^-24 of
  the largest |g'| (or g'^2) over three steps; LARS's momentum buffer is linear in d = r * (...)
  with coefficients summing to at most 2.71, and d carries the ratio's relative error.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

EPS24 = 2.0 ** -24
RATIO_RTOL = 1e-5
W_ATOL = 1e-5


# ---- the fp64 reference -------------------------------------------------------------------------

def _ref_ratio(adapt, wn, other, value):
    if not adapt:
        return 1.0
    if math.isnan(wn) or math.isnan(other):
        return float("nan")          # a NaN norm reaches the weights; it is never clamped to 1
    return value() if wn > 0 and other > 0 else 1.0


class Ref:
    """LAMB / LARS per tensor.  rows: one (lr, weight_decay, adapt) per tensor."""

    def __init__(self, kind, ws, rows, dtype=torch.float64, **hp):
        self.kind, self.rows, self.hp, self.dtype = kind, rows, hp, dtype
        self.w = [w.detach().to("cpu", dtype).clone() for w in ws]
        self.m = [torch.zeros_like(w) for w in self.w]      # LAMB exp_avg / LARS momentum buffer
        self.v = [torch.zeros_like(w) for w in self.w]
        self.t, self.first = 0, True
        self.ratios = [1.0] * len(self.w)
        self.dmax = 0.0           # largest |d| LARS fed its momentum buffer
        self.gmax = 0.0           # largest |g'|

    def reset_state(self):
        for t in self.m + self.v:
            t.zero_()
        self.t, self.first = 0, True

    def step(self, grads, grad_scale=1.0, clip=1.0):
        self.t += 1
        h = self.hp
        for i, (w, g) in enumerate(zip(self.w, grads)):
            lr, wd, adapt = self.rows[i]
            gp = g.detach().to("cpu", self.dtype) * (grad_scale * clip)
            if gp.numel() and bool(torch.isfinite(gp).all()):
                self.gmax = max(self.gmax, float(gp.abs().max()))
            wn = float(torch.linalg.vector_norm(w))
            if self.kind == "lamb":
                b1, b2 = h["betas"]
                self.m[i] = b1 * self.m[i] + (1 - b1) * gp
                self.v[i] = b2 * self.v[i] + (1 - b2) * gp * gp
                u = (self.m[i] / (1 - b1 ** self.t)) / ((self.v[i] / (1 - b2 ** self.t)).sqrt() + h["eps"]) + wd * w
                un = float(torch.linalg.vector_norm(u))
                r = _ref_ratio(adapt, wn, un, lambda: wn / un)
                self.w[i] = w - lr * r * u
            else:
                gn = float(torch.linalg.vector_norm(gp))
                r = _ref_ratio(adapt, wn, gn, lambda: h["trust_coefficient"] * wn / (gn + wd * wn + h["eps"]))
                d = r * (gp + wd * w)
                if d.numel() and bool(torch.isfinite(d).all()):
                    self.dmax = max(self.dmax, float(d.abs().max()))
                if h["momentum"]:
                    self.m[i] = d.clone() if self.first else h["momentum"] * self.m[i] + (1 - h["dampening"]) * d
                    d = d + h["momentum"] * self.m[i] if h["nesterov"] else self.m[i]
                self.w[i] = w - lr * d
            self.ratios[i] = r
        self.first = False


LAMB_HP = dict(betas=(0.9, 0.999), eps=1e-6)
LARS_HP = dict(momentum=0.9, dampening=0.0, nesterov=False, trust_coefficient=0.02, eps=1e-8)


# ---- the kernel-test layout ----------------------------------------------------------------------

def _layout():
    """(sizes, index of the all-zero tensor, index of the tensor with an all-zero gradient): padding
    (1, 65), a chunk edge (LAYER_CHUNK, + 64), a tensor of several chunks, more chunks than blocks at
    max_blocks=1, and both r = 1 guards."""
    from kubeml_amd.ops.kernels import LAYER_CHUNK as LC
    return [1, 64, 65, LC, LC + 64, 5 * LC + 192, 100, 130], 6, 7


def _rows(kind, n, adapt=None):
    """Per-tensor (lr, weight_decay, adapt): lr and decay differ from tensor to tensor, adapt is off
    on tensors 1 and 2 unless given."""
    lr0 = 1e-2 if kind == "lamb" else 0.1
    rows = []
    for i in range(n):
        a = (i not in (1, 2)) if adapt is None else adapt
        rows.append((lr0 * (1 + 0.25 * (i % 3)), 0.0 if i % 4 == 3 else 0.01 * (1 + i % 2), a))
    return rows


def _values(seed=0, steps=3):
    sizes, zero_w, zero_g = _layout()
    gen = torch.Generator().manual_seed(seed)
    ws = [torch.randn(n, generator=gen) for n in sizes]
    ws[zero_w].zero_()
    grads = []
    for k in range(steps):
        gs = [torch.randn(n, generator=gen) * (0.5 + k) for n in sizes]
        gs[zero_g].zero_()
        grads.append(gs)
    return ws, grads


def _space(ws):
    from kubeml_amd.nn.flat import FlatParamSpace
    return FlatParamSpace([torch.nn.Parameter(w.clone().to(dev)) for w in ws], device=dev, reverse=False)


def _run(kind, ws, grads, rows, hp, max_blocks=0, grad_scale=0.5):
    """The launchers, step by step, on a FlatParamSpace of ``ws``; everything the steps wrote."""
    from kubeml_amd.ops import kernels as K
    sp = _space(ws)
    chunks, ranges = K.layer_tables(sp.offsets, sp.numel, dev)
    table = torch.tensor([[lr, wd, float(a), 0.0] for lr, wd, a in rows], device=dev)
    part = torch.zeros(2 * chunks.shape[0], device=dev)
    ratio = torch.full((len(rows),), -7.0, device=dev)
    m = torch.zeros(sp.numel, device=dev)
    v = torch.zeros(sp.numel, device=dev)
    for k, gs in enumerate(grads):
        sp.grad.zero_()
        for p, g in zip(sp.params, gs):
            p.grad.copy_(g)
        if kind == "lamb":
            b1, b2 = hp["betas"]
            K.lamb_moments_(sp.master, sp.grad, m, v, chunks, ranges, table, part, ratio, k + 1, b1, b2, hp["eps"],
                            grad_scale=grad_scale, max_blocks=max_blocks)
            K.lamb_apply_(sp.master, m, v, sp.shadow, chunks, table, ratio, k + 1, b1, b2, hp["eps"],
                          max_blocks=max_blocks)
        else:
            K.lars_norms_(sp.master, sp.grad, chunks, ranges, table, part, ratio,
                          trust_coefficient=hp["trust_coefficient"], eps=hp["eps"], grad_scale=grad_scale,
                          max_blocks=max_blocks)
            K.lars_apply_(sp.master, sp.grad, m if hp["momentum"] else None, sp.shadow, chunks, table, ratio,
                          momentum=hp["momentum"], dampening=hp["dampening"], nesterov=hp["nesterov"], first=(k == 0),
                          grad_scale=grad_scale, max_blocks=max_blocks)
    torch.cuda.synchronize()
    return dict(sp=sp, master=sp.master.clone(), shadow=sp.shadow.clone(), m=m, v=v, ratio=ratio.clone())


def _tensor(out, buf, i):
    o, n = out["sp"].offsets[i]
    return out[buf][o:o + n]


def _padding_mask(sp):
    mask = torch.ones(sp.numel, dtype=torch.bool, device=dev)
    for o, n in sp.offsets:
        mask[o:o + n] = False
    return mask


def _sumsq_bound(chunks_of_tensor):
    """Worst-case relative error of one tensor's fp32 sum of squares: LAYER_CHUNK / 256 terms per
    thread of a chunk, the block fold (wave 6, LDS 2), a lane's share of the tensor's partials, the
    butterfly 6."""
    from kubeml_amd.ops.kernels import LAYER_CHUNK
    return (LAYER_CHUNK // 256 + 8 + -(-chunks_of_tensor // 64) + 6) * EPS24


CASES = [("lamb", LAMB_HP), ("lars", LARS_HP), ("lars", dict(LARS_HP, nesterov=True, dampening=0.1))]
IDS = ["lamb", "lars", "lars_nesterov"]


@pytest.fixture(scope="module")
def runs():
    """Reference and default-grid kernel run of every case, computed once and left unchanged."""
    ws, grads = _values()
    out = {}
    for name, (kind, hp) in zip(IDS, CASES):
        rows = _rows(kind, len(ws))
        ref = Ref(kind, ws, rows, **hp)
        for gs in grads:
            ref.step(gs, grad_scale=0.5)
        out[name] = (kind, hp, rows, ref, _run(kind, ws, grads, rows, hp))
    return ws, grads, out


@pytest.mark.parametrize("name", IDS)
def test_three_steps_match_the_fp64_reference(runs, name):
    ws, grads, out = runs
    kind, hp, rows, ref, got = out[name]
    # both guards were exercised, and so was adaptation
    _, zero_w, zero_g = _layout()
    assert any(r != 1.0 for r in ref.ratios) and ref.ratios[2] == 1.0 and ref.ratios[zero_g] == 1.0
    # the ratio's error bound for the longest tensor of the layout (6 chunks) fits the tolerance
    ratio_bound = 2 * (_sumsq_bound(6) / 2 + EPS24) + 4 * EPS24
    print(name, "ratio bound", ratio_bound)
    assert ratio_bound <= RATIO_RTOL
    ratios = got["ratio"].double().cpu()
    want = torch.tensor(ref.ratios, dtype=torch.float64)
    print(name, "ratio rel", float(((ratios - want).abs() / want).max()))
    assert torch.allclose(ratios, want, rtol=RATIO_RTOL, atol=0)
    for i in range(len(ws)):
        w = _tensor(got, "master", i).double().cpu()
        print(name, i, "weights max dev", float((w - ref.w[i]).abs().max()))
        assert torch.allclose(w, ref.w[i], rtol=0, atol=W_ATOL), (name, i)
        m = _tensor(got, "m", i).double().cpu()
        if kind == "lamb":
            v = _tensor(got, "v", i).double().cpu()
            assert torch.allclose(m, ref.m[i], rtol=0, atol=16 * EPS24 * ref.gmax), (name, i)
            assert torch.allclose(v, ref.v[i], rtol=0, atol=16 * EPS24 * ref.gmax ** 2), (name, i)
        else:
            assert torch.allclose(m, ref.m[i], rtol=0, atol=3 * (RATIO_RTOL + 8 * EPS24) * ref.dmax), (name, i)
    assert float((got["master"] - _run_initial(ws)).abs().max()) > 1e-3
    assert torch.equal(got["shadow"], got["master"].to(torch.bfloat16))


def _run_initial(ws):
    return _space(ws).master.clone()


@pytest.mark.parametrize("name", IDS)
def test_padding_stays_zero(runs, name):
    got = runs[2][name][4]
    pad = _padding_mask(got["sp"])
    assert int(pad.sum()) > 0
    for buf in ("master", "m", "v", "shadow"):
        assert not bool(got[buf][pad].ne(0).any()), buf


@pytest.mark.parametrize("name", IDS)
def test_bits_do_not_depend_on_the_grid(runs, name):
    from kubeml_amd.ops import kernels as K
    ws, grads, out = runs
    kind, hp, rows, _, got = out[name]
    for max_blocks in (0, 1, 3):
        again = _run(kind, ws, grads, rows, hp, max_blocks=max_blocks)
        for buf in ("master", "m", "v", "shadow", "ratio"):
            assert torch.equal(again[buf], got[buf]), (max_blocks, buf)
    assert not bool(K._COUNTERS.bufs[got["master"].device].any())     # the ticket counter is back at 0


@pytest.mark.parametrize("name", IDS)
def test_no_leak_across_tensors(runs, name):
    """Other values in ONE tensor (weights and gradients): every other tensor's weights, state and
    ratio keep their bits."""
    ws, grads, out = runs
    kind, hp, rows, _, got = out[name]
    changed = 4                                 # LAYER_CHUNK + 64: two chunks, neighbours on both sides
    ws2 = [w.clone() for w in ws]
    ws2[changed] = ws2[changed] * 1.5 + 0.25
    grads2 = [[g.clone() for g in gs] for gs in grads]
    for gs in grads2:
        gs[changed] = gs[changed] * -2.0
    other = _run(kind, ws2, grads2, rows, hp)
    for i in range(len(ws)):
        same = [torch.equal(_tensor(other, b, i), _tensor(got, b, i)) for b in ("master", "m", "v", "shadow")]
        same.append(bool(other["ratio"][i] == got["ratio"][i]))
        assert all(same) == (i != changed), (i, same)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("name", IDS[:2])
def test_non_finite_gradient_poisons_its_tensor_only(runs, name, bad):
    ws, grads, out = runs
    kind, hp, rows, _, got = out[name]
    hit = 3                                     # one chunk of LAYER_CHUNK elements, adapt on
    assert rows[hit][2]
    grads2 = [[g.clone() for g in gs] for gs in grads[:1]]
    grads2[0][hit][1234] = bad
    clean = _run(kind, ws, grads[:1], rows, hp)
    dirty = _run(kind, ws, grads2, rows, hp)
    ref = Ref(kind, ws, rows, **hp)
    ref.step(grads2[0], grad_scale=0.5)
    for i in range(len(ws)):
        w = _tensor(dirty, "master", i)
        if i != hit:
            assert torch.equal(w, _tensor(clean, "master", i)) and torch.equal(_tensor(dirty, "m", i),
                                                                               _tensor(clean, "m", i)), i
            continue
        assert math.isnan(ref.ratios[i]) or bad == float("inf")
        assert not bool(torch.isfinite(w).all())
        assert torch.allclose(w.double().cpu(), ref.w[i], rtol=0, atol=W_ATOL, equal_nan=True)
        if math.isnan(ref.ratios[i]):           # a NaN norm: the whole tensor, not one element
            assert bool(torch.isnan(w).all()) and math.isnan(float(dirty["ratio"][i]))


@pytest.mark.parametrize("name", IDS[:2])
def test_a_tensor_whose_fold_takes_several_rounds(name):
    """300 chunks and a 64-element tail in one tensor: a lane of the folding wave adds five
    partials, in two rounds of loads (256 partials per round), between two small neighbours."""
    from kubeml_amd.ops.kernels import LAYER_CHUNK as LC
    kind, hp = CASES[IDS.index(name)]
    gen = torch.Generator().manual_seed(7)
    sizes = [70, 300 * LC + 64, 3 * LC]
    ws = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) for n in sizes]]
    rows = _rows(kind, 3, adapt=True)
    ref = Ref(kind, ws, rows, **hp)
    ref.step(grads[0], grad_scale=0.5)
    got = _run(kind, ws, grads, rows, hp)
    assert 2 * (_sumsq_bound(301) / 2 + EPS24) + 4 * EPS24 <= RATIO_RTOL
    want = torch.tensor(ref.ratios, dtype=torch.float64)
    ratios = got["ratio"].double().cpu()
    print(name, "ratio rel", float(((ratios - want).abs() / want).max()))
    assert torch.allclose(ratios, want, rtol=RATIO_RTOL, atol=0)
    for i in range(3):
        assert torch.allclose(_tensor(got, "master", i).double().cpu(), ref.w[i], rtol=0, atol=W_ATOL), i
    one = _run(kind, ws, grads, rows, hp, max_blocks=1)
    assert torch.equal(one["master"], got["master"]) and torch.equal(one["ratio"], got["ratio"])


def _opt(kind, params, hp, **kw):
    from kubeml_amd.optim import LAMB, LARS
    return LAMB(params, **hp, **kw) if kind == "lamb" else LARS(params, **hp, **kw)


@pytest.mark.parametrize("name", IDS[:2])
def test_clipping_equals_clip_then_step(runs, name):
    """Optimizer classes with max_grad_norm on the kernel layout (two groups, adapt on / off): the
    reference fed torch's clip coefficient of the fp64 global norm."""
    ws, grads, out = runs
    kind, hp = out[name][0], out[name][1]
    sp = _space(ws)
    half = len(ws) // 2
    lr = 1e-2 if kind == "lamb" else 0.1
    groups = [dict(params=sp.params[:half], weight_decay=0.01, adapt=True),
              dict(params=sp.params[half:], weight_decay=0.0, adapt=False, lr=lr / 2)]
    THR = 100.0      # the norm grows with the step: about 64, 192, 321
    opt = _opt(kind, groups, hp, lr=lr, max_grad_norm=THR)
    opt.set_grad_scale(0.5)
    rows = [(lr, 0.01, True)] * half + [(lr / 2, 0.0, False)] * (len(ws) - half)
    ref = Ref(kind, ws, rows, **hp)
    clipped = 0
    for gs in grads:
        sp.grad.zero_()
        for p, g in zip(sp.params, gs):
            p.grad.copy_(g)
        nrm = 0.5 * math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        coef = min(1.0, THR / (nrm + 1e-6))
        clipped += coef < 1.0
        ref.step(gs, grad_scale=0.5, clip=coef)
        opt.step()
        assert abs(float(opt.grad_norm_tensor()) - nrm) <= 1e-5 * nrm
    assert 0 < clipped < len(grads), "the threshold must clip some steps and not others"
    ratios = opt.trust_ratios().double().cpu()
    assert torch.allclose(ratios, torch.tensor(ref.ratios, dtype=torch.float64), rtol=RATIO_RTOL, atol=0)
    for i, p in enumerate(sp.params):
        assert torch.allclose(p.detach().double().cpu(), ref.w[i], rtol=0, atol=W_ATOL), i
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def test_launchers_reject_bad_arguments():
    from kubeml_amd.ops import kernels as K
    n, C, T = 256, 2, 2
    f = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    w, g, m, v, sh = f(n), f(n), f(n), f(n), f(n, dt=torch.bfloat16)
    chunks = torch.tensor([[0, 128, 0], [128, 128, 1]], dtype=torch.int32, device=dev)
    ranges = torch.tensor([[0, 1], [1, 1]], dtype=torch.int32, device=dev)
    hp, part, ratio = f(T, 4), f(2 * C), f(T)

    def moments(**kw):
        a = dict(w=w, g=g, m=m, v=v, chunks=chunks, ranges=ranges, hp=hp, part=part, ratio=ratio)
        a.update(kw)
        K.lamb_moments_(a["w"], a["g"], a["m"], a["v"], a["chunks"], a["ranges"], a["hp"], a["part"], a["ratio"], 1)

    def norms(**kw):
        a = dict(w=w, g=g, chunks=chunks, ranges=ranges, hp=hp, part=part, ratio=ratio)
        a.update(kw)
        K.lars_norms_(a["w"], a["g"], a["chunks"], a["ranges"], a["hp"], a["part"], a["ratio"])

    moments()
    norms()
    K.lamb_apply_(w, m, v, sh, chunks, hp, ratio, 1)
    K.lars_apply_(w, g, m, sh, chunks, hp, ratio)
    big = f(n + 64)
    bad = [dict(g=big[1:1 + n]),                              # misaligned buffer
           dict(w=f(n + 32), g=f(n + 32), m=f(n + 32), v=f(n + 32)),     # n % 64 != 0
           dict(g=f(n, dt=torch.float64)),                    # wrong dtype
           dict(g=torch.zeros(n)),                            # wrong device
           dict(chunks=chunks.to(torch.int64)),
           dict(chunks=f(C, 3)),
           dict(chunks=torch.zeros(C, 4, dtype=torch.int32, device=dev)),         # table shapes
           dict(hp=f(T, 2)),
           dict(ranges=ranges[:1]),
           dict(ratio=f(T + 1)),
           dict(part=f(C))]
    for kw in bad:
        with pytest.raises(ValueError):
            moments(**kw)
        with pytest.raises(ValueError):
            norms(**{k: t for k, t in kw.items() if k not in ("m", "v")})
    for kw in (dict(shadow=f(n + 8, dt=torch.bfloat16)[1:n + 1]), dict(shadow=f(n)), dict(hp=f(T, 2)),
               dict(chunks=f(C, 3)), dict(ratio=f(T + 1))):
        a = dict(shadow=sh, chunks=chunks, hp=hp, ratio=ratio)
        a.update(kw)
        with pytest.raises(ValueError):
            K.lamb_apply_(w, m, v, a["shadow"], a["chunks"], a["hp"], a["ratio"], 1)
        with pytest.raises(ValueError):
            K.lars_apply_(w, g, m, a["shadow"], a["chunks"], a["hp"], a["ratio"])
    with pytest.raises(ValueError):
        K.lars_apply_(w, g, None, sh, chunks, hp, ratio, momentum=0.9)
    torch.cuda.synchronize()
    assert not bool(w.ne(0).any())


# ---- whole models ------------------------------------------------------------------------------

def _lenet():
    from kubeml_amd.models.lenet import LeNet
    from kubeml_amd.nn import cross_entropy, flatten_module
    torch.manual_seed(0)
    m = LeNet().to(dev)
    sp = flatten_module(m)
    m.train()
    g = torch.Generator().manual_seed(1)
    x = (4 * torch.randn(32, 1, 28, 28, generator=g)).to(dev)
    y = torch.randint(0, 10, (32,), generator=g).to(dev)
    return m, sp, lambda: cross_entropy(m(x), y)


def _bert():
    from kubeml_amd.models.bert import bert_tiny_mlm
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    V = 1003                       # not a multiple of 8: the decoder's padded rows / columns
    m = bert_tiny_mlm(vocab=V, dropout=0.0).to(dev)     # 2 layers, hidden 128
    sp = flatten_module(m)
    m.train()
    g = torch.Generator().manual_seed(3)
    B, L, P = 2, 128, 20
    ids = torch.randint(0, V, (B, L), generator=g).to(dev)
    tt = torch.randint(0, 2, (B, L), generator=g).to(dev)
    pos = torch.stack([torch.randperm(L, generator=g)[:P].sort().values for _ in range(B)]).to(dev)
    lab = torch.randint(0, V, (B, P), generator=g).to(dev)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[0, L - 5:] = 0
    mask = mask.to(dev)
    return m, sp, lambda: m(ids, tt, mask, pos, lab)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
@pytest.mark.parametrize("make", [_lenet, _bert], ids=["lenet", "bert_2layer"])
def test_optimizer_classes_on_models(make, kind):
    """One backward, two steps, against the reference applied per named parameter; layerwise_groups
    turns adaptation off on every bias and norm weight."""
    from kubeml_amd.optim import layerwise_groups
    m, sp, loss = make()
    hp = LAMB_HP if kind == "lamb" else LARS_HP
    lr = 1e-2 if kind == "lamb" else 0.1
    opt = _opt(kind, layerwise_groups(m, 0.01), hp, lr=lr)
    sp.zero_grad()
    loss().backward()
    sp.finish_grads()
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    seen, uniq = set(), []
    for n, p in named:                     # tied weights appear once
        if id(p) not in seen:
            seen.add(id(p))
            uniq.append((n, p))
    grads = [p.grad.detach().clone() for _, p in uniq]
    rows = [(lr, 0.01 if p.ndim > 1 else 0.0, p.ndim > 1) for _, p in uniq]
    ref = Ref(kind, [p for _, p in uniq], rows, **hp)
    w0 = sp.master.clone()
    for _ in range(2):
        ref.step(grads)
        opt.step()
    torch.cuda.synchronize()
    assert float((sp.master - w0).abs().max()) > 1e-4
    ratios = opt.trust_ratios().double().cpu()
    index = {id(p): i for i, p in enumerate(sp.params)}
    adapted = 0
    for k, (n, p) in enumerate(uniq):
        r = float(ratios[index[id(p)]])
        if p.ndim <= 1:
            assert r == 1.0, n
        else:
            adapted += ref.ratios[k] != 1.0
            assert abs(r - ref.ratios[k]) <= RATIO_RTOL * abs(ref.ratios[k]), (n, r, ref.ratios[k])
        dev_ = float((p.detach().double().cpu() - ref.w[k]).abs().max())
        assert dev_ <= W_ATOL, (n, dev_)
    assert adapted > 0
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def _r18_lars():
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import LARS, layerwise_groups
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    opt = LARS(layerwise_groups(m, 1e-4), lr=0.5, momentum=0.9, trust_coefficient=0.02)
    g = torch.Generator(device=dev).manual_seed(11)
    xs = torch.randn(5, 8, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (5, 8), device=dev, generator=g)
    return m, sp, opt, xs, ys


def _between(opt, k):
    if k == 3:
        opt.set_lr(0.25)          # no re-capture: the next replay reads the per-tensor table
    if k == 4:
        opt.reset_state()         # ... and the first-step flag and the zeroed momentum


def test_graphed_lars_step_equals_eager_and_follows_set_lr_and_reset():
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn import backward_loss, cross_entropy
    m, sp, opt, xs, ys = _r18_lars()
    eager, eratio = [], []
    for k in range(5):
        _between(opt, k)
        sp.zero_grad()
        backward_loss(cross_entropy(m(xs[k]), ys[k]))
        opt.step()
        eager.append(sp.master.clone())
        eratio.append(opt.trust_ratios().clone())
    assert not torch.equal(eager[0], eager[1]) and bool((eratio[0] != 1.0).any())
    m, sp, opt, xs, ys = _r18_lars()
    x, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    i = torch.zeros((), dtype=torch.int64, device=dev)

    def pre():
        x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
        y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

    def post():
        i.add_(1)
    w0 = sp.master.clone()
    step = make_train_step(m, sp, opt, cross_entropy, x, y, pre=pre, post=post, extra_state=[i])
    assert step.ride_plan is None
    step.capture()
    torch.cuda.synchronize()
    assert step.captured and torch.equal(sp.master, w0) and int(i) == 0
    for k in range(5):
        _between(opt, k)
        step()
        torch.cuda.synchronize()
        assert torch.equal(sp.master, eager[k]), (k, float((sp.master - eager[k]).abs().max()))
        assert torch.equal(opt.trust_ratios(), eratio[k]), k
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def test_kubemodel_step_captures_lamb_and_keeps_it_across_an_lr_change():
    """KubeModel.step with LAMB runs as one captured graph; a ``_config_optimizer`` call whose fresh
    optimizer differs in the LR only keeps the resident one (its moments, its graph) and retunes
    it: the third step equals, bit for bit, the one after a direct ``set_lr``, and differs from the
    one at the old LR."""
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import LAMB, layerwise_groups
    from kubeml_amd.sdk.model import KubeModel

    class M(KubeModel):
        def configure_optimizers(self):
            return LAMB(layerwise_groups(self._network, 0.01), lr=self.lr)

    g = torch.Generator(device=dev).manual_seed(11)
    xs = torch.randn(3, 8, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (3, 8), device=dev, generator=g)

    def run(how):
        torch.manual_seed(0)
        net = resnet18(10).to(dev)
        k = M(net, None, gpu=True)
        k.device = torch.device("cuda", 0)
        k._flat = flatten_module(net)
        k.lr = 2e-3
        k._config_optimizer()
        opt = k.optimizer
        assert type(opt) is LAMB
        for i in range(2):
            k.step(xs[i], ys[i])
        assert len(k._graphs) == 1
        st = next(iter(k._graphs.values()))["step"]
        assert st.captured and st.use_graph
        if how == "config":
            k.lr = 1e-3
            k._config_optimizer()
            assert k.optimizer is opt and [gr["lr"] for gr in opt.param_groups] == [1e-3, 1e-3]
        elif how == "set_lr":
            opt.set_lr(1e-3)
        assert len(k._graphs) == 1 and next(iter(k._graphs.values()))["step"] is st
        k.step(xs[2], ys[2])
        torch.cuda.synchronize()
        assert float(opt.step_tensor(k.device)) == 3.0       # the moments carried on: step 3, not 1
        assert bool(torch.isfinite(opt.trust_ratios()).all())
        return k._flat.master.clone()
    kept, direct, old_lr = run("config"), run("set_lr"), run("none")
    assert torch.equal(kept, direct)
    assert not torch.equal(kept, old_lr)
