"""LAMB / LARS without a GPU: the chunk table of the layer-wise launches (a pure-Python function),
the per-tensor torch paths against an fp64 reference written here, group validation, reset_state,
the shard fall-back and the unchanged ``from_torch``."""
import math

import pytest
import torch


# ---- chunk table ---------------------------------------------------------------------------------

def _offsets(module):
    """The offsets FlatParamSpace would give ``module``'s parameters (reverse registration order,
    storage shapes, 64-aligned regions), without allocating its buffers."""
    from kubeml_amd.nn.flat import ALIGN, _storage_spec
    seen, uniq = set(), []
    for p in module.parameters():
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            uniq.append(p)
    offsets, off = [], 0
    for p in reversed(uniq):
        n = math.prod(_storage_spec(p)[0])
        offsets.append((off, n))
        off += -(-n // ALIGN) * ALIGN
    return offsets, max(off, ALIGN)


def _resnet34():
    from kubeml_amd.models.resnet import resnet34
    return resnet34(1000)


def _bert_base():
    from kubeml_amd.models.bert import bert_base_mlm
    return bert_base_mlm()


def _on_meta(make):
    try:
        with torch.device("meta"):
            return make()
    except Exception:                     # a constructor that needs real values: build it on the CPU
        return make()


@pytest.mark.parametrize("make", [_resnet34, _bert_base], ids=["resnet34", "bert_base"])
def test_chunk_table_properties(make):
    from kubeml_amd.ops.kernels import LAYER_CHUNK, layer_chunks
    offsets, numel = _offsets(_on_meta(make))
    assert len(offsets) > 100 and numel > 20e6
    chunks, ranges = layer_chunks(offsets, numel)
    assert len(ranges) == len(offsets)
    pos = 0                                    # chunks walk the space in order ...
    for t, ((o, n), (first, cnt)) in enumerate(zip(offsets, ranges)):
        padded = -(-n // 64) * 64
        assert pos == o                        # ... so every region is covered exactly once
        own = chunks[first:first + cnt]        # a tensor's chunks are consecutive
        assert cnt == -(-padded // LAYER_CHUNK)
        for s, ln, tid in own:
            assert tid == t and s == pos and ln % 64 == 0 and 0 < ln <= LAYER_CHUNK
            assert o <= s and s + ln <= o + padded          # inside its tensor
            pos += ln
        assert pos == o + padded
    assert pos == numel and sum(c for _, c in ranges) == len(chunks)
    assert [f for f, _ in ranges] == [sum(c for _, c in ranges[:t]) for t in range(len(ranges))]
    assert max(c for _, c in ranges) > 64      # a tensor whose fold takes several partials per lane


def test_chunk_table_rejects_bad_layouts():
    from kubeml_amd.ops.kernels import layer_chunks
    assert layer_chunks([(0, 1), (64, 65)], 192) == ([(0, 64, 0), (64, 128, 1)], [(0, 1), (1, 1)])
    assert layer_chunks([(0, 0)], 64) == ([], [(0, 0)])
    for offsets, numel in (([(0, 10), (32, 10)], 128), ([(0, 100), (64, 10)], 192), ([(0, 100)], 64),
                           ([(0, 64)], 100), ([(0, 64)], 2 ** 31)):
        with pytest.raises(ValueError):
            layer_chunks(offsets, numel)


# ---- CPU paths against the fp64 reference ------------------------------------------------------------

def _ratio(adapt, wn, other, value):
    if not adapt:
        return 1.0
    if math.isnan(wn) or math.isnan(other):
        return float("nan")
    return value() if wn > 0 and other > 0 else 1.0


def _ref_steps(kind, ws, grads_per_step, rows, hp, grad_scale=1.0):
    """fp64, per tensor, the formulas of the issue; returns (weights, ratios of the last step)."""
    w = [x.detach().double().clone() for x in ws]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    ratios = [1.0] * len(w)
    for t, grads in enumerate(grads_per_step, 1):
        for i, g in enumerate(grads):
            lr, wd, adapt = rows[i]
            gp = g.double() * grad_scale
            wn = float(w[i].norm())
            if kind == "lamb":
                b1, b2 = hp["betas"]
                m[i] = b1 * m[i] + (1 - b1) * gp
                v[i] = b2 * v[i] + (1 - b2) * gp * gp
                u = (m[i] / (1 - b1 ** t)) / ((v[i] / (1 - b2 ** t)).sqrt() + hp["eps"]) + wd * w[i]
                un = float(u.norm())
                r = _ratio(adapt, wn, un, lambda: wn / un)
                w[i] = w[i] - lr * r * u
            else:
                gn = float(gp.norm())
                r = _ratio(adapt, wn, gn, lambda: hp["trust_coefficient"] * wn / (gn + wd * wn + hp["eps"]))
                d = r * (gp + wd * w[i])
                if hp["momentum"]:
                    m[i] = d.clone() if t == 1 else hp["momentum"] * m[i] + (1 - hp["dampening"]) * d
                    d = d + hp["momentum"] * m[i] if hp["nesterov"] else m[i]
                w[i] = w[i] - lr * d
            ratios[i] = r
    return w, ratios


HP = {"lamb": dict(betas=(0.9, 0.999), eps=1e-6),
      "lars": dict(momentum=0.9, dampening=0.1, nesterov=True, trust_coefficient=0.02, eps=1e-8)}


def _params():
    gen = torch.Generator().manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in ((7, 5), (5,), (3, 4, 2), (1,), (6,))]
    with torch.no_grad():
        ps[4].zero_()                           # |w| = 0: ratio 1
    grads = [[torch.randn(p.shape, generator=gen) * (1 + k) for p in ps] for k in range(3)]
    for gs in grads:
        gs[3].zero_()                           # |g| = 0
    return ps, grads


@pytest.mark.parametrize("grouped", [False, True], ids=["one_group", "groups"])
@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_cpu_path_matches_fp64_reference(kind, grouped):
    from kubeml_amd.optim import LAMB, LARS
    ps, grads = _params()
    lr = 1e-2 if kind == "lamb" else 0.1
    if grouped:
        groups = [dict(params=[ps[0], ps[2]], weight_decay=0.01),
                  dict(params=[ps[1], ps[3], ps[4]], weight_decay=0.0, adapt=False, lr=lr / 4)]
        rows = [(lr, 0.01, True), (lr / 4, 0.0, False), (lr, 0.01, True), (lr / 4, 0.0, False), (lr / 4, 0.0, False)]
    else:
        groups = ps
        rows = [(lr, 0.01, True)] * len(ps)
    cls = LAMB if kind == "lamb" else LARS
    opt = cls(groups, lr=lr, weight_decay=0.01, **HP[kind])
    opt.set_grad_scale(0.5)
    want, ratios = _ref_steps(kind, ps, grads, rows, HP[kind], grad_scale=0.5)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    for i, p in enumerate(ps):
        # fp32 torch ops against fp64: a few roundings of values up to ~4 per step
        assert torch.allclose(p.detach().double(), want[i], rtol=0, atol=1e-5), i
    got = dict(zip([id(p) for g in opt.param_groups for p in g["params"]], opt.trust_ratios().tolist()))
    for i, p in enumerate(ps):
        assert abs(got[id(p)] - ratios[i]) <= 1e-5 * abs(ratios[i]), (i, got[id(p)], ratios[i])
    if not grouped:
        assert ratios[3] == 1.0 or kind == "lamb"      # LARS: |g| = 0
        assert any(r != 1.0 for r in ratios)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_cpu_flat_space_takes_the_torch_path(kind):
    """Parameters in a CPU FlatParamSpace (views of one buffer) step like loose ones."""
    from kubeml_amd.nn.flat import FlatParamSpace
    from kubeml_amd.optim import LAMB, LARS
    ps, grads = _params()
    w0 = [p.detach().clone() for p in ps]
    sp = FlatParamSpace(ps, device="cpu")
    lr = 1e-2 if kind == "lamb" else 0.1
    opt = (LAMB if kind == "lamb" else LARS)(ps, lr=lr, weight_decay=0.01, **HP[kind])
    want, _ = _ref_steps(kind, w0, grads[:2], [(lr, 0.01, True)] * len(ps), HP[kind])
    for gs in grads[:2]:
        sp.zero_grad()
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        opt.step()
    for i, p in enumerate(ps):
        assert torch.allclose(p.detach().double(), want[i], rtol=0, atol=1e-5), i


def test_nan_norm_is_not_clamped_on_the_cpu_path():
    from kubeml_amd.optim import LAMB, LARS
    for cls, kw in ((LAMB, dict(lr=1e-2)), (LARS, dict(lr=0.1))):
        a, b = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
        opt = cls([a, b], **kw)
        a.grad = torch.tensor([1.0, float("nan"), 1.0, 1.0])
        b.grad = torch.ones(4)
        opt.step()
        r = opt.trust_ratios()
        assert math.isnan(float(r[0])) and bool(torch.isnan(a).all())
        assert math.isfinite(float(r[1])) and bool(torch.isfinite(b).all())


# ---- groups, state, plans ---------------------------------------------------------------------------

def test_group_validation():
    from kubeml_amd.optim import LAMB, LARS, layerwise_groups
    a, b = torch.nn.Parameter(torch.ones(3, 3)), torch.nn.Parameter(torch.ones(3))
    opt = LAMB([dict(params=[a]), dict(params=[b], adapt=False, weight_decay=0.0, lr=1e-4)], lr=1e-3)
    assert opt.grouped and [g["adapt"] for g in opt.param_groups] == [True, False]
    with pytest.raises(ValueError, match="betas"):
        LAMB([dict(params=[a]), dict(params=[b], betas=(0.8, 0.999))], lr=1e-3)
    with pytest.raises(ValueError, match="momentum"):
        LARS([dict(params=[a]), dict(params=[b], momentum=0.5)], lr=0.1)
    with pytest.raises(ValueError, match="trust_coefficient"):
        LARS([dict(params=[a]), dict(params=[b], trust_coefficient=0.5)], lr=0.1)
    with pytest.raises(ValueError):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.ones(2))], eps=1e-3))
    # a row per tensor, not per group: more than the 8 groups of the granule-table optimizers
    many = [dict(params=[torch.nn.Parameter(torch.ones(2, 2))], lr=1e-3 * (k + 1)) for k in range(12)]
    assert len(LARS(many, lr=0.1).param_groups) == 12
    with pytest.raises(ValueError):
        LAMB([a], lr=1e-3, max_grad_norm=0.0)
    m = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    groups = layerwise_groups(m, 0.05)
    assert [(g["weight_decay"], g["adapt"], [p.ndim for p in g["params"]]) for g in groups] == \
        [(0.05, True, [2]), (0.0, False, [1, 1, 1])]
    assert LAMB.kind == "lamb" and LARS.kind == "lars"


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_reset_state_zeroes_moments_and_step(kind):
    """After reset_state() the next steps repeat, bit for bit, what a fresh optimizer does from the
    same weights (K-AVG round boundary)."""
    from kubeml_amd.optim import LAMB, LARS
    cls = LAMB if kind == "lamb" else LARS
    lr = 1e-2 if kind == "lamb" else 0.1
    ps, grads = _params()
    opt = cls(ps, lr=lr, **HP[kind])
    for gs in grads[:2]:
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
    assert len(opt.state) > 0 and (opt._step_host == 2 if kind == "lamb" else not opt._first)
    opt.reset_state()
    assert opt._step_host == 0 and len(opt.state) == 0 and opt._first
    twin = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    fresh = cls(twin, lr=lr, **HP[kind])
    for gs in grads[1:]:
        for p, q, g in zip(ps, twin, gs):
            p.grad, q.grad = g.clone(), g.clone()
        opt.step()
        fresh.step()
    for p, q in zip(ps, twin):
        assert torch.equal(p, q)


def test_no_ranged_steps_so_shard_plans_fall_back():
    from kubeml_amd.engine.dp import optimizer_can_shard
    from kubeml_amd.optim import LAMB, LARS, SGD
    ps, _ = _params()
    for opt in (LAMB(ps, lr=1e-3), LARS(ps, lr=0.1)):
        assert not opt.supports_ranges() and not opt.supports_shard_range()
        assert not optimizer_can_shard(opt)
        with pytest.raises(ValueError):
            opt.step_range(0, 64)
    from kubeml_amd.nn.flat import FlatParamSpace
    FlatParamSpace(ps, device="cpu")
    assert optimizer_can_shard(SGD(ps, lr=0.1))             # what the shard plans do take


def test_set_lr_grad_scale_and_max_grad_norm():
    from kubeml_amd.optim import LAMB, with_max_grad_norm
    ps, grads = _params()
    opt = LAMB([dict(params=ps[:2]), dict(params=ps[2:], adapt=False)], lr=1e-3, max_grad_norm=1.0)
    opt.set_lr([5e-4, 2e-4])
    assert [g["lr"] for g in opt.param_groups] == [5e-4, 2e-4]
    opt.set_max_grad_norm(0.5)
    assert opt.clips and opt.param_groups[1]["max_grad_norm"] == 0.5
    for p, g in zip(ps, grads[0]):
        p.grad = g.clone()
    opt.set_grad_scale(0.5)
    opt.step()
    nrm = 0.5 * math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[0]))
    assert abs(float(opt.grad_norm_tensor()) - nrm) <= 1e-5 * nrm
    plain = with_max_grad_norm(opt, None)
    assert type(plain) is LAMB and not plain.clips and [g["adapt"] for g in plain.param_groups] == [True, False]


def test_from_torch_is_unchanged_for_sgd_adam_adamw():
    from kubeml_amd.optim import SGD, Adam, AdamW, LAMB, from_torch
    p = [torch.nn.Parameter(torch.ones(3))]
    for topt, cls in ((torch.optim.SGD(p, lr=0.1, momentum=0.9), SGD), (torch.optim.Adam(p, lr=1e-3), Adam),
                      (torch.optim.AdamW(p, lr=1e-3), AdamW)):
        got = from_torch(topt)
        assert type(got) is cls and got.param_groups[0]["lr"] == topt.param_groups[0]["lr"]
    with pytest.raises(TypeError):
        from_torch(torch.optim.RMSprop(p, lr=0.1))
    lamb = LAMB(p, lr=1e-3)
    assert from_torch(lamb) is lamb
