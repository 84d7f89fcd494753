"""Global-norm gradient clipping on the MI355X: the one-launch deterministic norm kernel, the clip
coefficient consumed inside the fused SGD / Adam launches, the optimizers' ``max_grad_norm``, the
graph-captured step that follows a changed threshold, and the drop-in ``clip_grad_norm_``."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = "cuda"

EPS24 = 2.0 ** -24


def _terms(n, grid):
    """Squares one thread of the norm kernel accumulates for (n, grid): its float4 groups
    (grid-stride over grid * 256 threads) plus at most one element of the n % 4 tail."""
    return 4 * -(-(n >> 2) // (grid * 256)) + (1 if n % 4 else 0)


def _sumsq_bound(n, grid):
    """Worst-case relative error of the kernel's sum of squares: recursive fp32 summation of T
    non-negative terms per thread, plus the fixed folds (accumulator pairs 2, wave 6, LDS 2,
    partials 3, wave 6, LDS 2 = 21 <= 32 additions on any path)."""
    return (_terms(n, grid) + 32) * EPS24


def _norm(g, max_norm, grad_scale=1.0, max_blocks=0):
    from kubeml_amd.ops import kernels as K
    out = torch.full((3,), -7.0, device=dev)
    thr = torch.full((1,), float(max_norm), device=dev)
    K.grad_norm_(g, out, thr, grad_scale=grad_scale, max_blocks=max_blocks)
    return out


@pytest.mark.parametrize("max_blocks", [0, 1, 7])
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1025, 10007, 2 ** 20 + 5])
def test_norm_matches_fp64(n, max_blocks):
    from kubeml_amd.ops import kernels as K
    g = torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
    grid = K.grad_norm_blocks(n, max_blocks)
    assert 1 <= grid <= 1024 and (max_blocks == 0 or grid <= max_blocks)
    ss = float((g.double() ** 2).sum())
    nrm = 0.25 * math.sqrt(ss)
    bound = _sumsq_bound(n, grid)
    # the norm: half the sum's relative error (square root), one rounding each for sqrtf and the scale
    nb = bound / 2 + 2 * EPS24
    # the coefficient: the norm's error, the + 1e-6 and the division, one rounding each
    cb = nb + 2 * EPS24
    for factor in (0.5, 2.0):            # threshold below the norm (clips) and above it (does not)
        mx = float(torch.tensor(factor * nrm, dtype=torch.float32))
        out = _norm(g, mx, grad_scale=0.25, max_blocks=max_blocks).double().cpu()
        print(n, max_blocks, grid, "sumsq rel", abs(out[0].item() - ss) / ss, "bound", bound)
        assert abs(out[0].item() - ss) <= bound * ss
        assert abs(out[1].item() - nrm) <= nb * nrm
        want = min(1.0, mx / (nrm + 1e-6))
        if factor > 1:
            assert out[2].item() == 1.0
        else:
            assert abs(out[2].item() - want) <= cb * want


def test_norm_rejects_a_misaligned_buffer():
    g = torch.randn(1025, device=dev)
    with pytest.raises(ValueError):
        _norm(g[1:], 1.0)


def test_norm_is_deterministic_and_leaves_its_counter_zero():
    from kubeml_amd.ops import kernels as K
    g = torch.randn(2 ** 20 + 5, device=dev)
    first = _norm(g, 1.0).clone()
    assert bool(torch.isfinite(first).all()) and first[0] > 0
    for _ in range(19):
        assert torch.equal(_norm(g, 1.0), first)
    torch.cuda.synchronize()
    assert not bool(K._COUNTERS.bufs[g.device].any())
    # another size through the same counter / partial workspace
    h = torch.randn(10007, device=dev)
    out = _norm(h, 1.0)
    ss = float((h.double() ** 2).sum())
    assert abs(float(out[0]) - ss) <= _sumsq_bound(10007, K.grad_norm_blocks(10007)) * ss
    assert not bool(K._COUNTERS.bufs[g.device].any())


def test_non_finite_gradients_poison_or_zero_the_coefficient():
    g = torch.randn(10007, device=dev)
    g[4321] = float("inf")
    out = _norm(g, 1.0).cpu()
    assert math.isinf(out[1].item()) and out[2].item() == 0.0
    g[4321] = float("nan")
    out = _norm(g, 1.0).cpu()
    assert math.isnan(out[1].item()) and math.isnan(out[2].item())


def test_fused_updates_consume_the_coefficient():
    """sgd_ / adam_ with clip_dev against torch's clip_grad_norm_ + optimizer; gradients scaled so
    steps 0 and 2 clip (norm ~ 10) and step 1 does not (norm ~ 0.1)."""
    from kubeml_amd.ops import kernels as K
    n = 10007
    gen = torch.Generator(device=dev).manual_seed(5)
    grads = [torch.randn(n, device=dev, generator=gen) * s for s in (0.1, 0.001, 0.1)]
    out = torch.zeros(3, device=dev)
    thr = torch.ones(1, device=dev)
    w = torch.randn(n, device=dev, generator=gen)
    mom = torch.zeros(n, device=dev)
    sh = torch.empty(n, dtype=torch.bfloat16, device=dev)
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=1e-4)
    coefs = []
    for it, g in enumerate(grads):
        p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p], 1.0)
        opt.step()
        K.grad_norm_(g, out, thr)
        coefs.append(float(out[2]))
        K.sgd_(w, g, mom, sh, 0.1, wd=1e-4, momentum=0.9, first=(it == 0), clip_dev=out[2:3])
    assert coefs[0] < 0.2 and coefs[1] == 1.0 and coefs[2] < 0.2, coefs
    assert torch.allclose(w, p.data, atol=1e-5)
    assert torch.equal(sh, w.to(torch.bfloat16))
    # adamw
    w2 = torch.randn(n, device=dev, generator=gen)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    p2 = torch.nn.Parameter(w2.clone())
    opt2 = torch.optim.AdamW([p2], lr=1e-3, weight_decay=0.01)
    for it, g in enumerate(grads):
        p2.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p2], 1.0)
        opt2.step()
        K.grad_norm_(g, out, thr)
        K.adam_(w2, g, m, v, None, 1e-3, it + 1, wd=0.01, decoupled=True, clip_dev=out[2:3])
    assert torch.allclose(w2, p2.data, atol=1e-5)


def test_a_far_threshold_changes_nothing():
    """Coefficient exactly 1: weights, state and shadow equal the call without clip_dev bit for bit."""
    from kubeml_amd.ops import kernels as K
    n = 10007
    g = torch.randn(n, device=dev)
    out = _norm(g, 1e30)
    assert float(out[2]) == 1.0
    w = torch.randn(n, device=dev)
    wa, wb = w.clone(), w.clone()
    ma, mb = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sa, sb = (torch.empty(n, dtype=torch.bfloat16, device=dev) for _ in range(2))
    for it in range(2):
        K.sgd_(wa, g, ma, sa, 0.1, wd=1e-4, momentum=0.9, first=(it == 0), grad_scale=0.5, clip_dev=out[2:3])
        K.sgd_(wb, g, mb, sb, 0.1, wd=1e-4, momentum=0.9, first=(it == 0), grad_scale=0.5)
    assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(sa, sb)
    wa, wb = w.clone(), w.clone()
    va, vb = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    ma.zero_(), mb.zero_()
    for it in range(2):
        K.adam_(wa, g, ma, va, sa, 1e-3, it + 1, wd=0.01, decoupled=True, grad_scale=0.5, clip_dev=out[2:3])
        K.adam_(wb, g, mb, vb, sb, 1e-3, it + 1, wd=0.01, decoupled=True, grad_scale=0.5)
    assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(sa, sb)


# ---- whole models ------------------------------------------------------------------------------

def _lenet():
    from kubeml_amd.models.lenet import LeNet
    from kubeml_amd.nn import cross_entropy, flatten_module
    torch.manual_seed(0)
    m = LeNet().to(dev)
    sp = flatten_module(m)
    m.train()
    g = torch.Generator().manual_seed(1)
    # inputs of std 4: the gradient norm starts near 1 and falls to about 0.5 within three steps, so
    # a threshold of 0.5 clips some steps and not others
    x = (4 * torch.randn(32, 1, 28, 28, generator=g)).to(dev)
    y = torch.randint(0, 10, (32,), generator=g).to(dev)
    return m, sp, lambda: cross_entropy(m(x), y)


def _resnet18():
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import cross_entropy, flatten_module
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    sp = flatten_module(m)
    m.train()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(8, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (8,), generator=g).to(dev)
    return m, sp, lambda: cross_entropy(m(x), y)


def _bert():
    from kubeml_amd.models.bert import bert_tiny_mlm
    from kubeml_amd.nn import flatten_module
    torch.manual_seed(0)
    V = 1003                       # not a multiple of 8: the decoder's padded rows / columns
    m = bert_tiny_mlm(vocab=V, dropout=0.0).to(dev)
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


def _param_norm(m):
    return math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in m.parameters() if p.grad is not None))


@pytest.fixture(scope="module")
def resnet18_backward():
    """(model, space, fp64 per-parameter norm, the final flat gradient) after one eager backward."""
    m, sp, loss = _resnet18()
    sp.zero_grad()
    loss().backward()
    sp.finish_grads()
    return m, sp, _param_norm(m), sp.grad.clone()


def _check_flat_norm(m, sp, ref):
    from kubeml_amd.ops import kernels as K
    out = _norm(sp.grad, 1.0)
    got = float(out[1])
    bound = _sumsq_bound(sp.grad.numel(), K.grad_norm_blocks(sp.grad.numel())) / 2 + 2 * EPS24
    print(type(m).__name__, "flat", got, "per-parameter", ref, "rel", abs(got - ref) / ref, "bound", bound)
    assert ref > 0 and abs(got - ref) <= bound * ref


@pytest.mark.parametrize("make", [_lenet, _bert], ids=["lenet", "bert_tiny_v1003"])
def test_flat_norm_equals_per_parameter_norm(make):
    """Alignment gaps and padded channels / rows of the flat gradient buffer hold zeros."""
    m, sp, loss = make()
    sp.zero_grad()
    loss().backward()
    sp.finish_grads()
    _check_flat_norm(m, sp, _param_norm(m))


def test_flat_norm_equals_per_parameter_norm_resnet18(resnet18_backward):
    m, sp, ref, g0 = resnet18_backward
    sp.grad.copy_(g0)
    _check_flat_norm(m, sp, ref)


def test_nn_utils_clip_grad_norm(resnet18_backward):
    """The drop-in on a model whose backward defers 3x3 folds: device norm returned, flat gradient
    (and so every p.grad view) scaled in place by torch's coefficient."""
    from kubeml_amd.nn.utils import clip_grad_norm_
    from kubeml_amd.ops import kernels as K
    m, sp, ref, g0 = resnet18_backward
    sp.grad.copy_(g0)
    mx = 0.5 * ref
    got = clip_grad_norm_(m.parameters(), mx)
    assert got.is_cuda and got.dim() == 0
    bound = _sumsq_bound(g0.numel(), K.grad_norm_blocks(g0.numel())) / 2 + 2 * EPS24
    assert abs(float(got) - ref) <= bound * ref
    coef = torch.tensor(mx, dtype=torch.float32) / (got.cpu() + 1e-6)
    assert 0.49 < float(coef) < 0.51
    assert torch.allclose(sp.grad, g0 * coef.to(dev), rtol=4 * EPS24, atol=0)
    assert abs(_param_norm(m) - mx) <= 1e-5 * mx
    # above the norm: untouched
    sp.grad.copy_(g0)
    clip_grad_norm_(m.parameters(), 2.0 * ref)
    assert torch.equal(sp.grad, g0)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("kind", ["adamw", "sgdm"])
def test_optimizer_max_grad_norm_matches_torch_clip_then_step(kind):
    """Three eager steps of a flattened LeNet against a torch twin fed the same gradients:
    clip_grad_norm_ then the torch optimizer's step."""
    from kubeml_amd.optim import SGD, AdamW
    m, sp, loss = _lenet()
    params = list(m.parameters())
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    if kind == "adamw":
        opt = AdamW(params, lr=1e-3, weight_decay=1e-2, max_grad_norm=0.5)
        ref = torch.optim.AdamW(twin, lr=1e-3, weight_decay=1e-2)
    else:
        opt = SGD(params, lr=0.05, momentum=0.9, max_grad_norm=0.5)
        ref = torch.optim.SGD(twin, lr=0.05, momentum=0.9)
    w0 = [p.detach().clone() for p in params]
    clipped = 0
    for _ in range(3):
        opt.zero_grad()
        loss().backward()
        sp.finish_grads()
        for p, q in zip(params, twin):
            q.grad = p.grad.detach().clone()
        nrm = torch.nn.utils.clip_grad_norm_(twin, 0.5)
        clipped += float(nrm) > 0.5
        ref.step()
        opt.step()
        assert abs(float(opt.grad_norm_tensor()) - float(nrm)) <= 1e-5 * float(nrm)
    assert clipped > 0, "the threshold never clipped: the test would show nothing"
    for p, q, w in zip(params, twin, w0):
        # the tolerance of test_models_gpu's LeNet check (0.03), on the update itself
        assert _rel(p.detach() - w, q.detach() - w) < 0.03
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def test_clipping_on_a_gpu_needs_one_flat_space():
    from kubeml_amd.optim import SGD
    m, sp, loss = _lenet()
    extra = torch.nn.Parameter(torch.zeros(8, device=dev))
    opt = SGD(list(m.parameters()) + [extra], lr=0.1, max_grad_norm=1.0)
    sp.zero_grad()
    loss().backward()
    extra.grad = torch.ones_like(extra)
    with pytest.raises(ValueError):
        opt.step()


def _r18_step_setup(thr):
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    opt = SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, max_grad_norm=thr)
    g = torch.Generator(device=dev).manual_seed(11)
    xs = torch.randn(4, 8, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (4, 8), device=dev, generator=g)
    return m, sp, opt, xs, ys


def test_graphed_step_clips_and_follows_the_threshold():
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn import backward_loss, cross_entropy
    THR, FAR = 0.05, 1e4
    # eager: three clipped steps, then one with the threshold far above the norm
    m, sp, opt, xs, ys = _r18_step_setup(THR)
    eager, enorm = [], []
    for k in range(4):
        if k == 3:
            opt.set_max_grad_norm(FAR)
        sp.zero_grad()
        backward_loss(cross_entropy(m(xs[k]), ys[k]))
        opt.step()
        eager.append(sp.master.clone())
        enorm.append(opt.grad_norm_tensor(sp.device).clone())
    assert all(float(n) > THR for n in enorm[:3]) and float(enorm[3]) < FAR, enorm
    # graphed
    m, sp, opt, xs, ys = _r18_step_setup(THR)
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
    assert torch.equal(sp.master, w0) and int(i) == 0
    for k in range(4):
        if k == 3:
            opt.set_max_grad_norm(FAR)        # no re-capture: the next replay reads the scalar
        step()
        torch.cuda.synchronize()
        assert torch.equal(sp.master, eager[k]), (k, float((sp.master - eager[k]).abs().max()))
        assert torch.equal(opt.grad_norm_tensor(sp.device), enorm[k]), k
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def test_kubemodel_step_clips_in_the_graph(monkeypatch):
    """KubeModel.step(max_grad_norm=): clipping is part of the graph key, a changed value refills
    the device scalar of the same graph, last_grad_norm() reads the norm; the eager
    (KUBEML_NO_GRAPH) path agrees to rounding (the bound of test_engine_gpu's graph / eager pair)."""
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    from kubeml_amd.sdk.model import KubeModel

    class M(KubeModel):
        pass

    def km():
        torch.manual_seed(0)
        net = resnet18(10).to(dev)
        k = M(net, None, gpu=True)
        k.device = torch.device("cuda", 0)
        k._flat = flatten_module(net)
        k.optimizer = SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        return k
    g = torch.Generator(device=dev).manual_seed(11)
    xs = torch.randn(3, 8, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (3, 8), device=dev, generator=g)
    thrs = (0.05, 0.05, 1e4)
    runs = []
    for graph in (True, False):
        if graph:
            monkeypatch.delenv("KUBEML_NO_GRAPH", raising=False)
        else:
            monkeypatch.setenv("KUBEML_NO_GRAPH", "1")
        k = km()
        norms = []
        for i, thr in enumerate(thrs):
            k.step(xs[i], ys[i], max_grad_norm=thr)
            norms.append(k.last_grad_norm())
        torch.cuda.synchronize()
        assert k.optimizer.clips and k.optimizer.param_groups[0]["max_grad_norm"] == 1e4
        if graph:
            assert len(k._graphs) == 1 and all(key[-1] is True for key in k._graphs)
        runs.append((k._flat.master.clone(), norms))
    (wa, na), (wb, nb) = runs
    assert na[0] > 0.05 and na[1] > 0.05 and na[2] < 1e4
    assert all(abs(a - b) <= 1e-4 * b for a, b in zip(na, nb)), (na, nb)
    torch.manual_seed(0)
    w0 = flatten_module(resnet18(10).to(dev)).master
    upd = float((wb - w0).abs().max())
    d = float((wa - wb).abs().max())
    print("update", upd, "graph - eager", d, "norms", na, nb)
    assert upd > 1e-3 and d <= 1e-4 * upd, (d, upd)
