"""Global-norm gradient clipping without a GPU: the optimizers' torch path, the SDK plumbing and the
step builder's plan decisions."""
import pytest
import torch
import torch.nn.functional as F


def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.ReLU(), torch.nn.Linear(16, 5))


def _data(k):
    g = torch.Generator().manual_seed(10 + k)
    # step 1's batch is scaled down so its gradient stays under the threshold
    return torch.randn(9, 12, generator=g) * (0.01 if k == 1 else 3.0), torch.randint(0, 5, (9,), generator=g)


def _pair(kind, flat, thr):
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD, Adam, AdamW
    ours, ref = _mlp(), _mlp()
    if flat:
        flatten_module(ours)
    if kind == "sgd":
        return ours, ref, SGD(ours.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True,
                              max_grad_norm=thr), \
            torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True)
    if kind == "adam":
        return ours, ref, Adam(ours.parameters(), lr=1e-2, weight_decay=1e-3, max_grad_norm=thr), \
            torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-3)
    return ours, ref, AdamW(ours.parameters(), lr=1e-2, max_grad_norm=thr), torch.optim.AdamW(ref.parameters(), lr=1e-2)


@pytest.mark.parametrize("flat", [False, True], ids=["loose", "cpu_flat_space"])
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_cpu_optimizers_clip_like_torch(kind, flat):
    thr = 0.5
    ours, ref, opt, topt = _pair(kind, flat, thr)
    clipped = []
    for k in range(3):
        x, y = _data(k)
        opt.zero_grad()
        topt.zero_grad()
        F.cross_entropy(ours(x), y).backward()
        F.cross_entropy(ref(x), y).backward()
        nrm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), thr))
        clipped.append(nrm > thr)
        topt.step()
        opt.step()
        assert abs(float(opt.grad_norm_tensor("cpu")) - nrm) <= 1e-6 * nrm
    assert clipped == [True, False, True], clipped
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-6), float((p - q).abs().max())


def test_grad_scale_enters_the_norm():
    """The norm is that of the averaged gradient: grad * grad_scale, as the data-parallel step sets it."""
    from kubeml_amd.optim import SGD
    a = torch.nn.Parameter(torch.ones(4))
    b = torch.nn.Parameter(torch.ones(4))
    oa, ob = SGD([a], lr=1.0, max_grad_norm=1.0), SGD([b], lr=1.0, max_grad_norm=1.0)
    oa.set_grad_scale(0.25)
    a.grad = torch.full((4,), 8.0)        # averaged: 2 each, norm 4 -> coefficient 1/4
    b.grad = torch.full((4,), 2.0)
    oa.step()
    ob.step()
    assert float(oa.grad_norm_tensor("cpu")) == pytest.approx(4.0)
    assert torch.allclose(a, b) and torch.allclose(a, torch.full((4,), 0.5), atol=1e-6)


def test_arguments_and_conversions():
    from kubeml_amd.optim import SGD, AdamW, from_torch, with_max_grad_norm
    from kubeml_amd.sdk.model import _same_but_lr
    ps = list(_mlp().parameters())
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            SGD(ps, lr=0.1, max_grad_norm=bad)
    plain, clip = SGD(ps, lr=0.1, momentum=0.9), SGD(ps, lr=0.1, momentum=0.9, max_grad_norm=1.0)
    assert not plain.clips and clip.clips and clip.defaults["max_grad_norm"] == 1.0
    with pytest.raises(ValueError):
        plain.set_max_grad_norm(1.0)      # on / off is a different step: fixed at construction
    with pytest.raises(ValueError):
        plain.grad_norm_tensor("cpu")
    clip.set_max_grad_norm(2.0)
    assert clip.param_groups[0]["max_grad_norm"] == 2.0
    # a changed setting is a new optimizer for the SDK, a changed learning rate is not
    assert not _same_but_lr(plain, clip) and not _same_but_lr(clip, plain)
    assert _same_but_lr(clip, SGD(ps, lr=0.3, momentum=0.9, max_grad_norm=2.0))
    assert not _same_but_lr(clip, SGD(ps, lr=0.1, momentum=0.9, max_grad_norm=1.0))
    for t in (torch.optim.SGD(ps, lr=0.1, momentum=0.9), torch.optim.Adam(ps), torch.optim.AdamW(ps)):
        f = from_torch(t)
        assert f.param_groups[0]["max_grad_norm"] is None and not f.clips
    w = with_max_grad_norm(AdamW(ps, lr=3e-4, betas=(0.8, 0.9), weight_decay=0.1), 1.0)
    assert type(w) is AdamW and w.clips
    assert {k: w.defaults[k] for k in ("lr", "betas", "weight_decay")} == {"lr": 3e-4, "betas": (0.8, 0.9),
                                                                           "weight_decay": 0.1}
    # a clipping optimizer has no ranged / sharded step
    with pytest.raises(ValueError):
        clip.step_range(0, 4)


def _kube(net, opt):
    from kubeml_amd.sdk.model import KubeModel
    km = KubeModel.__new__(KubeModel)
    km.device = torch.device("cpu")
    km._network, km.optimizer = net, opt
    km._sync_mode, km._graphs, km._shards, km._flat, km._dry = "local", {}, {}, None, False
    return km


@pytest.mark.parametrize("fused", [False, True], ids=["torch_optimizer", "fused_optimizer"])
def test_kubemodel_step_clips_on_the_cpu_path(fused):
    from kubeml_amd.optim import SGD
    from kubeml_amd.sdk.model import KubeModel
    net, ref = _mlp(), _mlp()
    mk = SGD if fused else torch.optim.SGD
    km = _kube(net, mk(net.parameters(), lr=0.1, momentum=0.9))
    topt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    fwd = lambda n, x, y: F.cross_entropy(n(x), y)
    for k, thr in enumerate((0.5, 0.5, 0.25)):          # a changed value keeps the optimizer and its state
        x, y = _data(k)
        topt.zero_grad()
        F.cross_entropy(ref(x), y).backward()
        nrm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), thr))
        topt.step()
        before = km.optimizer
        KubeModel.step(km, x, y, forward=fwd, max_grad_norm=thr)
        assert k == 0 or km.optimizer is before
        assert abs(km.last_grad_norm() - nrm) <= 1e-6 * nrm
    for p, q in zip(net.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-6)
    if fused:
        assert km.optimizer.clips and km.optimizer.param_groups[0]["max_grad_norm"] == 0.25
        # the next train task's fresh, non-clipping optimizer does not replace the resident one
        km.configure_optimizers = lambda: SGD(net.parameters(), lr=0.05, momentum=0.9)
        kept = km.optimizer
        KubeModel._config_optimizer(km)
        assert km.optimizer is kept and kept.param_groups[0]["lr"] == 0.05


def test_kubemodel_step_refuses_to_turn_clipping_on_mid_training():
    from kubeml_amd.optim import SGD
    from kubeml_amd.sdk.model import KubeModel
    net = _mlp()
    km = _kube(net, SGD(net.parameters(), lr=0.1, momentum=0.9))
    fwd = lambda n, x, y: F.cross_entropy(n(x), y)
    KubeModel.step(km, *_data(0), forward=fwd)
    with pytest.raises(ValueError):
        KubeModel.step(km, *_data(1), forward=fwd, max_grad_norm=1.0)


def test_clipping_optimizer_cannot_shard():
    """The step builder's decision as a unit: the ZeRO-1 plans need a range update and no clipping."""
    from kubeml_amd.engine.dp import optimizer_can_shard, optimizer_clips
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    m = _mlp()
    flatten_module(m)
    plain = SGD(m.parameters(), lr=0.1, momentum=0.9)
    clip = SGD(m.parameters(), lr=0.1, momentum=0.9, max_grad_norm=1.0)
    assert optimizer_can_shard(plain) and not optimizer_clips(plain)
    assert optimizer_clips(clip) and not optimizer_can_shard(clip)
    assert plain.supports_ranges() and not clip.supports_ranges()
    assert not optimizer_clips(torch.optim.SGD(m.parameters(), lr=0.1))


def test_step_builder_takes_the_whole_gradient_path_when_clipping():
    """make_train_step with a clipping optimizer: no per-stage updates (opt_overlap), no riders, a
    shard plan falls back to the all-reduce plan -- and the step equals the eager loop."""
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    from kubeml_amd.parallel.plan import parse_plan

    def setup():
        torch.manual_seed(0)
        m = resnet18(10)
        m.train()
        sp = flatten_module(m)
        return m, sp, SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=0.1)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(4, 3, 32, 32, generator=g) for _ in range(2)]
    ys = [torch.randint(0, 10, (4,), generator=g) for _ in range(2)]
    m, sp, opt = setup()
    x, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    step = make_train_step(m, sp, opt, F.cross_entropy, x, y, opt_overlap=True, ride=True,
                           plan=parse_plan("peer:shardride:fp32:256"))
    assert step.segment_opt is None and step.ride_plan is None and step.shard_step is None
    for k in range(2):
        x.copy_(xs[k])
        y.copy_(ys[k])
        step()
        assert float(opt.grad_norm_tensor("cpu")) > 0.1      # both steps clip
    m2, sp2, opt2 = setup()
    for k in range(2):
        opt2.zero_grad()
        F.cross_entropy(m2(xs[k]), ys[k]).backward()
        opt2.step()
    assert torch.allclose(sp.master, sp2.master, atol=1e-7)
