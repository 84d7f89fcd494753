"""Device-side LR schedules on the MI355X: the ``kml_lr_schedule`` launch alone against the fp32 twin and
fp64, every fused optimizer under a device schedule against host ``set_lr`` on the same gradients, and the
captured train step (plain, SGD riders, with an EMA, through ``KubeModel.step``) against one eager
host-``set_lr`` trajectory."""
import functools
import math

import pytest
import torch

from kubeml_amd.optim import LRSchedule, lr_factor

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
F32 = torch.float32


def _lr(base, f):
    """The fp32 product the kernel writes, as a Python float."""
    return float(torch.tensor(base, dtype=F32) * f)


# ------------------------------------------------------------------ the kernel alone
def _factor64(x, kind, warmup, total, m, ws, power):
    if warmup > 0 and x < warmup:
        return ws + (1.0 - ws) * (x / warmup)
    q = min(max((x - warmup) / (total - warmup), 0.0), 1.0)
    d = (1.0 - q) ** power if kind == "polynomial" else 0.5 * (1.0 + math.cos(math.pi * q))
    return m + (1.0 - m) * d


EXACT = [("constant", {}), ("linear", {}), ("polynomial", dict(power=1.0)), ("step", dict(milestones=(10, 30), gamma=0.1))]
CLOSE = [("cosine", {}), ("polynomial", dict(power=2.0))]
LAYOUTS = [(1, 1), (3, 2), (5, 4)]          # lr scalar, [G, 2] group table, [T, 4] layer-wise table


@pytest.mark.parametrize("rows,stride", LAYOUTS, ids=["scalar", "groups", "layers"])
@pytest.mark.parametrize("kind,extra", EXACT + CLOSE, ids=[k + "".join(f"-{v}" for v in e.values()) for k, e in EXACT + CLOSE])
def test_kernel_against_the_twin(kind, extra, rows, stride):
    """t = 0 .. 56 at warmup 7, total 53.  constant / linear / polynomial(1) / step: the twin's bits.  cosine
    and polynomial(2): within 1e-6 of the fp64 factor (f in [0, 1], ~8 fp32 roundings plus cosf / powf at a few
    ulp).  Everything of the table but column 0 of its rows, and a guard band behind it, keeps its bits; the
    counter advances by exactly one per launch and not at all with advance = 0."""
    from kubeml_amd.ops import kernels as K
    shape = dict(kind=kind, warmup=7.0, total=53.0, min_ratio=0.05, warmup_start=0.1, **extra)
    guard = 8
    g = torch.Generator().manual_seed(rows)
    table = torch.randn((rows + guard) * stride, generator=g).to(dev)
    before = table.clone()
    base_host = (torch.rand(rows, generator=g) * 0.1 + 1e-3)
    base = base_host.to(dev)
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    pos = torch.tensor([0.0, 1.0], device=dev)
    last = torch.zeros(2, device=dev)
    lr_words = torch.zeros((rows + guard) * stride, dtype=torch.bool)
    lr_words[:rows * stride:stride] = True
    worst = 0.0
    for t in range(57):
        K.lr_schedule_(table, rows, stride, base, ctl, pos, last, 0 if t == 0 else 1, **shape)
        got, c, l = table.cpu(), ctl.cpu(), last.cpu()
        assert c.tolist() == [t, 0, 0, 0]
        assert torch.equal(got[~lr_words], before.cpu()[~lr_words]), t
        f = lr_factor(t, 0.0, 1.0, **shape)
        assert float(l[0]) == float(t)
        if (kind, extra) in EXACT:
            assert torch.equal(l[1], f), (t, float(l[1]), float(f))
            assert torch.equal(got[lr_words], base_host * f), t
        else:
            f64 = _factor64(float(t), kind, 7.0, 53.0, 0.05, 0.1, extra.get("power", 1.0))
            worst = max(worst, abs(float(l[1]) - f64))
            assert torch.equal(got[lr_words], base_host * l[1]), t        # the product itself is one rounding
    if (kind, extra) in CLOSE:
        print(f"{kind} {extra}: max |f - f64| = {worst:.3g}")
        assert worst <= 1e-6
    # advance = 0 rewrites the same LR at the same t
    snap = table.clone()
    K.lr_schedule_(table, rows, stride, base, ctl, pos, last, 0, **shape)
    assert ctl.cpu().tolist() == [56, 0, 0, 0] and torch.equal(table, snap)


def test_kernel_follows_the_position_and_the_base_in_device_memory():
    """x0, dx and base are read at run time: (3, 1/17) with warmup 0.5, total 10, base changed between launches."""
    from kubeml_amd.ops import kernels as K
    shape = dict(kind="linear", warmup=0.5, total=10.0, warmup_start=0.1)
    out, base = torch.zeros(1, device=dev), torch.tensor([0.3], device=dev)
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    pos = torch.tensor([3.0, 1.0 / 17.0], device=dev)
    last = torch.zeros(2, device=dev)
    for t in range(1, 125):
        if t == 60:
            base.fill_(0.7)
        K.lr_schedule_(out, 1, 1, base, ctl, pos, last, 1, **shape)
        f = lr_factor(t, 3.0, 1.0 / 17.0, **shape)
        assert float(out) == _lr(0.3 if t < 60 else 0.7, f), t
    assert float(out) == 0.0 and float(last[1]) == 0.0          # x passed total: min_ratio 0, held


def test_launcher_argument_checks():
    from kubeml_amd.ops import kernels as K
    ctl = torch.zeros(4, dtype=torch.int32, device=dev)
    pos, last = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    out, base = torch.zeros(6, device=dev), torch.zeros(3, device=dev)
    ok = dict(kind="linear", warmup=1.0, total=5.0)
    K.lr_schedule_(out, 3, 2, base, ctl, pos, last, 0, **ok)
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 4, 2, base, ctl, pos, last, 0, **ok)            # rows past the table
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 3, 2, base[:2], ctl, pos, last, 0, **ok)        # base shorter than rows
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 3, 2, base, ctl, pos, last, 2, **ok)            # advance
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 3, 2, base, ctl, pos, last, 0, kind="linear", warmup=5.0, total=5.0)
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 3, 2, base, ctl, pos, last, 0, kind="step", warmup=0.0, total=None,
                       milestones=tuple(range(9)))
    with pytest.raises(TypeError):
        K.lr_schedule_(out, 3, 2, base, ctl.float(), pos, last, 0, **ok)
    with pytest.raises(ValueError):
        K.lr_schedule_(out, 3, 2, base, ctl.cpu(), pos, last, 0, **ok)


# ------------------------------------------------------------------ every optimizer on a small flat space
SHAPE = dict(kind="linear", warmup=3, total=10, warmup_start=0.1)


def _small(kind):
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import LAMB, LARS, SGD, AdamW, layerwise_groups, no_decay_groups
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.LayerNorm(32)).to(dev)
    sp = flatten_module(net)
    if kind == "sgdm":
        opt = SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    elif kind == "adamw":
        opt = AdamW(net.parameters(), lr=1e-2, weight_decay=0.01)
    elif kind == "adamw2":
        groups = no_decay_groups(net, 0.01)
        groups[1]["lr"] = 5e-3
        opt = AdamW(groups, lr=1e-2)
    elif kind == "lamb":
        opt = LAMB(layerwise_groups(net, 0.01), lr=2e-2)
    else:
        groups = layerwise_groups(net, 1e-4)
        groups[1]["lr"] = 0.02
        opt = LARS(groups, lr=0.5, momentum=0.9, trust_coefficient=0.02)
    return net, sp, opt


@pytest.mark.parametrize("kind", ["sgdm", "adamw", "adamw2", "lamb", "lars"])
def test_device_schedule_equals_host_set_lr(kind):
    """12 steps on the same gradients: the device schedule against host set_lr(base * twin(s)) before every
    step.  Master, bf16 shadow and every state buffer, bit for bit."""
    steps = 12
    (_, spa, oa), (_, spb, ob) = _small(kind), _small(kind)
    bases = [g["lr"] for g in oa.param_groups]
    sched = LRSchedule(oa, **SHAPE)
    assert sched.t == 0 and sched.last_lr() == [_lr(b, lr_factor(0, 0.0, 1.0, **SHAPE)) for b in bases]
    g = torch.Generator(device=dev).manual_seed(5)
    grads = torch.randn(steps, spa.numel, device=dev, generator=g) * 0.1
    for s in range(steps):
        f = lr_factor(s, 0.0, 1.0, **SHAPE)
        ob.set_lr([_lr(b, f) for b in bases] if len(bases) > 1 else _lr(bases[0], f))
        for sp, opt in ((spa, oa), (spb, ob)):
            sp.grad.copy_(grads[s])
            opt.step()
        sched.step()
        assert sched.last_lr() == [_lr(b, lr_factor(s + 1, 0.0, 1.0, **SHAPE)) for b in bases], s
    torch.cuda.synchronize()
    assert sched.t == steps
    assert float((spa.master - _small(kind)[1].master).abs().max()) > 1e-4        # it trained
    assert torch.equal(spa.master, spb.master)
    assert torch.equal(spa.shadow, spb.shadow)
    ba, bb = oa.state_buffers(spa), ob.state_buffers(spb)
    assert set(ba) == set(bb)
    for name in ba:
        assert torch.equal(ba[name], bb[name]), name
    # the other columns of a table are the optimizer's: weight decay (and adapt) as the host wrote them
    for ta, tb in zip(oa._tables.values(), ob._tables.values()):
        assert torch.equal(ta.hp[:, 1:], tb.hp[:, 1:])


def test_set_lr_and_reset_state_on_the_device():
    _, sp, opt = _small("adamw2")
    sched = LRSchedule(opt, **SHAPE)
    for _ in range(5):
        sched.step()
    f = lr_factor(5, 0.0, 1.0, **SHAPE)
    opt.set_lr([0.2, 0.4])
    assert sched.t == 5 and sched.last_lr() == [_lr(0.2, f), _lr(0.4, f)]
    gid, hp = opt.group_tables(sp)                       # an eager step's refresh keeps the scheduled column
    assert hp[:, 0].cpu().tolist() == [_lr(0.2, f), _lr(0.4, f)]
    opt.reset_state()
    assert sched.t == 5 and hp[:, 0].cpu().tolist() == [_lr(0.2, f), _lr(0.4, f)]
    sd = sched.state_dict()
    _, _, other = _small("adamw2")
    s2 = LRSchedule(other, **SHAPE)
    s2.load_state_dict(sd)
    assert s2.t == 5 and s2.last_lr() == sched.last_lr()
    assert torch.equal(other._tables[next(iter(other._tables))].hp, hp)
    # a new position zeroes t and rewrites the LR; the next step follows it
    sched.set_position(2.0, 0.125)
    assert sched.t == 0 and sched.last_lr() == [_lr(b, lr_factor(0, 2.0, 0.125, **SHAPE)) for b in (0.2, 0.4)]
    sched.step()
    assert sched.t == 1 and hp[:, 0].cpu().tolist() == [_lr(b, lr_factor(1, 2.0, 0.125, **SHAPE)) for b in (0.2, 0.4)]


# ------------------------------------------------------------------ captured steps
BASE = 0.02
REPLAYS = 8
CAP = dict(kind="linear", warmup=3, total=10, warmup_start=0.1)


def _resnet_step(device_schedule, use_graph, ride, ema=False):
    """resnet18 at batch 32 (the engine tests' model), SGD with momentum; the batch of replay i is picked on the
    device.  Returns what the run left behind."""
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import cross_entropy, flatten_module
    from kubeml_amd.optim import EMA, SGD
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    opt = SGD(m.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-4)
    sched = LRSchedule(opt, **CAP) if device_schedule else None
    avg = EMA(m, decay=0.9, warmup=False) if ema else None
    xs, ys = _data()
    x, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    i = torch.zeros((), dtype=torch.int64, device=dev)

    def pre():
        x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
        y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

    def post():
        i.add_(1)
    step = make_train_step(m, sp, opt, cross_entropy, x, y, pre=pre, post=post, extra_state=[i], ride=ride,
                           use_graph=use_graph, ema=avg, lr_schedule=sched)
    if use_graph:
        step.capture()
    if sched is not None:
        # capturing neither advanced the schedule nor left a later step's LR behind
        assert sched.t == 0 and sched.last_lr() == [_lr(BASE, lr_factor(0, 0.0, 1.0, **CAP))]
        assert float(opt.lr_tensor(dev)) == sched.last_lr()[0]
    for s in range(REPLAYS):
        if sched is None:
            opt.set_lr(_lr(BASE, lr_factor(s, 0.0, 1.0, **CAP)))
        step()
        if sched is not None:
            assert sched.last_lr() == [_lr(BASE, lr_factor(s + 1, 0.0, 1.0, **CAP))], s
            assert sched.t == s + 1
    torch.cuda.synchronize()
    return dict(master=sp.master.clone(), shadow=sp.shadow.clone(), mom=opt.state_buffers(sp)["momentum"].clone(),
                step=step, sched=sched, ema=avg)


@functools.lru_cache(maxsize=None)
def _data():
    g = torch.Generator(device=dev).manual_seed(11)
    xs = torch.randn(REPLAYS + 2, 32, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (REPLAYS + 2, 32), device=dev, generator=g)
    return xs, ys


@functools.lru_cache(maxsize=None)
def _host_reference():
    """The eager trajectory with host set_lr(base * twin(s)) before step s: computed once, never written."""
    r = _resnet_step(False, use_graph=False, ride=False)
    return {k: r[k] for k in ("master", "shadow", "mom")}


def _same(run):
    ref = _host_reference()
    for k in ("master", "shadow", "mom"):
        assert torch.equal(run[k], ref[k]), k


def test_captured_step_moves_the_lr_every_replay():
    """Capture, then 8 replays: last_lr() after replay s is base * twin(s + 1), the first replay ran with lr(0)
    (warmup_start 0.1: a capture that advanced the schedule would show), weights equal the eager host-set_lr
    run bit for bit."""
    run = _resnet_step(True, use_graph=True, ride=False)
    assert run["step"].captured and run["step"].g_all is not None
    _same(run)


def test_captured_step_with_sgd_riders_reads_the_new_lr(monkeypatch):
    """The step of test_engine_gpu.py::test_ride_sgd_in_backward_launches_is_bit_exact: layer4 + fc are updated by
    rider blocks inside the next backward's launches.  A rider that read a stale LR would move those weights
    with the wrong step."""
    monkeypatch.setenv("KUBEML_RIDE_PLAN", "4f:321")
    run = _resnet_step(True, use_graph=True, ride=True)
    assert run["step"].ride_plan is not None
    _same(run)


def test_captured_step_with_an_ema_advances_both_counters_once():
    run = _resnet_step(True, use_graph=True, ride=False, ema=True)
    _same(run)
    assert run["sched"].t == REPLAYS
    assert run["ema"].ctl.cpu().tolist()[:2] == [REPLAYS, REPLAYS]


def test_kubemodel_step_carries_the_schedule(monkeypatch):
    """KubeModel.step builds its captured step with the model's schedule; the dry warm-up pass leaves t alone."""
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    from kubeml_amd.sdk.model import KubeModel
    monkeypatch.delenv("KUBEML_NO_GRAPH", raising=False)
    monkeypatch.setenv("KUBEML_RIDE_PLAN", "4f:321")       # (the step rides by default)

    class M(KubeModel):
        pass
    torch.manual_seed(0)
    net = resnet18(10).to(dev)
    net.train()
    km = M(net, None, gpu=True)
    km.device = dev
    km._flat = flatten_module(net)
    km.optimizer = SGD(net.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-4)
    km.lr_schedule = LRSchedule(km.optimizer, **CAP)
    xs, ys = _data()
    km._dry = True
    km.step(xs[0], ys[0])                      # the warm-up task's pass: captured, nothing replayed
    km._dry = False
    assert len(km._graphs) == 1 and km.lr_schedule.t == 0
    assert km.last_lr() == [_lr(BASE, lr_factor(0, 0.0, 1.0, **CAP))]
    for s in range(REPLAYS):
        km.step(xs[s], ys[s])
        assert km.last_lr() == [_lr(BASE, lr_factor(s + 1, 0.0, 1.0, **CAP))]
    torch.cuda.synchronize()
    assert len(km._graphs) == 1
    sp = km._flat
    _same(dict(master=sp.master, shadow=sp.shadow, mom=km.optimizer.state_buffers(sp)["momentum"]))
