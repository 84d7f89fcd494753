"""Device-side LR schedules, the parts that need no GPU: the fp32 twin ``optim.lr_factor`` against fp64 and
against the ``transformers`` schedules, ``optim.LRSchedule`` on the CPU path (the twin writes
``param_groups[k]["lr"]``), and ``KubeModel.configure_lr_schedule`` with position measured in epochs."""
import math

import numpy as np
import pytest
import torch

from kubeml_amd.optim import SGD, AdamW, LRSchedule, lr_factor

F32 = torch.float32
KINDS = [("constant", {}), ("linear", {}), ("polynomial", dict(power=1.0)), ("polynomial", dict(power=2.0)),
         ("cosine", {}), ("step", dict(milestones=(10, 30), gamma=0.1))]


def factor64(t, x0, dx, kind, warmup=0.0, total=None, min_ratio=0.0, warmup_start=0.0, power=1.0, gamma=0.1,
             milestones=()):
    """The issue's formulas in Python floats (fp64).  The position is the fp32 one (its two roundings are the
    definition of x: a milestone or the end of the warm-up compares against that value)."""
    x = float(torch.tensor(float(x0), dtype=F32) + torch.tensor(float(t), dtype=F32) * torch.tensor(float(dx), dtype=F32))
    if warmup > 0 and x < float(np.float32(warmup)):
        return warmup_start + (1.0 - warmup_start) * (x / warmup)
    if kind == "step":
        return gamma ** sum(1 for m in milestones if float(np.float32(m)) <= x)
    q = min(max((x - warmup) / (total - warmup), 0.0), 1.0)
    d = {"constant": 1.0, "linear": 1.0 - q, "polynomial": (1.0 - q) ** power,
         "cosine": 0.5 * (1.0 + math.cos(math.pi * q))}[kind]
    return min_ratio + (1.0 - min_ratio) * d


@pytest.mark.parametrize("kind,extra", KINDS, ids=[k + "".join(f"-{v}" for v in e.values()) for k, e in KINDS])
@pytest.mark.parametrize("x0,dx,warmup,total", [(0.0, 1.0, 7.0, 53.0), (3.0, 1.0 / 17.0, 0.5, 10.0)],
                         ids=["steps", "epochs"])
def test_twin_against_fp64(kind, extra, x0, dx, warmup, total):
    """|f - f64| <= 1e-6: f is in [0, 1] and goes through at most ~8 fp32 roundings of 6e-8 each, plus cosf /
    powf at a few ulp."""
    kw = dict(kind=kind, warmup=warmup, total=total, min_ratio=0.05, warmup_start=0.1, **extra)
    # t up to total + 3 in units of the position: x reaches total + 3 * dx at least
    n = int(math.ceil((total - x0) / dx)) + 3
    worst = 0.0
    for t in range(n + 1):
        f = lr_factor(t, x0, dx, **kw)
        assert f.dtype == F32 and f.dim() == 0
        worst = max(worst, abs(float(f) - factor64(t, x0, dx, **kw)))
    print(f"{kind} {extra}: max |f - f64| = {worst:.3g}")
    assert worst <= 1e-6


def test_twin_against_transformers():
    """|lr - hf| <= 1e-6 * base for s in [0, total] (HF's cosine is not clamped past total; ours holds
    min_ratio)."""
    tr = pytest.importorskip("transformers")
    base, warmup, total = 1e-3, 7, 53
    cases = [("linear", {}, tr.get_linear_schedule_with_warmup, {}),
             ("cosine", {}, tr.get_cosine_schedule_with_warmup, {}),
             ("polynomial", dict(power=2.0, min_ratio=0.01), tr.get_polynomial_decay_schedule_with_warmup,
              dict(power=2.0, lr_end=base / 100))]
    for kind, ours, hf, hf_kw in cases:
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=base)
        sched = hf(opt, num_warmup_steps=warmup, num_training_steps=total, **hf_kw)
        worst = 0.0
        for s in range(total + 1):
            lr = float(torch.tensor(base, dtype=F32) * lr_factor(s, 0.0, 1.0, kind, warmup=warmup, total=total, **ours))
            worst = max(worst, abs(lr - sched.get_last_lr()[0]))
            opt.step()
            sched.step()
        print(f"{kind}: max |lr - hf| = {worst:.3g}")
        assert worst <= 1e-6 * base, kind


def _net(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def test_cpu_sgd_with_a_schedule_equals_torch_sgd_with_lambdalr():
    """20 steps, bit for bit.  The base LR is a power of two: LambdaLR forms base * f in fp64, which is then
    exact and rounds to the fp32 product the twin writes."""
    base = 0.125
    shape = dict(kind="linear", warmup=3, total=15, warmup_start=0.1, min_ratio=0.05)
    a, b = _net(), _net()
    oa = SGD(a.parameters(), lr=base, momentum=0.9, weight_decay=1e-3)
    sa = LRSchedule(oa, **shape)
    ob = torch.optim.SGD(b.parameters(), lr=base, momentum=0.9, weight_decay=1e-3)
    sb = torch.optim.lr_scheduler.LambdaLR(ob, lambda s: float(lr_factor(s, 0.0, 1.0, **shape)))
    g = torch.Generator().manual_seed(3)
    for s in range(20):
        x, y = torch.randn(8, 6, generator=g), torch.randint(0, 3, (8,), generator=g)
        for net, opt, sched in ((a, oa, sa), (b, ob, sb)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(net(x), y).backward()
            opt.step()
            sched.step()
        assert sa.last_lr() == [oa.param_groups[0]["lr"]] == sb.get_last_lr(), s
        assert sa.t == s + 1
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_attach_writes_lr0_and_step_s_runs_with_f_of_s():
    net = _net()
    opt = AdamW([{"params": [net[0].weight, net[2].weight]}, {"params": [net[0].bias, net[2].bias], "lr": 0.02}],
                lr=0.01)
    sched = LRSchedule(opt, "cosine", warmup=2, total=9, warmup_start=0.25)
    for s in range(12):
        f = lr_factor(s, 0.0, 1.0, "cosine", warmup=2, total=9, warmup_start=0.25)
        want = [float(torch.tensor(b, dtype=F32) * f) for b in (0.01, 0.02)]
        assert [g["lr"] for g in opt.param_groups] == want == sched.last_lr()
        assert sched.last_factor() == float(f)
        sched.step()
    assert sched.last_lr() == [0.0, 0.0]          # past total: min_ratio, held


def test_set_lr_moves_the_base_without_moving_t():
    net = _net()
    opt = SGD(net.parameters(), lr=0.1, momentum=0.9)
    sched = LRSchedule(opt, "linear", warmup=4, total=10)
    for _ in range(6):
        sched.step()
    f = lr_factor(6, 0.0, 1.0, "linear", warmup=4, total=10)
    assert sched.t == 6 and sched.last_lr() == [float(torch.tensor(0.1, dtype=F32) * f)]
    opt.set_lr(0.4)
    assert sched.t == 6 and sched.base_lrs == [0.4]
    assert sched.last_lr() == [opt.param_groups[0]["lr"]] == [float(torch.tensor(0.4, dtype=F32) * f)]
    with pytest.raises(ValueError):
        opt.set_lr([0.1, 0.2])
    # K-AVG round boundary: the optimizer's state goes, the schedule stays
    opt.reset_state()
    assert sched.t == 6 and sched.last_lr() == [float(torch.tensor(0.4, dtype=F32) * f)]
    sched.step()
    assert sched.t == 7


def test_set_position_zeroes_t_and_rewrites_the_lr():
    opt = SGD(_net().parameters(), lr=0.5)
    sched = LRSchedule(opt, "step", milestones=(1, 2), gamma=0.5)
    for _ in range(5):
        sched.step()
    sched.set_position(1.0, 0.25)
    assert sched.t == 0 and sched.last_lr() == [0.25]
    for i in range(1, 6):
        sched.step()
        assert sched.last_lr() == [0.25 if i < 4 else 0.125], i       # x = 1 + i / 4 reaches 2 at i = 4


def test_state_dict_round_trip():
    shape = dict(kind="polynomial", warmup=2, total=20, power=2.0, min_ratio=0.1)
    a = LRSchedule(SGD(_net().parameters(), lr=0.3), **shape)
    a.set_position(0.5, 0.5)
    for _ in range(7):
        a.step()
    sd = a.state_dict()
    assert sd["t"] == 7 and sd["x0"] == 0.5 and sd["dx"] == 0.5 and sd["base_lrs"] == [0.3]
    b = LRSchedule(SGD(_net().parameters(), lr=0.01), **shape)
    b.load_state_dict(sd)
    assert b.t == 7 and b.last_lr() == a.last_lr() and b.optimizer.param_groups[0]["lr"] == a.last_lr()[0]
    a.step(), b.step()
    assert b.last_lr() == a.last_lr()
    other = LRSchedule(SGD(_net().parameters(), lr=0.01), "linear", total=20)
    with pytest.raises(ValueError):
        other.load_state_dict(sd)


def test_argument_errors():
    def opt():
        return SGD(_net().parameters(), lr=0.1)
    with pytest.raises(ValueError):
        LRSchedule(opt(), "linear", warmup=10, total=10)
    with pytest.raises(ValueError):
        LRSchedule(opt(), "linear", warmup=10, total=5)
    with pytest.raises(ValueError):
        LRSchedule(opt(), "cosine", warmup=1)                       # no total
    with pytest.raises(ValueError):
        LRSchedule(opt(), "step", milestones=tuple(range(1, 10)))   # nine milestones
    with pytest.raises(ValueError):
        LRSchedule(opt(), "exponential", total=10)
    with pytest.raises(ValueError):
        lr_factor(0, 0.0, 1.0, "warm", total=10)
    with pytest.raises(TypeError):
        LRSchedule(torch.optim.SGD(_net().parameters(), lr=0.1), "linear", total=10)
    o = opt()
    LRSchedule(o, "constant", total=1)
    with pytest.raises(ValueError):
        LRSchedule(o, "constant", total=1)                          # one schedule per optimizer
    with pytest.raises(ValueError):
        lr_factor(1 << 24, 0.0, 1.0, "linear", total=10)            # float(t) would stop being exact
    s = LRSchedule(opt(), "linear", total=10)
    s._bound = (1 << 24) - 1
    with pytest.raises(ValueError):
        s.step()


def test_make_train_step_runs_the_schedule_after_the_optimizer():
    """The step builder on a CPU flat space (no graph): step s runs with base * f(s), and the weights are those
    of a host set_lr before every step."""
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn.flat import flatten_module
    shape = dict(kind="linear", warmup=3, total=8, warmup_start=0.1)
    base = 0.2

    def run(device_schedule):
        net = _net(1)
        sp = flatten_module(net)
        opt = SGD(net.parameters(), lr=base, momentum=0.9)
        sched = LRSchedule(opt, **shape) if device_schedule else None
        g = torch.Generator().manual_seed(5)
        x, y = torch.randn(8, 6, generator=g), torch.randint(0, 3, (8,), generator=g)
        step = make_train_step(net, sp, opt, torch.nn.functional.cross_entropy, x, y, use_graph=False,
                               lr_schedule=sched)
        for s in range(10):
            lr = float(torch.tensor(base, dtype=F32) * lr_factor(s, 0.0, 1.0, **shape))
            if device_schedule:
                assert sched.t == s and sched.last_lr() == [lr]
            else:
                opt.set_lr(lr)
            step()
        return sp.master.clone()
    assert torch.equal(run(True), run(False))
    with pytest.raises(ValueError):
        net = _net(1)
        sp = flatten_module(net)
        other = LRSchedule(SGD(net.parameters(), lr=0.1), "linear", total=5)
        make_train_step(net, sp, SGD(net.parameters(), lr=0.1), torch.nn.functional.cross_entropy,
                        torch.zeros(2, 6), torch.zeros(2, dtype=torch.long), use_graph=False, lr_schedule=other)


def test_step_max_grad_norm_rebuilds_the_optimizer_and_keeps_the_schedule():
    """step(max_grad_norm=) replaces a non-clipping fused optimizer: the schedule moves over with its
    position and base LR, and the eager step advances it after the update."""
    from kubeml_amd.sdk.model import KubeModel

    class M(KubeModel):
        pass
    net = _net()
    km = M(net, None)
    km.device = torch.device("cpu")
    km.optimizer = SGD(net.parameters(), lr=0.1, momentum=0.9)
    shape = dict(kind="linear", warmup=2, total=6, warmup_start=0.1)
    km.lr_schedule = LRSchedule(km.optimizer, **shape)
    km.lr_schedule.step()
    old = km.optimizer
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(8, 6, generator=g), torch.randint(0, 3, (8,), generator=g)
    km.step(x, y, torch.nn.functional.cross_entropy, max_grad_norm=1.0)
    assert km.optimizer is not old and km.optimizer.clips and km.lr_schedule.optimizer is km.optimizer
    assert km.lr_schedule.base_lrs == [0.1] and km.lr_schedule.t == 2
    assert km.last_lr() == [float(torch.tensor(0.1, dtype=F32) * lr_factor(2, 0.0, 1.0, **shape))]


# ------------------------------------------------------------------ KubeModel: position in epochs
def _toy_store(root):
    from kubeml_amd.store.shards import ShardStore
    rng = np.random.default_rng(0)
    st = ShardStore(root)
    x = rng.integers(0, 255, (64 * 4 + 40, 28, 28)).astype(np.uint8)      # five documents, the last one short
    y = rng.integers(0, 10, len(x)).astype(np.int64)
    st.create("toy", x, y, x[:64], y[:64])
    return st


def _run_epochs(store, store_dir, cfg, epochs=2, K=2):
    from kubeml_amd.models.lenet import LeNet
    from kubeml_amd.sdk.context import TaskContext, reset_task, set_task
    from kubeml_amd.sdk.dataset import KubeDataset
    from kubeml_amd.sdk.model import KubeModel

    class DS(KubeDataset):
        def __init__(self):
            super().__init__("toy")

        def __getitem__(self, i):
            return torch.from_numpy(self.data[i].astype(np.float32) / 255.0).unsqueeze(0), int(self.labels[i])

        def __len__(self):
            return len(self.data)

    class Net(KubeModel):
        seen = []

        def configure_optimizers(self):
            return torch.optim.SGD(self.parameters(), lr=0.05 * self.epoch, momentum=0.9)    # the peak moves

        def configure_lr_schedule(self):
            return cfg

        def train(self, batch, idx):
            x, y = batch
            if self.lr_schedule is not None:
                self.seen.append((self.epoch, self.lr_schedule.t, self.last_lr()[0]))
            return self.step(x, y, torch.nn.functional.cross_entropy)

    torch.manual_seed(0)
    km, extras = None, []
    for e in range(1, epochs + 1):
        ctx = TaskContext(job_id="j", N=1, K=K, task="train", func_id=0, lr=0.05, batch_size=32, epoch=e,
                          store=store, store_dir=store_dir)
        tok = set_task(ctx)
        try:
            if km is None:
                km = Net(LeNet(), DS())
            km.start()
            extras.append(dict(ctx.extra))
        finally:
            reset_task(tok)
    return km, Net.seen, extras


def test_kubemodel_measures_position_in_epochs(tmp_path):
    store = _toy_store(str(tmp_path))
    shape = dict(kind="cosine", warmup=1.5, total=3.0, warmup_start=0.1, min_ratio=0.01)
    cfg = dict(kind="cosine", warmup_epochs=1.5, total_epochs=3.0, warmup_start=0.1, min_ratio=0.01)
    km, seen, extras = _run_epochs(store, str(tmp_path), cfg)
    steps = -(-(64 * 4 + 40) // 32)          # K = 2 at batch 32: one document (two batches) per round, ten in all
    assert [e for e, _, _ in seen] == [1] * steps + [2] * steps
    # t restarts at 0 with every task: epoch 2 starts where the twin says, not at t carried over
    assert [t for _, t, _ in seen] == list(range(steps)) * 2
    for e, i, lr in seen:
        f = lr_factor(i, float(e), 1.0 / steps, **shape)
        assert lr == float(torch.tensor(0.05 * e, dtype=F32) * f), (e, i)
    assert km.lr_schedule.t == steps
    end = float(torch.tensor(0.1, dtype=F32) * lr_factor(steps, 2.0, 1.0 / steps, **shape))
    assert km.last_lr() == [end] and extras[-1]["lr"] == end
    assert type(km.optimizer) is SGD and km.lr_schedule.optimizer is km.optimizer      # one resident optimizer


def test_kubemodel_without_a_schedule_builds_none(tmp_path):
    store = _toy_store(str(tmp_path))
    km, seen, extras = _run_epochs(store, str(tmp_path), None, epochs=1)
    assert km.lr_schedule is None and not seen and "lr" not in extras[0]
    assert type(km.optimizer) is torch.optim.SGD and km.last_lr() == [0.05]


def test_kubemodel_rejects_step_units(tmp_path):
    store = _toy_store(str(tmp_path))
    with pytest.raises(ValueError):
        _run_epochs(store, str(tmp_path), dict(kind="linear", warmup=5, total=90), epochs=1)
