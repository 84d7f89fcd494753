"""Per-group lr / weight decay in the fused optimizers on the MI355X: the grouped kernels against
the single-group ones (bit for bit) and against torch.optim, the optimizer classes, the captured
step and the launchers' rejections."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = "cuda"

GRAN = 64
N = GRAN * 37               # 2368 elements: 592 float4 (more than one 256-thread block)
STEPS = 3
CLIP = 0.5
# (lr, weight_decay) of the three groups
HP = {"sgd": [(0.1, 1e-4), (0.05, 0.0), (0.02, 1e-2)],
      "adam": [(1e-3, 0.01), (5e-4, 0.0), (2e-3, 0.1)]}
KINDS = ("sgd", "sgd_nesterov", "adam", "adamw")
MODES = ("whole", "one_block", "slice", "clip")


def _granule_groups(ngran, G=3, seed=5):
    """A fixed assignment in which neighbouring granules always differ (so the four granules under
    one wave's 256 elements carry different groups)."""
    g = torch.Generator().manual_seed(seed)
    hop = torch.randint(1, G, (ngran,), generator=g)           # 1 .. G-1: never stays
    return (torch.cumsum(hop, 0) % G).to(torch.uint8)


def _inputs(n, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.randn(n, device=dev, generator=g)
    grads = [torch.randn(n, device=dev, generator=g) for _ in range(STEPS)]
    return w, grads


def _mode_args(mode, n):
    """(start of the range, max_blocks, clip coefficient or None)"""
    return (5 * GRAN if mode == "slice" else 0, 1 if mode == "one_block" else 0, CLIP if mode == "clip" else None)


class _Run:
    """master / state / shadow after STEPS steps."""

    def __init__(self, w, kind):
        self.w = w.clone()
        self.s1 = torch.zeros_like(w)                # momentum / exp_avg
        self.s2 = torch.zeros_like(w)                # exp_avg_sq
        self.sh = torch.zeros(w.numel(), dtype=torch.bfloat16, device=w.device)
        self.kind = kind

    def tensors(self):
        return (self.w, self.s1, self.sh) if self.kind.startswith("sgd") else (self.w, self.s1, self.s2, self.sh)


def _grouped(kind, mode, w, grads, gid, hp_rows):
    from kubeml_amd.ops import kernels as K
    n = w.numel()
    a, mb, clip = _mode_args(mode, n)
    r = _Run(w, kind)
    gid_d = gid.to(dev)
    hp = torch.tensor(hp_rows, dtype=torch.float32, device=dev)
    cd = None if clip is None else torch.tensor([clip], device=dev)
    for it, g in enumerate(grads):
        if kind.startswith("sgd"):
            K.sgd_groups_(r.w[a:], g[a:], r.s1[a:], r.sh[a:], gid_d, hp, a, momentum=0.9,
                          nesterov=kind == "sgd_nesterov", first=it == 0, max_blocks=mb, clip_dev=cd)
        else:
            K.adam_groups_(r.w[a:], g[a:], r.s1[a:], r.s2[a:], r.sh[a:], gid_d, hp, it + 1, a,
                           decoupled=kind == "adamw", max_blocks=mb, clip_dev=cd)
    return r


def _single(kind, mode, w, grads, lr, wd):
    """The same range with ONE (lr, wd) through the single-group launchers."""
    from kubeml_amd.ops import kernels as K
    a, mb, clip = _mode_args(mode, w.numel())
    r = _Run(w, kind)
    cd = None if clip is None else torch.tensor([clip], device=dev)
    for it, g in enumerate(grads):
        if kind.startswith("sgd"):
            K.sgd_(r.w[a:], g[a:], r.s1[a:], r.sh[a:], lr, wd=wd, momentum=0.9, nesterov=kind == "sgd_nesterov",
                   first=it == 0, max_blocks=mb, clip_dev=cd)
        else:
            K.adam_(r.w[a:], g[a:], r.s1[a:], r.s2[a:], r.sh[a:], lr, it + 1, wd=wd, decoupled=kind == "adamw",
                    max_blocks=mb, clip_dev=cd)
    return r


def _assert_bitwise(got, kind, mode, w, grads, gid, hp_rows):
    elem_group = gid.long().repeat_interleave(GRAN).to(dev)
    a = _mode_args(mode, w.numel())[0]
    start = _Run(w, kind)
    for k, (lr, wd) in enumerate(hp_rows):
        ref = _single(kind, mode, w, grads, lr, wd)
        mask = elem_group == k
        assert int(mask[a:].sum()) > 0
        for j, (t, rt) in enumerate(zip(got.tensors(), ref.tensors())):     # master, state, bf16 shadow
            assert torch.equal(t[mask], rt[mask]), (kind, mode, k, j)
    # nothing before the range's start was touched
    for t, t0 in zip(got.tensors(), start.tensors()):
        assert torch.equal(t[:a], t0[:a])


@pytest.fixture(scope="module")
def small():
    w, grads = _inputs(N)
    return w, grads, _granule_groups(N // GRAN)


def test_neighbouring_granules_differ(small):
    gid = small[2]
    assert gid.numel() == 37 and set(gid.tolist()) == {0, 1, 2}
    assert bool((gid[1:] != gid[:-1]).all())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_kernel_equals_single_group_launches_bitwise(small, kind, mode):
    w, grads, gid = small
    rows = HP["sgd" if kind.startswith("sgd") else "adam"]
    got = _grouped(kind, mode, w, grads, gid, rows)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.w).all())
    _assert_bitwise(got, kind, mode, w, grads, gid, rows)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_kernel_matches_torch(small, kind, mode):
    """torch.optim with the same three groups on fp32 clones of the range's elements."""
    w, grads, gid = small
    rows = HP["sgd" if kind.startswith("sgd") else "adam"]
    a, _, clip = _mode_args(mode, N)
    got = _grouped(kind, mode, w, grads, gid, rows)
    elem_group = gid.long().repeat_interleave(GRAN).to(dev)
    masks = [(elem_group == k) & (torch.arange(N, device=dev) >= a) for k in range(len(rows))]
    ps = [torch.nn.Parameter(w[m].clone()) for m in masks]
    groups = [{"params": [p], "lr": lr, "weight_decay": wd} for p, (lr, wd) in zip(ps, rows)]
    if kind.startswith("sgd"):
        topt = torch.optim.SGD(groups, lr=0.1, momentum=0.9, nesterov=kind == "sgd_nesterov")
    elif kind == "adam":
        topt = torch.optim.Adam(groups, lr=1e-3)
    else:
        topt = torch.optim.AdamW(groups, lr=1e-3)
    for g in grads:
        for p, m in zip(ps, masks):
            p.grad = g[m] * (1.0 if clip is None else clip)
        topt.step()
    for p, m in zip(ps, masks):
        assert torch.allclose(got.w[m], p.data, atol=1e-5), float((got.w[m] - p.data).abs().max())
    assert torch.equal(got.sh[a:], got.w[a:].to(torch.bfloat16))


def test_grouped_adam_large_grid_iterates():
    """4.3 M elements: more float4 than the full-size grid covers in one pass of its two-group unroll
    (2048 blocks x 256 threads x 4 elements x 2)."""
    n = GRAN * 67200
    assert n > 2048 * 256 * 4 * 2
    g = torch.Generator(device=dev).manual_seed(3)
    w = torch.randn(n, device=dev, generator=g)
    grads = [torch.randn(n, device=dev, generator=g)]
    gid = _granule_groups(n // GRAN)
    got = _grouped("adamw", "whole", w, grads, gid, HP["adam"])
    _assert_bitwise(got, "adamw", "whole", w, grads, gid, HP["adam"])


# ---- optimizer level -------------------------------------------------------------------------

def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(33, 10), torch.nn.LayerNorm(10), torch.nn.Linear(10, 7))


def _two_groups(net, lrs):
    no_decay = [p for p in net.parameters() if p.ndim <= 1]
    decay = [p for p in net.parameters() if p.ndim > 1]
    return [{"params": decay, "weight_decay": 0.01, "lr": lrs[0]},
            {"params": no_decay, "weight_decay": 0.0, "lr": lrs[1]}]


def _torch_opt(kind, net):
    if kind == "adamw":
        return torch.optim.AdamW(_two_groups(net, (1e-2, 5e-3)), lr=1e-2)
    return torch.optim.SGD(_two_groups(net, (0.1, 0.05)), lr=0.1, momentum=0.9)


@pytest.mark.parametrize("thr", [None, 1.0], ids=["plain", "max_grad_norm"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_from_torch_grouped_optimizer_matches_torch(kind, thr):
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import from_torch, with_max_grad_norm
    ref = _net().to(dev)
    ours = copy.deepcopy(ref)
    sp = flatten_module(ours)
    # regions that are no multiple of the granule, decay and no-decay regions interleaved
    assert any(n % GRAN for _, n in sp.offsets)
    opt = from_torch(_torch_opt(kind, ours))
    assert opt.grouped
    if thr is not None:
        opt = with_max_grad_norm(opt, thr)
    gids = opt.group_ids(sp).tolist()
    assert sum(a != b for a, b in zip(gids, gids[1:])) >= 3, gids
    topt = _torch_opt(kind, ref)
    gen = torch.Generator(device=dev).manual_seed(1)
    for _ in range(STEPS):
        for p, q in zip(ours.parameters(), ref.parameters()):
            gr = torch.randn(q.shape, device=dev, generator=gen)
            p.grad.copy_(gr)
            q.grad = gr.clone()
        if thr is not None:
            nrm = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), thr))
            assert nrm > thr                      # one global norm over both groups, and it clips
        opt.step()
        topt.step()
        if thr is not None:
            assert abs(float(opt.grad_norm_tensor(sp.device)) - nrm) <= 1e-5 * nrm
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-5), float((p - q).abs().max())
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


def test_eager_step_follows_direct_writes_to_param_groups():
    """An LR scheduler writes param_groups[k]["lr"] itself; user code may change a group's decay."""
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import from_torch
    ref = _net().to(dev)
    ours = copy.deepcopy(ref)
    flatten_module(ours)
    opt, topt = from_torch(_torch_opt("adamw", ours)), _torch_opt("adamw", ref)
    gen = torch.Generator(device=dev).manual_seed(4)
    for k in range(STEPS):
        if k == 1:
            for o in (opt, topt):
                o.param_groups[1]["lr"] = 2e-2
                o.param_groups[0]["weight_decay"] = 0.2
        for p, q in zip(ours.parameters(), ref.parameters()):
            gr = torch.randn(q.shape, device=dev, generator=gen)
            p.grad.copy_(gr)
            q.grad = gr.clone()
        opt.step()
        topt.step()
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.allclose(p, q, atol=1e-5), float((p - q).abs().max())


def test_grouped_optimizer_needs_one_flat_space_on_the_gpu():
    from kubeml_amd.optim import AdamW
    net = _net().to(dev)
    with pytest.raises(ValueError, match="flat space"):
        AdamW(_two_groups(net, (1e-2, 5e-3)), lr=1e-2)         # loose GPU parameters


def test_captured_step_follows_per_group_lr():
    """set_lr([a, b]) between replays of ONE capture: the weights equal the eager loop's, bit for bit."""
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    schedule = [None, (5e-3, 1e-3), (2e-3, 4e-3)]
    g = torch.Generator(device=dev).manual_seed(7)
    xs = torch.randn(3, 16, 33, device=dev, generator=g)
    ys = torch.randint(0, 7, (3, 16), device=dev, generator=g)

    def build():
        net = _net().to(dev)
        sp = flatten_module(net)
        return net, sp, AdamW(_two_groups(net, (1e-2, 5e-3)), lr=1e-2)

    x, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    net, sp, opt = build()
    eager = []
    for k, lrs in enumerate(schedule):
        if lrs is not None:
            opt.set_lr(lrs)
        x.copy_(xs[k])
        y.copy_(ys[k])
        sp.zero_grad()
        F.cross_entropy(net(x), y).backward()
        opt.step()
        eager.append(sp.master.clone())
    net, sp, opt = build()
    i = torch.zeros((), dtype=torch.int64, device=dev)

    def pre():
        x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
        y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

    def post():
        i.add_(1)
    w0 = sp.master.clone()
    step = make_train_step(net, sp, opt, F.cross_entropy, x, y, pre=pre, post=post, extra_state=[i])
    step.capture()
    torch.cuda.synchronize()
    assert torch.equal(sp.master, w0) and int(i) == 0
    for k, lrs in enumerate(schedule):
        if lrs is not None:
            opt.set_lr(lrs)                       # no re-capture: the replay reads the table
        step()
        torch.cuda.synchronize()
        assert torch.equal(sp.master, eager[k]), (k, float((sp.master - eager[k]).abs().max()))
    assert not torch.equal(eager[2], eager[1])
    assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16))


# ---- rejections ------------------------------------------------------------------------------

def _raw_args(kind, w, g, s1, s2, sh, gid, hp, G, elem0, n):
    if kind == "sgd":
        return ("kml_sgd_groups", "p p p p p p i l f f i p i f l i p f f p s",
                (w.data_ptr(), g.data_ptr(), s1.data_ptr(), sh.data_ptr(), gid.data_ptr(), hp.data_ptr(), G, elem0,
                 0.9, 0.0, 0, None, 1, 1.0, n, 0, None, 0.0, 0.0, None, None))
    return ("kml_adam_groups", "p p p p p p p i l p f f f f i f l i p s",
            (w.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), sh.data_ptr(), gid.data_ptr(), hp.data_ptr(), G,
             elem0, None, 1.0, 0.9, 0.999, 1e-8, 1, 1.0, n, 0, None, None))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_rejections_launch_nothing(kind):
    from kubeml_amd._native import HIP
    from kubeml_amd.ops import kernels as K
    n = GRAN * 8
    g0 = torch.Generator(device=dev).manual_seed(2)
    w = torch.randn(n, device=dev, generator=g0)
    g = torch.randn(n, device=dev, generator=g0)
    s1, s2 = torch.zeros_like(w), torch.zeros_like(w)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    gid = torch.zeros(n // GRAN, dtype=torch.uint8, device=dev)
    hp = torch.tensor([[0.1, 0.0]] * 9, device=dev)
    before = [t.clone() for t in (w, s1, s2, sh)]

    def launch(lo, hi, hp_t, elem0):
        if kind == "sgd":
            K.sgd_groups_(w[lo:hi], g[lo:hi], s1[lo:hi], sh[lo:hi], gid, hp_t, elem0, momentum=0.9, first=True)
        else:
            K.adam_groups_(w[lo:hi], g[lo:hi], s1[lo:hi], s2[lo:hi], sh[lo:hi], gid, hp_t, 1, elem0)
    hp3 = hp[:3].contiguous()
    with pytest.raises(ValueError, match="granule"):
        launch(0, n - 4, hp3, 0)                       # n % 64 != 0
    with pytest.raises(ValueError, match="granule"):
        launch(32, 32 + 4 * GRAN, hp3, 32)             # the range does not start on a granule
    with pytest.raises(ValueError, match="groups"):
        launch(0, n, hp, 0)                            # G = 9
    with pytest.raises(ValueError):
        launch(0, n, hp3, 2 * GRAN)                    # the range runs past the gid table
    # the C entry points refuse the same arguments (hipErrorInvalidValue = 1) before any launch
    INVALID = 1
    for G, elem0, nn, off in ((3, 0, n - 4, 0), (3, 32, 4 * GRAN, 0), (9, 0, n, 0), (0, 0, n, 0), (3, 0, GRAN, 1)):
        name, sig, args = _raw_args(kind, w[off:], g[off:], s1[off:], s2[off:], sh, gid, hp, G, elem0, nn)
        assert HIP.fn(name, sig)(*args) == INVALID, (G, elem0, nn, off)
    torch.cuda.synchronize()
    for t, t0 in zip((w, s1, s2, sh), before):
        assert torch.equal(t, t0)
