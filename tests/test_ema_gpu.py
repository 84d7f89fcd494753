"""Weight EMA on the MI355X: the update launch against its stock-torch twin bit for bit, the
ticket and the device counters, capture, the swap launch, the graphed train step, evaluation on the
averaged weights, and two ranks packed on one GPU.

The twin (``kubeml_amd.optim.ema.update_twin``) runs its three torch operations on the same device,
so special values (inf - inf, NaN payloads) go through the same hardware; for the element update it
takes the weight ``a`` the launch left in ``aout`` and ``a`` itself is checked against the fp32
formula on its own."""
import hashlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16


def _bits(t):
    return t.contiguous().view(I32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _vectors(n, seed):
    """(ema, w) with +-0, denormals, +-inf, inf - inf and a NaN with a payload on either side."""
    g = torch.Generator(device=dev).manual_seed(seed)
    e = torch.randn(n, device=dev, generator=g)
    w = torch.randn(n, device=dev, generator=g)
    nan_a = torch.tensor([0x7FC12345], dtype=I32, device=dev).view(F32)
    nan_b = torch.tensor([-4190958], dtype=I32, device=dev).view(F32)      # 0xFFC00D12
    inf = float("inf")
    if n == 4:
        e.copy_(torch.tensor([0.0, 1e-40, inf, 1.5], device=dev))
        w.copy_(torch.tensor([-0.0, -3e-41, 2.0, 0.0], device=dev))
        w[3:4] = nan_a
        return e, w
    sp_e = [0.0, -0.0, 1e-40, -1e-39, inf, -inf, inf, 1.0, -2.0, 3e-39]
    sp_w = [-0.0, 0.0, -3e-41, 1e-40, 1.0, 2.0, inf, inf, -inf, 3e-39]
    for base in (0, n - 16):           # the first block's first trip and the last, partial one
        e[base:base + 10] = torch.tensor(sp_e, device=dev)
        w[base:base + 10] = torch.tensor(sp_w, device=dev)
        w[base + 10:base + 11] = nan_a
        e[base + 11:base + 12] = nan_b
    return e, w


def _state():
    return (torch.zeros(4, dtype=I32, device=dev), torch.zeros(1, device=dev), torch.zeros(1, dtype=I32, device=dev))


def _launches(e, ws, decay, every, warmup, max_blocks):
    """Run one launch per weight vector; returns [(ema, ctl, aout)] after each, ticket checked."""
    from kubeml_amd.ops import kernels as K
    e = e.clone()
    ctl, aout, ticket = _state()
    out = []
    for w in ws:
        K.ema_update_(e, w, decay, every, warmup, ctl, aout, ticket, max_blocks=max_blocks)
        assert int(ticket) == 0
        out.append((e.clone(), ctl.clone(), aout.clone()))
    return out


# ------------------------------------------------------------------ the update launch
@pytest.mark.parametrize("n,max_blocks", [(4, 0), (4100, 2), (64 * 1024 + 4, 0)])
def test_update_matches_the_twin_bit_for_bit(n, max_blocks):
    from kubeml_amd.optim.ema import update_twin
    e0, w0 = _vectors(n, n)
    g = torch.Generator(device=dev).manual_seed(7)
    ws = [w0] + [w0 + 0.1 * torch.randn(n, device=dev, generator=g) for _ in range(3)]
    got = _launches(e0, ws, 0.9, 1, True, max_blocks)
    twin = e0.clone()
    tctl, taout = torch.zeros(4, dtype=I32), torch.zeros(1)
    for k, (e, ctl, aout) in enumerate(got):
        update_twin(twin, ws[k], 0.9, 1, True, tctl, taout, a=aout[0])
        assert _same_bits(e, twin), (k, int((_bits(e) != _bits(twin)).sum()))
        assert ctl.tolist() == tctl.tolist() == [k + 1, k + 1, 1, 0]
    # the special values took part: NaN stays, and (past n = 4) the first launch leaves infinities
    assert bool(torch.isnan(twin).any()) and (n == 4 or bool(torch.isinf(got[0][0]).any()))


@pytest.mark.parametrize("u", [0, 1, 7, 8, 50])
def test_weight_of_the_launch_is_the_fp32_formula(u):
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.optim.ema import decay_weight
    e, w = torch.zeros(4, device=dev), torch.ones(4, device=dev)
    ctl, aout, ticket = _state()
    ctl[1] = u
    K.ema_update_(e, w, 0.9999, 1, True, ctl, aout, ticket)
    want = decay_weight(0.9999, u, True)
    assert abs(int(_bits(aout.cpu())) - int(_bits(want.reshape(1)))) <= 1, (float(aout), float(want))
    assert ctl.tolist() == [1, u + 1, 1, 0] and int(ticket) == 0
    K.ema_update_(e, w, 0.75, 1, False, ctl, aout, ticket)
    assert float(aout) == 0.25


def test_result_does_not_depend_on_the_grid():
    n = 64 * 1024 + 4
    e0, w0 = _vectors(n, 3)
    ws = [w0, w0 * 0.5 + 1.0]
    runs = [_launches(e0, ws, 0.99, 1, True, mb) for mb in (1, 2, 0)]
    for r in runs[1:]:
        for (ea, ca, aa), (eb, cb, ab) in zip(runs[0], r):
            assert _same_bits(ea, eb) and torch.equal(ca, cb) and _same_bits(aa, ab)


@pytest.mark.parametrize("every", [1, 3])
def test_counters_and_gate(every):
    n = 4100
    e0, w0 = _vectors(n, 5)
    ws = [w0 + float(k) for k in range(7)]
    got = _launches(e0, ws, 0.5, every, False, 2)
    prev, updates = e0, 0
    for k, (e, ctl, aout) in enumerate(got):
        applied = (k + 1) % every == 0
        updates += applied
        assert ctl.tolist() == [k + 1, updates, int(applied), 0]
        assert _same_bits(e, prev) != applied           # a launch that does not apply touches nothing
        prev = e
    assert got[-1][1][:2].tolist() == [7, 7 // every]


def test_launcher_refuses_bad_arguments():
    from kubeml_amd.ops import kernels as K
    ctl, aout, ticket = _state()
    e, w = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    for args in ((e[:6], w[:6], 0.5, 1), (e[1:5], w[1:5], 0.5, 1), (e, w, 1.5, 1), (e, w, 0.5, 0), (e, w[:4], 0.5, 1)):
        with pytest.raises((ValueError, RuntimeError)):
            K.ema_update_(args[0], args[1], args[2], args[3], True, ctl, aout, ticket)
    with pytest.raises((ValueError, RuntimeError)):
        K.ema_swap_(e, w, None, 9)
    assert ctl.tolist() == [0, 0, 0, 0]


def test_one_captured_launch_follows_the_device_counters():
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.ops import kernels as K
    n = 4100
    e0, w0 = _vectors(n, 9)
    g = torch.Generator(device=dev).manual_seed(1)
    ws = [w0 + 0.1 * torch.randn(n, device=dev, generator=g) for _ in range(6)]
    eager = _launches(e0, ws, 0.9, 2, True, 0)
    e, w = e0.clone(), w0.clone()
    ctl, aout, ticket = _state()

    def body():
        K.ema_update_(e, w, 0.9, 2, True, ctl, aout, ticket)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        body()
    e.copy_(e0)
    ctl.zero_()
    aout.zero_()
    for k in range(6):
        w.copy_(ws[k])
        graph.replay()
        assert _same_bits(e, eager[k][0]) and torch.equal(ctl, eager[k][1]) and _same_bits(aout, eager[k][2]), k
        assert int(ticket) == 0
    assert ctl.tolist() == [6, 3, 1, 0]


# ------------------------------------------------------------------ the swap launch
@pytest.mark.parametrize("numel", [4100, 4098])     # whole float4 groups / a group that straddles n_params
def test_swap_exchanges_refreshes_the_shadow_and_restores(numel):
    from kubeml_amd.ops import kernels as K
    n = (numel + 40 + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(numel)
    state, ema = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g)
    ema[6] = float("inf")
    buf = torch.full((numel + 64,), 7.0, dtype=BF16, device=dev)
    shadow, guard = buf[:numel], buf[numel:]
    shadow.copy_(state[:numel])
    s0, e0, h0 = state.clone(), ema.clone(), shadow.clone()
    K.ema_swap_(state, ema, shadow, numel)
    assert _same_bits(state, e0) and _same_bits(ema, s0)
    assert shadow.numel() == numel and torch.equal(shadow.view(torch.int16), e0[:numel].to(BF16).view(torch.int16))
    assert bool((guard == 7.0).all())
    K.ema_swap_(state, ema, shadow, numel)
    assert _same_bits(state, s0) and _same_bits(ema, e0) and torch.equal(shadow.view(torch.int16), h0.view(torch.int16))
    assert bool((guard == 7.0).all())


# ------------------------------------------------------------------ the graphed train step
B = 32


def _batches(rank, steps):
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    xs = torch.randn(steps, B, 32, 32, 8, device=dev, generator=g).to(BF16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (steps, B), device=dev, generator=g)
    return xs, ys


def _model(opt_kind):
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD, AdamW
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    if opt_kind == "adamw":
        opt = AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    else:
        opt = SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    return m, sp, opt


def _train_step(m, sp, opt, xs, ys, ema, **kw):
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn import cross_entropy
    x, y = torch.empty_like(xs[0]), torch.empty_like(ys[0])
    i = torch.zeros((), dtype=torch.int64, device=dev)

    def pre():
        x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
        y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

    def post():
        i.add_(1)
    return make_train_step(m, sp, opt, cross_entropy, x, y, pre=pre, post=post, extra_state=[i], ema=ema, **kw)


def _advance(twin, sp, ema):
    """The twin's step from this replay's state prefix, with the weight the launch reports."""
    snap = sp.state[:sp.i64_off].clone()
    if int(ema.ctl[2]):
        twin.copy_(twin + (snap - twin) * ema.aout[0])


@pytest.mark.parametrize("opt_kind", ["sgdm", "adamw"])
def test_graphed_train_step_updates_the_ema_and_nothing_else(opt_kind):
    from kubeml_amd.optim import EMA
    steps = 4
    xs, ys = _batches(0, steps)
    runs = {}
    for with_ema in (True, False):
        m, sp, opt = _model(opt_kind)
        ema = EMA(m, decay=0.9, update_every=1, warmup=True) if with_ema else None
        step = _train_step(m, sp, opt, xs, ys, ema)
        if opt_kind == "sgdm":
            assert step.ride_plan is not None              # the SGD riders are on: the EMA comes after them
        s0 = sp.state.clone()
        step.capture()
        torch.cuda.synchronize()
        assert torch.equal(sp.state, s0)
        if with_ema:
            assert ema.ctl.tolist() == [0, 0, 0, 0] and torch.equal(ema.ema, s0[:sp.i64_off])   # capture applies nothing
            twin = ema.ema.clone()
        losses = []
        for k in range(steps):
            losses.append(step().detach().clone())
            torch.cuda.synchronize()
            if with_ema:
                _advance(twin, sp, ema)
                assert torch.equal(ema.ema, twin), k        # parameters and BN statistics alike
                assert ema.ctl.tolist() == [k + 1, k + 1, 1, 0]
        if with_ema:
            assert not torch.equal(ema.ema[sp.numel:], sp.state[sp.numel:sp.i64_off])   # BN statistics moved
            assert abs(ema.last_decay - min(0.9, steps / (9 + steps))) < 1e-6
        runs[with_ema] = (sp.state[:sp.i64_off].clone(), [t.clone() for t in opt.state_buffers(sp).values()],
                          torch.stack(losses))
    (wa, ba, la), (wb, bb, lb) = runs[True], runs[False]
    assert torch.equal(wa, wb) and torch.equal(la, lb) and len(ba) == len(bb) > 0
    assert all(torch.equal(a, b) for a, b in zip(ba, bb))


# ------------------------------------------------------------------ evaluation on the averaged weights
def test_applied_runs_the_captured_eval_graph_on_the_averaged_weights():
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import EMA
    from kubeml_amd.sdk.model import KubeModel

    class M(KubeModel):
        pass
    torch.manual_seed(0)
    net = resnet18(10).to(dev)
    k = M(net, None, gpu=True)
    k.device = dev
    sp = k._flat = flatten_module(net)
    k.ema = ema = EMA(net, decay=0.5, warmup=False)
    g = torch.Generator(device=dev).manual_seed(4)
    with torch.no_grad():
        sp.state[:sp.i64_off].add_(0.05 * torch.randn(sp.i64_off, device=dev, generator=g) * sp.state[:sp.i64_off].abs())
    sp.refresh_shadow()
    ema.update()
    net.eval()
    x, y = _batches(3, 1)
    x, y = x[0], y[0]

    def fwd(n, xx, yy):
        out = n(xx).float()
        return out, out.sum()
    with torch.no_grad():
        live, _ = k.evaluate(x, y, forward=fwd)
        graph = next(iter(k._eval_graphs.values()))["graph"]
        s0, h0 = sp.state.clone(), sp.shadow.clone()
        with ema.applied():
            avg, _ = k.evaluate(x, y, forward=fwd)
        again, _ = k.evaluate(x, y, forward=fwd)
        torch.cuda.synchronize()
        assert len(k._eval_graphs) == 1 and next(iter(k._eval_graphs.values()))["graph"] is graph
        assert torch.equal(sp.state, s0) and torch.equal(sp.shadow.view(torch.int16), h0.view(torch.int16))
        assert torch.equal(again, live) and not torch.equal(avg, live)
        # a second model loaded from the EMA's named tensors (its counters from the live model),
        # through the same captured path
        torch.manual_seed(1)
        net2 = resnet18(10).to(dev)
        k2 = M(net2, None, gpu=True)
        k2.device = dev
        k2._flat = flatten_module(net2)
        net2.load_state_dict({**net.state_dict(), **dict(ema.named_tensors())})
        k2._flat.refresh_shadow()
        net2.eval()
        want, _ = k2.evaluate(x, y, forward=fwd)
        torch.cuda.synchronize()
    assert torch.equal(avg, want), float((avg - want).abs().max())


# ------------------------------------------------------------------ two ranks packed on one GPU
WORLD, STEPS = 2, 3
SPECS = ("peer:shard:fp32:256", "peer:end:fp32:256")


def _digest(t):
    return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _rank_main(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    out = {}
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from kubeml_amd.optim import EMA
        from kubeml_amd.parallel.plan import parse_plan
        for spec in SPECS:
            m, sp, opt = _model("sgdm")
            ema = EMA(m, decay=0.9, warmup=True)
            xs, ys = _batches(rank, STEPS)
            step = _train_step(m, sp, opt, xs, ys, ema, plan=parse_plan(spec), world=world)
            transport = type(step.peer).__name__ if step.peer is not None else None
            step.capture()
            twin = ema.ema.clone()
            ok = True
            for _ in range(STEPS):
                step()
                torch.cuda.synchronize()
                _advance(twin, sp, ema)
                ok = ok and bool(torch.equal(ema.ema, twin))
            if step.peer is not None:
                step.peer.check()
            out[spec] = {"transport": transport, "twin": ok, "ctl": ema.ctl.tolist(),
                         "master": _digest(sp.master), "ema_params": _digest(ema.ema[:sp.numel]),
                         "moved": not bool(torch.equal(ema.ema[:sp.numel], sp.master))}
            if step.peer is not None:
                step.peer.close()
            del step
            dist.barrier()
        q.put((rank, out, None))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, None, repr(e) + traceback.format_exc()[-2500:]))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_one_gpu_keep_one_ema():
    """Each rank's EMA equals the twin advanced from that rank's own state snapshots (BN statistics
    included: they are per rank, each rank sees its own batches), and the parameter range of the
    EMA, like the master, is bit-identical across the ranks.  With an EMA the shard plan runs as
    the all-reduce plan."""
    import torch.multiprocessing as mp
    from kubeml_amd.runtime.pool import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in ps:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in ps]
    finally:
        for p in ps:
            p.join(30)
            if p.is_alive():
                p.kill()
    for rank, out, exc in res:
        assert exc is None, (rank, exc)
    res = {rank: out for rank, out, _ in res}
    for spec in SPECS:
        rs = [res[r][spec] for r in range(WORLD)]
        assert all(r["transport"] == "PeerAllReduce" for r in rs), (spec, [r["transport"] for r in rs])
        assert all(r["twin"] and r["moved"] for r in rs), (spec, rs)
        assert all(r["ctl"] == [STEPS, STEPS, 1, 0] for r in rs), (spec, rs)
        assert rs[0]["master"] == rs[1]["master"] and rs[0]["ema_params"] == rs[1]["ema_params"], (spec, rs)
