"""A device LR schedule under data parallelism: two ranks packed on the one GPU of the test box (the spawn
pattern of test_param_groups_multirank_gpu.py), resnet18 with the scalar fused SGD on the ``peer:shard``
plan, whose SGD update runs inside the reduce-scatter collective and reads the LR scalar there.

Each rank carries its own schedule launch at the end of its captured step.  After 6 scheduled steps the
ranks are bit-identical, and the update equals the one of ONE process that computes every rank's gradient
on the same kernels, sums them in rank order and drives the same optimizer with host
``set_lr(base * twin(s))`` before every step, to that file's tolerances."""
import hashlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 32
STEPS = 6
WORLD = 2
SPEC = "peer:shard:fp32:256"
BASE = 1e-2
SHAPE = dict(kind="linear", warmup=2, total=8, warmup_start=0.1)


def _digest(t):
    return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _batches(rank, steps, dev):
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    xs = torch.randn(steps, B, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (steps, B), device=dev, generator=g)
    return xs, ys


def _model(dev):
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    opt = SGD(m.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-4)
    return m, sp, opt


def _reference(world, dev, steps):
    """(first update, update after ``steps``) of the single-process data-parallel loop under host set_lr."""
    from kubeml_amd.nn import backward_loss, cross_entropy
    from kubeml_amd.optim import lr_factor
    m, sp, opt = _model(dev)
    w0 = sp.master.clone()
    data = [_batches(r, steps, dev) for r in range(world)]
    first = None
    for k in range(steps):
        gsum = None
        for r in range(world):
            xs, ys = data[r]
            sp.zero_grad()
            backward_loss(cross_entropy(m(xs[k]), ys[k]))
            sp.finish_grads()
            g = sp.grad.clone()
            gsum = g if gsum is None else gsum + g
        sp.grad.copy_(gsum)
        opt.set_grad_scale(1.0 / world)
        opt.set_lr(float(torch.tensor(BASE, dtype=torch.float32) * lr_factor(k, 0.0, 1.0, **SHAPE)))
        opt.step()
        if k == 0:
            first = (sp.master - w0).cpu()
    torch.cuda.synchronize()
    return first, (sp.master - w0).cpu()


def _rank_main(rank, world, port, q, ref_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from kubeml_amd.engine.dp import make_train_step
        from kubeml_amd.nn import cross_entropy
        from kubeml_amd.optim import LRSchedule, lr_factor
        from kubeml_amd.parallel.plan import parse_plan
        m, sp, opt = _model(dev)
        sched = LRSchedule(opt, **SHAPE)
        xs, ys = _batches(rank, STEPS, dev)
        x = torch.empty_like(xs[0])
        y = torch.empty_like(ys[0])
        i = torch.zeros((), dtype=torch.int64, device=dev)

        def pre():
            x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
            y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

        def post():
            i.add_(1)
        w0 = sp.master.clone()
        step = make_train_step(m, sp, opt, cross_entropy, x, y, pre=pre, post=post, extra_state=[i],
                               plan=parse_plan(SPEC), world=world, lr_schedule=sched)
        transport = type(step.peer).__name__ if step.peer is not None else None
        step.capture()
        t_captured = sched.t
        step()
        torch.cuda.synchronize()
        sp.sync_master()
        upd1 = (sp.master - w0).cpu()
        for _ in range(STEPS - 1):
            step()
        torch.cuda.synchronize()
        sp.sync_master()
        torch.cuda.synchronize()
        if step.peer is not None:
            step.peer.check()
        want = float(torch.tensor(BASE, dtype=torch.float32) * lr_factor(STEPS, 0.0, 1.0, **SHAPE))
        res = {"transport": transport, "digests": [_digest(sp.master), _digest(sp.shadow)],
               "shadow_is_bf16_master": bool(torch.equal(sp.shadow, sp.master.to(torch.bfloat16))),
               "finite": bool(torch.isfinite(sp.master).all()), "t_captured": t_captured, "t": sched.t,
               "lr": sched.last_lr(), "lr_want": [want]}
        if rank == 0:
            ref1, refn = torch.load(ref_path)
            upd = (sp.master - w0).cpu()
            res["rel"] = float((upd1 - ref1).norm() / ref1.norm())
            res["rel_final"] = float((upd - refn).norm() / refn.norm())
        if step.peer is not None:
            step.peer.close()
        del step
        dist.barrier()
        q.put((rank, res, None))
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, None, repr(e) + traceback.format_exc()[-2500:]))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _spawn(world, ref_path):
    import torch.multiprocessing as mp
    from kubeml_amd.runtime.pool import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, q, ref_path)) for r in range(world)]
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
    return {rank: out for rank, out, _ in res}


def test_scheduled_shard_step_two_ranks_one_gpu(tmp_path):
    dev = torch.device("cuda", 0)
    ref_path = os.path.join(str(tmp_path), "ref.pt")
    torch.save(_reference(WORLD, dev, STEPS), ref_path)
    torch.cuda.synchronize()
    res = _spawn(WORLD, ref_path)
    rs = [res[r] for r in range(WORLD)]
    print({k: v for k, v in rs[0].items() if k != "digests"})
    # the SGD update ran inside the collective (no fall-back to the all-reduce plan)
    assert all(r["transport"] == "PeerShard" for r in rs), [r["transport"] for r in rs]
    assert all(r["t_captured"] == 0 and r["t"] == STEPS for r in rs), [(r["t_captured"], r["t"]) for r in rs]
    assert all(r["lr"] == r["lr_want"] for r in rs), [(r["lr"], r["lr_want"]) for r in rs]
    assert all(r["finite"] for r in rs)
    assert all(r["digests"] == rs[0]["digests"] for r in rs), [r["digests"] for r in rs]
    assert all(r["shadow_is_bf16_master"] for r in rs)
    assert rs[0]["rel"] <= 1e-5, rs[0]["rel"]
    assert rs[0]["rel_final"] <= 1e-4, rs[0]["rel_final"]
