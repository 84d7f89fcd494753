"""LAMB under data parallelism: two ranks packed on the one GPU of the test box (the spawn pattern
of test_param_groups_multirank_gpu.py, its model and step count), under the default
``peer:shardride`` plan.

A layer-wise optimizer cannot update one flat range (a tensor's norms need its whole gradient, and
inside the shard step that would take a cross-rank sum of chunk norms), so the step builder runs
the plan as the exact end-of-backward all-reduce, with its warning.  Every rank then holds the
bit-identical summed gradient and the same chunk table, so the ranks' weights stay bit-identical.
The update is checked against ONE process that computes every rank's gradient on the same kernels,
sums them in rank order and applies LAMB to the sum."""
import hashlib
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

B = 32
STEPS = 3
WORLD = 2
SPECS = ("peer:shardride:fp32:256",)
KINDS = ("lamb",)


def _digest(t):
    return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _batches(rank, steps, dev):
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    xs = torch.randn(steps, B, 32, 32, 8, device=dev, generator=g).to(torch.bfloat16)
    xs[..., 3:] = 0
    ys = torch.randint(0, 10, (steps, B), device=dev, generator=g)
    return xs, ys


def _model(dev, opt_kind):
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import LAMB, layerwise_groups
    assert opt_kind == "lamb"
    torch.manual_seed(0)
    m = resnet18(10).to(dev)
    m.train()
    sp = flatten_module(m)
    groups = layerwise_groups(m, 1e-2)
    groups[1]["lr"] = 5e-4                     # the groups differ in the LR too
    opt = LAMB(groups, lr=1e-3)
    assert opt.grouped and opt.kind == "lamb"
    return m, sp, opt


def _reference(world, dev, opt_kind, steps):
    """(first update, update after ``steps``) of the single-process data-parallel loop."""
    from kubeml_amd.nn import backward_loss, cross_entropy
    m, sp, opt = _model(dev, opt_kind)
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
        opt.step()
        if k == 0:
            first = (sp.master - w0).cpu()
    torch.cuda.synchronize()
    return first, (sp.master - w0).cpu()


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _rank_main(rank, world, port, q, cases, ref_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    out = {}
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from kubeml_amd.engine.dp import make_train_step
        from kubeml_amd.nn import cross_entropy
        from kubeml_amd.parallel.plan import parse_plan
        seen = _Lines()
        logging.getLogger("kubeml.dp").addHandler(seen)
        for spec, opt_kind, steps in cases:
            m, sp, opt = _model(dev, opt_kind)
            xs, ys = _batches(rank, steps, dev)
            x = torch.empty_like(xs[0])
            y = torch.empty_like(ys[0])
            i = torch.zeros((), dtype=torch.int64, device=dev)

            def pre():
                x.copy_(xs.index_select(0, i.view(1)).squeeze(0))
                y.copy_(ys.index_select(0, i.view(1)).squeeze(0))

            def post():
                i.add_(1)
            w0 = sp.master.clone()
            seen.lines.clear()
            step = make_train_step(m, sp, opt, cross_entropy, x, y, pre=pre, post=post, extra_state=[i],
                                   plan=parse_plan(spec), world=world)
            warned = [ln for ln in seen.lines if "using the all-reduce plan" in ln]
            transport = type(step.peer).__name__ if step.peer is not None else None
            step.capture()
            step()
            torch.cuda.synchronize()
            sp.sync_master()
            upd1 = (sp.master - w0).cpu()
            for _ in range(steps - 1):
                step()
            torch.cuda.synchronize()
            sp.sync_master()
            torch.cuda.synchronize()
            if step.peer is not None:
                step.peer.check()
            res = {"transport": transport, "digests": [_digest(sp.master), _digest(sp.shadow)],
                   "shadow_is_bf16_master": bool(torch.equal(sp.shadow, sp.master.to(torch.bfloat16))),
                   "finite": bool(torch.isfinite(sp.master).all()), "warned": len(warned)}
            if rank == 0:
                ref1, refn = torch.load(os.path.join(ref_dir, opt_kind + ".pt"))
                upd = (sp.master - w0).cpu()
                res["rel"] = float((upd1 - ref1).norm() / ref1.norm())
                res["rel_final"] = float((upd - refn).norm() / refn.norm())
            out[spec + "/" + opt_kind] = res
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


def _spawn(world, cases, ref_dir):
    import torch.multiprocessing as mp
    from kubeml_amd.runtime.pool import free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_rank_main, args=(r, world, port, q, cases, ref_dir)) for r in range(world)]
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


def test_lamb_train_step_two_ranks_one_gpu(tmp_path):
    dev = torch.device("cuda", 0)
    for kind in KINDS:
        torch.save(_reference(WORLD, dev, kind, STEPS), os.path.join(str(tmp_path), kind + ".pt"))
    torch.cuda.synchronize()
    cases = [(spec, kind, STEPS) for spec in SPECS for kind in KINDS]
    res = _spawn(WORLD, cases, str(tmp_path))
    for key in res[0]:
        rs = [res[r][key] for r in range(WORLD)]
        print(key, {k: v for k, v in rs[0].items() if k != "digests"})
        # the shard plan falls back to the exact all-reduce, announced by one warning line
        assert all(r["transport"] == "PeerAllReduce" for r in rs), (key, [r["transport"] for r in rs])
        assert all(r["warned"] == 1 for r in rs), (key, [r["warned"] for r in rs])
        assert all(r["finite"] for r in rs), key
        assert all(r["digests"] == rs[0]["digests"] for r in rs), (key, [r["digests"] for r in rs])
        assert all(r["shadow_is_bf16_master"] for r in rs), key
        assert rs[0]["rel"] <= 1e-5, (key, rs[0]["rel"])
        assert rs[0]["rel_final"] <= 1e-4, (key, rs[0]["rel_final"])
