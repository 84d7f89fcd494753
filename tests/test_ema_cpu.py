"""Weight EMA on the CPU: the stock-torch twin of the update launch, gating, layout, swap-in
evaluation, checkpoints, K-AVG linearity, and a 2-worker job end to end."""
import json
import threading
import time
import types

import numpy as np
import pytest
import torch

from kubeml_amd.optim import EMA
from kubeml_amd.optim.ema import decay_weight

F32 = torch.float32


def _vec_space(v):
    """The attributes an EMA reads from a flat space, over one raw fp32 vector."""
    return types.SimpleNamespace(state=v, i64_off=v.numel(), numel=v.numel(), shadow=None, device=v.device,
                                 refresh_shadow=lambda: None)


def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


# ------------------------------------------------------------------ the twin
def test_ten_updates_equal_the_literal_loop_and_the_fp64_recurrence():
    g = torch.Generator().manual_seed(0)
    w = torch.randn(1000, generator=g)
    ws = [torch.randn(1000, generator=g) for _ in range(10)]
    ema = EMA(_vec_space(w), decay=0.5, warmup=True)
    e = w.clone()
    e64 = w.double()
    for u in range(10):
        w.copy_(ws[u])
        ema.update()
        # literal: every operation in fp32
        d = torch.minimum(torch.tensor(0.5, dtype=F32), torch.tensor(1 + u, dtype=F32) / torch.tensor(10 + u, dtype=F32))
        a = torch.tensor(1.0, dtype=F32) - d
        e = e + (ws[u] - e) * a
        assert torch.equal(ema.ema, e), u
        d64 = min(0.5, (1 + u) / (10 + u))
        assert ema.last_decay == pytest.approx(d64, rel=1e-6)
        assert (ema.last_decay == 0.5) == (u >= 8)
        e64 = e64 + (ws[u].double() - e64) * (1.0 - d64)
    assert ema.updates == 10 and ema.ctl.tolist() == [10, 10, 1, 0]
    assert float((ema.ema.double() - e64).abs().max()) <= 1e-6 * float(e64.abs().max())


def test_decay_weight_is_formed_in_fp32():
    for u in (0, 1, 7, 8, 50):
        a = decay_weight(0.9999, u, True)
        assert a.dtype == F32 and float(a) == pytest.approx(1 - min(0.9999, (1 + u) / (10 + u)), rel=1e-6)
    assert float(decay_weight(0.75, 3, False)) == 0.25


def test_argument_checks():
    v = torch.zeros(8)
    for kw in (dict(decay=-0.1), dict(decay=1.5), dict(update_every=0), dict(update_every=1.5), dict(update_every=True)):
        with pytest.raises(ValueError):
            EMA(_vec_space(v), **kw)


# ------------------------------------------------------------------ gating
def test_update_every_three_applies_the_third_and_sixth_call():
    w = torch.zeros(64)
    ema = EMA(_vec_space(w), decay=0.5, update_every=3, warmup=False)
    changed = []
    for k in range(7):
        w.add_(1.0)
        before = ema.ema.clone()
        ema.update()
        changed.append(not torch.equal(before, ema.ema))
    assert changed == [False, False, True, False, False, True, False]
    assert ema.ctl[:2].tolist() == [7, 2]


# ------------------------------------------------------------------ frozen / copying decays
def test_decay_one_freezes_and_decay_zero_copies():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(512, generator=g)
    init = w.clone()
    frozen = EMA(_vec_space(w), decay=1.0, warmup=False)
    copying = EMA(_vec_space(w), decay=0.0, warmup=False)
    for _ in range(3):
        w.copy_(torch.randn(512, generator=g) * 10)
        prev = copying.ema.clone()
        frozen.update()
        copying.update()
        assert torch.equal(frozen.ema, init)
        # a = 1: fl(e + fl(w - e)) = (w + (w - e) d1)(1 + d2), |d| <= 2^-24: half an ulp of w - e plus
        # half an ulp of the result, so at most one ulp of the larger of the two (where e and w
        # cancel, the difference is the larger one: an ulp of w alone is not what the form gives)
        _, ex = torch.frexp(torch.maximum((w - prev).abs(), copying.ema.abs()))
        assert bool(((copying.ema - w).abs() <= torch.ldexp(torch.ones(512), ex - 24)).all())
        assert int(_ulps(copying.ema, w).median()) == 0


# ------------------------------------------------------------------ layout
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(8)
        self.fc = torch.nn.Linear(8, 5)

    def forward(self, x):
        return self.fc(torch.relu(self.bn(self.conv(x))).mean((2, 3)))


def _flat_net(seed=0):
    from kubeml_amd.nn.flat import flatten_module
    torch.manual_seed(seed)
    net = _Net()
    with torch.no_grad():
        net.bn.running_mean.normal_()
        net.bn.running_var.uniform_(0.5, 2.0)
    return net, flatten_module(net, "cpu")


def _snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("flat", [True, False], ids=["flat_space", "plain_module"])
def test_named_tensors_cover_the_fp32_state_dict(flat):
    if flat:
        net, _ = _flat_net()
    else:
        torch.manual_seed(0)
        net = _Net()
    ema = EMA(net, decay=0.0, warmup=False)
    fp32 = {k: v for k, v in net.state_dict().items() if v.dtype == F32}
    named = dict(ema.named_tensors())
    assert list(named) == list(fp32) and "bn.running_mean" in named and "bn.num_batches_tracked" not in named
    for k, v in named.items():
        assert v.shape == fp32[k].shape
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p))
        net.bn.running_mean.add_(1.5)
    ema.update()
    for k, v in ema.named_tensors():
        assert torch.equal(v, net.state_dict()[k]), k


# ------------------------------------------------------------------ applied()
@pytest.mark.parametrize("flat", [True, False], ids=["flat_space", "plain_module"])
def test_applied_swaps_in_and_restores_bit_for_bit(flat):
    if flat:
        from kubeml_amd.nn.flat import FlatParamSpace, module_buffers
        torch.manual_seed(0)
        net = _Net()
        sp = FlatParamSpace(list(net.parameters()), device="cpu", with_shadow=True, buffers=module_buffers(net))
        net._kml_flat = sp
    else:
        torch.manual_seed(0)
        net, sp = _Net(), None
    ema = EMA(net, decay=0.5, warmup=False)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p))
        net.bn.running_var.mul_(3.0)
    if sp is not None:
        sp.refresh_shadow()
    ema.update()
    live = _snapshot(net)
    avg = {k: v.detach().clone() for k, v in ema.named_tensors()}
    shadow = None if sp is None else sp.shadow.clone()
    assert any(not torch.equal(avg[k], live[k]) for k in avg)
    with ema.applied():
        inside = net.state_dict()
        for k, v in avg.items():
            assert torch.equal(inside[k], v), k
        assert torch.equal(inside["bn.num_batches_tracked"], live["bn.num_batches_tracked"])
        if sp is not None:
            assert torch.equal(sp.shadow, sp.master.to(torch.bfloat16)) and not torch.equal(sp.shadow, shadow)
    with pytest.raises(RuntimeError, match="boom"):
        with ema.applied():
            raise RuntimeError("boom")
    for k, v in net.state_dict().items():
        assert torch.equal(v, live[k]), k
    for k, v in ema.named_tensors():
        assert torch.equal(v, avg[k]), k
    if sp is not None:
        assert torch.equal(sp.shadow, shadow)


# ------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip(tmp_path):
    from kubeml_amd.store.ckpt import load_checkpoint, load_state, save_checkpoint
    net, _ = _flat_net(0)
    ema = EMA(net, decay=0.5, update_every=2, warmup=True)
    for k in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p))
            net.bn.running_mean.add_(0.25)
        ema.update()
    live = _snapshot(net)
    avg = {k: v.detach().clone() for k, v in ema.named_tensors()}
    buf, ctl = ema.ema.clone(), ema.ctl.clone()
    with_ema, without = str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors")
    save_checkpoint(net, with_ema, job_id="j", epoch=1, ema=ema)
    save_checkpoint(net, without, job_id="j", epoch=1)
    keys = set(load_state(with_ema))
    assert {"ema." + k for k in avg} | {"ema.__ctl__"} == {k for k in keys if k.startswith("ema.")}
    assert not any(k.startswith("ema.") for k in load_state(without))
    side = json.load(open(with_ema + ".json"))
    assert side["ema"] == {"decay": 0.5, "updates": 1}
    for path in (with_ema, without):
        # a plain model, strictly: the live weights
        torch.manual_seed(5)
        plain = _Net()
        load_checkpoint(plain, path, strict=True)
        for k, v in plain.state_dict().items():
            assert torch.equal(v, live[k]), k
        # ema=: buffer and counters back, bit for bit (left alone when the file has none)
        net2, _ = _flat_net(7)
        ema2 = EMA(net2, decay=0.5, update_every=2, warmup=True)
        before = ema2.ema.clone()
        load_checkpoint(net2, path, ema=ema2)
        if path == with_ema:
            assert torch.equal(ema2.ema, buf) and torch.equal(ema2.ctl, ctl)
        else:
            assert torch.equal(ema2.ema, before) and ema2.ctl.tolist() == [0, 0, 0, 0]
        for k, v in net2.state_dict().items():
            assert torch.equal(v, live[k]), k
        # use_ema=True: the averaged weights (the live ones when the file has none)
        torch.manual_seed(6)
        served = _Net()
        load_checkpoint(served, path, use_ema=True)
        want = dict(live, **avg) if path == with_ema else live
        for k, v in served.state_dict().items():
            assert torch.equal(v, want[k]), k


# ------------------------------------------------------------------ K-AVG
def test_kavg_mean_of_emas_is_the_ema_of_the_mean_trajectory():
    from kubeml_amd.parallel.comm import ThreadComm
    from kubeml_amd.parallel.kavg import ModelAverager
    world, steps, decay = 2, 6, 0.9
    g = torch.Generator().manual_seed(3)
    w0 = torch.randn(4, 8, generator=g)
    deltas = [[torch.randn(4, 8, generator=g) * 0.1 for _ in range(steps)] for _ in range(world)]
    comms = ThreadComm.create(world)
    out, errs = [None] * world, []

    def worker(r):
        try:
            net = torch.nn.Linear(8, 4, bias=False)
            with torch.no_grad():
                net.weight.copy_(w0)
            ema = EMA(net, decay=decay, warmup=True)
            seen = []
            for t in range(steps):
                with torch.no_grad():
                    net.weight.add_(deltas[r][t])
                seen.append(net.weight.detach().clone())
                ema.update()
                if (t + 1) % 2 == 0:
                    ModelAverager(net).average_(comms[r], True)
            ema.average_(comms[r])
            out[r] = (ema.ema.clone(), seen)
        except Exception as e:  # pragma: no cover
            errs.append(e)
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert torch.equal(out[0][0], out[1][0])
    ref = w0.double().reshape(-1)
    for t in range(steps):
        mean = sum(out[r][1][t].double() for r in range(world)).reshape(-1) / world
        ref = ref + (mean - ref) * (1.0 - min(decay, (1 + t) / (10 + t)))
    assert float((out[0][0][:ref.numel()].double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_average_is_a_no_op_on_one_worker():
    from kubeml_amd.parallel.comm import LocalComm
    v = torch.randn(16)
    ema = EMA(_vec_space(v), decay=0.5)
    before = ema.ema.clone()
    ema.average_(LocalComm())
    ema.broadcast_(LocalComm(), 0)
    assert torch.equal(ema.ema, before)


# ------------------------------------------------------------------ the step builder on a CPU space
def test_make_train_step_updates_the_ema_last():
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.optim import SGD
    import torch.nn.functional as Fn

    def run(with_ema):
        net, sp = _flat_net(2)
        opt = SGD(net.parameters(), lr=0.1, momentum=0.9)
        ema = EMA(net, decay=0.5, warmup=False) if with_ema else None
        x, y = torch.randn(4, 3, 6, 6, generator=torch.Generator().manual_seed(9)), torch.tensor([0, 1, 2, 3])
        step = make_train_step(net, sp, opt, Fn.cross_entropy, x, y, use_graph=False, ema=ema)
        twin = sp.state[:sp.i64_off].clone()
        for _ in range(3):
            step()
            if with_ema:
                twin = twin + (sp.state[:sp.i64_off] - twin) * 0.5
                assert torch.equal(ema.ema, twin)
        return sp.state.clone()
    assert torch.equal(run(True), run(False))


# ------------------------------------------------------------------ KubeModel, 2 gloo workers
FUNCTION = '''
import torch
import torch.nn as nn
from torch.optim import SGD
from kubeml import KubeDataset, KubeModel
from kubeml_amd.data import transforms
from kubeml_amd.models.lenet import LeNet

USE_EMA = %s


class Data(KubeDataset):
    def __init__(self):
        super().__init__("mnist")
        self.transf = transforms.Compose([transforms.ToTensor(), transforms.Normalize((0.1307,), (0.3081,))])

    def __getitem__(self, index):
        return self.transf(self.data[index]), self.labels[index].astype("int64")

    def __len__(self):
        return len(self.data)


class Net(KubeModel):
    def __init__(self, network, dataset):
        super().__init__(network, dataset, gpu=False)

    def configure_optimizers(self):
        return SGD(self.parameters(), lr=self.lr, momentum=0.9)

    def configure_ema(self):
        return dict(decay=1.0, warmup=False) if USE_EMA else None

    def train(self, batch, batch_index):
        x, y = batch
        self.optimizer.zero_grad()
        loss = nn.functional.cross_entropy(self(x), y)
        loss.backward()
        self.optimizer.step()
        if self.ema is not None:
            self.ema.update()
        return loss.item()

    def validate(self, batch, batch_index):
        x, y = batch
        out = self(x)
        return out.argmax(1).eq(y).sum().item() * 100 / self.batch_size, nn.functional.cross_entropy(out, y).item()


def main():
    torch.manual_seed(42)
    return Net(LeNet(), Data()).start()
'''


def _mnist_like(n, seed):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 10, n).astype(np.int64)
    x = rng.integers(0, 40, (n, 28, 28)).astype(np.uint8)
    for i, k in enumerate(y):
        r, c = 2 + (k // 5) * 12, 2 + (k % 5) * 5
        x[i, r:r + 6, c:c + 5] = 250
    return x, y


def test_kubemodel_validates_and_checkpoints_the_frozen_ema(tmp_path):
    from kubeml_amd.api.types import TrainOptions, TrainRequest
    from kubeml_amd.client import KubemlClient
    from kubeml_amd.config import Config
    from kubeml_amd.control.server import KubeMLServer
    from kubeml_amd.models.lenet import LeNet
    from kubeml_amd.store.ckpt import ckpt_path, load_state
    cfg = Config()
    cfg.store_dir = str(tmp_path / "store")
    ports = {k: 0 for k in ("controller", "scheduler", "ps", "storage", "metrics")}
    srv = KubeMLServer(cfg, n_workers=2, use_gpu=False, task_timeout=300).start(ports=ports)
    try:
        c = KubemlClient(srv.url())
        (xtr, ytr), (xte, yte) = _mnist_like(512, 0), _mnist_like(256, 1)
        paths = {}
        for name, arr in (("xtr", xtr), ("ytr", ytr), ("xte", xte), ("yte", yte)):
            paths[name] = str(tmp_path / (name + ".npy"))
            np.save(paths[name], arr)
        c.datasets.create("mnist", paths["xtr"], paths["ytr"], paths["xte"], paths["yte"])
        runs = {}
        for tag, flag in (("ema", "True"), ("plain", "False")):
            code = tmp_path / f"fn_{tag}.py"
            code.write_text(FUNCTION % flag)
            c.functions.create(tag, str(code))
            req = TrainRequest(batch_size=64, epochs=1, dataset="mnist", lr=0.05, function_name=tag,
                               options=TrainOptions(default_parallelism=2, static_parallelism=True, validate_every=0,
                                                    k=2, goal_accuracy=100))
            jid = c.networks.train(req)
            t0 = time.time()
            while c.tasks.status(jid)["state"] == "running" and time.time() - t0 < 300:
                time.sleep(0.1)
            assert c.tasks.status(jid)["state"] == "finished"
            ep = [json.loads(l) for l in c.logs(jid).decode().splitlines()
                  if l.startswith("{") and '"epoch finished"' in l]
            runs[tag] = (jid, c.histories.get(jid).data, ep)
        (jid, h_ema, ep_ema), (jid_plain, h_plain, ep_plain) = runs["ema"], runs["plain"]
        # the EMA does not disturb training
        assert h_ema.train_loss == h_plain.train_loss and len(h_ema.train_loss) == 1
        assert ep_ema[0]["checksums"] == ep_plain[0]["checksums"] and ep_ema[0]["checksums"]
        # the validation loss is the initial model's (the frozen EMA), not the trained weights'
        torch.manual_seed(42)
        init = LeNet().eval()
        x = ((torch.from_numpy(xte).float() / 255.0 - 0.1307) / 0.3081).unsqueeze(1)
        y = torch.from_numpy(yte)
        with torch.no_grad():
            losses = [float(torch.nn.functional.cross_entropy(init(x[i:i + 64]), y[i:i + 64])) for i in range(0, 256, 64)]
        want = sum(losses) / len(losses)
        assert len(h_ema.validation_loss) == 1
        assert h_ema.validation_loss[0] == pytest.approx(want, rel=1e-5)
        # ... by a hundred times the tolerance of the equality above
        assert abs(h_plain.validation_loss[0] - want) > 1e-3 * want
        # the checkpoint carries the EMA: the initial weights; the live tensors are the trained ones
        sd = load_state(ckpt_path(cfg.store_dir, jid))
        for k, v in init.state_dict().items():
            assert torch.equal(sd["ema." + k], v), k
        ticks, updates = sd["ema.__ctl__"].tolist()[:2]
        assert ticks == updates > 0
        assert any(not torch.equal(sd[k], v) for k, v in init.state_dict().items())
        assert not any(k.startswith("ema.") for k in load_state(ckpt_path(cfg.store_dir, jid_plain)))
        side = json.load(open(ckpt_path(cfg.store_dir, jid) + ".json"))
        assert side["ema"]["decay"] == 1.0 and side["ema"]["updates"] > 0
    finally:
        srv.stop()
