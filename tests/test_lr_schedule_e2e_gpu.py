"""examples/function_resnet34_schedule.py through the controller on one GPU worker: the warm-up task, two
train epochs with validation.  The job's epoch log carries the LR every epoch ended on, which is the twin at
position ``epoch + 1`` times the peak LR (LARS, a table row per tensor: the layer-wise launch path)."""
import json
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_schedule_function_on_gpu_worker(tmp_path):
    from kubeml_amd.api.types import TrainOptions, TrainRequest
    from kubeml_amd.client import KubemlClient
    from kubeml_amd.config import Config
    from kubeml_amd.control.server import KubeMLServer
    from kubeml_amd.optim import lr_factor
    cfg = Config()
    cfg.store_dir = str(tmp_path / "store")
    srv = KubeMLServer(cfg, n_workers=1, use_gpu=True, task_timeout=600).start(
        ports={k: 0 for k in ("controller", "scheduler", "ps", "storage", "metrics")})
    try:
        c = KubemlClient(srv.url())
        rng = np.random.default_rng(0)
        arrs = {"xtr": rng.integers(0, 256, (640 + 40, 32, 32, 3), dtype=np.uint8),      # a short last document
                "ytr": rng.integers(0, 10, 680).astype(np.int64),
                "xte": rng.integers(0, 256, (128, 32, 32, 3), dtype=np.uint8),
                "yte": rng.integers(0, 10, 128).astype(np.int64)}
        paths = {}
        for k, v in arrs.items():
            paths[k] = str(tmp_path / f"{k}.npy")
            np.save(paths[k], v)
        c.datasets.create("cifar10", paths["xtr"], paths["ytr"], paths["xte"], paths["yte"])
        c.functions.create("sched", os.path.join(ROOT, "examples", "function_resnet34_schedule.py"))
        lr = 0.5
        jid = c.networks.train(TrainRequest(batch_size=128, epochs=2, dataset="cifar10", lr=lr, function_name="sched",
                                            options=TrainOptions(default_parallelism=1, static_parallelism=True,
                                                                 validate_every=1, k=-1)))
        t0 = time.time()
        while c.tasks.status(jid)["state"] == "running":
            assert time.time() - t0 < 600
            time.sleep(0.2)
        st = c.tasks.status(jid)
        assert st["state"] == "finished", (st, c.logs(jid).decode()[-3000:])
        h = c.histories.get(jid).data
        assert len(h.train_loss) == 2 and all(np.isfinite(h.train_loss))
        ep = [json.loads(l) for l in c.logs(jid).decode().splitlines() if l.startswith("{") and '"epoch finished"' in l]
        assert len(ep) == 2
        # 680 samples at batch 128: six steps per epoch; after the last one x = epoch + 6 * fp32(1 / 6)
        shape = dict(kind="cosine", warmup=5, total=90, warmup_start=0.1, min_ratio=0.0)
        for e, line in zip((1, 2), ep):
            want = float(torch.tensor(lr, dtype=torch.float32) * lr_factor(6, float(e), 1.0 / 6, **shape))
            assert line["lr"] == want, (e, line["lr"], want)
    finally:
        srv.stop()
