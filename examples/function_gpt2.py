"""GPT-2 small causal language-model training function (the decoder-only counterpart of
function_bert.py; the reference has no transformer workload, so this follows its function
shape, ml/experiments/kubeml/function_resnet34.py:47-104, on the GPT-2 model).

Dataset: token ids uploaded through the storage API like any other dataset —
``kubeml dataset create --traindata ids.npy --trainlabels seg.npy ...`` with ``ids.npy`` an
int64 ``[N, L]`` array of BPE ids (L <= 1024) and ``seg.npy`` an int64 ``[N]`` array (unused;
the storage format needs a label per sample).  Every position is scored against the next
token of its sequence; the last position of a sequence has no target.

Model: HuggingFace-layout GPT2LMHeadModel (kubeml_amd/models/gpt.py) on the hand-written MFMA
GEMM and causal flash-attention kernels; optimizer AdamW (fused single launch on the GPU).
Validation reports next-token accuracy (%) and loss.

GPU path: label shift (one HIP kernel), forward, loss, backward and AdamW of a batch are ONE
hipGraph replay (``self.step(..., forward=...)``); validation is a captured eval forward.
Train with ``kubeml train -f gpt2 --K 1 --grad-sync`` for synchronous data parallelism with
persistent Adam moments.  CPU workers run the same recipe with stock torch ops.

``KUBEML_GPT2_PRESET=tiny`` builds the 2-layer test model (vocab 1000) instead of GPT-2 small.
``KUBEML_GPT2_ACT=gelu_tanh`` selects the tanh-approximated GELU of the released GPT-2 checkpoints
(HF ``gelu_new``) instead of the erf GELU — set it when fine-tuning from released weights.
"""
import os
from typing import Tuple

import numpy as np
import torch
from torch.optim import AdamW

from kubeml import KubeDataset, KubeModel
from kubeml_amd.models.gpt import gpt2_small, gpt2_tiny


class TokenDataset(KubeDataset):
    def __init__(self, name="lm_tokens"):
        super().__init__(name)

    def collate_batch(self, data: np.ndarray, labels: np.ndarray):
        return (torch.from_numpy(np.ascontiguousarray(data).astype(np.int64)),
                torch.from_numpy(np.ascontiguousarray(labels).reshape(-1).astype(np.int64)))

    def __getitem__(self, i):
        return self.data[i], int(self.labels[i])

    def __len__(self):
        return len(self.data) if self.data is not None else 0


class KubeGPT2(KubeModel):
    def __init__(self, network, dataset):
        super().__init__(network, dataset, gpu=True)

        # captured with the step / eval graphs, so created once (their identity keys the graphs)
        def fwd_train(net, ids, seg):
            return net(ids, labels=ids)

        def fwd_val(net, ids, seg):
            loss, correct = net(ids, labels=ids, return_correct=True)
            return correct, loss
        self._fwd_train, self._fwd_val = fwd_train, fwd_val

    def configure_optimizers(self) -> torch.optim.Optimizer:
        return AdamW(self.parameters(), lr=self.lr, weight_decay=0.01)

    def train(self, batch, batch_index) -> float:
        ids, seg = batch
        if ids.is_cuda:
            return self.step(ids, seg, forward=self._fwd_train)   # device loss: read back once per task
        self.optimizer.zero_grad()
        loss = self(ids, labels=ids)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def validate(self, batch, batch_index) -> Tuple[float, float]:
        ids, seg = batch
        scored = ids.shape[0] * (ids.shape[1] - 1)   # every position but the last of a sequence
        if ids.is_cuda:
            correct, loss = self.evaluate(ids, seg, forward=self._fwd_val)
        else:
            loss, correct = self(ids, labels=ids, return_correct=True)
        return correct * 100 / max(1, scored), loss

    def infer(self, data):
        ids = torch.tensor(data, dtype=torch.int64, device=self.device)
        return self(ids).float().argmax(-1)


def main():
    act = os.environ.get("KUBEML_GPT2_ACT", "") or "gelu"
    build = gpt2_tiny if os.environ.get("KUBEML_GPT2_PRESET", "") == "tiny" else gpt2_small
    net = build(activation=act)
    return KubeGPT2(net, TokenDataset()).start()
