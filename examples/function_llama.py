"""Llama-style causal language-model training function (the Llama counterpart of function_gpt2.py).

Dataset: token ids uploaded through the storage API like any other dataset —
``kubeml dataset create --traindata ids.npy --trainlabels seg.npy ...`` with ``ids.npy`` an
int64 ``[N, L]`` array of token ids and ``seg.npy`` an int64 ``[N]`` array (unused; the storage
format needs a label per sample).  Every position is scored against the next token of its
sequence; the last position of a sequence has no target.

Model: HuggingFace-layout LlamaForCausalLM (kubeml_amd/models/llama.py): RMSNorm, rotary
embedding, grouped-query causal flash attention and the gated SiLU MLP on hand-written kernels;
optimizer AdamW (fused single launch on the GPU).  Validation reports next-token accuracy (%) and
loss.

GPU path: label shift, forward, loss, backward and AdamW of a batch are ONE hipGraph replay
(``self.step(..., forward=...)``); validation is a captured eval forward.  CPU workers run the
same recipe with stock torch ops.

Default: 30 layers, hidden 576, 9 heads / 3 K/V heads, inter 1536, vocab 49152, tied head.
``KUBEML_LLAMA_PRESET=tiny`` builds the 2-layer test model (vocab 1000);
``KUBEML_LLAMA_CONFIG=/path/config.json`` builds what a HF checkpoint's config describes.
"""
import os
from typing import Tuple

import numpy as np
import torch
from torch.optim import AdamW

from kubeml import KubeDataset, KubeModel
from kubeml_amd.models.llama import LlamaForCausalLM, llama_tiny


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


class KubeLlama(KubeModel):
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
        return self(ids).float().argmax(-1)   # next-position argmax


def main():
    cfg = os.environ.get("KUBEML_LLAMA_CONFIG", "")
    if os.environ.get("KUBEML_LLAMA_PRESET", "") == "tiny":
        net = llama_tiny()
    elif cfg:
        net = LlamaForCausalLM.from_hf_config(cfg)
    else:
        net = LlamaForCausalLM(vocab=49152, hidden=576, layers=30, heads=9, kv_heads=3, inter=1536, max_pos=2048,
                               tie_word_embeddings=True)
    return KubeLlama(net, TokenDataset()).start()
