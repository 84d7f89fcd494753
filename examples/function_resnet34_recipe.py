"""ResNet-34 / CIFAR-10 with the large-batch recipe: LARS with the trust ratio off on
biases and BN weights (``layerwise_groups``), label smoothing 0.1, and mixup / CutMix.

The data side of the recipe runs inside the launches the plain function already has:
``prepare`` mixes every sample with another row of the batch inside the augment kernel
(one ``lam ~ Beta(alpha, alpha)`` per step, drawn on the device, so every replay of the
captured step mixes anew) and returns packed ``[B, 3]`` targets ``(label, partner label,
lam)``; the fused cross-entropy scores the logits against the smoothed two-label target.
Validation batches are never mixed and are scored against the plain labels.

The loss object is created once, in ``__init__``: ``step`` keys its captured graph on the
identity of ``loss_fn``, so a loss created per batch would capture a new graph per batch.
"""
from typing import Tuple

import torch

from kubeml import KubeModel
from kubeml_amd.models.resnet import resnet34
from kubeml_amd.nn import CrossEntropyLoss
from kubeml_amd.optim import LARS, layerwise_groups
from kubeml_amd.sdk.vision import IMAGENET_MEAN, IMAGENET_STD, ImageDataset, prepare


class Cifar10Dataset(ImageDataset):
    def __init__(self):
        super().__init__("cifar10", mean=IMAGENET_MEAN, std=IMAGENET_STD, crop_pad=4, flip=True,
                         mixup_alpha=0.2, cutmix_alpha=1.0, mix_prob=1.0, switch_prob=0.5)


class KubeResnet34Recipe(KubeModel):
    def __init__(self, network, dataset):
        super().__init__(network, dataset, gpu=True)
        self.criterion = CrossEntropyLoss(label_smoothing=0.1)

    def configure_optimizers(self) -> torch.optim.Optimizer:
        lr = self.lr * (0.1 if self.epoch > 80 else 1.0)
        return LARS(layerwise_groups(self._network, 1e-4), lr=lr, momentum=0.9)

    def train(self, batch, batch_index) -> float:
        x, t = prepare(batch, self._dataset, train=True, seed=self.args._func_id)   # t: packed targets
        return self.step(x, t, loss_fn=self.criterion)

    def validate(self, batch, batch_index) -> Tuple[float, float]:
        x, y = prepare(batch, self._dataset, train=False)
        correct, loss = self.evaluate(x, y)
        return correct * 100 / self.batch_size, loss

    def infer(self, data):
        x = torch.tensor(data, dtype=torch.uint8, device=self.device)
        x, _ = prepare((x, torch.zeros(x.shape[0], dtype=torch.int64, device=self.device)), self._dataset,
                       train=False)
        return self(x).float().argmax(1)


def main():
    resnet = resnet34()
    dataset = Cifar10Dataset()
    kubenet = KubeResnet34Recipe(resnet, dataset)
    return kubenet.start()
