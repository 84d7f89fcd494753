"""ResNet-34 / CIFAR-10 with LARS and a per-step learning-rate schedule written on the device: five
epochs of linear warm-up from a tenth of the peak, then cosine decay to zero at epoch 90.

``configure_lr_schedule`` measures position in epochs.  The LR of ``configure_optimizers`` is the peak;
at the start of every train task the worker sets the position to ``epoch + i / steps`` over the steps it
is about to run, and the captured step's last launch (``kml_lr_schedule``) writes the next step's LR into
the per-tensor table LARS reads.  Nothing runs on the host between replays, and every worker crosses
``[epoch, epoch + 1)`` once per epoch whatever its shard size, K or the epoch's parallelism.
"""
from typing import Tuple

import torch

from kubeml import KubeModel
from kubeml_amd.models.resnet import resnet34
from kubeml_amd.optim import LARS, layerwise_groups
from kubeml_amd.sdk.vision import IMAGENET_MEAN, IMAGENET_STD, ImageDataset, prepare


class Cifar10Dataset(ImageDataset):
    def __init__(self):
        super().__init__("cifar10", mean=IMAGENET_MEAN, std=IMAGENET_STD, crop_pad=4, flip=True)


class KubeResnet34Schedule(KubeModel):
    def __init__(self, network, dataset):
        super().__init__(network, dataset, gpu=True)

    def configure_optimizers(self) -> torch.optim.Optimizer:
        return LARS(layerwise_groups(self._network, 1e-4), lr=self.lr, momentum=0.9)      # the peak LR

    def configure_lr_schedule(self):
        return dict(kind="cosine", warmup_epochs=5, total_epochs=90, warmup_start=0.1, min_ratio=0.0)

    def train(self, batch, batch_index) -> float:
        x, y = prepare(batch, self._dataset, train=True, seed=self.args._func_id)
        return self.step(x, y)

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
    kubenet = KubeResnet34Schedule(resnet, dataset)
    return kubenet.start()
