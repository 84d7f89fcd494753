"""ResNet-50 with the ImageNet input pipeline: images stored larger than the network's input,
RandomResizedCrop(224) + flip for training, Resize(256) + CenterCrop(224) for validation.

The function of ``function_resnet50.py`` on a dataset stored at 256 x 256 (``python
tools/make_datasets.py --names imagenet_synth``; any stored size of at least 224 does).  The uint8
images stay resident on the device and ``prepare`` turns a batch into the 224 x 224 bf16 input in
one launch (``kml_augment_resample``): every sample's crop box follows torchvision's
``RandomResizedCrop.get_params`` from device counters, so a replay of the captured step draws new
crops, and the resize is torch's / PIL's antialiased bilinear filter applied to the crop.
Validation batches are resized so that the shorter side is ``eval_resize`` (256) and cropped at the
centre.  mixup / CutMix (``mixup_alpha=`` / ``cutmix_alpha=``) mix inside the same launch.
"""
from typing import Tuple

import torch
from torch.optim import SGD

from kubeml import KubeModel
from kubeml_amd.models.resnet import resnet50
from kubeml_amd.sdk.vision import IMAGENET_MEAN, IMAGENET_STD, ImageDataset, prepare


class ImageNetStoredLarger(ImageDataset):
    def __init__(self, name="imagenet_synth"):
        super().__init__(name, mean=IMAGENET_MEAN, std=IMAGENET_STD, flip=True, random_resized_crop=224,
                         rrc_scale=(0.08, 1.0), rrc_ratio=(3 / 4, 4 / 3), eval_resize=256)


class KubeResnet50(KubeModel):
    def __init__(self, network, dataset):
        super().__init__(network, dataset, gpu=True)

    def configure_optimizers(self) -> torch.optim.Optimizer:
        return SGD(self.parameters(), lr=self.lr, momentum=0.9, weight_decay=1e-4)

    def train(self, batch, batch_index) -> float:
        x, y = prepare(batch, self._dataset, train=True, seed=self.args._func_id)
        return self.step(x, y)  # one hipGraph replay; device loss (no host sync)

    def validate(self, batch, batch_index) -> Tuple[float, float]:
        x, y = prepare(batch, self._dataset, train=False)
        correct, loss = self.evaluate(x, y)
        return correct * 100 / self.batch_size, loss

    def infer(self, data):
        x = torch.tensor(data, dtype=torch.uint8, device=self.device)
        x, _ = prepare((x, torch.zeros(len(x), dtype=torch.int64, device=self.device)), self._dataset, train=False)
        return self(x).float().argmax(1)


def main():
    return KubeResnet50(resnet50(1000), ImageNetStoredLarger()).start()
