"""The torchvision transforms the reference's functions use, without torchvision
(not available on the target image): ``Compose``, ``ToTensor``, ``Normalize``,
``RandomHorizontalFlip``, ``RandomCrop(size, padding)``, ``ToPILImage`` (identity on
arrays), and the ImageNet chain ``RandomResizedCrop(size, scale, ratio)``, ``Resize(size)``,
``CenterCrop(size)``.  Semantics follow torchvision on HWC uint8 numpy input
(function_lenet.py:57-60, function_resnet34.py:17-30).

These are the per-sample CPU path (CPU workers, parity tests).  The GPU path for the
CIFAR functions is the fused on-device ``kml_augment`` kernel
(:func:`kubeml_amd.ops.kernels.augment`) fed by ``KubeDataset.collate_batch``; for the
ImageNet chain it is ``kml_augment_resample`` (:func:`kubeml_amd.ops.kernels.augment_resample`).
"""
from __future__ import annotations

import math
import random
from typing import Sequence

import numpy as np
import torch


class Compose:
    def __init__(self, ts):
        self.ts = list(ts)

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class ToPILImage:
    """Identity on HWC arrays (the pipeline stays in numpy)."""

    def __call__(self, x):
        return np.asarray(x)


class ToTensor:
    """HWC (or HW) uint8 → CHW float in [0, 1]; float arrays are not rescaled."""

    def __call__(self, x):
        if isinstance(x, torch.Tensor):
            return x
        a = np.asarray(x)
        if a.ndim == 2:
            a = a[:, :, None]
        t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
        if a.dtype == np.uint8:
            return t.float().div_(255.0)
        return t.float()


class Normalize:
    def __init__(self, mean: Sequence[float], std: Sequence[float]):
        self.mean = torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)

    def __call__(self, t: torch.Tensor):
        return (t - self.mean) / self.std


class RandomHorizontalFlip:
    def __init__(self, p: float = 0.5):
        self.p = p

    def __call__(self, x):
        if random.random() < self.p:
            if isinstance(x, torch.Tensor):
                return x.flip(-1)
            return np.ascontiguousarray(np.asarray(x)[:, ::-1])
        return x


class RandomCrop:
    def __init__(self, size, padding: int = 0):
        self.size = (size, size) if isinstance(size, int) else tuple(size)
        self.padding = padding

    def __call__(self, x):
        a = np.asarray(x)
        p = self.padding
        if p:
            pad = ((p, p), (p, p)) + (((0, 0),) if a.ndim == 3 else ())
            a = np.pad(a, pad)
        h, w = a.shape[:2]
        th, tw = self.size
        i = random.randint(0, h - th)
        j = random.randint(0, w - tw)
        return a[i:i + th, j:j + tw]


def _size(size):
    hw = (size, size) if isinstance(size, int) else tuple(size)
    if len(hw) != 2 or not all(isinstance(v, int) and v >= 1 for v in hw):
        raise ValueError(f"size must be a positive int or (h, w), got {size!r}")
    return hw


def _resize(a: np.ndarray, size) -> np.ndarray:
    """HWC (or HW) uint8 -> ``size`` with the antialiased bilinear filter PIL uses (torch's
    ``F.interpolate(mode="bilinear", antialias=True)``), rounded to the nearest uint8 as PIL does."""
    a = np.asarray(a)
    t = torch.from_numpy(np.ascontiguousarray(a if a.ndim == 3 else a[:, :, None])).permute(2, 0, 1)[None].float()
    o = torch.nn.functional.interpolate(t, size=tuple(size), mode="bilinear", antialias=True, align_corners=False)
    o = o.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0).numpy()
    return o if a.ndim == 3 else o[:, :, 0]


def rrc_params(Hs: int, Ws: int, scale, ratio, uniform, randint):
    """torchvision's ``RandomResizedCrop.get_params`` as ``(i, j, h, w)`` over an ``Hs x Ws`` image,
    drawing from ``uniform(a, b)`` and ``randint(n)`` (an integer in ``[0, n)``): up to ten tries
    of an area share and a log-uniform aspect ratio, then the central crop at the nearest
    allowed ratio."""
    area = Hs * Ws
    lr0, lr1 = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * uniform(scale[0], scale[1])
        r = math.exp(uniform(lr0, lr1))
        w, h = int(round(math.sqrt(target * r))), int(round(math.sqrt(target / r)))
        if 0 < w <= Ws and 0 < h <= Hs:
            return randint(Hs - h + 1), randint(Ws - w + 1), h, w
    in_ratio = Ws / Hs
    w, h = Ws, Hs
    if in_ratio < ratio[0]:
        h = min(max(int(round(Ws / ratio[0])), 1), Hs)
    elif in_ratio > ratio[1]:
        w = min(max(int(round(Hs * ratio[1])), 1), Ws)
    return (Hs - h) // 2, (Ws - w) // 2, h, w


class RandomResizedCrop:
    """A random box of ``scale`` of the area and a log-uniform aspect ratio in ``ratio`` (ten
    tries, then the central crop at the nearest allowed ratio: torchvision's ``get_params``),
    resized to ``size``."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.size = _size(size)
        self.scale, self.ratio = tuple(float(v) for v in scale), tuple(float(v) for v in ratio)
        if not 0 < self.scale[0] <= self.scale[1] or not 0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError(f"scale {tuple(scale)} and ratio {tuple(ratio)} must be ranges 0 < lo <= hi")

    def get_params(self, H: int, W: int):
        """``(i, j, h, w)``: the box ``[i, i + h) x [j, j + w)`` of an ``H x W`` image."""
        return rrc_params(H, W, self.scale, self.ratio, random.uniform, random.randrange)

    def __call__(self, x):
        a = np.asarray(x)
        i, j, h, w = self.get_params(*a.shape[:2])
        return _resize(a[i:i + h, j:j + w], self.size)


class Resize:
    """An int: the shorter side becomes ``size`` and the other ``int(size * long / short)``;
    a pair: exactly ``(h, w)``."""

    def __init__(self, size):
        self.size = size if isinstance(size, int) else _size(size)
        if isinstance(size, int) and size < 1:
            raise ValueError(f"size must be positive, got {size}")

    def __call__(self, x):
        a = np.asarray(x)
        H, W = a.shape[:2]
        if not isinstance(self.size, int):
            return _resize(a, self.size)
        s = self.size
        return _resize(a, (int(s * H / W), s) if W <= H else (s, int(s * W / H)))


class CenterCrop:
    """The central ``size`` window, from ``int(round((H - h) / 2.0))``; a smaller image is an
    error (torchvision would pad)."""

    def __init__(self, size):
        self.size = _size(size)

    def __call__(self, x):
        a = np.asarray(x)
        H, W = a.shape[:2]
        h, w = self.size
        if h > H or w > W:
            raise ValueError(f"CenterCrop {h} x {w} of a {H} x {W} image")
        i, j = int(round((H - h) / 2.0)), int(round((W - w) / 2.0))
        return a[i:i + h, j:j + w]
