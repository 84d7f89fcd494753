"""Image-classification helpers for user functions (CIFAR/MNIST-style datasets).

The reference's CIFAR functions run torchvision transforms per sample in a
``DataLoader`` (function_resnet34.py:17-44).  On MI355X that host path would cap a
worker far below the GPU's rate, so :class:`ImageDataset` hands whole uint8 batches
to the device (``collate_batch``) and :func:`prepare` runs the fused augmentation
kernel there (random crop with zero padding, horizontal flip, normalisation, NHWC
bf16 with channels padded to 8).  On CPU workers the same code falls back to the
numpy/torch transforms with identical semantics, so functions stay portable.
A dataset stored larger than the network's input (ImageNet) sets ``random_resized_crop``:
RandomResizedCrop for training and Resize + CenterCrop for validation, also one launch.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np
import torch

from .dataset import KubeDataset

CIFAR10_MEAN, CIFAR10_STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class ImageDataset(KubeDataset):
    """uint8 ``[N, H, W, C]`` images + integer labels; batches are ``(uint8 tensor, int64 labels)``.

    ``mixup_alpha`` / ``cutmix_alpha`` > 0 switch on mixup / CutMix for training batches:
    :func:`prepare` then mixes every sample with another row of the batch (one ``lam ~
    Beta(alpha, alpha)`` per step) and returns packed fp32 ``[B, 3]`` targets ``(label, partner
    label, lam)`` that ``cross_entropy`` / ``CrossEntropyLoss`` accept.  ``mix_prob``: the
    probability that a step mixes at all; ``switch_prob``: the share of CutMix steps when both
    alphas are set.

    ``random_resized_crop`` (an int or ``(H, W)``; ``None`` leaves everything as above) stores
    the images at one size and feeds the network another, the ImageNet recipe: training batches
    are ``RandomResizedCrop(size, rrc_scale, rrc_ratio)`` + flip, validation batches
    ``Resize(eval_resize)`` + ``CenterCrop(size)`` with ``eval_resize`` defaulting to
    ``round(size / 0.875)`` (256 for 224; the larger side of a pair).  Both use torch's antialiased
    bilinear filter (``F.interpolate(..., antialias=True)``, PIL's) on the crop, "crop, then
    resize"; on the GPU the raw values are resampled in fp32 and rounded once, to bf16, with no
    rounding to uint8 in between as PIL has.  ``crop_pad`` is ignored then."""

    def __init__(self, dataset: str, mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 crop_pad: int = 4, flip: bool = True, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
                 mix_prob: float = 1.0, switch_prob: float = 0.5, random_resized_crop=None,
                 rrc_scale: Sequence[float] = (0.08, 1.0), rrc_ratio: Sequence[float] = (3.0 / 4.0, 4.0 / 3.0),
                 eval_resize=None):
        super().__init__(dataset)
        self.mean, self.std = tuple(mean), tuple(std)
        self.crop_pad, self.flip = crop_pad, flip
        if mixup_alpha < 0 or cutmix_alpha < 0 or not 0 <= mix_prob <= 1 or not 0 <= switch_prob <= 1:
            raise ValueError("mixup_alpha / cutmix_alpha must be >= 0, mix_prob / switch_prob in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(mix_prob), float(switch_prob)
        self.rrc_size = None
        self.rrc_scale, self.rrc_ratio = tuple(float(v) for v in rrc_scale), tuple(float(v) for v in rrc_ratio)
        self.eval_resize = eval_resize
        if random_resized_crop is not None:
            hw = (random_resized_crop,) * 2 if isinstance(random_resized_crop, int) else tuple(random_resized_crop)
            if len(hw) != 2 or not all(isinstance(v, int) and v >= 1 for v in hw):
                raise ValueError(f"random_resized_crop must be a positive int or (H, W), got {random_resized_crop!r}")
            if len(self.rrc_scale) != 2 or not 0 < self.rrc_scale[0] <= self.rrc_scale[1] < float("inf"):
                raise ValueError(f"rrc_scale must be a range 0 < s0 <= s1, got {tuple(rrc_scale)}")
            if len(self.rrc_ratio) != 2 or not 0 < self.rrc_ratio[0] <= self.rrc_ratio[1] < float("inf"):
                raise ValueError(f"rrc_ratio must be a range 0 < r0 <= r1, got {tuple(rrc_ratio)}")
            if eval_resize is None:
                self.eval_resize = int(round(max(hw) / 0.875))
            elif not isinstance(eval_resize, int) or eval_resize < 1:
                raise ValueError(f"eval_resize must be a positive int, got {eval_resize!r}")
            self.rrc_size = hw

    @property
    def mixes(self) -> bool:
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    def collate_batch(self, data: np.ndarray, labels: np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(data))
        if x.dim() == 3:  # [N, H, W] grayscale
            x = x.unsqueeze(-1)
        y = torch.from_numpy(np.ascontiguousarray(labels).reshape(-1).astype(np.int64))
        return x, y

    def __getitem__(self, i):
        return self.data[i], int(self.labels[i])

    def __len__(self):
        return len(self.data) if self.data is not None else 0


_CTRS = {}


def prepare(batch: Tuple[torch.Tensor, torch.Tensor], ds: ImageDataset, train: bool, seed: int = 0):
    """Device batch → (model input, labels).  GPU: one fused augment kernel launch;
    CPU: the same ops in torch (NCHW float32).  A training batch of a dataset with mixup /
    CutMix switched on comes back mixed, with packed fp32 ``[B, 3]`` targets in place of the
    labels (see :class:`ImageDataset`); validation batches are never mixed.  A dataset with
    ``random_resized_crop`` set goes through the resample launch instead (RandomResizedCrop for
    training, Resize + CenterCrop for validation batches); its ``crop_pad`` is not used."""
    x, y = batch
    mix = train and getattr(ds, "mixes", False)
    rrc = getattr(ds, "rrc_size", None)
    if x.is_cuda:
        from ..ops import kernels as K
        key = (x.device, seed)
        ctr = _CTRS.get(key)
        if ctr is None:
            ctr = torch.tensor([float(seed), 0.0, 0.0], dtype=torch.float32, device=x.device)
            _CTRS[key] = ctr
        if x.dtype != torch.uint8:
            raise TypeError("GPU augmentation expects uint8 images")
        B = x.shape[0]
        if rrc is not None:
            m = dict(mixup_alpha=ds.mixup_alpha, cutmix_alpha=ds.cutmix_alpha, mix_prob=ds.mix_prob,
                     switch_prob=ds.switch_prob) if mix else {}
            xb, yb = K.augment_resample(x.contiguous(), y.contiguous(), ctr, B, rrc, train=train, flip=ds.flip,
                                        scale=ds.rrc_scale, ratio=ds.rrc_ratio, resize=ds.eval_resize, mean=ds.mean,
                                        std=ds.std, **m)
            K.advance_counter_(ctr, B, B)
            return xb, yb
        if mix:
            xb, tb = K.augment_mix(x.contiguous(), y.contiguous(), ctr, B, pad=ds.crop_pad, flip=ds.flip, train=True,
                                   mean=ds.mean, std=ds.std, mixup_alpha=ds.mixup_alpha,
                                   cutmix_alpha=ds.cutmix_alpha, mix_prob=ds.mix_prob, switch_prob=ds.switch_prob)
            K.advance_counter_(ctr, B, B)
            return xb, tb
        xb, yb = K.augment(x.contiguous(), y.contiguous(), ctr, B, pad=ds.crop_pad if train else 0,
                           flip=ds.flip and train, train=train, mean=ds.mean, std=ds.std)
        K.advance_counter_(ctr, B, B)
        return xb, yb
    xf = x.permute(0, 3, 1, 2).float()
    if rrc is not None:
        xf = _resample_cpu(xf, ds, train)
    xf = xf.div_(255.0)
    if train and rrc is None:
        p = ds.crop_pad
        if p:
            B, C, H, W = xf.shape
            xp = torch.nn.functional.pad(xf, (p, p, p, p))
            ii = torch.randint(0, 2 * p + 1, (B,))
            jj = torch.randint(0, 2 * p + 1, (B,))
            xf = torch.stack([xp[b, :, ii[b]:ii[b] + H, jj[b]:jj[b] + W] for b in range(B)])
        if ds.flip:
            m = torch.rand(xf.shape[0]) < 0.5
            xf[m] = xf[m].flip(-1)
    mean = torch.tensor(ds.mean[: xf.shape[1]]).view(1, -1, 1, 1)
    std = torch.tensor(ds.std[: xf.shape[1]]).view(1, -1, 1, 1)
    xn = (xf - mean) / std
    return _mix_cpu(xn, y, ds) if mix else (xn, y)


def _resample_cpu(xf, ds: ImageDataset, train: bool):
    """The resample launch in stock torch on an NCHW fp32 batch of raw values: boxes and flips
    from torch's RNG, ``F.interpolate(..., antialias=True)`` on each crop (training), or the
    whole image resized and its centre window (validation)."""
    from ..data.transforms import rrc_params
    from ..ops.kernels import resize_geometry
    Ho, Wo = ds.rrc_size
    B, _, Hs, Ws = xf.shape
    kw = dict(mode="bilinear", antialias=True, align_corners=False)
    if not train:
        Rh, Rw, oy, ox = resize_geometry(Hs, Ws, ds.eval_resize, (Ho, Wo))
        return torch.nn.functional.interpolate(xf, size=(Rh, Rw), **kw)[:, :, oy:oy + Ho, ox:ox + Wo].contiguous()
    uniform = lambda a, b: a + (b - a) * float(torch.rand(()))
    randint = lambda n: int(torch.randint(0, n, ()))
    out = []
    for b in range(B):
        i, j, h, w = rrc_params(Hs, Ws, ds.rrc_scale, ds.rrc_ratio, uniform, randint)
        o = torch.nn.functional.interpolate(xf[b:b + 1, :, i:i + h, j:j + w], size=(Ho, Wo), **kw)
        out.append(o.flip(-1) if ds.flip and float(torch.rand(())) < 0.5 else o)
    return torch.cat(out)


def _mix_cpu(x, y, ds: ImageDataset):
    """mixup / CutMix of a normalised NCHW batch in torch ops (torch's RNG): the plan of the
    GPU kernel — one lam, one partner shift and one box per step."""
    B, _, H, W = x.shape
    yf = y.float()
    lam, r = 1.0, 0
    if B > 1:
        r = 1 + int(torch.randint(0, B - 1, ()))
        if float(torch.rand(())) < ds.mix_prob:
            cut = ds.cutmix_alpha > 0 and (ds.mixup_alpha <= 0 or float(torch.rand(())) < ds.switch_prob)
            alpha = ds.cutmix_alpha if cut else ds.mixup_alpha
            lam = float(torch.distributions.Beta(alpha, alpha).sample())
            xp = x.roll(-r, 0)           # row b's partner is row (b + r) % B
            if cut:
                ratio = (1.0 - lam) ** 0.5
                cw, ch = int(W * ratio), int(H * ratio)
                cx, cy = int(torch.randint(0, W, ())), int(torch.randint(0, H, ()))
                x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, W)
                y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, H)
                x = x.clone()
                x[:, :, y0:y1, x0:x1] = xp[:, :, y0:y1, x0:x1]
                lam = 1.0 - (x1 - x0) * (y1 - y0) / (H * W)
            else:
                x = lam * x + (1.0 - lam) * xp
    return x, torch.stack([yf, yf.roll(-r, 0), torch.full_like(yf, lam)], 1)
