"""RandomResizedCrop / Resize + CenterCrop without a GPU: the crop geometry, the numpy transforms,
``prepare`` on CPU tensors, argument validation, the sampling twin the GPU plan is compared with,
and the written-out tap rule against torch's antialiased bilinear filter."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kubeml_amd.data import transforms as T
from kubeml_amd.ops.kernels import resize_geometry
from kubeml_amd.sdk.vision import ImageDataset, prepare

AA = dict(mode="bilinear", antialias=True, align_corners=False)


@pytest.mark.parametrize("args,want", [((40, 48, 36, 32), (36, 43, 2, 6)), ((48, 40, 36, 32), (43, 36, 6, 2)),
                                       ((256, 256, 256, 224), (256, 256, 16, 16)),
                                       ((500, 375, 256, 224), (341, 256, 58, 16)), ((64, 64, 37, 32), (37, 37, 2, 2))])
def test_resize_geometry_table(args, want):
    assert resize_geometry(*args) == want


def test_resize_geometry_rejects_a_crop_larger_than_the_resized_image():
    with pytest.raises(ValueError):
        resize_geometry(40, 48, 30, 32)
    with pytest.raises(ValueError):
        resize_geometry(40, 48, 36, (32, 44))
    assert resize_geometry(40, 48, 36, (32, 43)) == (36, 43, 2, 0)


# ---------------------------------------------------------------------------------------
# the tap rule
# ---------------------------------------------------------------------------------------

def _axis_matrix(n_in, n_out):
    """[n_out, n_in] fp64 weights of the rule, written out."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for o in range(n_out):
        centre = scale * (o + 0.5)
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((k - centre + 0.5) / support)) for k in range(lo, hi)]
        m[o, lo:hi] = torch.tensor(w, dtype=torch.float64) / sum(w)
    return m


@pytest.mark.parametrize("src,dst", [((40, 48), (32, 24)), ((20, 20), (32, 32)), ((64, 64), (8, 8)),
                                     ((40, 48), (36, 43)), ((48, 40), (43, 36))])
def test_written_out_tap_rule_is_torchs_antialiased_bilinear(src, dst):
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x = torch.randint(0, 256, (2, 3) + src, generator=g).double()
    want = F.interpolate(x, size=dst, **AA)
    got = torch.einsum("yh,bchw,xw->bcyx", _axis_matrix(src[0], dst[0]), x, _axis_matrix(src[1], dst[1]))
    err = float((got - want).abs().max())
    print(f"{src} -> {dst}: max |twin - torch| = {err:.3e}")
    assert err <= 1e-12 * 255


# ---------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------

def _img(H, W, C=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


def _ref_u8(a, size):
    t = torch.from_numpy(a).permute(2, 0, 1)[None].double()
    return F.interpolate(t, size=size, **AA)[0].permute(1, 2, 0)


def test_resize_and_center_crop():
    a = _img(40, 48)
    r = T.Resize(36)(a)
    assert r.shape == (36, 43, 3) and r.dtype == np.uint8
    assert float((torch.from_numpy(r).double() - _ref_u8(a, (36, 43))).abs().max()) <= 1.0
    assert T.Resize(36)(np.ascontiguousarray(a.transpose(1, 0, 2))).shape == (43, 36, 3)
    assert T.Resize((10, 12))(a).shape == (10, 12, 3)
    assert T.Resize(20)(a[:, :, 0]).shape == (20, 24)
    c = T.CenterCrop(32)(r)
    Rh, Rw, oy, ox = resize_geometry(40, 48, 36, 32)
    assert np.array_equal(c, r[oy:oy + 32, ox:ox + 32])
    with pytest.raises(ValueError):
        T.CenterCrop(37)(r)
    t = T.Compose([T.Resize(36), T.CenterCrop(32), T.ToTensor()])(a)
    assert t.shape == (3, 32, 32) and t.dtype == torch.float32 and 0.0 <= float(t.min()) and float(t.max()) <= 1.0


def test_random_resized_crop_parameters_and_values():
    random.seed(11)
    tr = T.RandomResizedCrop(24)
    H, W = 40, 48
    seen = set()
    for _ in range(200):
        i, j, h, w = tr.get_params(H, W)
        seen.add((i, j, h, w))
        assert 0 <= i and i + h <= H and 0 <= j and j + w <= W and h >= 1 and w >= 1
        assert 0.08 * H * W - (w + h) / 2 - 1 <= w * h <= H * W + (w + h) / 2 + 1
        assert (w - 0.5) / (h + 0.5) <= 4 / 3 * (1 + 1e-9) and (w + 0.5) / (h - 0.5) >= 3 / 4 * (1 - 1e-9)
    assert len(seen) > 150
    a = _img(H, W, seed=3)
    random.seed(5)
    i, j, h, w = tr.get_params(H, W)
    random.seed(5)
    out = tr(a)
    assert out.shape == (24, 24, 3) and out.dtype == np.uint8
    ref = _ref_u8(np.ascontiguousarray(a[i:i + h, j:j + w]), (24, 24))
    assert float((torch.from_numpy(out).double() - ref).abs().max()) <= 1.0
    # ten rejections: the central crop at the nearest allowed ratio
    assert T.RandomResizedCrop(8, scale=(1, 1), ratio=(2, 2)).get_params(32, 32) == (8, 0, 16, 32)
    assert T.RandomResizedCrop(8, scale=(1, 1), ratio=(0.5, 0.5)).get_params(32, 32) == (0, 8, 32, 16)
    for bad in (dict(scale=(0, 1)), dict(ratio=(2, 1)), dict(scale=(0.5, 0.2))):
        with pytest.raises(ValueError):
            T.RandomResizedCrop(8, **bad)


# ---------------------------------------------------------------------------------------
# ImageDataset / prepare on CPU tensors
# ---------------------------------------------------------------------------------------

@pytest.fixture
def image_dataset(tmp_path):
    """ImageDataset factory over a tiny shard store."""
    from kubeml_amd.sdk.context import TaskContext, reset_task, set_task
    from kubeml_amd.store.shards import ShardStore
    rng = np.random.default_rng(0)
    st = ShardStore(str(tmp_path))
    x = rng.integers(0, 256, (16, 40, 48, 3), dtype=np.uint8)
    y = rng.integers(0, 10, 16).astype(np.int64)
    st.create("tiny", x, y, x[:8], y[:8])
    tok = set_task(TaskContext(store=st))
    try:
        yield lambda **kw: ImageDataset("tiny", **kw)
    finally:
        reset_task(tok)


def _batch(B=6, H=40, W=48, C=3):
    g = torch.Generator().manual_seed(B)
    return torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=g), torch.arange(B) + 10


def test_prepare_cpu_shapes_eval_determinism_and_mixing(image_dataset):
    ds = image_dataset(random_resized_crop=32)
    assert ds.rrc_size == (32, 32) and ds.eval_resize == 37
    ds.eval_resize = 36
    x, y = _batch()
    torch.manual_seed(0)
    xt, yt = prepare((x, y), ds, True)
    assert xt.shape == (6, 3, 32, 32) and xt.dtype == torch.float32 and torch.equal(yt, y)
    xe, ye = prepare((x, y), ds, False)
    xe2, _ = prepare((x, y), ds, False)
    assert xe.shape == (6, 3, 32, 32) and torch.equal(xe, xe2) and torch.equal(ye, y)
    Rh, Rw, oy, ox = resize_geometry(40, 48, 36, 32)
    ref = F.interpolate(x.permute(0, 3, 1, 2).double(), size=(Rh, Rw), **AA)[:, :, oy:oy + 32, ox:ox + 32] / 255.0
    mean = torch.tensor(ds.mean, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(ds.std, dtype=torch.float64).view(1, 3, 1, 1)
    assert float((xe.double() - (ref - mean) / std).abs().max()) < 1e-4
    dm = image_dataset(random_resized_crop=(32, 24), mixup_alpha=1.0)
    xm, tm = prepare((x, y), dm, True)
    assert xm.shape == (6, 3, 32, 24) and tm.shape == (6, 3) and tm.dtype == torch.float32
    assert torch.equal(tm[:, 0], y.float()) and 0.0 <= float(tm[0, 2]) <= 1.0
    _, ym = prepare((x, y), dm, False)
    assert torch.equal(ym, y)                                    # validation batches are never mixed
    # without random_resized_crop nothing changes: the stored size goes through
    xo, _ = prepare((x, y), image_dataset(crop_pad=0, flip=False), True)
    assert xo.shape == (6, 3, 40, 48)


@pytest.mark.parametrize("bad", [dict(rrc_scale=(0.0, 1.0)), dict(rrc_scale=(0.5, 0.2)), dict(rrc_ratio=(2.0, 1.0)),
                                 dict(rrc_ratio=(0.0, 1.0)), dict(eval_resize=0), dict(eval_resize=36.5),
                                 dict(random_resized_crop=0), dict(random_resized_crop=(32, 32, 3))])
def test_image_dataset_argument_validation(image_dataset, bad):
    kw = dict(random_resized_crop=32)
    kw.update(bad)
    with pytest.raises(ValueError):
        image_dataset(**kw)


def test_image_dataset_defaults_stay_off(image_dataset):
    ds = image_dataset()
    assert ds.rrc_size is None
    assert image_dataset(random_resized_crop=224).eval_resize == 256


# ---------------------------------------------------------------------------------------
# the sampling twin of the device plan
# ---------------------------------------------------------------------------------------

def area_shares(n, seed, Hs=256, Ws=256, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """Sorted area shares w * h / (Hs * Ws) of n float64 draws of torchvision's get_params with
    Python's RNG."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        _, _, h, w = T.rrc_params(Hs, Ws, scale, ratio, rng.uniform, rng.randrange)
        out.append(w * h / (Hs * Ws))
    return sorted(out)


def cdf_sup_distance(a, b):
    """sup |F_a - F_b| of two sorted samples."""
    a, b = np.asarray(a), np.asarray(b)
    pts = np.concatenate([a, b])
    fa = np.searchsorted(a, pts, side="right") / len(a)
    fb = np.searchsorted(b, pts, side="right") / len(b)
    return float(np.abs(fa - fb).max())


def dkw_bound(n, m, p=1e-6):
    """Dvoretzky-Kiefer-Wolfowitz: each empirical CDF is within sqrt(ln(2 / p) / (2 n)) of the true
    one except with probability p."""
    return math.sqrt(math.log(2 / p) / (2 * n)) + math.sqrt(math.log(2 / p) / (2 * m))


def test_twin_against_twin_stays_inside_the_dkw_bound():
    d = cdf_sup_distance(area_shares(8192, 1), area_shares(65536, 2))
    bound = dkw_bound(8192, 65536)
    print(f"twin vs twin sup-distance {d:.4f}, bound {bound:.4f}")
    assert abs(bound - 0.0398) < 1e-3
    assert d <= bound
