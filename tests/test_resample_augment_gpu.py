"""RandomResizedCrop and Resize + CenterCrop inside the augment launch, on the MI355X: the
resampled pixels against torch's antialiased bilinear filter in fp64 on the boxes the plan
read-back reports, the plan against torchvision's rules, mixing against the plain batch at the same
counters, graph replay, and ``prepare``.  Sources are uint8 noise: a misplaced tap is an error of
order 1."""
import functools
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
BF16 = torch.bfloat16
AA = dict(mode="bilinear", antialias=True, align_corners=False)
MEANS = {1: ((0.5,), (0.25,)), 3: ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
         4: ((0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25))}
N = 16


@functools.lru_cache(maxsize=None)
def _source(Hs, Ws, C):
    """(uint8 source on the device, the same on the host, labels): made once, never written to."""
    g = torch.Generator().manual_seed(Hs * 1000 + Ws * 10 + C)
    src = torch.randint(0, 256, (N, Hs, Ws, C), dtype=torch.uint8, generator=g)
    labels = torch.randperm(N, generator=g) + 100
    return src.to(dev), src, labels.to(dev)


def _ctr(seed=7.0, step=3.0, start=12.0):
    return torch.tensor([seed, step, start], dtype=torch.float32, device=dev)


def _normalise(r, C):
    """[C, H, W] fp64 raw values -> normalised [H, W, C]."""
    mean, std = (torch.tensor(v, dtype=torch.float64).view(C, 1, 1) for v in MEANS[C])
    return ((r / 255.0 - mean) / std).permute(1, 2, 0)


def _check(out, refs, extents, C, what):
    """|out - ref| <= 2^-8 |ref| + 2^-18 max(h, w) per element: half a bf16 ulp, plus the fp32
    rounding of the tap centres and weights (about three roundings of 2^-24 relative on a
    coordinate up to max(h, w), times the normalised value range and two axes).  Pad channels
    are exactly 0."""
    out = out.cpu()
    worst = 0.0
    for b, (ref, ext) in enumerate(zip(refs, extents)):
        err = (out[b, :, :, :C].double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -18 * ext
        worst = max(worst, float((err / bound).max()))
    print(f"{what}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    if out.shape[-1] > C:
        assert float(out[..., C:].float().abs().max()) == 0.0


def _train_refs(src_cpu, plan, start, size, C):
    """fp64 references of a train batch from the plan's rows [B, 6]."""
    refs, extents = [], []
    for b, row in enumerate(plan.tolist()):
        i, j, h, w, flip = (int(v) for v in row[:5])
        crop = src_cpu[(start + b) % N, i:i + h, j:j + w].permute(2, 0, 1)[None].double()
        r = F.interpolate(crop, size=size, **AA)[0]
        refs.append(_normalise(r.flip(-1) if flip else r, C))
        extents.append(max(h, w))
    return refs, extents


TRAIN_CASES = {
    "40x48-32x24-C3": dict(Hs=40, Ws=48, size=(32, 24), C=3),
    "40x48-32x24-C1": dict(Hs=40, Ws=48, size=(32, 24), C=1),
    "40x48-32x24-C4": dict(Hs=40, Ws=48, size=(32, 24), C=4),
    "upscale-20x20-32x32": dict(Hs=20, Ws=20, size=(32, 32), C=3),
    "downscale-64x64-8x8-whole": dict(Hs=64, Ws=64, size=(8, 8), C=3, scale=(1.0, 1.0), ratio=(1.0, 1.0)),
    "two-column-tiles-6x300-5x260": dict(Hs=6, Ws=300, size=(5, 260), C=3),
}


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_train_resampling_against_torch(case):
    from kubeml_amd.ops import kernels as K
    c = dict(TRAIN_CASES[case])
    Hs, Ws, size, C = c.pop("Hs"), c.pop("Ws"), c.pop("size"), c.pop("C")
    src, src_cpu, labels = _source(Hs, Ws, C)
    B, ctr = 8, _ctr()
    mean, std = MEANS[C]
    plan = K.rrc_plan(ctr, 1, B, Hs, Ws, N=N, **c)[0].cpu()
    out, lab = K.augment_resample(src, labels, ctr, B, size, mean=mean, std=std, **c)
    assert out.shape == (B,) + size + (8,) and out.dtype == BF16
    assert torch.equal(ctr.cpu(), torch.tensor([7.0, 3.0, 12.0]))            # the counter is only read
    if "scale" in c:
        assert torch.equal(plan[:, :4], torch.tensor([0.0, 0.0, Hs, Ws]).expand(B, 4))
    refs, extents = _train_refs(src_cpu, plan, 12, size, C)
    _check(out, refs, extents, C, case)
    sidx = (12 + torch.arange(B, device=dev)) % N
    assert lab.dtype == torch.int64 and torch.equal(lab, labels[sidx])


def _eval_refs(src_cpu, start, B, resize, crop, C):
    from kubeml_amd.ops.kernels import resize_geometry
    _, Hs, Ws, _ = src_cpu.shape
    Rh, Rw, oy, ox = resize_geometry(Hs, Ws, resize, crop)
    refs = []
    for b in range(B):
        whole = F.interpolate(src_cpu[(start + b) % N].permute(2, 0, 1)[None].double(), size=(Rh, Rw), **AA)[0]
        refs.append(_normalise(whole[:, oy:oy + crop, ox:ox + crop], C))
    return refs, [max(Hs, Ws)] * B


@pytest.mark.parametrize("Hs,Ws", [(40, 48), (48, 40)])
def test_eval_resize_center_crop(Hs, Ws):
    from kubeml_amd.ops import kernels as K
    src, src_cpu, labels = _source(Hs, Ws, 3)
    B = 8
    out, lab = K.augment_resample(src, labels, _ctr(step=3.0), B, 32, train=False, resize=36)
    refs, extents = _eval_refs(src_cpu, 12, B, 36, 32, 3)
    _check(out, refs, extents, 3, f"eval {Hs}x{Ws}")
    assert torch.equal(lab, labels[(12 + torch.arange(B, device=dev)) % N])
    again, _ = K.augment_resample(src, labels, _ctr(step=9.0), B, 32, train=False, resize=36)
    assert torch.equal(out, again)                                           # no randomness is read


def test_plan_invariants():
    from kubeml_amd.ops import kernels as K
    Hs, Ws, n, B = 40, 48, 16, 64
    s0, s1, r0, r1 = 0.08, 1.0, 3 / 4, 4 / 3
    p = K.rrc_plan(_ctr(), n, B, Hs, Ws)
    assert p.shape == (n, B, 6) and p.dtype == torch.float32
    assert torch.equal(p, K.rrc_plan(_ctr(), n, B, Hs, Ws))                  # a function of the counters
    p = p.cpu().double()
    i, j, h, w, flip, fb = (p[..., k] for k in range(6))
    assert bool((p == p.round()).all())
    assert bool(((i >= 0) & (j >= 0) & (h >= 1) & (w >= 1) & (i + h <= Hs) & (j + w <= Ws)).all())
    ok = fb == 0
    print(f"fallback rows {int((~ok).sum())} of {n * B}")
    area = w * h
    assert bool((area >= s0 * Hs * Ws - (w + h) / 2 - 1)[ok].all())
    assert bool((area <= s1 * Hs * Ws + (w + h) / 2 + 1)[ok].all())
    assert bool(((w - 0.5) / (h + 0.5) <= r1 * (1 + 1e-5)).all())
    assert bool(((w + 0.5) / (h - 0.5) >= r0 * (1 - 1e-5)).all())
    assert bool(((flip == 0) | (flip == 1)).all()) and 0 < int(flip.sum()) < n * B
    boxes = p[..., :4]
    assert len({tuple(r) for r in boxes[0].tolist()}) > B // 2               # between samples
    assert len({tuple(r) for r in boxes[:, 0].tolist()}) > n // 2            # between steps
    assert float(K.rrc_plan(_ctr(), n, B, Hs, Ws, flip=False)[..., 4].abs().max()) == 0.0
    assert torch.equal(K.rrc_plan(_ctr(), n, B, Hs, Ws, flip=False)[..., :4].cpu().double(), boxes)


@pytest.mark.parametrize("ratio,box", [((2.0, 2.0), (8, 0, 16, 32)), ((0.5, 0.5), (0, 8, 32, 16))])
def test_fallback_is_the_central_crop(ratio, box):
    from kubeml_amd.ops import kernels as K
    p = K.rrc_plan(_ctr(), 4, 16, 32, 32, scale=(1.0, 1.0), ratio=ratio).cpu()
    assert torch.equal(p[..., :4], torch.tensor(box, dtype=torch.float32).expand(4, 16, 4))
    assert bool((p[..., 5] == 1).all())


def test_a_samples_view_does_not_depend_on_its_batch_position():
    from kubeml_amd.ops import kernels as K
    src, _, labels = _source(40, 48, 3)
    a, la = K.augment_resample(src, labels, _ctr(start=0.0), 8, (32, 24))
    b, lb = K.augment_resample(src, labels, _ctr(start=4.0), 4, (32, 24))
    assert torch.equal(a[4:8], b) and torch.equal(la[4:8], lb)
    pa = K.rrc_plan(_ctr(start=0.0), 1, 8, 40, 48, N=N)
    pb = K.rrc_plan(_ctr(start=4.0), 1, 4, 40, 48, N=N)
    assert torch.equal(pa[0, 4:8], pb[0])


# ---------------------------------------------------------------------------------------
# distribution of the plan: gross errors only
# ---------------------------------------------------------------------------------------

def _twin_area_shares(n, seed, Hs=256, Ws=256, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """Area shares of n float64 draws of torchvision's get_params with Python's RNG."""
    from kubeml_amd.data.transforms import rrc_params
    rng = random.Random(seed)
    return sorted(h * w / (Hs * Ws) for _, _, h, w in
                  (rrc_params(Hs, Ws, scale, ratio, rng.uniform, rng.randrange) for _ in range(n)))


def test_plan_area_distribution_against_the_float64_twin():
    """sup-distance of the two empirical CDFs within the sum of the two DKW radii at failure
    probability 1e-6 each."""
    from kubeml_amd.ops import kernels as K
    p = K.rrc_plan(_ctr(), 128, 64, 256, 256).cpu().double().reshape(-1, 6)
    a = np.sort((p[:, 2] * p[:, 3] / (256 * 256)).numpy())
    b = np.asarray(_twin_area_shares(65536, 2))
    pts = np.concatenate([a, b])
    d = float(np.abs(np.searchsorted(a, pts, side="right") / len(a) -
                     np.searchsorted(b, pts, side="right") / len(b)).max())
    bound = math.sqrt(math.log(2e6) / (2 * 8192)) + math.sqrt(math.log(2e6) / (2 * 65536))
    print(f"device vs twin sup-distance {d:.4f}, bound {bound:.4f}, fallbacks {int(p[:, 5].sum())}")
    assert len(a) == 8192 and d <= bound


# ---------------------------------------------------------------------------------------
# mixing
# ---------------------------------------------------------------------------------------

def test_mixing_against_the_plain_batch():
    from kubeml_amd.ops import kernels as K
    src, _, labels = _source(40, 48, 3)
    B, ctr = 8, _ctr()
    A, lab = K.augment_resample(src, labels, ctr, B, 32)
    # both alphas 0: the plain batch and int64 labels
    Z, zl = K.augment_resample(src, labels, ctr, B, 32, mixup_alpha=0.0, cutmix_alpha=0.0)
    assert torch.equal(Z, A) and zl.dtype == torch.int64 and torch.equal(zl, lab)

    plan = K.mix_plan(ctr, 1, B, 32, 32, cutmix_alpha=1.0)[0]
    out, tgt = K.augment_resample(src, labels, ctr, B, 32, cutmix_alpha=1.0)
    assert int(plan[0]) == K.MIX_CUTMIX
    partner = (torch.arange(B, device=dev) + int(plan[1])) % B
    x0, y0, x1, y1 = (int(v) for v in plan[3:7])
    assert (x1 - x0) * (y1 - y0) > 0
    want = A.clone()
    want[:, y0:y1, x0:x1] = A[partner][:, y0:y1, x0:x1]
    assert torch.equal(out, want)
    assert tgt.dtype == torch.float32 and torch.equal(tgt[:, 0], lab.float())
    assert torch.equal(tgt[:, 1], lab[partner].float()) and torch.equal(tgt[:, 2], plan[2].expand(B))

    plan = K.mix_plan(ctr, 1, B, 32, 32, mixup_alpha=1.0)[0]
    out, tgt = K.augment_resample(src, labels, ctr, B, 32, mixup_alpha=1.0)
    assert int(plan[0]) == K.MIX_MIXUP and 0.0 < float(plan[2]) < 1.0
    partner = (torch.arange(B, device=dev) + int(plan[1])) % B
    lam = plan[2].cpu()
    om = torch.tensor(1.0) - lam                                             # fp32, as the kernel's
    # fmaf(lam, a, om * b): lam * a is exact in fp64, om * b is rounded to fp32 first, and the sum
    # is rounded once
    Af, Pf = A.cpu().float(), A[partner].cpu().float()
    want = (lam.double() * Af.double() + (om * Pf).double()).float().to(BF16)
    assert torch.equal(out.cpu(), want)
    assert not torch.equal(out, A)
    assert torch.equal(tgt[:, 0], lab.float()) and torch.equal(tgt[:, 1], lab[partner].float())
    assert torch.equal(tgt[:, 2], plan[2].expand(B))


# ---------------------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------------------

def test_a_captured_launch_draws_new_boxes_every_replay():
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.ops import kernels as K
    src, src_cpu, labels = _source(40, 48, 3)
    B, size = 8, (32, 24)
    start = torch.tensor([5.0, 0.0, 4.0], device=dev)
    ctr = start.clone()
    out = torch.empty((B,) + size + (8,), dtype=BF16, device=dev)
    lab = torch.empty((B,), dtype=torch.int64, device=dev)

    def body():
        K.augment_resample(src, labels, ctr, B, size, out=out, labels_out=lab)
        K.advance_counter_(ctr, B, N)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph):
        body()
    ctr.copy_(start)
    boxes = []
    for k in range(3):
        graph.replay()
        first = (4 + k * B) % N
        plan = K.rrc_plan(torch.tensor([5.0, float(k), float(first)], device=dev), 1, B, 40, 48, N=N)[0].cpu()
        refs, extents = _train_refs(src_cpu, plan, first, size, 3)
        _check(out.clone(), refs, extents, 3, f"replay {k}")
        assert torch.equal(lab, labels[(first + torch.arange(B, device=dev)) % N])
        boxes.append(plan[:, :4])
    assert not torch.equal(boxes[0], boxes[2])                               # the same samples, new boxes
    assert ctr.tolist() == [5.0, 3.0, float((4 + 3 * B) % N)]


# ---------------------------------------------------------------------------------------
# prepare
# ---------------------------------------------------------------------------------------

@pytest.fixture
def image_dataset(tmp_path):
    """ImageDataset factory over a tiny shard store."""
    from kubeml_amd.sdk.context import TaskContext, reset_task, set_task
    from kubeml_amd.sdk.vision import ImageDataset
    from kubeml_amd.store.shards import ShardStore
    rng = np.random.default_rng(0)
    st = ShardStore(str(tmp_path))
    x = rng.integers(0, 256, (16, 8, 8, 3), dtype=np.uint8)
    y = rng.integers(0, 10, 16).astype(np.int64)
    st.create("tiny", x, y, x[:8], y[:8])
    tok = set_task(TaskContext(store=st))
    try:
        yield lambda **kw: ImageDataset("tiny", **kw)
    finally:
        reset_task(tok)


def test_prepare_with_and_without_random_resized_crop(image_dataset):
    from kubeml_amd.ops import kernels as K
    from kubeml_amd.sdk.vision import prepare
    src, src_cpu, labels = _source(40, 48, 3)
    B = 8
    x, y = src[:B], labels[:B]
    ds = image_dataset(random_resized_crop=32, eval_resize=36)
    seed = 90210                                  # counters of this test alone: [seed, calls so far, 0]
    xt, yt = prepare((x, y), ds, True, seed=seed)
    assert xt.shape == (B, 32, 32, 8) and xt.dtype == BF16 and torch.equal(yt, y)
    plan = K.rrc_plan(torch.tensor([float(seed), 0.0, 0.0], device=dev), 1, B, 40, 48, N=B)[0].cpu()
    refs, extents = _train_refs(src_cpu, plan, 0, (32, 32), 3)
    _check(xt, refs, extents, 3, "prepare train")
    xe, ye = prepare((x, y), ds, False, seed=seed)
    refs, extents = _eval_refs(src_cpu, 0, B, 36, 32, 3)
    _check(xe, refs, extents, 3, "prepare eval")
    assert torch.equal(ye, y)
    xm, tm = prepare((x, y), image_dataset(random_resized_crop=32, mixup_alpha=1.0), True, seed=seed)
    assert xm.shape == (B, 32, 32, 8) and tm.shape == (B, 3) and torch.equal(tm[:, 0], y.float())
    # random_resized_crop=None: what K.augment returns today, called directly
    plain = image_dataset(crop_pad=2)
    seed = 90211
    for k, train in enumerate((True, False)):
        got, gl = prepare((x, y), plain, train, seed=seed)
        ctr = torch.tensor([float(seed), float(k), 0.0], device=dev)
        want, wl = K.augment(x.contiguous(), y.contiguous(), ctr, B, pad=2 if train else 0, flip=train, train=train,
                             mean=plain.mean, std=plain.std)
        assert got.shape == (B, 40, 48, 8) and torch.equal(got, want) and torch.equal(gl, wl)


def test_argument_errors():
    from kubeml_amd.ops import kernels as K
    src, _, labels = _source(40, 48, 3)
    ctr = _ctr()
    with pytest.raises(ValueError):
        K.augment_resample(src, labels, ctr, 8, 32, scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        K.augment_resample(src, labels, ctr, 8, 32, ratio=(2.0, 1.0))
    with pytest.raises(ValueError):
        K.augment_resample(src, labels, ctr, 8, 32, train=False, resize=30)   # 32 does not fit into 30 x 36
    with pytest.raises(ValueError):
        K.rrc_plan(ctr, 1, 8, 40, 48, scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        K.rrc_plan(ctr, 1, 8, 40, 48, ratio=(2.0, 1.0))
    five = torch.zeros((4, 8, 8, 5), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        K.augment_resample(five, labels, ctr, 2, 8, mean=(0.5,) * 5, std=(0.25,) * 5)
