"""Label smoothing, mixup and CutMix on a CPU worker: ``cross_entropy`` with soft targets is
torch's probability-target / label-smoothing form, and ``prepare`` mixes a training batch in
torch ops and hands back packed ``[B, 3]`` targets ``(label, partner label, lam)``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _packed(B, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B,), generator=g)
    y2 = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1] = 0.0, 1.0
    y2[2] = y[2]
    return y, y2, lam, torch.stack([y.float(), y2.float(), lam], 1)


def _q(y, y2, lam, C):
    return lam[:, None] * F.one_hot(y, C).float() + (1 - lam[:, None]) * F.one_hot(y2, C).float()


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_packed_targets_match_torch_probability_targets(eps):
    from kubeml_amd.nn import CrossEntropyLoss, cross_entropy
    torch.manual_seed(1)
    B, C = 13, 11
    logits = torch.randn(B, C, requires_grad=True)
    y, y2, lam, t = _packed(B, C)
    ref_in = logits.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_in, _q(y, y2, lam, C), label_smoothing=eps)
    loss, correct = cross_entropy(logits, t, label_smoothing=eps, return_correct=True)
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    assert int(correct) == int((logits.argmax(1) == y).sum())
    loss.backward()
    ref.backward()
    torch.testing.assert_close(logits.grad, ref_in.grad, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(CrossEntropyLoss(label_smoothing=eps)(logits, t), ref, rtol=1e-6, atol=1e-6)


def test_packed_invalid_row_is_left_out():
    from kubeml_amd.nn import cross_entropy
    torch.manual_seed(2)
    B, C = 8, 6
    logits = torch.randn(B, C + 2)      # padded rows: classes=C
    y, y2, lam, t = _packed(B, C)
    t[4, 0] = -1.0
    t[5, 1] = float(C)
    keep = torch.ones(B, dtype=torch.bool)
    keep[4] = keep[5] = False
    ref = F.cross_entropy(logits[keep][:, :C], _q(y, y2, lam, C)[keep], label_smoothing=0.1)
    loss, correct = cross_entropy(logits, t, classes=C, label_smoothing=0.1, return_correct=True)
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    assert int(correct) == int((logits[:, :C].argmax(1) == y)[keep].sum())


def test_integer_labels_with_smoothing_and_ignore_index_match_torch():
    from kubeml_amd.nn import CrossEntropyLoss, cross_entropy
    torch.manual_seed(3)
    B, C = 17, 9
    logits = torch.randn(B, C)
    y = torch.randint(0, C, (B,))
    y[3] = y[11] = -100
    ref = F.cross_entropy(logits, y, ignore_index=-100, label_smoothing=0.1)
    loss, correct = cross_entropy(logits, y, label_smoothing=0.1, return_correct=True)
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    assert int(correct) == int((logits.argmax(1) == y)[y != -100].sum())
    torch.testing.assert_close(CrossEntropyLoss(label_smoothing=0.1)(logits, y), ref, rtol=1e-6, atol=1e-6)
    # no smoothing: the call every existing user makes
    assert torch.equal(cross_entropy(logits, y), F.cross_entropy(logits, y, ignore_index=-100))


def test_error_cases():
    from kubeml_amd.nn import CrossEntropyLoss, cross_entropy
    logits = torch.randn(4, 5)
    y = torch.zeros(4, dtype=torch.int64)
    for eps in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            cross_entropy(logits, y, label_smoothing=eps)
        with pytest.raises(ValueError):
            CrossEntropyLoss(label_smoothing=eps)
    for bad in (torch.zeros(4), torch.zeros(4, 2), torch.zeros(3, 3), torch.zeros(4, 3, 1)):
        with pytest.raises(ValueError):
            cross_entropy(logits, bad)
    wide = torch.empty(0, 2 ** 24 + 8)     # no rows: only the shape is looked at
    with pytest.raises(ValueError):
        cross_entropy(wide, torch.zeros(0, 3))
    cross_entropy(wide, torch.zeros(0, 3), classes=2 ** 24)     # the limit is on the class count


@pytest.fixture
def image_dataset(tmp_path):
    """ImageDataset factory over a tiny shard store."""
    from kubeml_amd.sdk.context import TaskContext, reset_task, set_task
    from kubeml_amd.sdk.vision import ImageDataset
    from kubeml_amd.store.shards import ShardStore
    rng = np.random.default_rng(0)
    st = ShardStore(str(tmp_path))
    x = rng.integers(0, 256, (64, 8, 8, 3), dtype=np.uint8)
    y = rng.integers(0, 10, 64).astype(np.int64)
    st.create("tiny", x, y, x[:16], y[:16])
    tok = set_task(TaskContext(store=st))
    try:
        yield lambda **kw: ImageDataset("tiny", **{"crop_pad": 2, **kw})
    finally:
        reset_task(tok)


def _batch(B=12):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (B, 8, 8, 3), dtype=torch.uint8, generator=g)
    return x, torch.arange(B, dtype=torch.int64) + 20      # distinct labels: the partner is visible


@pytest.mark.parametrize("mixup,cutmix", [(1.0, 0.0), (0.0, 1.0), (0.4, 1.0)])
def test_prepare_mixes_training_batches(image_dataset, mixup, cutmix):
    from kubeml_amd.nn import cross_entropy
    from kubeml_amd.sdk.vision import prepare
    ds = image_dataset(mixup_alpha=mixup, cutmix_alpha=cutmix)
    x, y = _batch()
    B = x.shape[0]
    torch.manual_seed(7)
    for _ in range(8):
        xm, t = prepare((x, y), ds, train=True)
        assert xm.shape == (B, 3, 8, 8) and xm.dtype == torch.float32
        assert t.shape == (B, 3) and t.dtype == torch.float32
        assert torch.equal(t[:, 0].long(), y)
        lam = t[:, 2]
        assert bool((lam == lam[0]).all()) and 0.0 <= float(lam[0]) <= 1.0
        r = int(t[0, 1]) - int(t[0, 0])
        assert 1 <= r % B <= B - 1
        assert torch.equal(t[:, 1].long(), y.roll(-(r % B)))     # partner labels come from the batch
        assert torch.isfinite(cross_entropy(torch.randn(B, 40), t, label_smoothing=0.1))


def test_prepare_mixup_blends_with_the_partner(image_dataset):
    from kubeml_amd.sdk.vision import prepare
    ds = image_dataset(mixup_alpha=1.0, flip=False, crop_pad=0)     # no crop, no flip: the unmixed batch is known
    x, y = _batch()
    plain, labels = prepare((x, y), image_dataset(flip=False, crop_pad=0), train=True)
    assert labels.dtype == torch.int64
    torch.manual_seed(11)
    xm, t = prepare((x, y), ds, train=True)
    lam, r = float(t[0, 2]), (int(t[0, 1]) - int(t[0, 0])) % x.shape[0]
    torch.testing.assert_close(xm, lam * plain + (1 - lam) * plain.roll(-r, 0), rtol=1e-6, atol=1e-6)


def test_prepare_without_mixing_returns_labels(image_dataset):
    from kubeml_amd.sdk.vision import prepare
    x, y = _batch()
    off = image_dataset()                                   # both alphas 0
    xb, yb = prepare((x, y), off, train=True)
    assert yb.dtype == torch.int64 and torch.equal(yb, y)
    on = image_dataset(mixup_alpha=1.0, cutmix_alpha=1.0)
    xv, yv = prepare((x, y), on, train=False)               # validation is never mixed
    assert yv.dtype == torch.int64 and torch.equal(yv, y)
    xo, _ = prepare((x, y), off, train=False)
    assert torch.equal(xv, xo)
    one, t1 = prepare((x[:1], y[:1]), on, train=True)       # nothing to mix with
    assert t1.tolist() == [[20.0, 20.0, 1.0]]
    for kw in ({"mixup_alpha": -1.0}, {"mix_prob": 1.5}, {"switch_prob": -0.1}):
        with pytest.raises(ValueError):
            image_dataset(**kw)
