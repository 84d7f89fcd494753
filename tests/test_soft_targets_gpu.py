"""Soft-target cross-entropy (label smoothing, packed mixup / CutMix targets) and mixing inside
the augment launch, on the MI355X: the loss kernels against fp32 torch, the mix plan against the
analytic Beta moments, the mixed pixels against the plain augment kernel at the same counter,
graph replay, and a captured train step."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
BF16 = torch.bfloat16


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _loss_close(got, ref):
    got, ref = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (got, ref))
    print(f"loss {got:.6f} ref {ref:.6f}")
    return abs(got - ref) < 1e-3 * max(1.0, abs(ref))


# ---------------------------------------------------------------------------------------
# soft cross-entropy
# ---------------------------------------------------------------------------------------

CE_SHAPES = [(37, 1000, 1000, BF16), (37, 1000, 1000, torch.float32), (45, 77, 80, BF16), (45, 10, 10, BF16),
             (45, 30522, 30528, BF16), (1030, 1000, 1000, BF16)]
CE_IDS = [f"{b}x{c}in{ld}-{'bf16' if dt == BF16 else 'fp32'}" for b, c, ld, dt in CE_SHAPES]


@functools.lru_cache(maxsize=None)
def _ce_case(B, C, ld, dtype):
    """Logits, integer labels with one ignored row, and packed targets with the edge rows
    (lam 0, lam 1, y2 == y, y = -1): made once per shape, never written to."""
    g = torch.Generator(device=dev).manual_seed(B * 7 + C)
    full = (torch.randn(B, ld, device=dev, generator=g) * 3).to(dtype)
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    y2 = torch.randint(0, C, (B,), device=dev, generator=g)
    lam = torch.rand(B, device=dev, generator=g)
    lam[0], lam[1] = 0.0, 1.0
    y2[2] = y[2]
    labels = y.clone()
    labels[3] = -100
    packed = torch.stack([y.float(), y2.float(), lam], 1).contiguous()
    packed[4, 0] = -1.0
    ok = torch.ones(B, dtype=torch.bool, device=dev)
    ok[4] = False
    q = lam[:, None] * F.one_hot(y, C).float() + (1 - lam[:, None]) * F.one_hot(y2, C).float()
    return full, labels, packed, y, ok, q


def _check_grad(d, ref_grad, C, ld, dead_row, scale):
    err = _rel(d[:, :C], scale * ref_grad)
    print(f"relative gradient error {err:.3e}")
    assert err < 1e-2
    assert float(d[dead_row].float().abs().max()) == 0.0        # the invalid row
    if ld > C:
        assert float(d[:, C:].float().abs().max()) == 0.0       # pad columns: exactly 0


@pytest.mark.parametrize("B,C,ld,dtype", CE_SHAPES, ids=CE_IDS)
def test_soft_ce_integer_labels_smoothing(B, C, ld, dtype):
    """Label smoothing over integer labels with an ignored row, against torch's index-target form."""
    from kubeml_amd.ops import kernels as K
    full, labels, _, _, _, _ = _ce_case(B, C, ld, dtype)
    lr = full[:, :C].float().requires_grad_(True)
    ref = F.cross_entropy(lr, labels, ignore_index=-100, label_smoothing=0.1)
    valid = labels != -100
    correct = int((lr.argmax(1) == labels)[valid].sum())
    for _ in range(3 if B > 1024 else 1):      # the multi-block fold: its ticket resets itself
        out3, ws, tgt = K.ce_soft_fwd(full, labels, classes=C, label_smoothing=0.1)
        assert _loss_close(out3[0], ref)
        assert int(out3[1]) == correct and int(out3[2]) == int(valid.sum())
    ref.backward()
    go = torch.tensor([2.0], device=dev)
    d = K.ce_soft_bwd(full, tgt, ws, out3, grad_out=go, classes=C, label_smoothing=0.1)
    _check_grad(d, lr.grad, C, ld, 3, 2.0)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld,dtype", CE_SHAPES, ids=CE_IDS)
def test_soft_ce_packed_targets(B, C, ld, dtype, eps):
    """Packed (y, y2, lam) rows against torch's probability-target form; the row with y = -1 is
    left out of the mean and of ``valid`` and gets no gradient."""
    from kubeml_amd.ops import kernels as K
    full, _, packed, y, ok, q = _ce_case(B, C, ld, dtype)
    lr = full[:, :C].float().requires_grad_(True)
    ref = F.cross_entropy(lr[ok], q[ok], label_smoothing=eps)
    correct = int((lr.argmax(1) == y)[ok].sum())
    for _ in range(3 if B > 1024 else 1):
        out3, ws, tgt = K.ce_soft_fwd(full, packed, classes=C, label_smoothing=eps)
        assert _loss_close(out3[0], ref)
        assert int(out3[1]) == correct and int(out3[2]) == B - 1
    ref.backward()
    go = torch.tensor([2.0], device=dev)
    d = K.ce_soft_bwd(full, tgt, ws, out3, grad_out=go, classes=C, label_smoothing=eps)
    _check_grad(d, lr.grad, C, ld, 4, 2.0)


@pytest.mark.parametrize("B,C,ld,dtype", CE_SHAPES[:4], ids=CE_IDS[:4])
def test_soft_ce_with_hard_targets_equals_hard_kernels(B, C, ld, dtype):
    """lam = 1, eps = 0: only 0 * x[y2] is added to the loss, and the gradient is the hard one
    bit for bit."""
    from kubeml_amd.ops import kernels as K
    full, labels, packed, y, _, _ = _ce_case(B, C, ld, dtype)
    hard = packed.clone()
    hard[:, 0] = labels.float()          # row 3 ignored through y = -100
    hard[:, 2] = 1.0                     # y2 stays a random other class: its weight is 0
    o_h, ws_h, lab = K.ce_fwd(full, labels, classes=C)
    o_s, ws_s, tgt = K.ce_soft_fwd(full, hard, classes=C, label_smoothing=0.0)
    assert _loss_close(o_s[0], o_h[0])
    assert torch.equal(o_s[1:], o_h[1:])
    go = torch.tensor([2.0], device=dev)
    d_h = K.ce_bwd(full, lab, ws_h, o_h, grad_out=go, classes=C)
    d_s = K.ce_soft_bwd(full, tgt, ws_s, o_s, grad_out=go, classes=C, label_smoothing=0.0)
    torch.testing.assert_close(d_s, d_h, rtol=0, atol=0)


def test_hard_labels_without_smoothing_take_the_hard_kernels(monkeypatch):
    """cross_entropy(logits, int labels) and label_smoothing=0.0: the launches and the bits of
    K.ce_fwd / K.ce_bwd called directly."""
    from kubeml_amd.nn import CrossEntropyLoss, cross_entropy
    from kubeml_amd.ops import kernels as K
    full, labels, _, _, _, _ = _ce_case(37, 1000, 1000, BF16)
    o_h, ws_h, lab = K.ce_fwd(full, labels)
    d_h = K.ce_bwd(full, lab, ws_h, o_h, grad_out=torch.tensor([1.0], device=dev))

    def boom(*a, **k):
        raise AssertionError("soft kernels launched for hard labels")
    monkeypatch.setattr(K, "ce_soft_fwd", boom)
    monkeypatch.setattr(K, "ce_soft_bwd", boom)
    for fn in (lambda lg: cross_entropy(lg, labels), lambda lg: cross_entropy(lg, labels, label_smoothing=0.0),
               lambda lg: CrossEntropyLoss()(lg, labels)):
        lg = full.clone().requires_grad_(True)
        loss = fn(lg)
        loss.backward()
        assert torch.equal(loss.detach(), o_h[0])
        assert torch.equal(lg.grad, d_h)


@pytest.mark.parametrize("B,C,ld", [(16, 10, 16), (45, 1000, 1000), (33, 77, 80)])
def test_soft_ce_bwd_adds_bias_gradient(B, C, ld):
    """ce_soft_bwd(dbias=...): the same dlogits, and dbias = column sums of the bf16 dlogits,
    added or stored, reproducibly."""
    from kubeml_amd.ops import kernels as K
    g = torch.Generator(device=dev).manual_seed(8)
    logits = (torch.randn(B, ld, device=dev, generator=g) * 3).to(BF16)
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    y2 = torch.randint(0, C, (B,), device=dev, generator=g)
    packed = torch.stack([y.float(), y2.float(), torch.rand(B, device=dev, generator=g)], 1).contiguous()
    packed[3, 0] = -1.0
    packed[5, 1] = packed[5, 0]
    out3, ws, tgt = K.ce_soft_fwd(logits, packed, classes=C, label_smoothing=0.1)
    d0 = K.ce_soft_bwd(logits, tgt, ws, out3, classes=C, label_smoothing=0.1)
    db = torch.full((ld,), 0.25, device=dev)
    d1 = K.ce_soft_bwd(logits, tgt, ws, out3, classes=C, label_smoothing=0.1, dbias=db)
    torch.testing.assert_close(d1, d0, rtol=0, atol=0)
    sums = d0.float()[:, :C].sum(0)
    want = torch.full((ld,), 0.25, device=dev)
    want[:C] += sums
    torch.testing.assert_close(db, want, rtol=1e-5, atol=1e-6)
    db2 = torch.full((ld,), float("nan"), device=dev)
    K.ce_soft_bwd(logits, tgt, ws, out3, classes=C, label_smoothing=0.1, dbias=db2, accumulate=False)
    torch.testing.assert_close(db2[:C], sums, rtol=1e-5, atol=1e-6)
    db3 = torch.empty_like(db2)
    K.ce_soft_bwd(logits, tgt, ws, out3, classes=C, label_smoothing=0.1, dbias=db3, accumulate=False)
    assert torch.equal(db2[:C], db3[:C])


@pytest.mark.parametrize("M,fuses", [(2048, True), (64, False)])
def test_linear_bias_gradient_under_the_soft_loss(monkeypatch, M, fuses):
    """nn.Linear -> cross_entropy(label_smoothing=0.1): on the GEMM route (M >= 2048) the
    Linear's bias gradient is summed by the loss backward (the dbias launch runs), on the
    implicit-GEMM route by the Linear's own wgrad; both match fp32 torch."""
    from kubeml_amd.nn import cross_entropy, flatten_module
    from kubeml_amd.nn import modules as Mo
    from kubeml_amd.ops import kernels as K
    torch.manual_seed(3)
    ref = torch.nn.Linear(256, 1000).to(dev)
    lin = Mo.Linear(256, 1000).to(dev)
    lin.load_state_dict(ref.state_dict())
    flatten_module(lin)
    x = torch.randn(M, 256, device=dev).to(BF16)
    y = torch.randint(0, 1000, (M,), device=dev)
    fused = []
    real = K.ce_soft_bwd
    monkeypatch.setattr(K, "ce_soft_bwd", lambda *a, **k: (fused.append(k.get("dbias") is not None), real(*a, **k))[1])
    loss = cross_entropy(lin(x), y, label_smoothing=0.1)
    loss.backward()
    assert fused == [fuses]
    lr = ref(x.float())
    ref_loss = F.cross_entropy(lr, y, label_smoothing=0.1)
    ref_loss.backward()
    assert _loss_close(loss, ref_loss)
    assert _rel(lin.bias.grad, ref.bias.grad) < 1e-2
    assert _rel(lin.weight.grad, ref.weight.grad) < 1e-2


# ---------------------------------------------------------------------------------------
# mix plan
# ---------------------------------------------------------------------------------------

N_PLAN = 4096


def _ctr(seed=7.0, step=3.0, start=40.0):
    return torch.tensor([seed, step, start], dtype=torch.float32, device=dev)


@pytest.mark.parametrize("alpha", [0.2, 1.0, 4.0])
def test_mix_plan_lam_is_beta_distributed(alpha):
    """lam ~ Beta(alpha, alpha): mean 1/2 and variance 1 / (4 (2 alpha + 1)) within 5 and 6
    standard errors of the analytic moments over 4096 steps."""
    from kubeml_amd.ops import kernels as K
    p = K.mix_plan(_ctr(), N_PLAN, 5, 32, 32, mixup_alpha=alpha)
    assert torch.equal(p, K.mix_plan(_ctr(), N_PLAN, 5, 32, 32, mixup_alpha=alpha))    # a function of the counter
    p = p.cpu().double()
    mode, r, lam, applied = p[:, 0], p[:, 1], p[:, 2], p[:, 7]
    assert bool((mode == K.MIX_MIXUP).all()) and bool((applied == 1).all())
    assert float(lam.min()) >= 0.0 and float(lam.max()) <= 1.0
    var = 1.0 / (4 * (2 * alpha + 1))
    mean_err, var_err = abs(float(lam.mean()) - 0.5), abs(float(lam.var()) - var)
    mean_tol = 5 * math.sqrt(var / N_PLAN)
    var_tol = 6 * var * math.sqrt((2 - 6 / (2 * alpha + 3)) / N_PLAN)
    print(f"alpha {alpha}: mean off by {mean_err:.5f} (tol {mean_tol:.5f}), variance off by {var_err:.5f} "
          f"(tol {var_tol:.5f})")
    assert mean_err < mean_tol and var_err < var_tol
    assert sorted(set(r.tolist())) == [1.0, 2.0, 3.0, 4.0]        # every shift of B = 5
    assert len(set(lam.tolist())) > N_PLAN // 2


def test_mix_plan_apply_and_switch_draws():
    from kubeml_amd.ops import kernels as K
    se = lambda pr: 5 * math.sqrt(pr * (1 - pr) / N_PLAN)
    p = K.mix_plan(_ctr(), N_PLAN, 5, 32, 32, mixup_alpha=1.0, mix_prob=0.25).cpu()
    applied = p[:, 7] == 1
    frac = float(applied.float().mean())
    print(f"applied fraction {frac:.4f}")
    assert abs(frac - 0.25) < se(0.25)
    assert bool((p[~applied, 2] == 1.0).all()) and bool((p[~applied, 0] == K.MIX_NONE).all())
    assert bool((p[applied, 0] == K.MIX_MIXUP).all())
    assert bool(((p[:, 1] >= 1) & (p[:, 1] <= 4)).all())
    p = K.mix_plan(_ctr(), N_PLAN, 5, 32, 32, mixup_alpha=1.0, cutmix_alpha=1.0, switch_prob=0.5).cpu()
    share = float((p[:, 0] == K.MIX_CUTMIX).float().mean())
    print(f"cutmix share {share:.4f}")
    assert abs(share - 0.5) < se(0.5)
    assert bool(((p[:, 0] == K.MIX_CUTMIX) | (p[:, 0] == K.MIX_MIXUP)).all())
    # a batch of one has nothing to mix with
    p = K.mix_plan(_ctr(), 64, 1, 32, 32, mixup_alpha=1.0, cutmix_alpha=1.0).cpu()
    assert bool((p[:, 0] == K.MIX_NONE).all()) and bool((p[:, 1] == 0).all()) and bool((p[:, 2] == 1.0).all())


@pytest.mark.parametrize("H,W", [(32, 32), (224, 224), (5, 7)])
def test_mix_plan_cutmix_box(H, W):
    """The box lies inside the image and lam is the share of the image outside the clipped box,
    exactly in fp32."""
    from kubeml_amd.ops import kernels as K
    # checked on the host: its fp32 division is the correctly rounded one (a device division by a
    # scalar is a multiplication by the rounded reciprocal)
    p = K.mix_plan(_ctr(), N_PLAN, 8, H, W, cutmix_alpha=1.0).cpu()
    assert bool((p[:, 0] == K.MIX_CUTMIX).all())
    x0, y0, x1, y1 = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    assert bool(((0 <= x0) & (x0 <= x1) & (x1 <= W)).all()) and bool(((0 <= y0) & (y0 <= y1) & (y1 <= H)).all())
    area = (x1 - x0) * (y1 - y0)
    assert torch.equal(p[:, 2], 1.0 - area / float(H * W))
    assert float(area.max()) > 0 and float(p[:, 2].min()) >= 0.0 and float(p[:, 2].max()) <= 1.0
    assert len(set(x0.tolist())) > 1 and len(set(y1.tolist())) > 1


# ---------------------------------------------------------------------------------------
# augment_mix
# ---------------------------------------------------------------------------------------

MIX_CASES = {
    "wraps-the-dataset": dict(N=50, B=16, H=32, W=32, C=3, CP=8, ctr=(7.0, 3.0, 40.0)),
    "5x5x1": dict(N=6, B=2, H=5, W=5, C=1, CP=8, ctr=(7.0, 3.0, 1.0)),
    "batch-of-one": dict(N=9, B=1, H=8, W=8, C=3, CP=8, ctr=(7.0, 3.0, 8.0)),
    "CP16": dict(N=20, B=4, H=8, W=12, C=3, CP=16, ctr=(11.0, 5.0, 18.0)),
}


@pytest.mark.parametrize("mode", ["mixup", "cutmix"])
@pytest.mark.parametrize("case", list(MIX_CASES))
def test_augment_mix_pixels_and_targets(case, mode):
    from kubeml_amd.ops import kernels as K
    c = MIX_CASES[case]
    N, B, H, W, C, CP = c["N"], c["B"], c["H"], c["W"], c["C"], c["CP"]
    g = torch.Generator(device=dev).manual_seed(N)
    src = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randperm(N, device=dev, generator=g) + 100
    mean, std = (0.4914, 0.4822, 0.4465)[:C], (0.2023, 0.1994, 0.2010)[:C]
    mix = dict(mixup_alpha=1.0) if mode == "mixup" else dict(cutmix_alpha=1.0)
    ctr = torch.tensor(c["ctr"], dtype=torch.float32, device=dev)
    A, lab = K.augment(src, labels, ctr, B, CP=CP, pad=2, flip=True, train=True, mean=mean, std=std)
    plan = K.mix_plan(ctr, 1, B, H, W, **mix)[0]
    out, tgt = K.augment_mix(src, labels, ctr, B, CP=CP, pad=2, flip=True, train=True, mean=mean, std=std, **mix)
    assert torch.equal(ctr.cpu(), torch.tensor(c["ctr"]))          # the counter is only read
    pmode, r = int(plan[0]), int(plan[1])
    lam = plan[2]
    partner = (torch.arange(B, device=dev) + r) % B
    assert torch.equal(tgt[:, 0], lab.float()) and torch.equal(tgt[:, 1], lab[partner].float())
    assert torch.equal(tgt[:, 2], lam.expand(B))                   # bit-equal to the plan's
    assert float(out[..., C:].float().abs().max()) == 0.0          # pad channels
    Af, Pf = A.float(), A[partner].float()
    if B == 1:
        assert pmode == K.MIX_NONE and float(lam) == 1.0 and torch.equal(out, A)
    elif mode == "cutmix":
        assert pmode == K.MIX_CUTMIX
        x0, y0, x1, y1 = (int(v) for v in plan[3:7])
        want = A.clone()
        want[:, y0:y1, x0:x1] = A[partner][:, y0:y1, x0:x1]
        assert torch.equal(out, want)
    else:
        assert pmode == K.MIX_MIXUP and 0.0 < float(lam) < 1.0
        lam = float(lam)
        bound = 1.01 * 2.0 ** -8 * (lam * Af.abs() + (1 - lam) * Pf.abs()) + 1e-6
        err = (out.float() - (lam * Af + (1 - lam) * Pf)).abs()
        print(f"worst error / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        assert not torch.equal(out, A)


def test_augment_mix_draws_a_new_plan_every_graph_replay():
    from kubeml_amd.engine.step import capture_graph
    from kubeml_amd.ops import kernels as K
    N, B, H, W = 64, 8, 16, 16
    g = torch.Generator(device=dev).manual_seed(2)
    src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.arange(N, device=dev)
    start = torch.tensor([5.0, 9.0, 56.0], device=dev)
    ctr = start.clone()
    out = torch.empty((B, H, W, 8), dtype=BF16, device=dev)
    tgt = torch.empty((B, 3), device=dev)

    def body():
        K.augment_mix(src, labels, ctr, B, out=out, targets_out=tgt, mixup_alpha=1.0)
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
    want = K.mix_plan(start, 3, B, H, W, mixup_alpha=1.0)
    seen = []
    for k in range(3):
        graph.replay()
        t = tgt.clone()
        first = (56 + k * B) % N
        assert int(t[0, 0]) == first                                 # the batch start advanced too
        assert torch.equal(t[:, 2], want[k, 2].expand(B))
        assert int(t[0, 1]) == (first + (0 + int(want[k, 1])) % B) % N
        seen.append(float(t[0, 2]))
    assert len(set(seen)) > 1, seen
    assert ctr.tolist() == [5.0, 12.0, float((56 + 3 * B) % N)]


# ---------------------------------------------------------------------------------------
# captured train step
# ---------------------------------------------------------------------------------------

def _train_setup():
    from kubeml_amd.models.resnet import resnet18
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    torch.manual_seed(1234)
    m = resnet18(num_classes=10).to(dev)
    m.train()
    sp = flatten_module(m)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    return m, sp, opt


def test_train_step_with_packed_targets_and_smoothing():
    """make_train_step with CrossEntropyLoss(label_smoothing=0.1) on packed targets: the captured
    step's first update equals the eager step bit for bit, and its loss is torch's on the model's
    own logits."""
    from kubeml_amd.engine.dp import make_train_step
    from kubeml_amd.nn import CrossEntropyLoss
    from kubeml_amd.ops import kernels as K
    B = 32
    g = torch.Generator(device=dev).manual_seed(4)
    src = torch.randint(0, 256, (64, 32, 32, 3), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 10, (64,), device=dev, generator=g)
    x, t = K.augment_mix(src, labels, _ctr(3.0, 1.0, 0.0), B, mixup_alpha=1.0)
    assert t.shape == (B, 3) and 0.0 < float(t[0, 2]) < 1.0
    states, losses = [], []
    for use_graph in (True, False):
        m, sp, opt = _train_setup()
        st = make_train_step(m, sp, opt, CrossEntropyLoss(label_smoothing=0.1), x.clone(), t.clone(),
                             use_graph=use_graph)
        st.capture()
        assert st.captured is use_graph
        losses.append(float(st().detach()))
        torch.cuda.synchronize()
        states.append(sp.state.clone())
    assert losses[0] == losses[1], losses
    assert torch.equal(states[0], states[1]), float((states[0] - states[1]).abs().max())
    m, sp, opt = _train_setup()
    assert not torch.equal(states[0], sp.state)
    with torch.no_grad():
        logits = m(x).float()
    y, y2, lam = t[:, 0].long(), t[:, 1].long(), t[:, 2:3]
    q = lam * F.one_hot(y, 10).float() + (1 - lam) * F.one_hot(y2, 10).float()
    assert _loss_close(losses[0], F.cross_entropy(logits, q, label_smoothing=0.1))
