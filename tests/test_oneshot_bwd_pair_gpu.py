"""The grouped one-shot backward of the single-tap convs (ops.kernels._ONESHOT_PAIR_ON): layer3's
unrolled 2x2-map convs (one-shot dgrad + folded one-shot wgrad that writes the 3x3 gradient
directly: no 1x1-form scratch, no fold pass) and layer4's centre-tap convs on 1x1 maps (one-shot
dgrad + one-shot wgrad), each as ONE k_conv_pair launch, against fp32 ``F.conv2d`` autograd.

Tolerances are those tests/test_kernels_gpu.py uses for the same bodies: relative L2 < 1e-2 for
dX / dW (bf16 inputs, fp32 accumulation, bf16 dX), < 2e-2 for BN partial rows summed over rows.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = "cuda"
ARGS = (3, 3, (1, 1), (1, 1))


def _bf(t):
    return t.to(torch.bfloat16)


def _rel(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


_CASES = {}


def _case(B, H, C, Co):
    """Inputs and the fp32 autograd reference of one conv, computed once per shape."""
    key = (B, H, C, Co)
    if key not in _CASES:
        g = torch.Generator(device=dev).manual_seed(100 + B + H)
        x = _bf(torch.randn(B, H, H, C, device=dev, generator=g))
        w = _bf(torch.randn(Co, 3, 3, C, device=dev, generator=g) * (1.0 / (9 * C) ** 0.5))
        dy = _bf(torch.randn(B, H, H, Co, device=dev, generator=g))
        add = _bf(torch.randn(B, H, H, C, device=dev, generator=g))
        xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
        wr = w.float().permute(0, 3, 1, 2).requires_grad_(True)
        F.conv2d(xr, wr, padding=1).backward(dy.float().permute(0, 3, 1, 2))
        _CASES[key] = (x, w, dy, add, xr.grad.permute(0, 2, 3, 1).contiguous(),
                       wr.grad.permute(0, 2, 3, 1).contiguous())
    return _CASES[key]


def _canaried(shape, fill):
    """A tensor of ``shape`` inside a larger NaN buffer: (tensor, the NaN tail after it)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 1024,), float("nan"), device=dev)
    t = buf[:n].view(shape)
    if fill is not None:
        t.copy_(fill)
    return t, buf[n:]


@pytest.mark.parametrize("B", [256, 40, 1])
def test_unrolled_conv_folded_pair(B):
    """Unrolled conv on the default plan: dX with an addend; dW stored into a NaN-filled
    (K,3,3,C) buffer (every element written) and added onto a random one; nothing past the
    buffer is touched.  B = 40 / 1: zero-filled pixel rows of the K-strided wgrad panels and
    the M tail of the dgrad."""
    from kubeml_amd.ops import kernels as K
    C = Co = 256
    x, w, dy, add, dx_ref, dw_ref = _case(B, 2, C, Co)
    dplan, wplan, grouped = K.bwd_plans(x.shape, Co, *ARGS, unroll=True)
    assert dplan[4] == K.ONESHOT and wplan[4] == K.FOLD22 and grouped
    dw, tail = _canaried((Co, 3, 3, C), None)
    dx = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, wu=K.GATHER22, accumulate=False)
    assert dx.shape == (B, 2, 2, C)
    e_dx, e_dw = _rel(dx, dx_ref + add.float()), _rel(dw, dw_ref)
    print(f"B={B} folded pair: rel dx {e_dx:.3e} dw {e_dw:.3e}")
    assert not torch.isnan(dw).any()
    assert e_dx < 1e-2 and e_dw < 1e-2
    assert torch.isnan(tail).all()
    r0 = torch.randn(Co, 3, 3, C, device=dev)
    dw2, tail2 = _canaried((Co, 3, 3, C), r0)
    K.conv_bwd(dy, w, x, dw2, *ARGS, addend=add, wu=K.GATHER22, accumulate=True)
    assert torch.isnan(tail2).all()
    assert _rel(dw2 - r0, dw_ref) < 1e-2
    # a materialised unrolled weight takes the same route
    dw3 = torch.empty(Co, 3, 3, C, device=dev)
    dx3 = K.conv_bwd(dy, w, x, dw3, *ARGS, addend=add, wu=K.unrolled_weight(w), accumulate=False)
    assert torch.equal(dx3, dx) and torch.equal(dw3, dw)


@pytest.mark.parametrize("plans", ["_ONESHOT_PAIR_U22_FULL", "_ONESHOT_PAIR_U22_HALF"])
@pytest.mark.parametrize("B", [256, 40])
def test_unrolled_pair_panel_passes(plans, B, monkeypatch):
    """Both instantiated dgrad panel depths of the unrolled pair (K in one pass or two halves:
    128 / 64 KB of LDS per block), whichever is the default: same checks against fp32."""
    from kubeml_amd.ops import kernels as K
    monkeypatch.setattr(K, "_ONESHOT_PAIR_U22", getattr(K, plans))
    C = Co = 256
    x, w, dy, add, dx_ref, dw_ref = _case(B, 2, C, Co)
    assert K.bwd_plans(x.shape, Co, *ARGS, unroll=True) == getattr(K, plans) + (True,)
    dw, tail = _canaried((Co, 3, 3, C), None)
    dx = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, wu=K.GATHER22, accumulate=False)
    assert not torch.isnan(dw).any() and torch.isnan(tail).all()
    assert _rel(dx, dx_ref + add.float()) < 1e-2 and _rel(dw, dw_ref) < 1e-2


@pytest.mark.parametrize("B", [256, 40])
def test_layer4_centre_tap_pair(B):
    """3x3 conv on a 1x1 map (centre tap only), C = Cout = 512: one-shot dgrad + one-shot wgrad
    grouped.  With accumulate=False only the centre tap is written, as on the implicit-GEMM
    route (its wgrad GEMM has N = one tap x C columns): the other eight taps of a NaN-filled dw
    stay NaN."""
    from kubeml_amd.ops import kernels as K
    C = Co = 512
    x, w, dy, add, dx_ref, dw_ref = _case(B, 1, C, Co)
    dplan, wplan, grouped = K.bwd_plans(x.shape, Co, *ARGS)
    assert dplan[4] == K.ONESHOT and wplan[4] == K.ONESHOT and grouped
    dw, tail = _canaried((Co, 3, 3, C), None)
    dx = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, accumulate=False)
    e_dx, e_dw = _rel(dx, dx_ref + add.float()), _rel(dw[:, 1, 1, :], dw_ref[:, 1, 1, :])
    print(f"B={B} layer4 pair: rel dx {e_dx:.3e} dw {e_dw:.3e}")
    assert e_dx < 1e-2 and e_dw < 1e-2
    centre = torch.zeros(3, 3, dtype=torch.bool, device=dev)
    centre[1, 1] = True
    assert torch.isnan(dw[:, ~centre, :]).all() and not torch.isnan(dw[:, 1, 1, :]).any()
    assert torch.isnan(tail).all()
    # the implicit-GEMM route leaves the same eight taps alone
    base_d = K.plan_conv("dgrad", B, C, Co)
    base_w = K.plan_conv("wgrad", Co, C, B)
    dw_old = torch.full((Co, 3, 3, C), float("nan"), device=dev)
    K.conv_bwd(dy, w, x, dw_old, *ARGS, addend=add, accumulate=False, dcfg=base_d, wcfg=base_w)
    assert torch.equal(torch.isnan(dw_old), torch.isnan(dw))
    r0 = torch.randn(Co, 3, 3, C, device=dev)
    dw2 = r0.clone()
    K.conv_bwd(dy, w, x, dw2, *ARGS, addend=add, accumulate=True)
    assert _rel(dw2[:, 1, 1, :] - r0[:, 1, 1, :], dw_ref[:, 1, 1, :]) < 1e-2
    dw2[:, 1, 1, :] = r0[:, 1, 1, :]
    assert torch.equal(dw2, r0)


def test_folded_pair_consumer_bn_epilogue():
    """bnf + bnf_mask through the one-shot dgrad of the pair: masked dX and the folded partial
    rows against the implicit-GEMM plans forced by dcfg / wcfg (the comparison of
    test_conv_halo_dgrad)."""
    from kubeml_amd.ops import kernels as K
    B, C, Co = 256, 256, 256
    x, w, dy, add, dx_ref, dw_ref = _case(B, 2, C, Co)
    g = torch.Generator(device=dev).manual_seed(7)
    yb = _bf(torch.randn(B, 2, 2, C, device=dev, generator=g))
    c = _bf(torch.randn(B, 2, 2, C, device=dev, generator=g))
    mean = torch.randn(C, device=dev, generator=g) * 0.1
    rstd = torch.rand(C, device=dev, generator=g) + 0.5
    base_d = K.plan_conv("dgrad", B, 4 * C, 4 * Co)
    base_w = K.plan_conv("wgrad", 4 * Co, 4 * C, B)
    assert base_d[4] != K.ONESHOT and base_w[4] != K.ONESHOT
    scratch = torch.empty(4 * Co, 1, 1, 4 * C, device=dev)
    r_ref = K.conv_bwd(dy, w, x, scratch, *ARGS, addend=add, bnf=(yb, c, mean, rstd), bnf_mask=True,
                       wu=K.GATHER22, dcfg=base_d, wcfg=base_w)
    dw = torch.empty(Co, 3, 3, C, device=dev)
    r = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, bnf=(yb, c, mean, rstd), bnf_mask=True, wu=K.GATHER22,
                   accumulate=False)
    assert _rel(r[0], r_ref[0]) < 1e-2
    masked = (dx_ref + add.float()) * (yb.float() > 0)
    assert _rel(r[0], masked) < 1e-2
    (p1, g1), (p0, g0) = r[1], r_ref[1]
    e = _rel(p1.view(g1, 2 * C).sum(0), p0.view(g0, 2 * C).sum(0))
    print(f"folded pair bnf rows: rel {e:.3e} (G {g1} vs {g0})")
    assert e < 2e-2
    assert _rel(dw, dw_ref) < 1e-2


@pytest.mark.parametrize("B", [256, 40])
def test_folded_dw_agrees_with_scratch_and_fold(B):
    """Folded dW against the 1x1-form scratch + fold22_multi of the implicit-GEMM route on the
    same inputs: both are fp32 sums of the same bf16 products in a different order."""
    from kubeml_amd.ops import kernels as K
    C = Co = 256
    x, w, dy, add, _, _ = _case(B, 2, C, Co)
    scratch = torch.empty(4 * Co, 1, 1, 4 * C, device=dev)
    dx_old = K.conv_bwd(dy, w, x, scratch, *ARGS, addend=add, wu=K.GATHER22)
    dw_old = torch.empty(Co, 3, 3, C, device=dev)
    K.fold22_multi([(scratch, dw_old, False)])
    dw = torch.empty(Co, 3, 3, C, device=dev)
    dx = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, wu=K.GATHER22, accumulate=False)
    e_dw, e_dx = _rel(dw, dw_old), _rel(dx, dx_old)
    print(f"B={B} folded vs scratch+fold: rel dw {e_dw:.3e} dx {e_dx:.3e}")
    assert e_dw < 1e-3
    assert e_dx < 1e-2


@pytest.mark.parametrize("shape", [(256, 2, 256), (40, 2, 256), (256, 1, 512)])
def test_oneshot_pair_is_deterministic(shape):
    from kubeml_amd.ops import kernels as K
    B, H, C = shape
    x, w, dy, add, _, _ = _case(B, H, C, C)
    wu = K.GATHER22 if H == 2 else None
    outs = []
    for _ in range(2):
        dw = torch.zeros(C, 3, 3, C, device=dev)
        dx = K.conv_bwd(dy, w, x, dw, *ARGS, addend=add, wu=wu, accumulate=False)
        outs.append((dx, dw))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _block_step(planes, hw, on, monkeypatch):
    from kubeml_amd.models.resnet import BasicBlock
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.ops import kernels as K
    monkeypatch.setattr(K, "_ONESHOT_PAIR_ON", on)
    folds = []
    fold22 = K.fold22_multi
    monkeypatch.setattr(K, "fold22_multi", lambda jobs: (folds.append(len(jobs)), fold22(jobs))[1])
    torch.manual_seed(31)
    blk = BasicBlock(planes, planes).to(dev)
    blk.train()
    sp = flatten_module(blk)
    g = torch.Generator(device=dev).manual_seed(32)
    x = _bf(torch.randn(256, hw, hw, planes, device=dev, generator=g)).requires_grad_(True)
    dy = _bf(torch.randn(256, hw, hw, planes, device=dev, generator=g))
    sp.zero_grad()
    y = blk(x)
    y.backward(dy)
    pending = len(sp._folds)
    sp.finish_grads()
    torch.cuda.synchronize()
    return x.grad.clone(), sp.grad.clone(), y.detach().clone(), sum(folds), pending


@pytest.mark.parametrize("planes,hw", [(256, 2), (512, 1)])
def test_basic_block_switch_on_off(planes, hw, monkeypatch):
    """One non-downsampling BasicBlock of layer3 / layer4, batch 256, forward + backward through
    BlockFn with the one-shot pair on and off: same parameter and input gradients; with it on
    no fold launch runs and none is pending after backward."""
    dx1, g1, y1, folds1, pend1 = _block_step(planes, hw, True, monkeypatch)
    dx0, g0, y0, folds0, pend0 = _block_step(planes, hw, False, monkeypatch)
    assert torch.equal(y1, y0)
    e_dx, e_g = _rel(dx1, dx0), _rel(g1, g0)
    print(f"block {planes}@{hw}x{hw}: rel dx {e_dx:.3e} grads {e_g:.3e} folds on/off {folds1}/{folds0}")
    assert e_dx < 1e-2 and e_g < 1e-2
    assert folds1 == 0 and pend1 == 0 and pend0 == 0
    if hw == 2:
        assert folds0 == 2     # the implicit-GEMM route folds both unrolled convs' scratches
