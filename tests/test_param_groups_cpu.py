"""Parameter groups with their own lr / weight decay, without a GPU: the optimizers' torch path over
a CPU flat space and over loose parameters, the conversions, the helper and the SDK plumbing."""
import pytest
import torch
import torch.nn.functional as F


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(33, 10), torch.nn.LayerNorm(10), torch.nn.Linear(10, 7))


def _data(k):
    g = torch.Generator().manual_seed(20 + k)
    return torch.randn(9, 33, generator=g), torch.randint(0, 7, (9,), generator=g)


def _groups(net, lrs=(0.05, 0.02), wds=(0.01, 0.0)):
    """The BERT idiom: weights decay, biases and LayerNorm do not; each group with an LR of its own."""
    decay = [p for p in net.parameters() if p.ndim > 1]
    rest = [p for p in net.parameters() if p.ndim <= 1]
    return [{"params": decay, "lr": lrs[0], "weight_decay": wds[0]},
            {"params": rest, "lr": lrs[1], "weight_decay": wds[1]}]


def _make(kind, net, fused):
    from kubeml_amd import optim
    mod = optim if fused else torch.optim
    if kind == "sgd":
        return mod.SGD(_groups(net), lr=0.1, momentum=0.9, nesterov=True)
    if kind == "adam":
        return mod.Adam(_groups(net), lr=1e-2)
    return mod.AdamW(_groups(net), lr=1e-2)


@pytest.mark.parametrize("flat", [False, True], ids=["loose", "cpu_flat_space"])
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_grouped_cpu_optimizers_match_torch(kind, flat):
    from kubeml_amd.nn import flatten_module
    ours, ref = _net(), _net()
    if flat:
        flatten_module(ours)
    opt, topt = _make(kind, ours, True), _make(kind, ref, False)
    assert opt.grouped and len(opt.param_groups) == 2
    for k in range(3):
        x, y = _data(k)
        opt.zero_grad()
        topt.zero_grad()
        F.cross_entropy(ours(x), y).backward()
        F.cross_entropy(ref(x), y).backward()
        opt.step()
        topt.step()
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.allclose(p, q), float((p - q).abs().max())


def test_grouped_sgd_step_range_on_a_cpu_flat_space():
    """The ranged step (two ranges that tile the space) applies each element's own group."""
    from kubeml_amd.nn import flatten_module
    ours, ref = _net(), _net()
    space = flatten_module(ours)
    opt, topt = _make("sgd", ours, True), _make("sgd", ref, False)
    cut = 64 * (space.numel // 128)
    assert 0 < cut < space.numel
    for k in range(3):
        x, y = _data(k)
        opt.zero_grad()
        topt.zero_grad()
        F.cross_entropy(ours(x), y).backward()
        F.cross_entropy(ref(x), y).backward()
        opt.step_range(0, cut)
        opt.step_range(cut, space.numel)
        opt.finish_ranges()
        topt.step()
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.allclose(p, q), float((p - q).abs().max())
    with pytest.raises(ValueError):
        opt.step_range(32, space.numel)          # a grouped range starts on a granule


def test_group_ids_follow_the_flat_layout():
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import AdamW
    net = _net()
    space = flatten_module(net)
    opt = AdamW(_groups(net), lr=1e-2)
    gid = opt.group_ids(space)
    assert gid.dtype == torch.uint8 and gid.numel() == space.numel // 64
    for k, g in enumerate(opt.param_groups):
        for p in g["params"]:
            o, n = space.offsets[space._index[id(p)]]
            assert set(gid[o // 64:(o + n + 63) // 64].tolist()) == {k}
    assert set(gid.tolist()) == {0, 1}


def test_single_group_is_not_grouped():
    from kubeml_amd.optim import SGD
    opt = SGD(_net().parameters(), lr=0.1, momentum=0.9)
    assert not opt.grouped
    opt.set_lr(0.3)
    assert opt.param_groups[0]["lr"] == 0.3
    with pytest.raises(ValueError):
        opt.set_lr([0.1, 0.2])


def test_set_lr_per_group():
    from kubeml_amd.optim import AdamW
    opt = AdamW(_groups(_net()), lr=1e-2)
    opt.set_lr([0.3, 0.4])
    assert [g["lr"] for g in opt.param_groups] == [0.3, 0.4]
    assert float(opt.lr_tensor(torch.device("cpu"))) == pytest.approx(0.3)     # group 0's scalar
    opt.set_lr(0.5)
    assert [g["lr"] for g in opt.param_groups] == [0.5, 0.5]
    with pytest.raises(ValueError):
        opt.set_lr([0.1, 0.2, 0.3])


def test_groups_may_differ_in_lr_and_weight_decay_only():
    from kubeml_amd.optim import SGD, Adam, AdamW
    net = _net()
    g = _groups(net)
    for cls, key, val in ((Adam, "betas", (0.8, 0.99)), (AdamW, "eps", 1e-6), (SGD, "momentum", 0.5),
                          (SGD, "nesterov", True), (SGD, "dampening", 0.1), (AdamW, "max_grad_norm", 1.0)):
        bad = [dict(g[0]), dict(g[1], **{key: val})]
        with pytest.raises(ValueError, match=key):
            cls(bad, lr=0.1)
    ps = list(net.parameters())
    nine = [{"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.1 * (i + 1)} for i in range(9)]
    with pytest.raises(ValueError, match="at most 8"):
        SGD(nine, lr=0.1)
    assert len(SGD(nine[:8], lr=0.1).param_groups) == 8
    assert len(ps) == 6


def test_add_param_group_is_checked_like_the_constructor():
    from kubeml_amd.optim import SGD
    net = _net()
    g = _groups(net)
    opt = SGD([g[0]], lr=0.1, momentum=0.9)
    assert not opt.grouped
    with pytest.raises(ValueError, match="momentum"):
        opt.add_param_group(dict(g[1], momentum=0.5))
    opt = SGD([g[0]], lr=0.1, momentum=0.9)
    opt.add_param_group(dict(g[1]))
    assert opt.grouped and opt.param_groups[1]["momentum"] == 0.9


def test_from_torch_keeps_the_groups():
    from kubeml_amd.optim import SGD, Adam, AdamW, from_torch, with_max_grad_norm
    net = _net()
    cases = ((torch.optim.AdamW(_groups(net), lr=1e-2, betas=(0.8, 0.99), eps=1e-6), AdamW),
             (torch.optim.Adam(_groups(net), lr=1e-2), Adam),
             (torch.optim.SGD(_groups(net), lr=0.1, momentum=0.9, nesterov=True), SGD))
    for topt, cls in cases:
        f = from_torch(topt)
        assert type(f) is cls and f.grouped and len(f.param_groups) == 2
        for fg, tg in zip(f.param_groups, topt.param_groups):
            assert [id(p) for p in fg["params"]] == [id(p) for p in tg["params"]]
            for key in fg:
                if key not in ("params", "max_grad_norm"):
                    assert fg[key] == tg[key], key
        assert [g["weight_decay"] for g in f.param_groups] == [0.01, 0.0]
        assert [g["lr"] for g in f.param_groups] == [0.05, 0.02]
        w = with_max_grad_norm(f, 1.0)
        assert type(w) is cls and w.clips and w.grouped
        for wg, fg in zip(w.param_groups, f.param_groups):
            assert [id(p) for p in wg["params"]] == [id(p) for p in fg["params"]]
            assert wg["lr"] == fg["lr"] and wg["weight_decay"] == fg["weight_decay"]
            assert wg["max_grad_norm"] == 1.0
    # a single group converts as it always did
    one = from_torch(torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4))
    assert not one.grouped and one.param_groups[0]["weight_decay"] == 1e-4 and one.param_groups[0]["momentum"] == 0.9


def test_from_torch_raises_for_what_it_cannot_represent():
    from kubeml_amd.optim import from_torch
    net = _net()
    g = _groups(net)
    with pytest.raises(ValueError, match="betas"):
        from_torch(torch.optim.AdamW([dict(g[0]), dict(g[1], betas=(0.8, 0.9))], lr=1e-2))
    with pytest.raises(ValueError, match="momentum"):
        from_torch(torch.optim.SGD([dict(g[0]), dict(g[1], momentum=0.5)], lr=0.1, momentum=0.9))


def test_no_decay_groups():
    from kubeml_amd.optim import AdamW, no_decay_groups
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Flatten(),
                              torch.nn.Linear(8, 4))
    net[3].bias.requires_grad_(False)              # a frozen parameter is in neither group
    groups = no_decay_groups(net, 0.01)
    assert [g["weight_decay"] for g in groups] == [0.01, 0.0]
    low = {id(p) for p in net.parameters() if p.ndim <= 1 and p.requires_grad}
    assert {id(p) for p in groups[1]["params"]} == low and len(low) == 3
    assert {id(p) for p in groups[0]["params"]} == {id(net[0].weight), id(net[3].weight)}
    opt = AdamW(groups, lr=1e-3)
    assert opt.grouped and [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    # nothing to exempt: one group
    assert len(no_decay_groups(torch.nn.Linear(4, 4, bias=False), 0.1)) == 1


def _kube(net, opt):
    from kubeml_amd.sdk.model import KubeModel
    km = KubeModel.__new__(KubeModel)
    km.device = torch.device("cpu")
    km._network, km.optimizer = net, opt
    km._sync_mode, km._graphs, km._shards, km._flat, km._dry = "local", {}, {}, None, False
    return km


def test_config_optimizer_retunes_each_group():
    from kubeml_amd.optim import AdamW
    from kubeml_amd.sdk.model import KubeModel
    net = _net()
    kept = AdamW(_groups(net), lr=1e-2)
    km = _kube(net, kept)
    km.configure_optimizers = lambda: AdamW(_groups(net, lrs=(0.004, 0.001)), lr=1e-2)
    KubeModel._config_optimizer(km)
    assert km.optimizer is kept
    assert [g["lr"] for g in kept.param_groups] == [0.004, 0.001]
    assert [g["weight_decay"] for g in kept.param_groups] == [0.01, 0.0]
    # other groups' values: a new optimizer
    km.configure_optimizers = lambda: AdamW(_groups(net, wds=(0.1, 0.0)), lr=1e-2)
    KubeModel._config_optimizer(km)
    assert km.optimizer is not kept


def test_step_builder_keeps_grouped_sgd_off_the_scalar_routes():
    """The launches that bake one scalar lr / weight decay in (riders, the in-collective update)
    are for the single-group SGD; a grouped optimizer still shards."""
    from kubeml_amd.engine.dp import _scalar_sgd, optimizer_can_shard, optimizer_grouped
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    from kubeml_amd.parallel.peer import _one_group
    net = _net()
    flatten_module(net)
    one, two = SGD(net.parameters(), lr=0.1, momentum=0.9), SGD(_groups(net), lr=0.1, momentum=0.9)
    assert _scalar_sgd(one) and not optimizer_grouped(one)
    assert optimizer_grouped(two) and not _scalar_sgd(two)
    assert optimizer_can_shard(one) and optimizer_can_shard(two)
    _one_group(one)
    with pytest.raises(ValueError):
        _one_group(two)


def test_sgd_operands_and_state_tensors():
    """The accessor hands out what the optimizer's own launches use, and state_tensors() stays the set
    a graph snapshot restores: state buffers, step count and first flag, never lr or clip scratch."""
    from kubeml_amd.nn import flatten_module
    from kubeml_amd.optim import SGD
    torch.manual_seed(0)
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n)) for n in (5, 64, 130)])
    space = flatten_module(net)
    assert space.numel == 320            # 64-aligned regions: 64 + 64 + 192
    cpu = torch.device("cpu")
    opt = SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=0.01, nesterov=True)
    op = opt.sgd_operands(space)
    assert op.mom is opt.state_buffers(space)["momentum"] and op.mom.numel() == 320
    assert op.lr is opt.lr_tensor(cpu) and float(op.lr) == pytest.approx(0.1)
    assert op.first is opt.first_tensor(cpu) and float(op.first) == 1.0
    assert tuple(op[3:]) == (0.01, 0.9, 0.0, True)
    space.grad.copy_(torch.randn(320))
    d = space.grad.add(space.master.detach(), alpha=0.01)
    opt.step_range(0, 320)               # the first step writes the buffer the accessor returned: buf := d
    assert opt.sgd_operands(space).mom is op.mom and torch.equal(op.mom, d)
    plain = SGD(net.parameters(), lr=0.2)
    op0 = plain.sgd_operands(space)
    assert op0.mom is None and op0.first is None
    assert op0.lr is plain.lr_tensor(cpu) and tuple(op0[3:]) == (0.0, 0.0, 0.0, False)

    clip = SGD(net.parameters(), lr=0.1, momentum=0.9, max_grad_norm=1.0)
    op = clip.sgd_operands(space)
    scratch = [op.lr, clip.max_norm_tensor(cpu), clip._norm_out_tensor(cpu)]
    clip.prepare()
    held = {t.data_ptr() for t in clip.state_tensors()}
    assert {op.mom.data_ptr(), op.first.data_ptr()} <= held
    assert not held & {t.data_ptr() for t in scratch}
