"""The BatchNorm kernels request every per-channel operand (gamma, beta, running / saved statistics,
old gradients) at their top, before the row reduction, for a thread's first two channels
(bn.hip BN_HOIST; 512 channels at 256 threads) and inside the coefficient loop for later ones.

A hoisted load is predicated as its use is: on a non-null pointer, on block 0 for the bookkeeping
vectors, on ``accumulate`` for the old gradients.  So every case here runs with operands given and
``None``, with channel counts on both sides of the hoisting bound (8 .. 512 below it; 1024 one step
and 2048 three steps past it; 96 and 2056 on the fallback kernels), into NaN-guarded buffers, and is
judged per element and per channel against the fp64 references of bn_reference.py.
"""
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu

dev = "cuda"
GUARD = 1024
NAN = float("nan")

# (M, C): the channel count per thread is what matters, not the size
SHAPES = [(2, 8), (37, 64), (37, 512), (37, 1024), (37, 2048), (37, 96)]
FWD_SHAPES = SHAPES + [(37, 2056)]          # nine channels per thread on the fallback kernel
REG = {8: True, 64: True, 512: True, 1024: True, 2048: True, 96: False, 2056: False}


def _K():
    from kubeml_amd.ops import kernels as K
    return K


_CACHE = {}


def _memo(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _inputs(M, C, seed=5):
    return _memo(("in", M, C, seed), lambda: R.make_inputs(M, C, seed=seed, device=dev))


def _stats(M, C, G, seed=5):
    """fp32 statistics as handed to the kernel: final sums (G = 0) or G partial rows."""
    x = _inputs(M, C, seed)["x"]
    if G == 0:
        return _memo(("st", M, C, seed), lambda: R.stats32(x))
    return _memo(("rows", M, C, G, seed), lambda: R.stat_rows(x, G, seed=G))


def _saved(M, C):
    return _memo(("sv", M, C), lambda: R.saved32(_inputs(M, C)["x"]))


def _guarded(n, dtype=torch.float32, init=None):
    buf = torch.full((n + GUARD,), NAN, dtype=dtype, device=dev)
    if init is not None:
        buf[:n] = init.reshape(-1)
    return buf


def _band_intact(*pairs):
    for buf, n in pairs:
        assert torch.isnan(buf[n:]).all(), "guard band written"


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: bits differ"


# ------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------

# res, relu, gamma / beta given, saved statistics given, running statistics given
VARIANTS = [(True, True, True, True, True), (False, False, False, False, True), (True, True, True, False, False),
            (False, False, True, True, False), (True, False, True, True, True), (False, True, False, True, True),
            (True, False, False, False, False), (False, True, True, False, True)]


def _apply(M, C, G, res, relu, affine, save, run, seed=5, training=True, rm=None, rv=None):
    """One bn_apply into guarded outputs, checked against fp64; returns the outputs."""
    K, d = _K(), _inputs(M, C, seed)
    stats = _stats(M, C, G, seed)
    sbuf = _guarded(stats.numel(), init=stats)
    ch = R.chan_from_stats(stats, M) if training else R.chan_eval(d["run_mean"], d["run_var"])
    o = dict(y=_guarded(M * C, torch.bfloat16), mean=_guarded(C), rstd=_guarded(C),
             rm=_guarded(C, init=d["run_mean"]) if rm is None else rm,
             rv=_guarded(C, init=d["run_var"]) if rv is None else rv)
    old_rm, old_rv = o["rm"][:C].clone(), o["rv"][:C].clone()
    gamma, beta = (d["gamma"], d["beta"]) if affine else (None, None)
    K.bn_apply(d["x"], sbuf[:stats.numel()], gamma, beta, y=o["y"][:M * C].view(M, C),
               res=d["res"] if res else None, save_mean=o["mean"][:C] if save else None,
               save_rstd=o["rstd"][:C] if save else None, run_mean=o["rm"][:C] if run else None,
               run_var=o["rv"][:C] if run else None, relu=relu, training=training, stats_rows=G)

    def check():
        torch.cuda.synchronize()
        _band_intact((o["y"], M * C), (o["mean"], C), (o["rstd"], C), (o["rm"], C), (o["rv"], C),
                     (sbuf, stats.numel()))
        R.accept_y(o["y"][:M * C].view(M, C), d["x"], ch, d["gamma"] if affine else torch.ones_like(d["gamma"]),
                   d["beta"] if affine else torch.zeros_like(d["beta"]), res=d["res"] if res else None, relu=relu)
        if training and save:
            R.accept_saved(o["mean"][:C], o["rstd"][:C], ch)
        else:
            assert torch.isnan(o["mean"]).all() and torch.isnan(o["rstd"]).all()
        if training and run:
            R.accept_running(o["rm"][:C], o["rv"][:C], old_rm, old_rv, ch, M)
        else:   # not given, or eval mode: bit-unchanged
            _same_bits(o["rm"][:C], old_rm, "run_mean")
            _same_bits(o["rv"][:C], old_rv, "run_var")
    o["check"] = check
    return o


@pytest.mark.parametrize("G", [0, 1, 8, 33])
@pytest.mark.parametrize("M,C", FWD_SHAPES)
def test_forward_training(M, C, G):
    assert _K().bn_plan(_K().BN_PLAN_APPLY, M, C, G)["reg"] == REG[C]
    for res, relu, affine, save, run in VARIANTS:
        _apply(M, C, G, res, relu, affine, save, run)["check"]()


@pytest.mark.parametrize("M,C", [(2100, 256), (1031, 512)])
def test_forward_two_chunks_per_thread(M, C):
    """V = 2 kernels hoist one channel iteration: C = 256 is all hoisted, C = 512 half in the loop."""
    assert _K().bn_plan(_K().BN_PLAN_APPLY, M, C, 8)["v"] == 2
    for res, relu, affine, save, run in VARIANTS[:4]:
        _apply(M, C, 8, res, relu, affine, save, run)["check"]()


@pytest.mark.parametrize("M,C", [(37, 64), (37, 1024), (37, 96)])
def test_running_statistics_over_three_launches(M, C):
    """The same run_mean / run_var through three launches with different inputs.  Each step of the
    fp64 recurrence is judged from the fp32 values the launch found in the buffers (what the
    previous launch stored), so a stale or doubled read fails at the second launch."""
    d = _inputs(M, C)
    rm, rv = _guarded(C, init=d["run_mean"]), _guarded(C, init=d["run_var"])
    seen = [rm[:C].clone()]
    for seed in (5, 6, 7):
        _apply(M, C, 8, False, False, True, True, True, seed=seed, rm=rm, rv=rv)["check"]()
        seen.append(rm[:C].clone())
    assert all(not torch.equal(a, b) for a, b in zip(seen, seen[1:]))


@pytest.mark.parametrize("M,C", [(1, 8), (37, 512), (37, 1024)])
def test_eval_mode(M, C):
    for res, relu, affine in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        _apply(M, C, 0, res, relu, affine, True, True, training=False)["check"]()


# ------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------

def _bwd(M, C, G, has_y, has_dres, dg, db, prev, affine=True):
    """One bn_bwd (G > 0: partial rows) into dg / db (guarded [C] buffers) -> check()."""
    K, d = _K(), _inputs(M, C)
    mean, rstd = _saved(M, C)
    ymask = d["ymask"] if has_y else None
    pbuf = None
    if G > 0:
        rows = _memo(("brows", M, C, G, has_y), lambda: R.bwd_rows(d["dy"], ymask, d["x"], mean, rstd, G, seed=G))
        pbuf = _guarded(G * 2 * C, init=rows)
        br = R.BwdRef(d["dy"], ymask, d["x"], mean, rstd, rows=rows)
    else:
        br = _memo(("br", M, C, has_y), lambda: R.BwdRef(d["dy"], ymask, d["x"], mean, rstd))
    dx, dres = _guarded(M * C, torch.bfloat16), _guarded(M * C, torch.bfloat16)
    gamma = d["gamma"] if affine else torch.ones_like(d["gamma"])
    K.bn_bwd(d["dy"], ymask, d["x"], mean, rstd, gamma if affine else None, dg[:C], db[:C], dx=dx[:M * C].view(M, C),
             dres=dres[:M * C].view(M, C) if has_dres else None,
             partial=(pbuf[:G * 2 * C], G) if G > 0 else None, accumulate=prev is not None)

    def check():
        torch.cuda.synchronize()
        _band_intact((dx, M * C), (dg, C), (db, C))
        if pbuf is not None:
            _band_intact((pbuf, G * 2 * C))
        assert torch.isfinite(dg[:C]).all() and torch.isfinite(db[:C]).all()
        R.accept_dparams(dg[:C], db[:C], br, prev_dgamma=None if prev is None else prev[0],
                         prev_dbeta=None if prev is None else prev[1])
        R.accept_dx(dx[:M * C].view(M, C), d["dy"], ymask, d["x"], gamma, br)
        if has_dres:
            _band_intact((dres, M * C))
            R.accept_dres(dres[:M * C].view(M, C), d["dy"], ymask)
        else:
            assert torch.isnan(dres).all()
    return dict(dx=dx, dres=dres, check=check)


@pytest.mark.parametrize("G", [0, 1, 33])
@pytest.mark.parametrize("has_y", [True, False])
@pytest.mark.parametrize("M,C", SHAPES)
def test_backward(M, C, G, has_y):
    """accumulate=True twice into the same dgamma / dbeta: the second result is the first plus the
    sums.  accumulate=False into NaN (and without gamma): dgamma / dbeta finite and correct, dx
    never sees the NaN."""
    kind = _K().BN_PLAN_BWD_PARTIAL if G else _K().BN_PLAN_BWD
    assert _K().bn_plan(kind, M, C, G)["reg"] == REG[C]
    d = _inputs(M, C)
    dg, db = _guarded(C, init=d["prev_dgamma"]), _guarded(C, init=d["prev_dbeta"])
    _bwd(M, C, G, has_y, has_y, dg, db, prev=(d["prev_dgamma"], d["prev_dbeta"]))["check"]()
    first = dg[:C].clone(), db[:C].clone()
    _bwd(M, C, G, has_y, has_y, dg, db, prev=first)["check"]()
    dg, db = _guarded(C), _guarded(C)
    _bwd(M, C, G, has_y, not has_y, dg, db, prev=None, affine=False)["check"]()


# ------------------------------------------------------------------------------------------
# pair kernels
# ------------------------------------------------------------------------------------------

def test_apply_pair():
    """Two applies of different channel counts and row counts in one launch, one of them without
    affine parameters and running statistics: each half equals its single launch bit for bit."""
    K = _K()
    a_args, b_args = (37, 64, 7, True, False, True, True, True), (37, 512, 16, False, True, False, True, False)
    sa, sb = _apply(*a_args), _apply(*b_args)
    sa["check"]()
    sb["check"]()
    n0 = K.BN_PAIRS_LAUNCHED[0]
    with K.bn_apply_pair():
        pa, pb = _apply(*a_args), _apply(*b_args)
    assert K.BN_PAIRS_LAUNCHED[0] - n0 == 1
    pa["check"]()
    pb["check"]()
    for k in ("y", "mean", "rstd", "rm", "rv"):
        _same_bits(pa[k], sa[k], k)
        _same_bits(pb[k], sb[k], k)


def test_bwd_pair():
    """The backward pair: one half accumulates onto earlier gradients, the other overwrites NaN."""
    K = _K()
    da = _inputs(37, 64)

    def run(pair):
        dga, dba = _guarded(64, init=da["prev_dgamma"]), _guarded(64, init=da["prev_dbeta"])
        dgb, dbb = _guarded(512), _guarded(512)
        if pair:
            n0 = K.BNB_PAIRS[0]
            with K.bn_bwd_pair():
                a = _bwd(37, 64, 7, True, True, dga, dba, prev=(da["prev_dgamma"], da["prev_dbeta"]))
                b = _bwd(37, 512, 17, False, False, dgb, dbb, prev=None)
            assert K.BNB_PAIRS[0] - n0 == 1
        else:
            a = _bwd(37, 64, 7, True, True, dga, dba, prev=(da["prev_dgamma"], da["prev_dbeta"]))
            b = _bwd(37, 512, 17, False, False, dgb, dbb, prev=None)
        a["check"]()
        b["check"]()
        return a["dx"], a["dres"], dga, dba, b["dx"], dgb, dbb
    for i, (s, p) in enumerate(zip(run(False), run(True))):
        _same_bits(s, p, f"output {i}")


# ------------------------------------------------------------------------------------------
# stem: BN + ReLU + max-pool
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,s,p,G", [(3, 2, 1, 8), (3, 2, 1, 130), (2, 2, 0, 8), (3, 2, 1, 0)])
def test_bn_relu_maxpool_matches_unfused(k, s, p, G):
    """[2, 8, 8, 64] with partial rows (k = 2: the generic kernel) against bn_apply + maxpool_fwd,
    bit for bit; the counters arena moves by one per launch.  G = 130 runs the 512-thread variant,
    which sums the rows over 16 slices where bn_apply uses 8: its statistics are judged against
    fp64 instead, and its pooled values may sit one bf16 step (2^-7 relative) from the unfused ones."""
    K = _K()
    B, H, W, C = 2, 8, 8, 64
    M = B * H * W
    d = _inputs(M, C)
    x4 = d["x"].view(B, H, W, C)
    stats = _stats(M, C, G)
    ch = R.chan_from_stats(stats, M)
    ref = dict(mean=_guarded(C), rstd=_guarded(C), rm=_guarded(C, init=d["run_mean"]), rv=_guarded(C, init=d["run_var"]))
    y = K.bn_apply(d["x"], stats, d["gamma"], d["beta"], save_mean=ref["mean"][:C], save_rstd=ref["rstd"][:C],
                   run_mean=ref["rm"][:C], run_var=ref["rv"][:C], relu=True, stats_rows=G)
    R.accept_y(y, d["x"], ch, d["gamma"], d["beta"], relu=True)
    py, pidx = K.maxpool_fwd(y.view(B, H, W, C), k, s, p)
    got = dict(mean=_guarded(C), rstd=_guarded(C), rm=_guarded(C, init=d["run_mean"]), rv=_guarded(C, init=d["run_var"]))
    init = torch.tensor([0, 41, 2 ** 40, -3, 7], dtype=torch.int64, device=dev)
    cbuf = torch.full((5 + 8,), -77, dtype=torch.int64, device=dev)
    cbuf[:5] = init
    fy, fidx = K.bn_relu_maxpool(x4, stats, d["gamma"], d["beta"], k, s, p, save_mean=got["mean"][:C],
                                 save_rstd=got["rstd"][:C], run_mean=got["rm"][:C], run_var=got["rv"][:C],
                                 stats_rows=G, counters=cbuf[:5])
    torch.cuda.synchronize()
    assert torch.equal(cbuf[:5], init + 1) and (cbuf[5:] == -77).all()
    same_order = G < 128

    def pooled_match(a, b, ia, ib, what):
        if same_order:
            _same_bits(a, b, what)
            assert torch.equal(ia, ib)
        else:
            assert ((a.double() - b.double()).abs() <= R.P(-7) * b.double().abs()).all(), what
    pooled_match(fy, py, fidx, pidx, "pooled")
    for key in ("mean", "rstd", "rm", "rv"):
        _band_intact((got[key], C))
        if same_order:
            _same_bits(got[key], ref[key], key)
    R.accept_saved(got["mean"][:C], got["rstd"][:C], ch)
    R.accept_running(got["rm"][:C], got["rv"][:C], d["run_mean"], d["run_var"], ch, M)
    # a second launch without the optional vectors: the counters move once more, nothing else does
    fy2, fidx2 = K.bn_relu_maxpool(x4, stats, None, None, k, s, p, stats_rows=G, counters=cbuf[:5])
    torch.cuda.synchronize()
    assert torch.equal(cbuf[:5], init + 2) and (cbuf[5:] == -77).all()
    y1 = K.bn_apply(d["x"], stats, None, None, relu=True, stats_rows=G)
    py1, pidx1 = K.maxpool_fwd(y1.view(B, H, W, C), k, s, p)
    pooled_match(fy2, py1, fidx2, pidx1, "pooled, no affine")


# ------------------------------------------------------------------------------------------
# halo conv with the input's BN applied while the patch is staged
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("affine,track", [(True, True), (False, False)])
def test_halo_bnin_matches_bn_then_conv(affine, track):
    """conv_fwd_bnin on a [4, 4, 4, 128] input against bn_apply followed by conv_fwd: normalised
    input, statistics and conv output bit-identical (same rows, same order, same arithmetic)."""
    K = _K()
    B, H, C = 4, 4, 128
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    bf = lambda *s, k=1.0: (torch.randn(*s, generator=g, device=dev) * k).to(torch.bfloat16)
    x, w1, w2 = bf(B, H, H, C), bf(C, 3, 3, C, k=(9 * C) ** -0.5), bf(C, 3, 3, C, k=(9 * C) ** -0.5)
    d = _inputs(37, C)
    gamma, beta = (d["gamma"], d["beta"]) if affine else (None, None)
    assert K.bnin_ok(x.shape, C, 3, 3, (1, 1), (1, 1))
    G = K.conv_fwd_stats_rows(x.shape, C, 3, 3, (1, 1), (1, 1))
    rows = _guarded(G * 2 * C)
    c1 = K.conv_fwd(x, w1, 3, 3, (1, 1), (1, 1), stats=rows[:G * 2 * C], stats_part=True)
    st2 = torch.empty(2, G * 2 * C, device=dev)      # the second conv's own statistics rows
    outs = []
    for fold in (False, True):
        o = dict(mean=_guarded(C), rstd=_guarded(C), rm=_guarded(C, init=d["run_mean"]),
                 rv=_guarded(C, init=d["run_var"]), y=_guarded(c1.numel(), torch.bfloat16))
        y = o["y"][:c1.numel()].view_as(c1)
        rm, rv = (o["rm"][:C], o["rv"][:C]) if track else (None, None)
        if fold:
            o["o"] = K.conv_fwd_bnin(c1, w2, rows[:G * 2 * C], G, gamma, beta, o["mean"][:C], o["rstd"][:C], rm, rv,
                                     1e-5, 0.1, y, stats=st2[1])
        else:
            K.bn_apply(c1.view(-1, C), rows[:G * 2 * C], gamma, beta, y=y.view(-1, C), save_mean=o["mean"][:C],
                       save_rstd=o["rstd"][:C], run_mean=rm, run_var=rv, relu=True, stats_rows=G)
            o["o"] = K.conv_fwd(y, w2, 3, 3, (1, 1), (1, 1), stats=st2[0], stats_part=True)
        outs.append(o)
    torch.cuda.synchronize()
    _band_intact((rows, G * 2 * C))
    ch = R.chan_from_stats(rows[:G * 2 * C].view(G, 2 * C), B * H * H)
    ones, zeros = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    R.accept_y(outs[1]["y"][:c1.numel()].view(-1, C), c1.view(-1, C), ch, gamma if affine else ones,
               beta if affine else zeros, relu=True)
    for key in ("y", "mean", "rstd", "rm", "rv"):
        _band_intact((outs[1][key], outs[1][key].numel() - GUARD))
        _same_bits(outs[1][key], outs[0][key], key)
    if track:
        R.accept_running(outs[1]["rm"][:C], outs[1]["rv"][:C], d["run_mean"], d["run_var"], ch, B * H * H)
    _same_bits(outs[1]["o"], outs[0]["o"], "conv output")
    _same_bits(st2[1], st2[0], "conv output statistics rows")
