"""Every dispatch path of csrc/kernels/bn.hip against the fp64 references of bn_reference.py, per
element and per channel (no tensor norms), on inputs whose channels differ from each other.

Each case first asserts, through the host-only kml_bn_plan query (computed by the launchers' own
predicates), that its shape takes the path it names, then launches through the public wrappers of
kubeml_amd/ops/kernels.py.  Every output and the partial-row buffer is followed by a NaN guard band
that must stay NaN.  Statistics reach the apply kernels as fp64 sums rounded to fp32 (or as fp32
partial rows of G row groups built here, empty groups included); mean / rstd reach the backward as
fp64 values rounded to fp32.

Documented limit of E[x^2] - mean^2: the largest cancellation factor amp_c exercised is 4.1e6 (M = 2,
C = 8: a channel whose two samples round to nearly the same bf16 value); the constant channel
x == 3.0 of every shape has 9.0e5 (var clamps to 0, rstd = rsqrt(eps)), and over the other channels
of the larger shapes amp_c stays below about 150 (mean 3, std 0.25).  The last test prints the
largest value (BN_AMP_MAX) next to the largest error / bound ratio of every quantity.
"""
import pytest
import torch

import bn_reference as R

pytestmark = pytest.mark.gpu

dev = "cuda"
GUARD = 1024
NAN = float("nan")


def _K():
    from kubeml_amd.ops import kernels as K
    return K


# ------------------------------------------------------------------------------------------
# shared inputs and references (built once per shape, never modified)
# ------------------------------------------------------------------------------------------

_CACHE = {}


def _memo(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _inputs(M, C):
    return _memo(("in", M, C), lambda: R.make_inputs(M, C, seed=3, device=dev))


def _st32(M, C):
    return _memo(("st", M, C), lambda: R.stats32(_inputs(M, C)["x"]))


def _saved(M, C):
    return _memo(("sv", M, C), lambda: R.saved32(_inputs(M, C)["x"]))


def _bref(M, C, has_y):
    def make():
        d = _inputs(M, C)
        return R.BwdRef(d["dy"], d["ymask"] if has_y else None, d["x"], *_saved(M, C))
    return _memo(("br", M, C, has_y), make)


def _guarded(n, dtype=torch.float32, init=None):
    """n elements followed by a NaN band; the elements are NaN too unless init is given."""
    buf = torch.full((n + GUARD,), NAN, dtype=dtype, device=dev)
    if init is not None:
        buf[:n] = init.reshape(-1)
    return buf


def _band_intact(*pairs):
    for buf, n in pairs:
        assert torch.isnan(buf[n:]).all(), "guard band written"


def _plan(kind, M, C, G=0, **expect):
    p = _K().bn_plan(kind, M, C, G)
    for k, v in expect.items():
        assert p[k] == v, f"plan {p} at M={M} C={C} G={G}: expected {k}={v}"
    return p


# ------------------------------------------------------------------------------------------
# forward apply
# ------------------------------------------------------------------------------------------

class Apply:
    """One bn_apply case: launch() into fresh guarded outputs, check() them against fp64."""

    def __init__(self, M, C, G=0, res=False, relu=False, training=True):
        self.M, self.C, self.G, self.relu, self.training = M, C, G, relu, training
        self.d = d = _inputs(M, C)
        self.res = d["res"] if res else None
        if G > 0:
            rows = _memo(("rows", M, C, G), lambda: R.stat_rows(d["x"], G, seed=G))
            self.sbuf = _guarded(G * 2 * C, init=rows)
            self.stats = self.sbuf[:G * 2 * C]
            self.ch = R.chan_from_stats(rows, M)
        else:
            self.sbuf = None
            self.stats = _st32(M, C)
            self.ch = R.chan_from_stats(self.stats, M)
        if not training:
            self.ch = R.chan_eval(d["run_mean"], d["run_var"])

    def launch(self):
        K, d, M, C = _K(), self.d, self.M, self.C
        o = dict(y=_guarded(M * C, torch.bfloat16), mean=_guarded(C), rstd=_guarded(C),
                 rm=_guarded(C, init=d["run_mean"]), rv=_guarded(C, init=d["run_var"]))
        K.bn_apply(d["x"], self.stats, d["gamma"], d["beta"], y=o["y"][:M * C].view(M, C), res=self.res,
                   save_mean=o["mean"][:C], save_rstd=o["rstd"][:C], run_mean=o["rm"][:C], run_var=o["rv"][:C],
                   relu=self.relu, training=self.training, stats_rows=self.G)
        return o

    def check(self, o):
        d, M, C = self.d, self.M, self.C
        torch.cuda.synchronize()
        _band_intact((o["y"], M * C), (o["mean"], C), (o["rstd"], C), (o["rm"], C), (o["rv"], C))
        if self.sbuf is not None:
            _band_intact((self.sbuf, self.G * 2 * C))
        R.accept_y(o["y"][:M * C].view(M, C), d["x"], self.ch, d["gamma"], d["beta"], res=self.res, relu=self.relu)
        if self.training:
            R.accept_saved(o["mean"][:C], o["rstd"][:C], self.ch)
            R.accept_running(o["rm"][:C], o["rv"][:C], d["run_mean"], d["run_var"], self.ch, M)
        else:   # eval: running statistics bit-unchanged, saved statistics not written
            assert torch.equal(o["rm"][:C].view(torch.int32), d["run_mean"].view(torch.int32))
            assert torch.equal(o["rv"][:C].view(torch.int32), d["run_var"].view(torch.int32))
            assert torch.isnan(o["mean"]).all() and torch.isnan(o["rstd"]).all()

    def run(self):
        o = self.launch()
        self.check(o)
        return o


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("M,C,V", [(37, 64, 1), (1031, 512, 2), (1031, 1024, 4), (1031, 2048, 8), (2, 8, 1)])
def test_apply_register_path(M, C, V, res, relu):
    _plan(_K().BN_PLAN_APPLY, M, C, reg=True, v=V, pipe=False, early=False, wide=False, fold=False)
    Apply(M, C, res=res, relu=relu).run()


def test_apply_pipelined():
    """n8 = 2097600: one full batch of 1024 * 256 * 8 chunks and a second one of 448."""
    M, C = 262200, 64
    assert M * C // 8 - 1024 * 256 * 8 == 448
    _plan(_K().BN_PLAN_APPLY, M, C, reg=True, v=8, pipe=True)
    Apply(M, C, res=True, relu=True).run()
    for k in [k for k in _CACHE if k[1:3] == (M, C)]:
        del _CACHE[k]


@pytest.mark.parametrize("M", [37, 1000])
@pytest.mark.parametrize("C", [24, 96, 136, 1000])
def test_apply_fallback_path(M, C):
    _plan(_K().BN_PLAN_APPLY, M, C, reg=False, v=0, wide=False, fold=False)
    Apply(M, C, res=(C % 16 == 8), relu=(M == 37)).run()


@pytest.mark.parametrize("M,C,G,early", [
    (37, 64, 1, True), (37, 64, 7, True), (37, 64, 129, True),          # 8 slices x 16 rows, then one more
    (1031, 512, 1, True), (1031, 512, 7, True), (1031, 512, 17, True),  # one slice
    (1031, 1024, 1, False), (1031, 1024, 7, False), (1031, 1024, 17, False)])
def test_apply_partial_rows_register(M, C, G, early):
    _plan(_K().BN_PLAN_APPLY, M, C, G, reg=True, early=early, wide=False, fold=False)
    Apply(M, C, G=G, res=(G == 7), relu=(G != 1)).run()


@pytest.mark.parametrize("M,C,G,wide", [(1000, 96, 80, False), (1000, 96, 81, True), (1000, 96, 300, True),
                                        (1000, 24, 7, False), (1000, 1000, 16, False), (1000, 1000, 17, True),
                                        (7000, 96, 7, False)])      # grid-stride loop of the fallback
def test_apply_partial_rows_fallback(M, C, G, wide):
    _plan(_K().BN_PLAN_APPLY, M, C, G, reg=False, wide=wide, fold=False)
    Apply(M, C, G=G, res=wide, relu=True).run()


@pytest.mark.parametrize("M,C,G,reg", [(37, 64, 1025, True), (1031, 512, 129, True), (1000, 96, 700, False)])
def test_apply_partial_rows_folded(M, C, G, reg):
    _plan(_K().BN_PLAN_APPLY, M, C, G, reg=reg, fold=True, wide=False)
    Apply(M, C, G=G, res=True, relu=True).run()


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("M,C,reg", [(37, 64, True), (1, 8, True), (1000, 96, False)])
def test_apply_eval_mode(M, C, reg, res, relu):
    _plan(_K().BN_PLAN_APPLY, M, C, reg=reg)
    Apply(M, C, res=res, relu=relu, training=False).run()


# ------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------

class Bwd:
    """One bn_bwd case (full, or partial=(rows, G)): launch() / check() as Apply."""

    def __init__(self, M, C, G=0, has_y=True, has_dres=True, accumulate=True, long_shape=False):
        self.M, self.C, self.G, self.has_dres, self.accumulate = M, C, G, has_dres, accumulate
        self.d = d = _inputs(M, C)
        self.ymask = d["ymask"] if has_y else None
        self.mean, self.rstd = _saved(M, C)
        self.tol = R.sum_tol(M, long_shape)
        if G > 0:
            rows = _memo(("brows", M, C, G, has_y),
                         lambda: R.bwd_rows(d["dy"], self.ymask, d["x"], self.mean, self.rstd, G, seed=G))
            self.pbuf = _guarded(G * 2 * C, init=rows)
            self.br = R.BwdRef(d["dy"], self.ymask, d["x"], self.mean, self.rstd, rows=rows)
        else:
            self.pbuf = None
            self.br = _bref(M, C, has_y)

    def outputs(self):
        d, M, C = self.d, self.M, self.C
        return dict(dx=_guarded(M * C, torch.bfloat16), dres=_guarded(M * C, torch.bfloat16),
                    dg=_guarded(C, init=d["prev_dgamma"]), db=_guarded(C, init=d["prev_dbeta"]))

    def call(self, o):
        d, M, C = self.d, self.M, self.C
        _K().bn_bwd(d["dy"], self.ymask, d["x"], self.mean, self.rstd, d["gamma"], o["dg"][:C], o["db"][:C],
                    dx=o["dx"][:M * C].view(M, C), dres=o["dres"][:M * C].view(M, C) if self.has_dres else None,
                    partial=(self.pbuf[:self.G * 2 * C], self.G) if self.G > 0 else None,
                    accumulate=self.accumulate)

    def launch(self):
        o = self.outputs()
        self.call(o)
        return o

    def check(self, o):
        d, M, C = self.d, self.M, self.C
        torch.cuda.synchronize()
        _band_intact((o["dx"], M * C), (o["dg"], C), (o["db"], C))
        if self.pbuf is not None:
            _band_intact((self.pbuf, self.G * 2 * C))
        prev = self.accumulate
        R.accept_dparams(o["dg"][:C], o["db"][:C], self.br, self.tol,
                         prev_dgamma=d["prev_dgamma"] if prev else None, prev_dbeta=d["prev_dbeta"] if prev else None)
        R.accept_dx(o["dx"][:M * C].view(M, C), d["dy"], self.ymask, d["x"], d["gamma"], self.br, self.tol)
        if self.has_dres:
            _band_intact((o["dres"], M * C))
            R.accept_dres(o["dres"][:M * C].view(M, C), d["dy"], self.ymask)
        else:
            assert torch.isnan(o["dres"]).all()

    def run(self, reproducible=True):
        o = self.launch()
        self.check(o)
        if reproducible:
            o2 = self.launch()
            torch.cuda.synchronize()
            for k in ("dx", "dg", "db"):
                assert torch.equal(o[k].view(torch.int16), o2[k].view(torch.int16)), f"{k} differs between two launches"
        return o


def _same_bits(a, b, keys):
    for k in keys:
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), f"{k}: pair differs from single launches"


class _reduce_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        K = _K()
        self.old, K._BN_REDUCE = K._BN_REDUCE, self.mode

    def __exit__(self, *a):
        _K()._BN_REDUCE = self.old


@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("mode", ["fused", "ticket", "atomic"])
@pytest.mark.parametrize("M,C,V", [(37, 64, 1), (1031, 512, 2), (1031, 1024, 4)])
def test_bwd_register_shapes_every_reduce_mode(M, C, V, mode, accumulate):
    """dgamma / dbeta hold earlier random gradients: accumulate adds onto them, accumulate=False
    overwrites them, and dx never sees them.  (1031, 1024) also folds its 129 reduction rows."""
    _plan(_K().BN_PLAN_BWD, M, C, reg=True, v=V, pipe=False, early=(C <= 512), fold=(C == 1024))
    with _reduce_mode(mode):
        Bwd(M, C, accumulate=accumulate).run(reproducible=mode != "atomic")


def test_bwd_pipelined():
    M, C = 131100, 64
    assert M * C // 8 > 1024 * 256 * 4
    _plan(_K().BN_PLAN_BWD, M, C, reg=True, v=4, pipe=True)
    Bwd(M, C, long_shape=True).run()
    for k in [k for k in _CACHE if k[1:3] == (M, C)]:
        del _CACHE[k]


@pytest.mark.parametrize("has_y", [True, False])
@pytest.mark.parametrize("M,C,wide", [(37, 24, False), (1000, 24, False), (37, 96, False), (1000, 96, False),
                                      (1000, 136, False), (7000, 96, True)])
def test_bwd_fallback_path(M, C, wide, has_y):
    """(7000, 96): 84 reduction rows over 5 slices, the 1024-thread finish; its 256-thread twin
    grid-strides at the same shape through bn_bwd(partial=...) below."""
    _plan(_K().BN_PLAN_BWD, M, C, reg=False, wide=wide, fold=False)
    Bwd(M, C, has_y=has_y, has_dres=has_y, accumulate=not has_y).run()


@pytest.mark.parametrize("has_y,has_dres,accumulate", [(True, True, True), (False, False, False),
                                                       (True, False, False), (False, True, True)])
@pytest.mark.parametrize("M,C,G,expect", [
    (37, 64, 1, dict(reg=True, v=1, early=True, fold=False)),
    (37, 64, 7, dict(reg=True, v=1, early=True, fold=False)),
    (37, 64, 129, dict(reg=True, v=1, early=True, fold=False)),
    (1031, 1024, 17, dict(reg=True, v=4, early=False, fold=False)),
    (1031, 512, 129, dict(reg=True, v=2, early=True, fold=True)),
    (1000, 96, 81, dict(reg=False, wide=True, fold=False)),
    (7000, 96, 7, dict(reg=False, wide=False, fold=False)),
    (1000, 96, 700, dict(reg=False, wide=False, fold=True))])
def test_bwd_partial_rows(M, C, G, expect, has_y, has_dres, accumulate):
    _plan(_K().BN_PLAN_BWD_PARTIAL, M, C, G, **expect)
    Bwd(M, C, G=G, has_y=has_y, has_dres=has_dres, accumulate=accumulate).run()


# ------------------------------------------------------------------------------------------
# paired launches
# ------------------------------------------------------------------------------------------

_V_SHAPE = {1: (37, 64), 2: (1031, 512), 4: (1031, 1024)}


@pytest.mark.parametrize("va,vb,Ga,pairs", [(1, 1, 0, 1), (1, 2, 0, 1), (2, 1, 0, 1), (2, 2, 0, 1), (1, 1, 7, 1),
                                            (4, 1, 0, 0), ("fallback", 1, 0, 0)])
def test_apply_pair(va, vb, Ga, pairs):
    K = _K()
    sa = (37, 24) if va == "fallback" else _V_SHAPE[va]
    sb = (1000, 64) if vb == 1 and va == 1 else _V_SHAPE[vb]   # two different V = 1 tensors
    if va == "fallback":
        _plan(K.BN_PLAN_APPLY, *sa, reg=False)
    else:
        _plan(K.BN_PLAN_APPLY, *sa, Ga, reg=True, v=va, pipe=False, wide=False)
    _plan(K.BN_PLAN_APPLY, *sb, reg=True, v=vb, pipe=False)
    a, b = Apply(*sa, G=Ga, res=True, relu=True), Apply(*sb, res=False, relu=True)
    oa, ob = a.run(), b.run()
    n0 = K.BN_PAIRS_LAUNCHED[0]
    with K.bn_apply_pair():
        pa = a.launch()
        pb = b.launch()
    assert K.BN_PAIRS_LAUNCHED[0] - n0 == pairs
    a.check(pa)
    b.check(pb)
    keys = ("y", "mean", "rstd", "rm", "rv")
    _same_bits(oa, pa, keys)
    _same_bits(ob, pb, keys)


@pytest.mark.parametrize("va,vb", [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)])
@pytest.mark.parametrize("kinds", ["full-full", "full-partial", "partial-partial"])
def test_bwd_pair(kinds, va, vb):
    """Both calls record; V in {1, 2} pairs share one apply launch, a V = 4 member launches singly."""
    K = _K()
    ka, kb = kinds.split("-")
    sa = _V_SHAPE[va]
    sb = (1000, 64) if vb == 1 and va == 1 else _V_SHAPE[vb]
    Ga, Gb = (7 if ka == "partial" else 0), (17 if kb == "partial" else 0)
    _plan(K.BN_PLAN_BWD_PARTIAL if Ga else K.BN_PLAN_BWD, *sa, Ga, reg=True, v=va, pipe=False)
    _plan(K.BN_PLAN_BWD_PARTIAL if Gb else K.BN_PLAN_BWD, *sb, Gb, reg=True, v=vb, pipe=False)
    a, b = Bwd(*sa, G=Ga, accumulate=True), Bwd(*sb, G=Gb, has_y=False, accumulate=False)
    oa, ob = a.run(reproducible=False), b.run(reproducible=False)
    n0 = K.BNB_PAIRS[0]
    pa, pb = a.outputs(), b.outputs()
    with K.bn_bwd_pair():
        a.call(pa)
        b.call(pb)
    assert K.BNB_PAIRS[0] - n0 == 1
    a.check(pa)
    b.check(pb)
    _same_bits(oa, pa, ("dx", "dres", "dg", "db"))
    _same_bits(ob, pb, ("dx", "dres", "dg", "db"))


# ------------------------------------------------------------------------------------------
# statistics kernels
# ------------------------------------------------------------------------------------------

STAT_SHAPES = [(M, C) for M in (1, 37, 1031) for C in (8, 24, 64, 2048)] + [(4096, 64)]


@pytest.mark.parametrize("M,C", STAT_SHAPES)
def test_bn_stats(M, C):
    x = _inputs(M, C)["x"]
    buf = _guarded(2 * C, init=torch.zeros(2 * C, device=dev))
    _K().bn_stats(x, buf[:2 * C])
    torch.cuda.synchronize()
    _band_intact((buf, 2 * C))
    R.accept_stats(buf[:2 * C], x)


@pytest.mark.parametrize("M,C", STAT_SHAPES)
def test_bn_stats_part(M, C):
    K = _K()
    x = _inputs(M, C)["x"]
    part, G = K.bn_stats_part(x)
    assert G == K.HIP.raw("kml_bn_stats_rows", M, C) and part.numel() == G * 2 * C
    # the same launch into a NaN buffer: every one of the G rows is written, nothing after them
    buf = _guarded(G * 2 * C)
    K.HIP.call("kml_bn_stats_part", "p p l i s", x.data_ptr(), buf.data_ptr(), M, C, K._s())
    torch.cuda.synchronize()
    _band_intact((buf, G * 2 * C))
    assert not torch.isnan(buf[:G * 2 * C]).any()
    assert torch.equal(buf[:G * 2 * C], part)
    # the rows' fp64 total: each row is a chain of its own, the G rows are added exactly here
    R.accept_stats(part.view(G, 2 * C).double().sum(0), x)
    if M == 1:
        return
    # and bn_apply consumes them
    d = _inputs(M, C)
    ch = R.chan_from_stats(part.view(G, 2 * C), M)
    mean, rstd = _guarded(C), _guarded(C)
    y = K.bn_apply(x, part, d["gamma"], d["beta"], save_mean=mean[:C], save_rstd=rstd[:C], stats_rows=G)
    R.accept_y(y, x, ch, d["gamma"], d["beta"])
    R.accept_saved(mean[:C], rstd[:C], ch)


# ------------------------------------------------------------------------------------------
# ReLU alone
# ------------------------------------------------------------------------------------------

def _relu_input(n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    big, tiny = 3.3895313892515355e38, 1.1754943508222875e-38   # largest finite / smallest normal bf16
    table = torch.tensor([0.0, -0.0, big, -big, tiny, -tiny, float("inf"), -float("inf"), 1.0, -1.0],
                         device=dev).to(torch.bfloat16)
    t = torch.randn(n, generator=g, device=dev).to(torch.bfloat16)
    pick = torch.randint(0, 3 * table.numel(), (n,), generator=g, device=dev)
    t = torch.where(pick < table.numel(), table[pick % table.numel()], t)
    t[:table.numel() if n >= table.numel() else n] = table[:n]
    return t


@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (2048 * 256 + 257)])
def test_relu_fwd_bwd_exact(n):
    K = _K()
    x, dy = _relu_input(n, 1), _relu_input(n, 2).flip(0)
    y = K.relu_fwd(x)
    assert torch.equal(y, torch.relu(x))     # by value: the sign of a zero output is not specified
    dx = K.relu_bwd(dy, x)
    ref = torch.where(x.float() > 0, dy, torch.zeros_like(dy))
    assert torch.equal(dx.view(torch.int16), ref.view(torch.int16))


def test_zz_report_largest_error_to_bound_ratios():
    """Headroom report (printed with -s): the largest error / bound each acceptance function saw."""
    for k in sorted(R.RATIOS):
        print(f"BN_RATIO {k:10s} {R.RATIOS[k]:.4f}")
    print(f"BN_AMP_MAX {R.AMP_MAX[0]:.4g}")
    assert all(v <= 1.0 for v in R.RATIOS.values())
