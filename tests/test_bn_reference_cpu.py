"""The BatchNorm acceptance functions of bn_reference.py can fail: an fp32 twin of the formulas
(sequential sums) passes every one of them on the generator's inputs, and each of a fixed list of
wrong implementations is rejected by at least one."""
import pytest
import torch

import bn_reference as R

SHAPES = [(37, 8), (1000, 24), (1031, 256), (4096, 64)]


class Case:
    """Inputs, references and the twin's outputs at one shape (built once per shape)."""

    def __init__(self, M, C):
        self.M, self.C = M, C
        d = R.make_inputs(M, C, seed=1)
        self.d = d
        self.st32 = R.stats32(d["x"])
        self.ch = R.chan_from_stats(self.st32, M)
        self.mean32, self.rstd32 = R.saved32(d["x"])
        self.br = R.BwdRef(d["dy"], d["ymask"], d["x"], self.mean32, self.rstd32)
        self.stats = R.twin_stats(d["x"])
        self.fwd = R.twin_apply(d["x"], self.st32, d["gamma"], d["beta"], res=d["res"], relu=True,
                                run_mean=d["run_mean"], run_var=d["run_var"])
        self.bwd = R.twin_bwd(d["dy"], d["ymask"], d["x"], self.mean32, self.rstd32, d["gamma"])

    def judge_fwd(self, y, mean, rstd, rm, rv):
        d = self.d
        R.accept_y(y, d["x"], self.ch, d["gamma"], d["beta"], res=d["res"], relu=True)
        R.accept_saved(mean, rstd, self.ch)
        R.accept_running(rm, rv, d["run_mean"], d["run_var"], self.ch, self.M)

    def judge_bwd(self, dx, dres, dgamma, dbeta, prev=False):
        d = self.d
        R.accept_dparams(dgamma, dbeta, self.br, prev_dgamma=d["prev_dgamma"] if prev else None,
                         prev_dbeta=d["prev_dbeta"] if prev else None)
        R.accept_dx(dx, d["dy"], d["ymask"], d["x"], d["gamma"], self.br)
        R.accept_dres(dres, d["dy"], d["ymask"])


_CASES = {}


@pytest.fixture(params=SHAPES, ids=lambda s: f"M{s[0]}-C{s[1]}")
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(*request.param)
    return _CASES[request.param]


def test_generator_makes_channels_distinguishable(case):
    d, ch = case.d, case.ch
    g = d["gamma"]
    assert (g[::5] < 0).all() and g[R.ZERO_GAMMA_CH] == 0 and ((g.abs() >= 0.5) | (g == 0)).all()
    assert int((g < 0).sum()) == len(range(0, case.C, 5)) and int((g == 0).sum()) == 1
    assert (d["x"][:, R.CONST_CH] == 3.0).all() and ch.var[R.CONST_CH] == 0
    assert abs(float(ch.rstd[R.CONST_CH]) - R.EPS ** -0.5) < 1e-9
    # no two channels share a mean: a value landing on a neighbour's channel is an error
    m = torch.sort(ch.mean).values
    assert (m[1:] - m[:-1]).min() > 1e-4
    ym = d["ymask"].float()
    neg0 = (ym == 0) & torch.signbit(ym)
    pos0 = (ym == 0) & ~torch.signbit(ym)
    assert neg0.any() and pos0.any() and (ym < 0).any() and (ym > 0).any()


def test_fp32_twin_passes_every_acceptance_function(case):
    d = case.d
    R.accept_stats(case.stats, d["x"])
    case.judge_fwd(*case.fwd)
    case.judge_bwd(*case.bwd)
    # accumulate onto earlier gradients, eval mode, no residual / ReLU, partial rows
    dx, dres, dg, db = R.twin_bwd(d["dy"], d["ymask"], d["x"], case.mean32, case.rstd32, d["gamma"],
                                  prev_dgamma=d["prev_dgamma"], prev_dbeta=d["prev_dbeta"])
    case.judge_bwd(dx, dres, dg, db, prev=True)
    y = R.twin_apply(d["x"], None, d["gamma"], d["beta"], run_mean=d["run_mean"], run_var=d["run_var"],
                     training=False)[0]
    R.accept_y(y, d["x"], R.chan_eval(d["run_mean"], d["run_var"]), d["gamma"], d["beta"])
    rows = R.stat_rows(d["x"], 7, seed=2)
    chr_ = R.chan_from_stats(rows, case.M)
    y, mean, rstd, _, _ = R.twin_apply(d["x"], rows, d["gamma"], d["beta"])
    R.accept_y(y, d["x"], chr_, d["gamma"], d["beta"])
    R.accept_saved(mean, rstd, chr_)
    dx, dres, dg, db = R.twin_bwd(d["dy"], None, d["x"], case.mean32, case.rstd32, d["gamma"])
    br = R.BwdRef(d["dy"], None, d["x"], case.mean32, case.rstd32)
    R.accept_dparams(dg, db, br)
    R.accept_dx(dx, d["dy"], None, d["x"], d["gamma"], br)
    R.accept_dres(dres, d["dy"], None)


def _rejected(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def test_mutant_one_element_off_by_one_bf16_ulp(case):
    d = case.d
    y, mean, rstd, rm, rv = case.fwd
    y64 = torch.cat([R.y_ref(d["x"], case.ch, d["gamma"], d["beta"], d["res"], True)[0]])
    r = int((y64[:, 1].abs() > 0.5).nonzero()[0])
    bad = y.clone()
    bad[r, 1] = R.bf16_next(y[r, 1].reshape(1), y64[r, 1].reshape(1))[0]
    assert (bad != y).sum() == 1
    assert _rejected(case.judge_fwd, bad, mean, rstd, rm, rv)
    dx = case.bwd[0]
    d64 = R.dx_ref(d["dy"], d["ymask"], d["x"], d["gamma"], case.br)[0]
    r = int((d64[:, 1].abs() > 0.25).nonzero()[0])
    bad = dx.clone()
    bad[r, 1] = R.bf16_next(dx[r, 1].reshape(1), d64[r, 1].reshape(1))[0]
    assert _rejected(case.judge_bwd, bad, *case.bwd[1:])


def test_mutant_save_mean_swapped_with_neighbour(case):
    y, mean, rstd, rm, rv = case.fwd
    bad = mean.clone()
    bad[[4, 5]] = mean[[5, 4]]
    assert _rejected(case.judge_fwd, y, bad, rstd, rm, rv)
    # and a y whose channels 4 and 5 used each other's statistics
    d = case.d
    st = case.st32.clone().view(2, -1)
    st[:, [4, 5]] = st[:, [5, 4]]
    ybad = R.twin_apply(d["x"], st.reshape(-1), d["gamma"], d["beta"], res=d["res"], relu=True)[0]
    assert _rejected(case.judge_fwd, ybad, mean, rstd, rm, rv)


def test_mutant_last_row_dropped_from_the_sums(case):
    d = case.d
    short = R.twin_stats(d["x"][:-1])
    assert _rejected(R.accept_stats, short, d["x"])
    # dbeta: drop the last row whose ReLU mask keeps it, per channel
    dx, dres, dg, db = case.bwd
    keep = d["ymask"].float() > 0
    last = case.M - 1 - torch.flip(keep, [0]).int().argmax(0)
    cols = torch.arange(case.C)
    assert keep[last, cols].all()
    bad = db - d["dy"].float()[last, cols]
    assert _rejected(case.judge_bwd, dx, dres, dg, bad)


def test_mutant_relu_mask_keeps_zeros(case):
    d = case.d
    out = R.twin_bwd(d["dy"], d["ymask"], d["x"], case.mean32, case.rstd32, d["gamma"], ge=True)
    assert _rejected(case.judge_bwd, *out)
    # each output alone gives it away
    assert _rejected(R.accept_dres, out[1], d["dy"], d["ymask"])
    assert _rejected(R.accept_dx, out[0], d["dy"], d["ymask"], d["x"], d["gamma"], case.br)
    assert _rejected(R.accept_dparams, out[2], out[3], case.br)


def test_mutant_extra_bf16_rounding_before_the_residual_add(case):
    d = case.d
    y = R.twin_apply(d["x"], case.st32, d["gamma"], d["beta"], res=d["res"], relu=True, round_before_res=True)[0]
    assert _rejected(case.judge_fwd, y, *case.fwd[1:])


def test_mutant_running_variance_left_biased(case):
    d = case.d
    out = R.twin_apply(d["x"], case.st32, d["gamma"], d["beta"], res=d["res"], relu=True,
                       run_mean=d["run_mean"], run_var=d["run_var"], biased_running=True)
    assert torch.equal(out[0], case.fwd[0]) and torch.equal(out[3], case.fwd[3])
    assert _rejected(case.judge_fwd, *out)


def test_mutant_accumulate_adds_where_it_should_overwrite(case):
    d = case.d
    dx, dres, dg, db = R.twin_bwd(d["dy"], d["ymask"], d["x"], case.mean32, case.rstd32, d["gamma"],
                                  prev_dgamma=d["prev_dgamma"], prev_dbeta=d["prev_dbeta"])
    assert _rejected(case.judge_bwd, dx, dres, dg, db, prev=False)
    # and the reverse: overwriting where it should add
    assert _rejected(case.judge_bwd, *case.bwd, prev=True)


def test_nan_and_unwritten_outputs_are_rejected(case):
    y, mean, rstd, rm, rv = case.fwd
    bad = y.clone()
    bad[-1, -1] = float("nan")
    assert _rejected(case.judge_fwd, bad, mean, rstd, rm, rv)
    assert _rejected(case.judge_fwd, y, torch.full_like(mean, float("nan")), rstd, rm, rv)
