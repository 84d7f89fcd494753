"""fp64 BatchNorm references, inputs whose channels can be told apart, and elementwise /
per-channel acceptance functions.  Plain module: runs on any torch device, needs no GPU.

The references are written from the BatchNorm definition (not from bn.hip):

    sum_c = S x,  sumsq_c = S x^2,  mean = sum / M,  var = max(sumsq / M - mean^2, 0)
    y     = act((x - mean) * rstd * gamma + beta [+ res]),   rstd = 1 / sqrt(var + eps)
    running <- (1 - 0.1) * running + 0.1 * (mean | var * M / (M - 1))
    dz = dy * [y > 0],  dbeta = S dz,  dgamma = S dz * xhat,  dres = dz
    dx = gamma * rstd * (dz - dbeta / M - xhat * dgamma / M)

Every stage is judged on its own inputs: the forward apply is given statistics that are fp64 sums
rounded to fp32 (or fp32 partial rows) and the reference starts from those fp32 values; the backward
is given mean / rstd rounded to fp32 and the reference uses the rounded values.

Acceptance is per element and per channel: no element or channel is exempt and no norm is taken
over a tensor.  With P(e) = 2**e, u = P(-24), amp_c = (q_c / M + eps) / (var_c + eps) (the
cancellation factor of E[x^2] - mean^2) and A = |gamma| (|xhat| + |mean| rstd) + |beta| + |res|:

    sum, sumsq, dbeta, dgamma   |err| <= P(-14) * S|terms|        (fp32 chains of <= 1024 additions)
    save_mean                   |err| <= P(-22) |mean| + e_mean
    save_rstd                   rel   <= P(-20) amp + e_rstd
    y    |err| <= P(-8) |y64| + P(-18) A + (P(-20) amp + e_rstd) |gamma xhat| + |gamma| rstd e_mean
    dx   |err| <= P(-8) |dx64| + |ka| (P(-18) (|dz| + |kb| + |xhat kc|)
                  + tol (S|dz| + |xhat| S|dz xhat|) / M + P(-22) (|x| + |mean|) rstd |kc|)
    dres bit-exact (it is dy or +0)

P(-8) is the bf16 half-ulp: one extra intermediate bf16 rounding breaks it.

Terms that are not in the table the bounds came from, each derived from an operation the table
does not model (none is fitted to a kernel's output):

* e_mean, e_rstd — statistics given as G > 1 partial rows are first summed in fp32.  Any order of
  G - 1 additions errs by at most (G - 1) u S_g|row_g|, so with eS = (G - 1) u S_g|sum_g| and
  eQ = (G - 1) u S_g sumsq_g:  e_mean = eS / M and, to first order in d var / (var + eps),
  e_rstd = (eQ / M + 2 |mean| eS / M) / (var + eps)  (the factor 1 instead of 1/2 covers the
  second order).  Both are zero for final sums and for one row.
* accumulate — `grad += sum` rounds once more: u |prev + sum| is added to the dbeta / dgamma bound.
* running statistics — the mean / var bounds pushed through the update, plus its own fp32
  roundings (var * M, / (M - 1), two products, one addition: at most 5 u of the larger operand,
  taken as P(-21) (|0.9 old| + |0.1 new|)).  The reference uses the fp32 values of 0.1 and
  1 - 0.1, as the kernels receive them.
"""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = float(torch.tensor(1e-5, dtype=F32))          # the fp32 value the kernels are handed
MOM = float(torch.tensor(0.1, dtype=F32))
ONE_MINUS_MOM = float(torch.tensor(1.0, dtype=F32) - torch.tensor(0.1, dtype=F32))
SLAB = 32768                                        # rows of fp64 work per step
CONST_CH, ZERO_GAMMA_CH = 3, 6                      # x == 3.0 / gamma == 0 (neither is a negative-gamma channel)
U = 2.0 ** -24


def P(e):
    return 2.0 ** e


def sum_tol(M, long_shape=False):
    """Relative fp32 summation bound: chains of at most 1024 additions; the long pipelined shapes
    (long_shape) get min(P(-14) * ceil(M / 4096), P(-10))."""
    if not long_shape:
        return P(-14)
    return min(P(-14) * math.ceil(M / 4096), P(-10))


# ------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------

def make_inputs(M, C, seed=0, device="cpu"):
    """Seeded inputs with distinguishable channels: per-channel mean over [-3, 3] and std over
    [0.25, 4] (shuffled independently), gamma in +-[0.5, 1.5] with every fifth channel negative and
    one exactly 0, one constant channel (x == 3.0), and for the backward a ReLU output whose sign
    pattern holds +0.0, -0.0, negatives and positives."""
    assert C >= 8
    g = torch.Generator(device=device)
    g.manual_seed(1000003 * seed + 7919 * C + M)

    def perm():
        return torch.randperm(C, generator=g, device=device)

    def randn(*s):
        return torch.randn(*s, generator=g, device=device, dtype=F32)

    mu = torch.linspace(-3, 3, C, device=device, dtype=F32)[perm()]
    sd = torch.linspace(0.25, 4, C, device=device, dtype=F32)[perm()]
    x = randn(M, C) * sd + mu
    x[:, CONST_CH] = 3.0
    gamma = torch.linspace(0.5, 1.5, C, device=device, dtype=F32)[perm()]
    gamma[::5] *= -1
    gamma[ZERO_GAMMA_CH] = 0.0
    table = torch.tensor([0.0, -0.0, -1.5, 0.75, 2.0, -0.25], device=device, dtype=F32)
    ymask = table[torch.randint(0, table.numel(), (M, C), generator=g, device=device)]
    return dict(M=M, C=C, x=x.to(BF16), gamma=gamma, beta=randn(C), res=randn(M, C).to(BF16),
                dy=randn(M, C).to(BF16), ymask=ymask.to(BF16), run_mean=randn(C) * 0.5,
                run_var=torch.rand(C, generator=g, device=device, dtype=F32) + 0.5,
                prev_dgamma=randn(C), prev_dbeta=randn(C))


def group_ids(M, G, seed, device="cpu"):
    """Row -> group for a split of M rows into G contiguous groups; groups may be empty."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed * 7907 + G)
    cuts = torch.sort(torch.randint(0, M + 1, (G - 1,), generator=g)).values.to(device)
    return torch.bucketize(torch.arange(M, device=device), cuts, right=True)


def _group_rows(terms_a, terms_b, gid, G):
    """[G][a | b] fp64 group sums rounded to fp32."""
    C = terms_a.shape[1]
    rows = torch.zeros(G, 2 * C, dtype=F64, device=terms_a.device)
    rows[:, :C].index_add_(0, gid, terms_a)
    rows[:, C:].index_add_(0, gid, terms_b)
    return rows.to(F32)


def stat_rows(x, G, seed=0):
    """Partial [sum | sumsq] rows of G row groups, for bn_apply(stats_rows=G)."""
    xd = x.to(F64)
    return _group_rows(xd, xd * xd, group_ids(x.shape[0], G, seed, x.device), G)


def bwd_rows(dy, ymask, x, mean32, rstd32, G, seed=0):
    """Partial [dbeta | dgamma] rows of G row groups, for bn_bwd(partial=(rows, G))."""
    dz = _dz(dy, ymask)
    xh = (x.to(F64) - mean32.to(F64)) * rstd32.to(F64)
    return _group_rows(dz, dz * xh, group_ids(x.shape[0], G, seed, x.device), G)


# ------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------

def col_sums(x):
    """fp64 per-channel sum, sum of squares and sum of magnitudes of a [M][C] tensor."""
    C = x.shape[1]
    s, q, a = (torch.zeros(C, dtype=F64, device=x.device) for _ in range(3))
    for r in range(0, x.shape[0], SLAB):
        xd = x[r:r + SLAB].to(F64)
        s += xd.sum(0)
        q += (xd * xd).sum(0)
        a += xd.abs().sum(0)
    return s, q, a


def stats32(x):
    """[sum | sumsq] as fp64 sums rounded to fp32: what a forward-apply test feeds."""
    s, q, _ = col_sums(x)
    return torch.cat([s, q]).to(F32)


class Chan:
    """Per-channel fp64 normalisation constants and the error terms of how they were obtained."""

    def __init__(self, mean, var, amp, e_mean, e_rstd):
        self.mean, self.var, self.amp, self.e_mean, self.e_rstd = mean, var, amp, e_mean, e_rstd
        self.rstd = (var + EPS).rsqrt()


def chan_from_stats(stats, M):
    """stats: fp32 [2C] final sums or [G][2C] partial rows, exactly as given to the kernel."""
    rows = stats.to(F64) if stats.dim() == 2 else stats.to(F64).reshape(1, -1)
    G, C = rows.shape[0], rows.shape[1] // 2
    S, Q = rows[:, :C].sum(0), rows[:, C:].sum(0)
    mean = S / M
    var = (Q / M - mean * mean).clamp_min(0)
    amp = (Q / M + EPS) / (var + EPS)
    AMP_MAX[0] = max(AMP_MAX[0], float(amp.max()))
    eS = (G - 1) * U * rows[:, :C].abs().sum(0)
    eQ = (G - 1) * U * rows[:, C:].abs().sum(0)
    return Chan(mean, var, amp, eS / M, (eQ / M + 2 * mean.abs() * eS / M) / (var + EPS))


def chan_eval(run_mean, run_var):
    z = torch.zeros_like(run_mean, dtype=F64)
    return Chan(run_mean.to(F64), run_var.to(F64), z + 1.0, z, z.clone())


def saved32(x):
    """mean / rstd of x from fp64 statistics, rounded to fp32: what a backward test feeds."""
    s, q, _ = col_sums(x)
    M = x.shape[0]
    mean = s / M
    var = (q / M - mean * mean).clamp_min(0)
    return mean.to(F32), (var + EPS).rsqrt().to(F32)


def _dz(dy, ymask):
    d = dy.to(F64)
    return d if ymask is None else torch.where(ymask.to(F64) > 0, d, torch.zeros_like(d))


class BwdRef:
    """Per-channel fp64 dbeta / dgamma and the magnitude sums their bounds scale with.  With
    partial rows (fp32 [G][2C], as given to the kernel) the sums are those of the rows."""

    def __init__(self, dy, ymask, x, mean32, rstd32, rows=None):
        C = x.shape[1]
        self.M = x.shape[0]
        self.mean, self.rstd = mean32.to(F64), rstd32.to(F64)
        if rows is not None:
            r = rows.to(F64).reshape(-1, 2 * C)
            self.dbeta, self.dgamma = r[:, :C].sum(0), r[:, C:].sum(0)
            self.abs_dz, self.abs_dzx = r[:, :C].abs().sum(0), r[:, C:].abs().sum(0)
            return
        acc = [torch.zeros(C, dtype=F64, device=x.device) for _ in range(4)]
        for r in range(0, self.M, SLAB):
            dz = _dz(dy[r:r + SLAB], None if ymask is None else ymask[r:r + SLAB])
            t = dz * (x[r:r + SLAB].to(F64) - self.mean) * self.rstd
            for a, v in zip(acc, (dz.sum(0), t.sum(0), dz.abs().sum(0), t.abs().sum(0))):
                a += v
        self.dbeta, self.dgamma, self.abs_dz, self.abs_dzx = acc


def running_ref(run_mean, run_var, ch, M):
    unb = ch.var * (M / (M - 1) if M > 1 else 1.0)
    return (ONE_MINUS_MOM * run_mean.to(F64) + MOM * ch.mean, ONE_MINUS_MOM * run_var.to(F64) + MOM * unb)


# ------------------------------------------------------------------------------------------
# acceptance
# ------------------------------------------------------------------------------------------

RATIOS = {}   # quantity -> largest error / bound seen (headroom report)
AMP_MAX = [0.0]   # largest cancellation factor amp_c any training-mode reference was built with


def _accept(name, err, bound):
    """err, bound: same-shape fp64 tensors.  Every element must satisfy err <= bound."""
    if err.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(bad, torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst if math.isfinite(worst) else 1e30)
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{name}: error / bound = {worst:.4g} at {idx} "
                             f"(err {float(err.flatten()[i]):.6g}, bound {float(bound.flatten()[i]):.6g}; "
                             f"{int((ratio > 1).sum())} of {err.numel()} out of bound)")
    return worst


def accept_colsum(name, got, ref, absref, tol=P(-14), prev=None):
    """A per-channel fp32 sum against its fp64 value: |err| <= tol * S|terms| (+ u |prev + sum| when
    the kernel added it onto prev)."""
    bound = tol * absref
    if prev is not None:
        ref = ref + prev.to(F64)
        bound = bound + U * ref.abs()
    return _accept(name, (got.to(F64) - ref).abs(), bound)


def accept_stats(got, x, tol=P(-14)):
    C = x.shape[1]
    s, q, a = col_sums(x)
    return (accept_colsum("sum", got[:C], s, a, tol), accept_colsum("sumsq", got[C:], q, q, tol))


def accept_saved(save_mean, save_rstd, ch):
    a = _accept("save_mean", (save_mean.to(F64) - ch.mean).abs(), P(-22) * ch.mean.abs() + ch.e_mean)
    b = _accept("save_rstd", (save_rstd.to(F64) / ch.rstd - 1).abs(), P(-20) * ch.amp + ch.e_rstd)
    return a, b


def accept_running(run_mean, run_var, old_mean, old_var, ch, M):
    rm, rv = running_ref(old_mean, old_var, ch, M)
    k = M / (M - 1) if M > 1 else 1.0
    d_mean = P(-22) * ch.mean.abs() + ch.e_mean
    d_var = 2 * (ch.var + EPS) * (P(-20) * ch.amp + ch.e_rstd)      # rstd = (var + eps)^-1/2
    a = _accept("run_mean", (run_mean.to(F64) - rm).abs(),
                MOM * d_mean + P(-21) * (ONE_MINUS_MOM * old_mean.to(F64).abs() + MOM * ch.mean.abs()))
    b = _accept("run_var", (run_var.to(F64) - rv).abs(),
                MOM * k * d_var + P(-21) * (ONE_MINUS_MOM * old_var.to(F64).abs() + MOM * k * ch.var))
    return a, b


def y_ref(x, ch, gamma, beta, res=None, relu=False):
    """(y64, bound) for rows x."""
    g, b = gamma.to(F64), beta.to(F64)
    xh = (x.to(F64) - ch.mean) * ch.rstd
    y = xh * g + b
    A = g.abs() * (xh.abs() + ch.mean.abs() * ch.rstd) + b.abs()
    if res is not None:
        y = y + res.to(F64)
        A = A + res.to(F64).abs()
    if relu:
        y = y.clamp_min(0)
    bound = (P(-8) * y.abs() + P(-18) * A + (P(-20) * ch.amp + ch.e_rstd) * (g * xh).abs()
             + g.abs() * ch.rstd * ch.e_mean)
    return y, bound


def accept_y(y, x, ch, gamma, beta, res=None, relu=False, name="y"):
    worst = 0.0
    for r in range(0, x.shape[0], SLAB):
        y64, bound = y_ref(x[r:r + SLAB], ch, gamma, beta, None if res is None else res[r:r + SLAB], relu)
        worst = max(worst, _accept(name, (y[r:r + SLAB].to(F64) - y64).abs(), bound))
    return worst


def accept_dparams(dgamma, dbeta, br, tol=P(-14), prev_dgamma=None, prev_dbeta=None):
    return (accept_colsum("dbeta", dbeta, br.dbeta, br.abs_dz, tol, prev_dbeta),
            accept_colsum("dgamma", dgamma, br.dgamma, br.abs_dzx, tol, prev_dgamma))


def dx_ref(dy, ymask, x, gamma, br, tol=P(-14)):
    """(dx64, bound) for rows (dy, ymask, x) of the tensor br was built from."""
    M = br.M
    dz = _dz(dy, ymask)
    xd = x.to(F64)
    xh = (xd - br.mean) * br.rstd
    ka = gamma.to(F64) * br.rstd
    kb, kc = br.dbeta / M, br.dgamma / M
    dx = ka * (dz - kb - xh * kc)
    bound = P(-8) * dx.abs() + ka.abs() * (
        P(-18) * (dz.abs() + kb.abs() + (xh * kc).abs())
        + tol * (br.abs_dz + xh.abs() * br.abs_dzx) / M
        + P(-22) * (xd.abs() + br.mean.abs()) * br.rstd * kc.abs())
    return dx, bound


def accept_dx(dx, dy, ymask, x, gamma, br, tol=P(-14), name="dx"):
    worst = 0.0
    for r in range(0, x.shape[0], SLAB):
        sl = slice(r, r + SLAB)
        d64, bound = dx_ref(dy[sl], None if ymask is None else ymask[sl], x[sl], gamma, br, tol)
        worst = max(worst, _accept(name, (dx[sl].to(F64) - d64).abs(), bound))
    return worst


def accept_dres(dres, dy, ymask):
    """dres is dy where y > 0 (both zeros are not) and +0 elsewhere, bit for bit."""
    ref = dy if ymask is None else torch.where(ymask.float() > 0, dy, torch.zeros_like(dy))
    same = dres.view(torch.int16) == ref.view(torch.int16)
    RATIOS["dres"] = max(RATIOS.get("dres", 0.0), 0.0 if bool(same.all()) else 1e30)
    assert bool(same.all()), f"dres: {int((~same).sum())} of {same.numel()} elements differ in bits"
    return 0.0


# ------------------------------------------------------------------------------------------
# fp32 twin: the same formulas in fp32 with sequential sums (shows the bounds admit a correct
# fp32 implementation; its mutants show they reject wrong ones)
# ------------------------------------------------------------------------------------------

def seq_sum32(t):
    acc = torch.zeros(t.shape[1], dtype=F32, device=t.device)
    for r in range(t.shape[0]):
        acc = acc + t[r]
    return acc


def twin_stats(x):
    xf = x.to(F32)
    return torch.cat([seq_sum32(xf), seq_sum32(xf * xf)])


def twin_apply(x, stats, gamma, beta, res=None, relu=False, run_mean=None, run_var=None, training=True,
               round_before_res=False, biased_running=False):
    """-> y (bf16), save_mean, save_rstd, new run_mean, new run_var (fp32)."""
    M, C = x.shape
    Mf = torch.tensor(float(M), dtype=F32)
    if training:
        rows = stats.reshape(-1, 2 * C)
        st = rows[0].clone()
        for i in range(1, rows.shape[0]):
            st = st + rows[i]
        mean = st[:C] / Mf
        var = (st[C:] / Mf - mean * mean).clamp_min(0)
    else:
        mean, var = run_mean, run_var
    rstd = torch.rsqrt(var + torch.tensor(EPS, dtype=F32))
    scale = gamma * rstd
    shift = beta - mean * gamma * rstd
    v = x.to(F32) * scale + shift
    if round_before_res:
        v = v.to(BF16).to(F32)
    if res is not None:
        v = v + res.to(F32)
    if relu:
        v = v.clamp_min(0)
    rm = rv = None
    if training and run_mean is not None:
        unb = var if (M == 1 or biased_running) else var * Mf / torch.tensor(float(M - 1), dtype=F32)
        mom = torch.tensor(MOM, dtype=F32)
        rm = (1 - mom) * run_mean + mom * mean
        rv = (1 - mom) * run_var + mom * unb
    return v.to(BF16), mean, rstd, rm, rv


def twin_bwd(dy, ymask, x, mean32, rstd32, gamma, prev_dgamma=None, prev_dbeta=None, ge=False):
    """-> dx (bf16), dres (bf16), dgamma, dbeta (fp32; added onto prev_* when given)."""
    M = x.shape[0]
    d = dy.to(F32)
    if ymask is not None:
        keep = ymask.to(F32) >= 0 if ge else ymask.to(F32) > 0
        d = torch.where(keep, d, torch.zeros_like(d))
    xh = (x.to(F32) - mean32) * rstd32
    sb, sg = seq_sum32(d), seq_sum32(d * xh)
    invM = torch.tensor(1.0, dtype=F32) / torch.tensor(float(M), dtype=F32)
    dx = (gamma * rstd32) * (d - sb * invM - xh * (sg * invM))
    dgamma = sg if prev_dgamma is None else prev_dgamma + sg
    dbeta = sb if prev_dbeta is None else prev_dbeta + sb
    return dx.to(BF16), d.to(BF16), dgamma, dbeta


def bf16_next(t, away_from):
    """t moved by one bf16 ulp, away from the fp64 value away_from."""
    bits = t.view(torch.int16).to(torch.int32)
    up = t.to(F64) >= away_from                      # grow the magnitude for positive values when above
    step = torch.where(up == (t.to(F64) >= 0), 1, -1)
    return (bits + step).to(torch.int16).view(BF16)
