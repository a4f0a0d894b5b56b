"""Oracle for the memory-bound kernel family (batchnorm / elementwise / pool /
optim .hip): float64 references, per-element comparators, fp32 emulations of
the kernels' formulas and a named list of wrong implementations (mutants).

Not collected by pytest.  tests/test_membound_oracle_cpu.py proves on the CPU
that every comparator accepts the fp32 emulation and rejects every mutant;
tests/test_membound_gpu.py holds the HIP kernels to the same comparators.

Comparator policy
-----------------
Every comparison is per element or per channel, never normalised by a
tensor-wide maximum.  A check returns the worst ``error / bound`` ratio; it
passes when that ratio is <= 1 (NaN counts as infinite).  The four forms:

* ``pointwise``  bf16 output of a pointwise fp32 formula:
  |got - ref| <= 2^-8 |ref| + floor.  2^-8 |ref| is one bf16 ulp (a half-ulp
  rounding plus the reference sitting on a rounding boundary).  ``floor`` is
  one fp32 ulp (2^-23 |L|, the upper edge of the ulp inside a binade) of the
  largest intermediate of that element's formula, expressed in output
  units.  For a formula with several addends L is the sum of the addends'
  magnitudes, which bounds every intermediate and every partial sum, and
  the operands of a centring subtraction count separately (|x| + |mean|
  for x - mean), so cancellation is in the bound.
* ``reduction``  fp32 sum: |got - ref| <= K 2^-24 sum|term_i|, K = 512.  The
  longest chain of additions a term passes through in the row-lane kernels
  is 256 row-lanes summed serially, 32 partial rows per lane of the second
  pass, 6 shuffle steps and a few rows per thread: under 300.
* ``istd``  relative error <= 0.5 dvar / (var + eps) + 2^-22 with
  dvar = K 2^-24 (E[x^2] + 2 mean^2): the kernel forms E[x^2] - mean^2, and
  2^-22 is the room for rsqrtf.
* quantities downstream of the statistics are referenced from the kernel's
  OWN returned mean / istd (and dgamma / dbeta for dx), which are checked on
  their own, so statistics error and apply error never hide in one another.

Where a comparator is wider than the bare form above, and why
-------------------------------------------------------------
These were needed for the fp32 EMULATION to pass, i.e. no fp32
implementation of the formula can meet the bare form; every listed mutant is
still rejected with them.

* Adam / RMSProp ``m`` and ``v``: 4 * 2^-24 of the SUM OF THE ADDENDS'
  magnitudes (|b1 m| + |(1 - b1) g'|, b2 v + (1 - b2) g'^2), not of the
  result: where b1 m and (1 - b1) g' cancel, no fp32 implementation has
  relative accuracy in m.
* the float64 optimizer reference rounds the clipped and decayed gradient
  g' = clamp(g) + l2 w to fp32 before m, v and the step use it.  g' is one
  fp32 register in any implementation; v squares it, which doubles that one
  rounding, and with the products and the final add that is 5 * 2^-24 worst
  case against the 4 * 2^-24 allowed.  g' itself is covered by the check on
  the update (the l2 / clip mutants die there).
* softmax loss: the term of a row counts max(|lse - max|, 1), not
  |lse - max|: log(se) turns the RELATIVE error of the fp32 sum se into an
  ABSOLUTE error of the same size, however small log(se) is.
* fused bias grad ``db`` of bn_bwd_act: K 2^-24 sum|term| PLUS the sum of the
  terms' own pointwise floors.  The summed dpre are fp32 values each known
  only to its floor; in a constant channel they are pure cancellation
  residue and sum|term| is ~0.
* ``running_var``: the allowed error carries dvar (the istd form's variance
  uncertainty) through momentum * m / (m - 1), plus 4 * 2^-24 of the two
  addends for the four roundings of (1 - mom) rv + mom var; ``running_mean``
  has the latter only, from the kernel's own mean.
* eval-mode y: the floor has an extra 2^-22 |gamma istd (x - rm)| for the
  rsqrtf that the eval kernel evaluates per element (in training that error
  is checked on istd itself).
* sigmoid forward: floor = the smallest normal fp32, because 1 + exp(-x)
  leaves the fp32 range below x = -88.7.
* relu / lrelu ``dx`` is compared by VALUE (-0 == +0): dy * 0 gives -0 for a
  negative dy, but a kernel that selects 0 instead of multiplying is right
  too.  Their forward ``y`` is compared bit for bit.

Inputs adjusted so that no mutant survives (the rule of this suite: fix the
inputs, never loosen the comparator or drop the mutant):

* softmax logits are scaled so every row's largest logit is +100, not 60:
  exp(60) = 1.1e26 does not overflow fp32, so the mutant without the max
  shift survived at 60.
* the one-step optimizer tests use eps = 1e-2 and v0 ~ 1e-4: with the
  default 1e-8 "eps inside the square root" changes the update by 1e-8
  relative and cannot be seen by any test.
* BN channel 0 has mean 0.125 / std 0.25 so that "eps omitted" and the
  biased/unbiased mix-ups show against the cancellation-aware istd bound;
  channel 1 has |mean|/std = 16; channel 2 (when C >= 3) is constant, and dy
  is constant there too, which is what makes dx sit within the floor of 0.
* the activation inputs of length >= 2 end in an exact 0, and the fused /
  bias-grad inputs carry planted zeros in a live channel, so "derivative 1
  at y == 0" shows at the tail lengths too.
* a mutant that is mathematically identical to the right answer at a shape
  (for instance 1/(m-1) or a dropped row at m = 1, an off-by-one step count
  at t = 1000 where it moves the update by 3e-4 < 2^-10) is skipped at that
  shape through its ``applies`` predicate; every mutant is live at one shape
  at least, which the CPU gate asserts.
"""

import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # fp32 unit roundoff
BF16_ULP = 2.0 ** -8        # one bf16 ulp, relative
K_RED = 512                 # reduction chain allowance (see docstring)
RSQRT_REL = 2.0 ** -22      # rsqrtf
FLT_MIN = 2.0 ** -126       # smallest normal fp32
LOSS_GRAD_FLOOR = 2.0 ** -20  # x gscale: room for __expf / __logf

ACT_CODES = {"identity": 0, "tanh": 1, "sigmoid": 2, "lrelu": 3, "relu": 4}

ROWLANE_SHAPES = [(1, 8), (7, 8), (300, 8), (513, 24), (1000, 40),
                  (257, 256), (130, 264), (65, 520)]
ROWLANE_CAP_BN = (16387, 256)       # BN launchers: grid.x capped at 1024
ROWLANE_CAP_COLSUM = (32773, 256)   # col_sum / act_bwd_bias: kPartRows
SCALAR_SHAPES = [(64, 2), (1, 3), (1029, 300)]
SCALAR_CAP = (100003, 3)


def bf(t):
    return t.to(torch.bfloat16)


def d(t):
    return t.detach().cpu().double()


def f32(v):
    """A python scalar as the kernel sees it (a float argument)."""
    return float(torch.tensor(v, dtype=torch.float32))


def ulp32(v):
    return v.abs() * 2.0 ** -23


# ------------------------------------------------------------- comparators
def _ratio(got, ref, bound):
    got, ref = d(got), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    err = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs())
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.nan_to_num(r, nan=math.inf, posinf=math.inf)
    return float(r.max())


def pointwise(got, ref, floor):
    return _ratio(got, ref, BF16_ULP * ref.abs() + floor)


def reduction(got, ref, abs_sum, k=K_RED):
    return _ratio(got, ref, k * U32 * abs_sum)


def istd_check(got, var, ex2, mean, eps):
    ref = (var + eps).rsqrt()
    dvar = K_RED * U32 * (ex2 + 2 * mean * mean)
    return _ratio(got, ref, (0.5 * dvar / (var + eps) + RSQRT_REL) * ref)


def exact(got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    return 0.0 if got.shape == ref.shape and torch.equal(got, ref) \
        else math.inf


def bits_equal(got, ref):
    """bf16 bit equality (tells -0 from +0)."""
    return exact(bf(got).contiguous().view(torch.int16),
                 bf(ref).contiguous().view(torch.int16))


# -------------------------------------------------------------- activations
def act_ref(x, act, slope):
    """act(x) in x's own precision (float64 reference / fp32 emulation)."""
    if act == "tanh":
        return torch.tanh(x)
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    if act == "lrelu":
        return torch.where(x > 0, x, slope * x)
    if act == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x


def act_grad_from_y(y, act, slope):
    one = torch.ones_like(y)
    if act == "tanh":
        return 1.0 - y * y
    if act == "sigmoid":
        return y * (1.0 - y)
    if act == "lrelu":
        return torch.where(y > 0, one, slope * one)
    if act == "relu":
        return torch.where(y > 0, one, 0 * one)
    return one


def _act_grad_lrelu_one_at_zero(y, act, slope):
    if act in ("lrelu", "relu"):
        one = torch.ones_like(y)
        return torch.where(y >= 0, one, (slope if act == "lrelu" else 0) * one)
    return act_grad_from_y(y, act, slope)


def _act_grad_from_x(y, act, slope):
    # derivative evaluated as if the saved tensor were the PRE-activation
    if act == "tanh":
        return 1.0 - torch.tanh(y) ** 2
    if act == "sigmoid":
        s = torch.sigmoid(y)
        return s * (1.0 - s)
    return act_grad_from_y(y, act, slope)


def all_bf16_patterns():
    """Every bf16 bit pattern except NaNs and subnormals (+-0, +-inf stay)."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    expo = (bits >> 7) & 0xFF
    mant = bits & 0x7F
    keep = ~((expo == 0xFF) & (mant != 0)) & ~((expo == 0) & (mant != 0))
    bits = bits[keep]
    bits = torch.where(bits >= 1 << 15, bits - (1 << 16), bits)
    return bits.to(torch.int16).view(torch.bfloat16)


def act_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    if n is None:
        x = all_bf16_patterns()
    else:
        x = bf(torch.randn(n, generator=g) * 3)
        if n >= 2:
            x[-1] = 0.0     # an exact zero, in the tail kernel for odd n
    dy = bf(torch.randn(x.numel(), generator=g))
    return {"x": x, "dy": dy}


def act_y(inp, act, slope):
    """The bf16 activation output act_bwd is fed with (a true output)."""
    return bf(act_ref(d(inp["x"]), act, slope))


def act_emulate(inp, act, slope, grad=act_grad_from_y):
    x = inp["x"].float()
    y = bf(act_ref(x, act, slope))
    yb = act_y(inp, act, slope).float()
    dx = bf(inp["dy"].float() * grad(yb, act, slope))
    return {"y": y, "dx": dx}


def act_check(inp, out, act, slope, y_saved=None):
    """y_saved: the output the backward really consumed (autograd level:
    the kernel's own y); default is the correctly rounded one."""
    x, dy = d(inp["x"]), d(inp["dy"])
    yref = act_ref(x, act, slope)
    yb = d(act_y(inp, act, slope) if y_saved is None else y_saved)
    dxref = dy * act_grad_from_y(yb, act, slope)
    if act in ("relu", "lrelu"):
        # exact in fp32 for a power-of-two slope: y bit for bit; dx by
        # value, so that dy * 0 = -0 and a selected +0 both pass
        return {"y": bits_equal(out["y"], bf(yref)),
                "dx": exact(bf(out["dx"]), bf(dxref))}
    # tanh: relative accuracy only.  sigmoid: 1 + exp(-x) leaves the fp32
    # range for x < -88.7, where the true value is below the smallest normal
    # fp32 and the fast exp/rcp flush: floor = FLT_MIN.
    yfloor = torch.full_like(yref, FLT_MIN if act == "sigmoid" else 0.0)
    # dx = dy * act'(y): the intermediate "1" of 1 - y^2 / 1 - y scales to dy
    return {"y": pointwise(out["y"], yref, yfloor),
            "dx": pointwise(out["dx"], dxref, ulp32(dy))}


def _act_mut(grad):
    return lambda inp, act, slope: act_emulate(inp, act, slope, grad)


ACT_MUTANTS = {
    "lrelu_derivative_one_at_zero":
        (_act_mut(_act_grad_lrelu_one_at_zero),
         lambda act, n: act in ("lrelu", "relu") and (n is None or n >= 2)),
    "sigmoid_derivative_from_x":
        (_act_mut(_act_grad_from_x), lambda act, n: act == "sigmoid"),
}


# ---------------------------------------------------------------- batchnorm
BN_EPS = 1e-5
BN_MOM = 0.1


def bn_inputs(m, c, seed, act=None, slope=0.25):
    """Accuracy inputs.  act: make x a true activation output (fused path)."""
    g = torch.Generator().manual_seed(seed)
    mean = torch.rand(c, generator=g) * 8 - 4
    std = 0.25 + 1.75 * torch.rand(c, generator=g)
    mean[0], std[0] = 0.125, 0.25
    if c >= 2:
        mean[1], std[1] = 4.0, 0.25          # |mean| / std = 16
    x = mean + std * torch.randn(m, c, generator=g)
    const = 2 if c >= 3 else None
    if const is not None:
        x[:, const] = 1.375                   # var = 0
    if act is not None:
        x[0::5, max(c - 2, 0)] = 0.0          # exact zeros for relu / lrelu
        x = act_ref(bf(x).float(), act, slope)
    dy = torch.randn(m, c, generator=g) * 0.5
    if const is not None:
        dy[:, const] = 0.75
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[0] = -gamma[0]
    if c >= 3:
        gamma[c - 1] = 0.0
    return {
        "x": bf(x), "dy": bf(dy), "gamma": gamma,
        "beta": torch.randn(c, generator=g),
        "rm0": torch.randn(c, generator=g) * 0.5,
        "rv0": 0.5 + torch.rand(c, generator=g),
        "mom": BN_MOM, "eps": BN_EPS, "const": const,
    }


def pm1(m, c, seed):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randint(0, 2, (m, c), generator=g) * 2.0 - 1.0)


def bn_stats_emulate(x, eps, drop_last=False, dup_first=False,
                     unbiased_norm=False, no_eps=False):
    xf = x.float()
    m = xf.shape[0]
    if drop_last:
        xs = xf[:-1]
    elif dup_first:
        xs = torch.cat([xf, xf[:1]])
    else:
        xs = xf
    mu = xs.sum(0) / m
    var = ((xs * xs).sum(0) / m - mu * mu).clamp_min(0)
    v = var * m / (m - 1) if unbiased_norm and m > 1 else var
    istd = torch.rsqrt(v + (0.0 if no_eps else eps))
    return mu, var, istd


def bn_fwd_emulate(inp, biased_running=False, swap_momentum=False,
                   perm=None, **kw):
    x = inp["x"] if perm is None else inp["x"][:, perm]
    m = x.shape[0]
    mom, eps = f32(inp["mom"]), f32(inp["eps"])
    mu, var, istd = bn_stats_emulate(x, eps, **kw)
    unb = var if (biased_running or m == 1) else var * m / (m - 1)
    a, b = (mom, 1 - mom) if swap_momentum else (1 - mom, mom)
    y = bf(inp["gamma"] * ((x.float() - mu) * istd) + inp["beta"])
    return {"y": y, "mean": mu, "istd": istd,
            "rm": a * inp["rm0"] + b * mu, "rv": a * inp["rv0"] + b * unb}


def bn_fwd_check(inp, out):
    x = d(inp["x"])
    m = x.shape[0]
    mom, eps = f32(inp["mom"]), f32(inp["eps"])
    gamma, beta = d(inp["gamma"]), d(inp["beta"])
    mean = x.mean(0)
    ex2 = (x * x).mean(0)
    var = ((x - mean) ** 2).mean(0)
    unb = var * m / (m - 1) if m > 1 else var
    dvar = K_RED * U32 * (ex2 + 2 * mean * mean)
    mu_k, is_k = d(out["mean"]), d(out["istd"])
    r = {}
    r["mean"] = reduction(out["mean"], mean, x.abs().mean(0))
    r["istd"] = istd_check(out["istd"], var, ex2, mean, eps)
    # running buffers: a two-term fp32 formula, four roundings
    t0, t1 = (1 - mom) * d(inp["rm0"]), mom * mu_k
    r["running_mean"] = _ratio(out["rm"], t0 + t1,
                               4 * U32 * (t0.abs() + t1.abs()))
    t0, t1 = (1 - mom) * d(inp["rv0"]), mom * unb
    # dvar carried through mom * m / (m - 1) (that factor is at most 2),
    # plus the four roundings of the two-term formula
    r["running_var"] = _ratio(
        out["rv"], t0 + t1,
        mom * (unb / var.clamp_min(1e-300)).clamp_max(2) * dvar
        + 4 * U32 * (t0.abs() + t1.abs()))
    gi = gamma * is_k
    yref = gi * (x - mu_k) + beta
    big = (gi * x).abs() + (gi * mu_k).abs() + beta.abs()
    r["y"] = pointwise(out["y"], yref, ulp32(big))
    return r


def _group_swap_perm(c):
    p = torch.arange(c)
    if c >= 16:
        p[0:8], p[8:16] = torch.arange(8, 16), torch.arange(0, 8)
    else:
        p[0], p[1] = 1, 0
    return p


BN_FWD_MUTANTS = {
    "y_unbiased_variance":
        (lambda i: bn_fwd_emulate(i, unbiased_norm=True), lambda m, c: m > 1),
    "eps_omitted":
        (lambda i: bn_fwd_emulate(i, no_eps=True), lambda m, c: True),
    "running_var_biased":
        (lambda i: bn_fwd_emulate(i, biased_running=True),
         lambda m, c: m > 1),
    "momentum_wrong_operand":
        (lambda i: bn_fwd_emulate(i, swap_momentum=True), lambda m, c: True),
    "stats_missing_last_row":
        (lambda i: bn_fwd_emulate(i, drop_last=True), lambda m, c: m > 1),
    "stats_row0_twice":
        (lambda i: bn_fwd_emulate(i, dup_first=True), lambda m, c: True),
    "channel_groups_swapped":
        (lambda i: bn_fwd_emulate(i, perm=_group_swap_perm(i["x"].shape[1])),
         lambda m, c: c >= 2),
}


def bn_eval_emulate(inp, no_eps=False):
    eps = 0.0 if no_eps else f32(inp["eps"])
    istd = torch.rsqrt(inp["rv0"] + eps)
    return {"y": bf(inp["gamma"] * ((inp["x"].float() - inp["rm0"]) * istd)
                    + inp["beta"])}


def bn_eval_inputs(m, c, seed):
    inp = bn_inputs(m, c, seed)
    inp["rv0"][c - 1] = 0.0
    if c >= 3:                # keep a live gamma on the zero-variance entry
        inp["gamma"][c - 1] = 1.25
    return inp


def bn_eval_check(inp, out):
    x, eps = d(inp["x"]), f32(inp["eps"])
    gi = d(inp["gamma"]) * (d(inp["rv0"]) + eps).rsqrt()
    rm, beta = d(inp["rm0"]), d(inp["beta"])
    t = gi * (x - rm)
    big = (gi * x).abs() + (gi * rm).abs() + beta.abs()
    return {"y": pointwise(out["y"], t + beta,
                           ulp32(big) + RSQRT_REL * t.abs())}


BN_EVAL_MUTANTS = {
    "eps_omitted": (lambda i: bn_eval_emulate(i, no_eps=True),
                    lambda m, c: True),
}


def bn_bwd_inputs(m, c, seed, act=None, slope=0.25):
    """bn_inputs plus the fp32 (mean, istd) a forward pass would have saved."""
    inp = bn_inputs(m, c, seed, act, slope)
    mu, _, istd = bn_stats_emulate(inp["x"], f32(inp["eps"]))
    inp["mean"], inp["istd"] = mu, istd
    return inp


def bn_bwd_emulate(inp, act=None, slope=0.25, want_bias=True,
                   no_dbeta=False, no_dgamma=False, m_minus_1=False,
                   grad=act_grad_from_y, bias_drop_last=False):
    x, g = inp["x"].float(), inp["dy"].float()
    m = x.shape[0]
    mu, istd, gamma = inp["mean"], inp["istd"], inp["gamma"]
    xh = (x - mu) * istd
    dg, db = (g * xh).sum(0), g.sum(0)
    inv = torch.tensor(1.0, dtype=torch.float32) / \
        (m - 1 if m_minus_1 else m)
    t1 = 0 if no_dbeta else db * inv
    t2 = 0 if no_dgamma else xh * dg * inv
    dxf = gamma * istd * (g - t1 - t2)
    out = {"dgamma": dg, "dbeta": db}
    if act is None:
        out["dx"] = bf(dxf)
        return out
    dpre = dxf * grad(x, act, slope)
    out["dx"] = bf(dpre)
    if want_bias:
        out["db"] = (dpre[:-1] if bias_drop_last else dpre).sum(0)
    return out


def bn_bwd_check(inp, out, act=None, slope=0.25, want_bias=True):
    x, dy = d(inp["x"]), d(inp["dy"])
    m = x.shape[0]
    mu, istd, gamma = d(inp["mean"]), d(inp["istd"]), d(inp["gamma"])
    xh = (x - mu) * istd
    r = {}
    r["dgamma"] = reduction(out["dgamma"], (dy * xh).sum(0),
                            (dy * xh).abs().sum(0))
    r["dbeta"] = reduction(out["dbeta"], dy.sum(0), dy.abs().sum(0))
    # dx from the kernel's own dgamma / dbeta (each checked just above)
    dg_k, db_k = d(out["dgamma"]), d(out["dbeta"])
    gi = gamma * istd
    ref = gi * (dy - db_k / m - xh * dg_k / m)
    big = gi.abs() * (dy.abs() + (db_k / m).abs()
                      + (dg_k / m * istd).abs() * (x.abs() + mu.abs()))
    if act is not None:
        da = act_grad_from_y(x, act, slope)
        ref, big = ref * da, big * da.abs()
    r["dx"] = pointwise(out["dx"], ref, ulp32(big))
    if act is not None and want_bias:
        # the summed terms are fp32 values known only to within their own
        # pointwise floors (a constant channel sums pure residue)
        r["db"] = _ratio(out["db"], ref.sum(0),
                         K_RED * U32 * ref.abs().sum(0) + ulp32(big).sum(0))
    return r


BN_BWD_MUTANTS = {
    "dx_without_dbeta_term":
        (lambda i, **k: bn_bwd_emulate(i, no_dbeta=True, **k),
         lambda m, c, act: True),
    "dx_without_dgamma_term":
        (lambda i, **k: bn_bwd_emulate(i, no_dgamma=True, **k),
         lambda m, c, act: m > 1),
    "dx_with_one_over_m_minus_1":
        (lambda i, **k: bn_bwd_emulate(i, m_minus_1=True, **k),
         lambda m, c, act: m > 1),
    "fused_act_grad_from_preactivation":
        (lambda i, **k: bn_bwd_emulate(i, grad=_act_grad_from_x, **k),
         lambda m, c, act: act in ("tanh", "sigmoid") and m > 1),
    "fused_bias_grad_missing_last_row":
        (lambda i, **k: bn_bwd_emulate(i, bias_drop_last=True, **k),
         lambda m, c, act: act is not None and m > 1),
    "fused_lrelu_derivative_one_at_zero":
        (lambda i, **k: bn_bwd_emulate(i, grad=_act_grad_lrelu_one_at_zero,
                                       **k),
         lambda m, c, act: act in ("lrelu", "relu") and m > 1),
}


# ---------------------------------------------- col_sum / act_bwd_bias
def colsum_inputs(m, c, seed):
    g = torch.Generator().manual_seed(seed)
    a = bf(torch.randn(m, c, generator=g))
    y = bf(torch.randn(m, c, generator=g))
    y[0::4, 0] = 0.0
    return {"a": a, "y": y}


def colsum_emulate(inp, drop_last=False, dup_first=False):
    a = inp["a"].float()
    if drop_last:
        a = a[:-1]
    if dup_first:
        a = torch.cat([a, a[:1]])
    return {"sum": a.sum(0)}


def colsum_check(inp, out):
    a = d(inp["a"])
    return {"sum": reduction(out["sum"], a.sum(0), a.abs().sum(0))}


COLSUM_MUTANTS = {
    "missing_last_row": (lambda i: colsum_emulate(i, drop_last=True),
                         lambda m, c: m > 1),
    "row0_twice": (lambda i: colsum_emulate(i, dup_first=True),
                   lambda m, c: True),
}


def actbias_emulate(inp, act, slope, grad=act_grad_from_y, drop_last=False):
    dxf = inp["a"].float() * grad(_actbias_y(inp, act).float(), act, slope)
    return {"dx": bf(dxf), "db": (dxf[:-1] if drop_last else dxf).sum(0)}


def _actbias_y(inp, act):
    """A valid activation output for the saved-y operand."""
    y = inp["y"]
    if act == "tanh":
        return bf(torch.tanh(y.float()))
    if act == "sigmoid":
        return bf(torch.sigmoid(y.float()))
    if act == "relu":
        return bf(torch.relu(y.float()))
    return y


def actbias_check(inp, out, act, slope):
    dy = d(inp["a"])
    ref = dy * act_grad_from_y(d(_actbias_y(inp, act)), act, slope)
    return {"dx": pointwise(out["dx"], ref, ulp32(dy)),
            "db": reduction(out["db"], ref.sum(0), ref.abs().sum(0))}


ACTBIAS_MUTANTS = {
    "bias_grad_missing_last_row":
        (lambda i, a, s: actbias_emulate(i, a, s, drop_last=True),
         lambda m, c, act: m > 1),
    "lrelu_derivative_one_at_zero":
        (lambda i, a, s: actbias_emulate(i, a, s,
                                         grad=_act_grad_lrelu_one_at_zero),
         lambda m, c, act: act in ("lrelu", "relu")),
    "sigmoid_derivative_from_x":
        (lambda i, a, s: actbias_emulate(i, a, s, grad=_act_grad_from_x),
         lambda m, c, act: act == "sigmoid"),
}


# ------------------------------------------------------------ pool/upsample
POOL_KS = [(2, 1), (2, 2), (3, 2)]
POOL_HW = [(11, 11), (7, 10)]
POOL_C = [3, 8]
POOL_N = [1, 3]
UPSAMPLE_SCALES = [2, 3]


def pool_inputs(n, c, h, w, k, s, seed, ties):
    g = torch.Generator().manual_seed(seed)
    if ties:
        x = torch.randint(0, 3, (n, c, h, w), generator=g) * 0.5
    else:
        x = torch.randn(n, c, h, w, generator=g)
    ho, wo = (h - k) // s + 1, (w - k) // s + 1
    return {"x": bf(x), "dy": bf(torch.randn(n, c, ho, wo, generator=g)),
            "k": k, "s": s}


def pool_emulate(inp, pick="first"):
    x, dy, k, s = inp["x"].float(), inp["dy"].float(), inp["k"], inp["s"]
    n, c, h, w = x.shape
    u = F.unfold(x, k, stride=s).view(n, c, k * k, -1)
    mx = u.max(2).values
    eq = u == mx[:, :, None]
    if pick == "first":
        sel = eq & (eq.cumsum(2) == 1)
    elif pick == "last":
        sel = eq & (eq.flip(2).cumsum(2).flip(2) == 1)
    else:
        sel = eq
    gcol = sel.float() * dy.reshape(n, c, 1, -1)
    # fold only reaches the pixels the windows cover
    hc, wc = (dy.shape[2] - 1) * s + k, (dy.shape[3] - 1) * s + k
    gx = torch.zeros_like(x)
    gx[:, :, :hc, :wc] = F.fold(gcol.view(n, c * k * k, -1), (hc, wc), k,
                                stride=s)
    return {"y": bf(mx.view(dy.shape)), "dx": bf(gx)}


def pool_check(inp, out):
    x = d(inp["x"]).requires_grad_(True)
    dy, k, s = d(inp["dy"]), inp["k"], inp["s"]
    y = F.max_pool2d(x, k, s)
    (gx,) = torch.autograd.grad(y, x, dy, retain_graph=True)
    (gabs,) = torch.autograd.grad(y, x, dy.abs())
    # up to k*k addends: floor is one ulp of the largest partial sum
    return {"y": exact(bf(out["y"]), bf(y.detach())),
            "dx": pointwise(out["dx"], gx, ulp32(gabs))}


POOL_MUTANTS = {
    "ties_to_last_maximum": (lambda i: pool_emulate(i, "last"),
                             lambda ties: ties),
    "gradient_to_every_tied_maximum": (lambda i: pool_emulate(i, "all"),
                                       lambda ties: ties),
}


def upsample_inputs(n, c, h, w, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": bf(torch.randn(n, c, h, w, generator=g)),
            "dy": bf(torch.randn(n, c, h * scale, w * scale, generator=g)),
            "scale": scale}


def upsample_emulate(inp, average=False):
    x, dy, sc = inp["x"], inp["dy"].float(), inp["scale"]
    n, c, h, w = x.shape
    y = x.repeat_interleave(sc, 2).repeat_interleave(sc, 3)
    blk = dy.view(n, c, h, sc, w, sc)
    return {"y": y, "dx": bf(blk.mean((3, 5)) if average
                             else blk.sum((3, 5)))}


def upsample_check(inp, out):
    x, dy, sc = inp["x"], d(inp["dy"]), inp["scale"]
    n, c, h, w = x.shape
    y = F.interpolate(x.float(), scale_factor=sc, mode="nearest")
    blk = dy.view(n, c, h, sc, w, sc)
    return {"y": exact(bf(out["y"]), bf(y)),
            "dx": pointwise(out["dx"], blk.sum((3, 5)),
                            ulp32(blk.abs().sum((3, 5))))}


UPSAMPLE_MUTANTS = {
    "backward_averages": (lambda i: upsample_emulate(i, average=True),
                          lambda: True),
}


# ------------------------------------------------------------------- losses
BCE_N = [1, 200, 1024 * 256 + 3]      # the last one passes the grid cap
SOFTMAX_ROWS = [1, 5, 131]
SOFTMAX_COLS = [1, 10, 64, 65, 130, 1000]
BCE_SPAN = 90.0
SOFTMAX_SPAN = 100.0                  # see the module docstring


def bce_inputs(n, seed, soft):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 2 - 1) * BCE_SPAN
    x[0] = -BCE_SPAN if n == 1 else BCE_SPAN
    if n > 1:
        x[1] = -BCE_SPAN
    y = (torch.rand(n, generator=g) > 0.5).float()
    if soft:                              # smoothed and noisy, in [0, 1]
        y = (0.1 + 0.8 * y + 0.1 * torch.randn(n, generator=g)).clamp(0, 1)
    return {"x": bf(x), "y": bf(y), "soft": soft}


def bce_emulate(inp, summed=False, threshold=False):
    x, y = inp["x"].float(), inp["y"].float()
    if threshold:
        y = (y > 0.5).float()
    n = x.numel()
    loss = (x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum()
    gs = torch.tensor(1.0 if summed else 1.0 / n, dtype=torch.float32)
    sg = 1.0 / (1.0 + torch.exp(-x))
    return {"loss": loss if summed else loss / n, "dx": bf((sg - y) * gs)}


def bce_check(inp, out):
    x, y = d(inp["x"]), d(inp["y"])
    n = x.numel()
    t0, t1, t2 = x.clamp_min(0), x * y, torch.log1p(torch.exp(-x.abs()))
    gs = f32(1.0 / n)
    return {
        "loss": reduction(out["loss"].reshape(()), (t0 - t1 + t2).sum() / n,
                          (t0.abs() + t1.abs() + t2).sum() / n),
        "dx": pointwise(out["dx"], (torch.sigmoid(x) - y) * gs,
                        torch.full_like(x, LOSS_GRAD_FLOOR * gs)),
    }


BCE_MUTANTS = {
    "summed_instead_of_averaged": (lambda i: bce_emulate(i, summed=True),
                                   lambda n, soft: n > 1),
    "soft_labels_thresholded": (lambda i: bce_emulate(i, threshold=True),
                                lambda n, soft: soft),
}


def softmax_inputs(rows, cols, seed, soft):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    # every row's extreme logit is +SPAN
    idx = x.abs().argmax(1, keepdim=True)
    x = x * torch.sign(x.gather(1, idx)) / x.abs().gather(1, idx) \
        * SOFTMAX_SPAN
    if soft:
        y = torch.rand(rows, cols, generator=g)
        y = y / y.sum(1, keepdim=True)
    else:
        cls = torch.randint(0, cols, (rows,), generator=g)
        cls[0::2] = idx[0::2, 0]          # target = the dominant class
        y = F.one_hot(cls, cols).float()
    return {"x": bf(x), "y": bf(y), "soft": soft}


def softmax_emulate(inp, no_shift=False, threshold=False, bf16_probs=False):
    x, y = inp["x"].float(), inp["y"].float()
    if threshold:
        y = (y > 0.5).float()
    rows = x.shape[0]
    mx = torch.zeros(rows, 1) if no_shift else x.max(1, keepdim=True).values
    xs = x - mx
    lsm = torch.log(torch.exp(xs).sum(1, keepdim=True))
    p = torch.exp(xs - lsm)
    if bf16_probs:
        p = bf(p).float()
    gs = torch.tensor(1.0 / rows, dtype=torch.float32)
    return {"loss": (y * (lsm - xs)).sum() / rows, "dx": bf((p - y) * gs)}


def softmax_check(inp, out):
    x, y = d(inp["x"]), d(inp["y"])
    rows = x.shape[0]
    xs = x - x.max(1, keepdim=True).values
    lsm = torch.logsumexp(xs, 1, keepdim=True)
    gs = f32(1.0 / rows)
    # terms y*(lsm - xs): lsm = log(se) carries the RELATIVE error of se as
    # an ABSOLUTE error, so it counts as max(|lsm|, 1)
    terms = y * (lsm.abs().clamp_min(1.0) + xs.abs())
    return {
        "loss": reduction(out["loss"].reshape(()),
                          (y * (lsm - xs)).sum() / rows, terms.sum() / rows),
        "dx": pointwise(out["dx"], (torch.exp(xs - lsm) - y) * gs,
                        torch.full_like(x, LOSS_GRAD_FLOOR * gs)),
    }


SOFTMAX_MUTANTS = {
    "soft_labels_thresholded": (lambda i: softmax_emulate(i, threshold=True),
                                lambda rows, cols, soft: soft and cols > 1),
    "no_max_shift": (lambda i: softmax_emulate(i, no_shift=True),
                     lambda rows, cols, soft: True),
    # what the kernels did before this suite: probabilities stored as bf16
    # and subtracted from the target afterwards
    "probs_rounded_to_bf16": (lambda i: softmax_emulate(i, bf16_probs=True),
                              lambda rows, cols, soft: not soft
                              and cols > 1 and rows >= 5),
}


# --------------------------------------------------------------- optimizers
OPT_N = [1, 255, 1000, 2048 * 256 + 5]
OPT_T = [1, 2, 10, 1000]
OPT_HYPER = {"lr": 0.01, "b1": 0.5, "b2": 0.999, "decay": 0.95,
             "eps": 1e-2}             # eps: see the module docstring


def opt_inputs(n, seed, grad_bf16, clip, l2, t=1):
    g = torch.Generator().manual_seed(seed)
    grad = torch.randn(n, generator=g) * 3
    grad[0] = 2.5                      # the clip bites at n = 1 too
    inp = {"w": torch.randn(n, generator=g) + 0.5,
           "m": torch.randn(n, generator=g) * 0.1,
           "v": 1e-4 * (0.5 + torch.rand(n, generator=g)),
           "g": bf(grad) if grad_bf16 else grad,
           "clip": clip, "l2": l2, "t": t}
    inp["w"][0] = 1.5
    return inp


def _fma(a, b, c, T):
    """a * b + c rounded once to T, as the compiler's contraction does."""
    return (a.double() * b.double() + c.double()).to(T)


def _opt_core(inp, kind, T, sc, mutant=None):
    """One step; T: tensor dtype, sc: scalar conversion."""
    h = {k: sc(v) for k, v in OPT_HYPER.items()}
    w, g = inp["w"].to(T), inp["g"].to(T)
    clip, l2, t = sc(inp["clip"]), sc(inp["l2"]), inp["t"]
    one = torch.ones((), dtype=T)
    if mutant == "noop":
        return {"w": inp["w"].clone(), "m": inp["m"].clone(),
                "v": inp["v"].clone()}
    if mutant == "l2_before_clip":
        g = _fma(l2 * one, w, g, T)
    if clip > 0 and mutant != "clip_ignored":
        g = g.clamp(-clip, clip)
    if mutant not in ("l2_ignored", "l2_before_clip"):
        g = _fma(l2 * one, w, g, T)
    # the clipped, decayed gradient is ONE fp32 value that m, v and the step
    # all consume; the float64 reference starts from that value, so the
    # 4 * 2^-24 on m and v is not spent on g' * g' doubling its rounding
    g = g.float().to(T)
    if kind == "adam":
        b1, b2 = one * h["b1"], one * h["b2"]
        m = _fma(b1, inp["m"].to(T), (1 - b1) * g, T)
        v = _fma(b2, inp["v"].to(T), (1 - b2) * g * g, T)
        tt = t + {"bc_t_minus_1": -1, "bc_t_plus_1": 1}.get(mutant, 0)
        bc1, bc2 = 1 - b1 ** tt, 1 - b2 ** tt
        if mutant == "eps_inside_sqrt":
            den = (v / bc2 + h["eps"]).sqrt()
        else:
            den = (v / bc2).sqrt() + h["eps"]
        return {"w": w - h["lr"] * (m / bc1) / den, "m": m, "v": v}
    dc = one * h["decay"]
    a, b = (1 - dc, dc) if mutant == "decay_swapped" else (dc, 1 - dc)
    v = _fma(a, inp["v"].to(T), b * g * g, T)
    vh = v / (1 - dc ** t) if mutant == "adam_bias_correction" else v
    return {"w": w - h["lr"] * g / (vh.sqrt() + h["eps"]), "m": None, "v": v}


def opt_emulate(inp, kind, mutant=None):
    o = _opt_core(inp, kind, torch.float32, f32, mutant)
    return {k: (None if v is None else v.float()) for k, v in o.items()}


def opt_reference(inp, kind):
    return _opt_core(inp, kind, torch.float64, f32)


def opt_check(inp, out, kind, ref=None):
    """ref: opt_reference(inp, kind), to share it between several outputs."""
    if ref is None:
        ref = opt_reference(inp, kind)
    h = {k: f32(v) for k, v in OPT_HYPER.items()}
    w0, g = d(inp["w"]), d(inp["g"])
    clip, l2 = f32(inp["clip"]), f32(inp["l2"])
    gc = g.clamp(-clip, clip) if clip > 0 else g
    gp_abs = gc.abs() + (l2 * w0).abs()
    r = {}
    # m, v: 4 * 2^-24 relative to the addends (see the module docstring)
    if kind == "adam":
        r["m"] = _ratio(out["m"], ref["m"], 4 * U32 * (
            (h["b1"] * d(inp["m"])).abs() + (1 - h["b1"]) * gp_abs))
        a, b = h["b2"], 1 - h["b2"]
    else:
        a, b = h["decay"], 1 - h["decay"]
    r["v"] = _ratio(out["v"], ref["v"],
                    4 * U32 * (a * d(inp["v"]) + b * gp_abs * gp_abs))
    # the UPDATE, never the weight: 2^-10 of the step (a bf16 half-ulp of
    # it cannot bias training) plus one fp32 ulp of the weight it lands on
    dw_ref = ref["w"] - w0
    r["update"] = _ratio(d(out["w"]) - w0, dw_ref,
                         2.0 ** -10 * dw_ref.abs() + ulp32(w0))
    return r


def _opt_mut(name):
    return lambda inp, kind: opt_emulate(inp, kind, name)


OPT_MUTANTS = {
    "noop": (_opt_mut("noop"), lambda kind, clip, l2, t: True),
    "clip_ignored": (_opt_mut("clip_ignored"),
                     lambda kind, clip, l2, t: clip > 0),
    "l2_ignored": (_opt_mut("l2_ignored"), lambda kind, clip, l2, t: l2 > 0),
    "l2_before_clip": (_opt_mut("l2_before_clip"),
                       lambda kind, clip, l2, t: l2 > 0 and clip > 0),
    "bc_t_minus_1": (_opt_mut("bc_t_minus_1"),
                     lambda kind, clip, l2, t: kind == "adam" and t <= 10),
    "bc_t_plus_1": (_opt_mut("bc_t_plus_1"),
                    lambda kind, clip, l2, t: kind == "adam" and t <= 10),
    "eps_inside_sqrt": (_opt_mut("eps_inside_sqrt"),
                        lambda kind, clip, l2, t: kind == "adam"),
    "decay_swapped": (_opt_mut("decay_swapped"),
                      lambda kind, clip, l2, t: kind == "rmsprop"),
    "adam_bias_correction": (_opt_mut("adam_bias_correction"),
                             lambda kind, clip, l2, t: kind == "rmsprop"),
}

ALL_MUTANT_TABLES = {
    "act": ACT_MUTANTS, "bn_fwd": BN_FWD_MUTANTS, "bn_eval": BN_EVAL_MUTANTS,
    "bn_bwd": BN_BWD_MUTANTS, "col_sum": COLSUM_MUTANTS,
    "act_bwd_bias": ACTBIAS_MUTANTS, "pool": POOL_MUTANTS,
    "upsample": UPSAMPLE_MUTANTS, "bce": BCE_MUTANTS,
    "softmax": SOFTMAX_MUTANTS, "optim": OPT_MUTANTS,
}
MUTANT_COUNT = 38


def worst(ratios):
    return max(ratios.values()) if ratios else 0.0
