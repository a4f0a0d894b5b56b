"""The proof that tests/test_membound_gpu.py can fail.

For every op and every shape of the GPU file that is small enough for the
CPU (only the grid-cap shapes are left out), an fp32 torch emulation of the
kernel's formula must pass the comparators of membound_oracle, and every
listed mutant must be rejected by them.  No tolerance lives here.
"""

import pytest
import torch

import membound_oracle as O

BN_SHAPES = O.ROWLANE_SHAPES + O.SCALAR_SHAPES
FUSED_ACTS = ["tanh", "sigmoid", "lrelu", "relu"]
SLOPE = 0.25

KILLED = {}     # (table, mutant) -> number of cases that rejected it


def gate(table, name, emulate, check, mutants, applies_args):
    """emulate passes; every applicable mutant is rejected."""
    r = check(emulate())
    assert O.worst(r) <= 1.0, f"emulation rejected: {r}"
    for mname, (fn, applies) in mutants.items():
        if not applies(*applies_args):
            continue
        rm = check(fn())
        assert O.worst(rm) > 1.0, f"mutant {mname} survived: {rm}"
        KILLED[(table, mname)] = KILLED.get((table, mname), 0) + 1


def bind(fn, *a, **k):
    return lambda: fn(*a, **k)


def bound_mutants(table, *a, **k):
    return {n: (bind(fn, *a, **k), ap) for n, (fn, ap) in table.items()}


# ----------------------------------------------------------------------- BN
@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_bn_fwd(m, c):
    inp = O.bn_inputs(m, c, 100 + m)
    gate("bn_fwd", (m, c), bind(O.bn_fwd_emulate, inp),
         lambda o: O.bn_fwd_check(inp, o),
         bound_mutants(O.BN_FWD_MUTANTS, inp), (m, c))


@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_bn_eval(m, c):
    inp = O.bn_eval_inputs(m, c, 200 + m)
    gate("bn_eval", (m, c), bind(O.bn_eval_emulate, inp),
         lambda o: O.bn_eval_check(inp, o),
         bound_mutants(O.BN_EVAL_MUTANTS, inp), (m, c))


@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_bn_bwd(m, c):
    inp = O.bn_bwd_inputs(m, c, 300 + m)
    gate("bn_bwd", (m, c), bind(O.bn_bwd_emulate, inp),
         lambda o: O.bn_bwd_check(inp, o),
         bound_mutants(O.BN_BWD_MUTANTS, inp), (m, c, None))


@pytest.mark.parametrize("want_bias", [True, False])
@pytest.mark.parametrize("act", FUSED_ACTS)
@pytest.mark.parametrize("m,c", O.ROWLANE_SHAPES)
def test_bn_bwd_act(m, c, act, want_bias):
    inp = O.bn_bwd_inputs(m, c, 400 + m, act, SLOPE)
    kw = dict(act=act, slope=SLOPE, want_bias=want_bias)
    muts = bound_mutants(O.BN_BWD_MUTANTS, inp, **kw)
    if not want_bias:
        muts.pop("fused_bias_grad_missing_last_row")
    gate("bn_bwd", (m, c), bind(O.bn_bwd_emulate, inp, **kw),
         lambda o: O.bn_bwd_check(inp, o, **kw), muts, (m, c, act))


# ------------------------------------------------------ col_sum / bias grad
@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_col_sum(m, c):
    inp = O.colsum_inputs(m, c, 500 + m)
    gate("col_sum", (m, c), bind(O.colsum_emulate, inp),
         lambda o: O.colsum_check(inp, o),
         bound_mutants(O.COLSUM_MUTANTS, inp), (m, c))


@pytest.mark.parametrize("act", ["identity"] + FUSED_ACTS)
@pytest.mark.parametrize("m,c", O.ROWLANE_SHAPES)
def test_act_bwd_bias(m, c, act):
    inp = O.colsum_inputs(m, c, 600 + m)
    gate("act_bwd_bias", (m, c), bind(O.actbias_emulate, inp, act, SLOPE),
         lambda o: O.actbias_check(inp, o, act, SLOPE),
         bound_mutants(O.ACTBIAS_MUTANTS, inp, act, SLOPE), (m, c, act))


@pytest.mark.parametrize("m,c", BN_SHAPES)
def test_exact_inputs_catch_a_dropped_or_doubled_row(m, c):
    """The +-1 coverage identities of the GPU file, on the emulation."""
    x = O.pm1(m, c, 700 + m)
    inp = {"x": x, "gamma": torch.ones(c), "beta": torch.zeros(c),
           "rm0": torch.zeros(c), "rv0": torch.zeros(c), "mom": 1.0,
           "eps": O.BN_EPS}
    sx = x.double().sum(0)

    def identities(out):
        mean, rv = O.d(out["rm"]), O.d(out["rv"])
        s2 = rv * (m - 1 if m > 1 else m) + m * mean * mean
        return (torch.equal((mean * m).round(), sx)
                and torch.equal(s2.round(), torch.full((c,), float(m),
                                                       dtype=torch.float64)))

    assert identities(O.bn_fwd_emulate(inp))
    assert not identities(O.bn_fwd_emulate(inp, dup_first=True))
    if m > 1:
        assert not identities(O.bn_fwd_emulate(inp, drop_last=True))


# -------------------------------------------------------------- activations
@pytest.mark.parametrize("n", [None, 1, 7, 8, 9, 333])
@pytest.mark.parametrize("act", FUSED_ACTS)
def test_activations(act, n):
    inp = O.act_inputs(n, 800)
    gate("act", n, bind(O.act_emulate, inp, act, SLOPE),
         lambda o: O.act_check(inp, o, act, SLOPE),
         bound_mutants(O.ACT_MUTANTS, inp, act, SLOPE), (act, n))


# ------------------------------------------------------------ pool/upsample
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", O.POOL_N)
@pytest.mark.parametrize("c", O.POOL_C)
@pytest.mark.parametrize("h,w", O.POOL_HW)
@pytest.mark.parametrize("k,s", O.POOL_KS)
def test_maxpool(k, s, h, w, c, n, ties):
    inp = O.pool_inputs(n, c, h, w, k, s, 900 + h + k + s, ties)
    gate("pool", None, bind(O.pool_emulate, inp),
         lambda o: O.pool_check(inp, o),
         bound_mutants(O.POOL_MUTANTS, inp), (ties,))


@pytest.mark.parametrize("n", O.POOL_N)
@pytest.mark.parametrize("c", O.POOL_C)
@pytest.mark.parametrize("h,w", O.POOL_HW)
@pytest.mark.parametrize("scale", O.UPSAMPLE_SCALES)
def test_upsample(scale, h, w, c, n):
    inp = O.upsample_inputs(n, c, h, w, scale, 1000 + h)
    gate("upsample", None, bind(O.upsample_emulate, inp),
         lambda o: O.upsample_check(inp, o),
         bound_mutants(O.UPSAMPLE_MUTANTS, inp), ())


# ------------------------------------------------------------------- losses
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("n", O.BCE_N)
def test_bce(n, soft):
    inp = O.bce_inputs(n, 1100 + n % 97, soft)
    gate("bce", n, bind(O.bce_emulate, inp), lambda o: O.bce_check(inp, o),
         bound_mutants(O.BCE_MUTANTS, inp), (n, soft))


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("cols", O.SOFTMAX_COLS)
@pytest.mark.parametrize("rows", O.SOFTMAX_ROWS)
def test_softmax_xent(rows, cols, soft):
    inp = O.softmax_inputs(rows, cols, 1200 + rows + cols, soft)
    gate("softmax", (rows, cols), bind(O.softmax_emulate, inp),
         lambda o: O.softmax_check(inp, o),
         bound_mutants(O.SOFTMAX_MUTANTS, inp), (rows, cols, soft))


# --------------------------------------------------------------- optimizers
@pytest.mark.parametrize("l2", [0.0, 0.05])
@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("grad_bf16", [True, False])
@pytest.mark.parametrize("n", O.OPT_N)
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_optimizer_step(kind, n, grad_bf16, clip, l2):
    for t in (O.OPT_T if kind == "adam" and n <= 1000 else [1]):
        inp = O.opt_inputs(n, 1300 + n % 89, grad_bf16, clip, l2, t)
        gate("optim", n, bind(O.opt_emulate, inp, kind),
             lambda o: O.opt_check(inp, o, kind),
             bound_mutants(O.OPT_MUTANTS, inp, kind), (kind, clip, l2, t))


# ------------------------------------------------------------------- census
def test_every_listed_mutant_is_rejected_somewhere():
    """A silently emptied mutant list, or a mutant whose `applies` never
    fires, fails here.  Runs one case per gate itself, so it does not
    depend on which other tests were selected."""
    listed = {(t, n) for t, tab in O.ALL_MUTANT_TABLES.items() for n in tab}
    assert len(listed) == O.MUTANT_COUNT, len(listed)
    KILLED.clear()
    test_bn_fwd(513, 24)
    test_bn_eval(513, 24)
    test_bn_bwd(513, 24)
    test_bn_bwd_act(513, 24, "tanh", True)
    test_bn_bwd_act(513, 24, "lrelu", True)
    test_col_sum(513, 24)
    for act in ("sigmoid", "lrelu"):
        test_act_bwd_bias(513, 24, act)
        test_activations(act, None)
    test_maxpool(2, 1, 7, 10, 3, 1, True)
    test_upsample(2, 7, 10, 3, 1)
    test_bce(200, True)
    test_softmax_xent(5, 10, True)
    test_softmax_xent(131, 10, False)
    test_optimizer_step("adam", 255, True, 1.0, 0.05)
    test_optimizer_step("rmsprop", 255, True, 1.0, 0.05)
    missing = sorted(listed - set(KILLED))
    print(f"\n{len(listed)} mutants, each rejected in "
          f"{min(KILLED.values())}..{max(KILLED.values())} cases")
    assert not missing, f"never exercised: {missing}"
