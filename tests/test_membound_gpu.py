"""The memory-bound HIP kernels (batchnorm / elementwise / pool / optim)
against the float64 oracle of membound_oracle, through the `ext` entry
points so that each kernel stands alone, plus one autograd-level case per op.

Every bound is one of the oracle's comparator forms (see its docstring);
tests/test_membound_oracle_cpu.py proves that those comparators reject the
listed wrong implementations at these very shapes.

test_softmax_xent with hard labels is what a softmax that rounds its
probabilities to bf16 fails (mutant `probs_rounded_to_bf16` in the oracle).
"""

import pytest
import torch

import membound_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.25
ACTS = ["tanh", "sigmoid", "lrelu", "relu"]
RATIOS = {}     # (op, check) -> worst error / bound seen in this run


@pytest.fixture(autouse=True)
def _stop_the_run_on_a_gpu_fault():
    """A numeric failure goes on to the next test; a faulted GPU does not."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


def ext():
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    return hip_ext()


def dev(t):
    return t.to(DEV).contiguous()


def hold(op, ratios):
    for k, v in ratios.items():
        RATIOS[(op, k)] = max(RATIOS.get((op, k), 0.0), v)
    assert O.worst(ratios) <= 1.0, f"{op}: error/bound {ratios}"


def nhwc(t):
    return dev(t.permute(0, 2, 3, 1))


def nchw(t):
    return t.permute(0, 3, 1, 2)


BN_ALL = (O.ROWLANE_SHAPES + [O.ROWLANE_CAP_BN] + O.SCALAR_SHAPES
          + [O.SCALAR_CAP])
COLSUM_ALL = (O.ROWLANE_SHAPES + [O.ROWLANE_CAP_COLSUM] + O.SCALAR_SHAPES
              + [O.SCALAR_CAP])
BIAS_ALL = O.ROWLANE_SHAPES + [O.ROWLANE_CAP_COLSUM]


# ------------------------------------------------ coverage, exact arithmetic
@pytest.mark.parametrize("m,c", COLSUM_ALL)
def test_col_sum_reads_every_row_once(m, c):
    a = O.pm1(m, c, 1)
    got = ext().col_sum(dev(a))
    assert torch.equal(got.cpu().long(), a.long().sum(0))


@pytest.mark.parametrize("act,slope", [("identity", 0.0), ("relu", 0.0),
                                       ("lrelu", 0.5)])
@pytest.mark.parametrize("m,c", BIAS_ALL)
def test_act_bwd_bias_reads_every_row_once(m, c, act, slope):
    dy, y = O.pm1(m, c, 2), O.pm1(m, c, 3)
    dx, db = ext().act_bwd_bias(dev(dy), dev(y), O.ACT_CODES[act], slope)
    ref = dy.double() * O.act_grad_from_y(y.double(), act, slope)
    assert torch.equal(dx.cpu().double(), ref)
    assert torch.equal(db.cpu().double(), ref.sum(0))   # multiples of 0.5


@pytest.mark.parametrize("m,c", BN_ALL)
def test_bn_statistics_read_every_row_once(m, c):
    """+-1 inputs: every fp32 sum is exact in any order, and a row dropped
    or read twice moves sum(x^2) by exactly 1 in every channel."""
    x, dy = O.pm1(m, c, 4), O.pm1(m, c, 5)
    rm, rv = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    one = torch.ones(c, device=DEV)
    _, mean, istd = ext().bn_fwd_train(dev(x), one, torch.zeros_like(one),
                                       rm, rv, 1.0, O.BN_EPS)
    mu, var = rm.cpu().double(), rv.cpu().double()
    assert torch.equal((mu * m).round(), x.double().sum(0))
    s2 = var * (m - 1 if m > 1 else m) + m * mu * mu
    assert torch.equal(s2.round(), torch.full((c,), float(m)).double())
    _, _, dbeta = ext().bn_bwd(dev(x), dev(dy), mean, istd, one)
    assert torch.equal(dbeta.cpu().long(), dy.long().sum(0))


# -------------------------------------------------- accuracy, random inputs
def _bn_train(inp):
    rm, rv = dev(inp["rm0"].clone()), dev(inp["rv0"].clone())
    y, mean, istd = ext().bn_fwd_train(
        dev(inp["x"]), dev(inp["gamma"]), dev(inp["beta"]), rm, rv,
        inp["mom"], inp["eps"])
    return {"y": y, "mean": mean, "istd": istd, "rm": rm, "rv": rv}


@pytest.mark.parametrize("m,c", BN_ALL)
def test_bn_train_forward_backward(m, c):
    inp = O.bn_inputs(m, c, 100 + m)
    out = _bn_train(inp)
    hold("bn_fwd_train", O.bn_fwd_check(inp, out))
    # backward from the kernel's own statistics
    inp["mean"], inp["istd"] = out["mean"].cpu(), out["istd"].cpu()
    dx, dgamma, dbeta = ext().bn_bwd(dev(inp["x"]), dev(inp["dy"]),
                                     out["mean"], out["istd"],
                                     dev(inp["gamma"]))
    hold("bn_bwd", O.bn_bwd_check(
        inp, {"dx": dx, "dgamma": dgamma, "dbeta": dbeta}))


@pytest.mark.parametrize("want_bias", [True, False])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("m,c", O.ROWLANE_SHAPES + [O.ROWLANE_CAP_BN])
def test_bn_bwd_act(m, c, act, want_bias):
    inp = O.bn_bwd_inputs(m, c, 400 + m, act, SLOPE)
    dx, dgamma, dbeta, db = ext().bn_bwd_act(
        dev(inp["x"]), dev(inp["dy"]), dev(inp["mean"]), dev(inp["istd"]),
        dev(inp["gamma"]), O.ACT_CODES[act], SLOPE, want_bias)
    assert db.numel() == (c if want_bias else 0)
    hold("bn_bwd_act", O.bn_bwd_check(
        inp, {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "db": db},
        act=act, slope=SLOPE, want_bias=want_bias))


@pytest.mark.parametrize("m,c", O.ROWLANE_SHAPES + O.SCALAR_SHAPES)
def test_bn_eval(m, c):
    inp = O.bn_eval_inputs(m, c, 200 + m)
    y = ext().bn_fwd_eval(dev(inp["x"]), dev(inp["gamma"]),
                          dev(inp["beta"]), dev(inp["rm0"]),
                          dev(inp["rv0"]), inp["eps"])
    hold("bn_fwd_eval", O.bn_eval_check(inp, {"y": y}))


def test_batch_norm_4d_noncontiguous_autograd():
    from gan_deeplearning4j_amd.ops import gpu_ops

    n, c, h, w = 3, 24, 5, 7
    inp = O.bn_inputs(n * h * w, c, 77)
    x = dev(inp["x"]).view(n, h, w, c).permute(0, 3, 1, 2)
    # NCHW values in W-major storage: neither contiguous nor channels-last
    x = x.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    assert not x.is_contiguous() and x.shape == (n, c, h, w)
    gamma = dev(inp["gamma"]).requires_grad_(True)
    beta = dev(inp["beta"]).requires_grad_(True)
    rm, rv = dev(inp["rm0"].clone()), dev(inp["rv0"].clone())
    y = gpu_ops.batch_norm(x, gamma, beta, rm, rv, True, inp["mom"],
                           inp["eps"])
    dy4 = dev(inp["dy"]).view(n, h, w, c).permute(0, 3, 1, 2)
    y.backward(dy4)
    # the statistics the op used: the same deterministic kernels, directly
    ref = _bn_train(inp)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c)
    hold("gpu_ops.batch_norm", O.bn_fwd_check(
        inp, {"y": flat(y.detach()), "mean": ref["mean"],
              "istd": ref["istd"], "rm": rm, "rv": rv}))
    inp["mean"], inp["istd"] = ref["mean"].cpu(), ref["istd"].cpu()
    hold("gpu_ops.batch_norm", O.bn_bwd_check(
        inp, {"dx": flat(x.grad), "dgamma": gamma.grad,
              "dbeta": beta.grad}))


@pytest.mark.parametrize("m,c", COLSUM_ALL)
def test_col_sum_accuracy(m, c):
    inp = O.colsum_inputs(m, c, 500 + m)
    hold("col_sum", O.colsum_check(inp, {"sum": ext().col_sum(dev(inp["a"]))}))


@pytest.mark.parametrize("act", ["identity"] + ACTS)
@pytest.mark.parametrize("m,c", BIAS_ALL)
def test_act_bwd_bias_accuracy(m, c, act):
    inp = O.colsum_inputs(m, c, 600 + m)
    dx, db = ext().act_bwd_bias(dev(inp["a"]), dev(O._actbias_y(inp, act)),
                                O.ACT_CODES[act], SLOPE)
    hold("act_bwd_bias", O.actbias_check(inp, {"dx": dx, "db": db}, act,
                                         SLOPE))


# -------------------------------------------------------------- activations
@pytest.mark.parametrize("n", [None, 1, 7, 8, 9, 333])
@pytest.mark.parametrize("act", ACTS)
def test_activations(act, n):
    """n = None: every bf16 bit pattern but NaNs and subnormals."""
    inp = O.act_inputs(n, 800)
    code = O.ACT_CODES[act]
    y = ext().act_fwd(dev(inp["x"]), code, SLOPE)
    dx = ext().act_bwd(dev(inp["dy"]), dev(O.act_y(inp, act, SLOPE)), code,
                       SLOPE)
    hold("act_" + act, O.act_check(inp, {"y": y, "dx": dx}, act, SLOPE))


@pytest.mark.parametrize("act", ["tanh", "lrelu"])
def test_activation_autograd(act):
    from gan_deeplearning4j_amd.ops import gpu_ops

    inp = O.act_inputs(333, 801)
    x = dev(inp["x"]).requires_grad_(True)
    y = gpu_ops.activation(x, act, SLOPE)
    y.backward(dev(inp["dy"]))
    hold("gpu_ops.activation", O.act_check(
        inp, {"y": y.detach(), "dx": x.grad}, act, SLOPE,
        y_saved=y.detach()))


# ------------------------------------------------------------ pool/upsample
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("h,w", O.POOL_HW)
@pytest.mark.parametrize("k,s", O.POOL_KS)
def test_maxpool(k, s, h, w, ties):
    for c in O.POOL_C:
        for n in O.POOL_N:
            inp = O.pool_inputs(n, c, h, w, k, s, 900 + h + k + s, ties)
            y, am = ext().maxpool_fwd(nhwc(inp["x"]), n, h, w, c, k, s)
            dx = ext().maxpool_bwd(nhwc(inp["dy"]), am, n, h, w, c, k, s)
            hold("maxpool", O.pool_check(inp, {"y": nchw(y), "dx": nchw(dx)}))


@pytest.mark.parametrize("h,w", O.POOL_HW)
@pytest.mark.parametrize("scale", O.UPSAMPLE_SCALES)
def test_upsample(scale, h, w):
    for c in O.POOL_C:
        for n in O.POOL_N:
            inp = O.upsample_inputs(n, c, h, w, scale, 1000 + h)
            y = ext().upsample_fwd(nhwc(inp["x"]), n, h, w, c, scale)
            dx = ext().upsample_bwd(nhwc(inp["dy"]), n, h, w, c, scale)
            hold("upsample", O.upsample_check(
                inp, {"y": nchw(y), "dx": nchw(dx)}))


def test_pool_and_upsample_autograd():
    from gan_deeplearning4j_amd.ops import gpu_ops

    inp = O.pool_inputs(3, 8, 7, 10, 3, 2, 950, True)
    x = dev(inp["x"]).requires_grad_(True)
    y = gpu_ops.max_pool2d(x, 3, 2)
    y.backward(dev(inp["dy"]))
    hold("gpu_ops.max_pool2d", O.pool_check(
        inp, {"y": y.detach(), "dx": x.grad}))
    inp = O.upsample_inputs(3, 8, 7, 10, 3, 951)
    x = dev(inp["x"]).requires_grad_(True)
    y = gpu_ops.upsample_nearest2d(x, 3)
    y.backward(dev(inp["dy"]))
    hold("gpu_ops.upsample_nearest2d", O.upsample_check(
        inp, {"y": y.detach(), "dx": x.grad}))


# ------------------------------------------------------------------- losses
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("n", O.BCE_N)
def test_bce(n, soft):
    inp = O.bce_inputs(n, 1100 + n % 97, soft)
    x, y = dev(inp["x"]), dev(inp["y"])
    s = ext().bce_fwd(x, y)
    dx = ext().bce_bwd(x, y, 1.0 / n)
    hold("bce", O.bce_check(inp, {"loss": s.cpu().double() / n, "dx": dx}))


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("cols", O.SOFTMAX_COLS)
@pytest.mark.parametrize("rows", O.SOFTMAX_ROWS)
def test_softmax_xent(rows, cols, soft):
    inp = O.softmax_inputs(rows, cols, 1200 + rows + cols, soft)
    x, y = dev(inp["x"]), dev(inp["y"])
    s, probs = ext().softmax_xent_fwd(x, y)
    dx = ext().softmax_xent_bwd(probs, y, 1.0 / rows)
    hold("softmax_xent", O.softmax_check(
        inp, {"loss": s.cpu().double() / rows, "dx": dx}))


def test_losses_autograd():
    from gan_deeplearning4j_amd.ops import gpu_ops

    inp = O.bce_inputs(200, 1150, True)
    x = dev(inp["x"]).requires_grad_(True)
    loss = gpu_ops.bce_with_logits(x, dev(inp["y"]))
    loss.backward()
    hold("gpu_ops.bce_with_logits", O.bce_check(
        inp, {"loss": loss.detach(), "dx": x.grad}))
    inp = O.softmax_inputs(131, 10, 1250, False)
    x = dev(inp["x"]).requires_grad_(True)
    loss = gpu_ops.softmax_cross_entropy(x, dev(inp["y"]))
    loss.backward()
    hold("gpu_ops.softmax_cross_entropy", O.softmax_check(
        inp, {"loss": loss.detach(), "dx": x.grad}))


# --------------------------------------------------------------- optimizers
def _opt_step(kind, inp, param_bf16, t_on_device):
    h = O.OPT_HYPER
    w = dev(inp["w"].clone())
    param = w.to(torch.bfloat16) if param_bf16 else w
    master = w if param_bf16 else None
    m, v, g = dev(inp["m"].clone()), dev(inp["v"].clone()), dev(inp["g"])
    if kind == "adam":
        t_dev = torch.full((1,), inp["t"], dtype=torch.int32, device=DEV) \
            if t_on_device else None
        ext().fused_adam(param, g, master, m, v, h["lr"], h["b1"], h["b2"],
                         h["eps"], inp["clip"], inp["l2"], inp["t"], t_dev)
    else:
        ext().fused_rmsprop(param, g, master, v, h["lr"], h["decay"],
                            h["eps"], inp["clip"], inp["l2"])
    if param_bf16:
        assert torch.equal(param, master.to(torch.bfloat16))
    return {"w": w, "m": m, "v": v}


@pytest.mark.parametrize("l2", [0.0, 0.05])
@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("param_bf16", [True, False])
@pytest.mark.parametrize("grad_bf16", [True, False])
@pytest.mark.parametrize("n", O.OPT_N)
def test_fused_adam_step(n, grad_bf16, param_bf16, clip, l2):
    for t in O.OPT_T:
        inp = O.opt_inputs(n, 1300 + n % 89, grad_bf16, clip, l2, t)
        ref = O.opt_reference(inp, "adam")
        for t_on_device in (False, True):
            out = _opt_step("adam", inp, param_bf16, t_on_device)
            hold("fused_adam" + ("/t_dev" if t_on_device else "/host_t"),
                 O.opt_check(inp, out, "adam", ref))


@pytest.mark.parametrize("l2", [0.0, 0.05])
@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("param_bf16", [True, False])
@pytest.mark.parametrize("grad_bf16", [True, False])
@pytest.mark.parametrize("n", O.OPT_N)
def test_fused_rmsprop_step(n, grad_bf16, param_bf16, clip, l2):
    inp = O.opt_inputs(n, 1300 + n % 89, grad_bf16, clip, l2)
    out = _opt_step("rmsprop", inp, param_bf16, False)
    hold("fused_rmsprop", O.opt_check(inp, out, "rmsprop"))


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_updater_20_steps_match_cpu_updater(kind):
    from gan_deeplearning4j_amd.ops.optim import ParamSlot, Updater

    g = torch.Generator().manual_seed(1400)
    w0 = torch.randn(1000, generator=g)
    grads = [O.bf(torch.randn(1000, generator=g) * 3) for _ in range(20)]
    p_cpu = torch.nn.Parameter(w0.clone())
    p_gpu = torch.nn.Parameter(w0.clone().to(DEV, torch.bfloat16))
    s_gpu = ParamSlot(p_gpu, 0.01)
    s_gpu.master = w0.clone().to(DEV)      # not the bf16-rounded weights
    ups = [Updater([ParamSlot(p_cpu, 0.01)], kind=kind, grad_clip=1.0,
                   l2=0.05),
           Updater([s_gpu], kind=kind, grad_clip=1.0, l2=0.05)]
    for gr in grads:
        p_cpu.grad, p_gpu.grad = gr.float(), gr.to(DEV)
        for u in ups:
            u.step()
    ref = p_cpu.detach().double() - w0.double()
    got = s_gpu.master.cpu().double() - w0.double()
    # accumulated update: one bf16 ulp of it plus one fp32 ulp of the weight
    hold("updater_" + kind, {"accumulated_update": O._ratio(
        got, ref, O.BF16_ULP * ref.abs() + O.ulp32(w0.double()))})
    assert torch.equal(p_gpu.detach(), s_gpu.master.to(torch.bfloat16))


# ------------------------------------------------------------------- report
def test_report_worst_error_over_bound():
    """Last in the file: prints (with -s) the worst error/bound per op."""
    ops = {}
    for (op, chk), v in RATIOS.items():
        ops.setdefault(op, {})[chk] = v
    for op in sorted(ops):
        print(f"\n{op:34s} " + "  ".join(
            f"{k}={v:.3g}" for k, v in sorted(ops[op].items())), end="")
    print()
    assert all(v <= 1.0 for v in RATIOS.values())
