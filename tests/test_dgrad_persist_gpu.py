"""GPU numerics of the persistent class-fused direct dgrad / convT kernel
(conv_dgrad_direct_p in conv_dgrad_direct.hip).

Every case runs the persistent kernel (GDLJ_DGRAD_PERSIST=1, the default)
with the grid capped at 1 block (one block walks every tile), 3 blocks
(uneven split) and uncapped, and compares against the one-shot kernel
(GDLJ_DGRAD_PERSIST=0).  dx / y must be bit-identical: per output element
the accumulation sequence and the epilogue are the same; only the order
of the fp32 bias / BN partial sums differs.  Against an fp32 torch
reference the project's bounds for these paths apply.
"""

import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAPS = [1, 3, None]


def mk(shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return t.to(DEV, torch.bfloat16)


def relerr(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


def with_env(persist, cap, fn):
    """Run fn() with the two routing switches set, then restore them."""
    keys = ("GDLJ_DGRAD_PERSIST", "GDLJ_DGRAD_PERSIST_BLOCKS")
    old = {k: os.environ.get(k) for k in keys}
    os.environ["GDLJ_DGRAD_PERSIST"] = persist
    if cap is None:
        os.environ.pop("GDLJ_DGRAD_PERSIST_BLOCKS", None)
    else:
        os.environ["GDLJ_DGRAD_PERSIST_BLOCKS"] = str(cap)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def p_eligible(h, c8, ko8, r, pad):
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    return hip_ext().conv_dgrad_direct_p_eligible(h, h, c8, ko8, ko8, r, r,
                                                  2, pad)


# ------------------------------------------------------------ conv2d dgrad
DGRAD_SHAPES = [
    # batch, cin, h, cout, R, pad
    (4, 64, 32, 128, 4, 1),    # BM=128 class, 8 pixel tiles
    (4, 128, 16, 256, 4, 1),   # 8x8 class grid, 2 c-tiles, 2 co-chunks
    (4, 64, 32, 128, 5, 2),    # odd taps: asymmetric union region
    (3, 128, 16, 256, 4, 1),   # odd image count
    (4, 128, 32, 128, 4, 1),   # BM=128 with two c-tiles
    (4, 64, 32, 128, 7, 3),    # large taps: BM=64 tile, one c-tile
]


@functools.lru_cache(maxsize=None)
def dgrad_case(nb, cin, h, cout, r, pad):
    x = mk((nb, cin, h, h), 50, 0.5)
    w = mk((cout, cin, r, r), 51, 0.2)
    ho = (h + 2 * pad - r) // 2 + 1
    gout = mk((nb, cout, ho, ho), 52)
    xr = x.float().cpu().requires_grad_(True)
    F.conv2d(xr, w.float().cpu(), None, stride=2, padding=pad).backward(
        gout.float().cpu())
    return x, w, gout, xr.grad


def run_dgrad(x, w, gout, pad):
    from gan_deeplearning4j_amd.ops import gpu_ops

    x2 = x.detach().clone().requires_grad_(True)
    y = gpu_ops.conv2d(x2, w, None, 2, pad, "identity")
    y.backward(gout)
    return x2.grad


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("nb,cin,h,cout,r,pad", DGRAD_SHAPES)
def test_dgrad_persist_matches_oneshot(nb, cin, h, cout, r, pad, cap):
    assert p_eligible(h, cin, cout, r, pad) != 0
    x, w, gout, ref = dgrad_case(nb, cin, h, cout, r, pad)
    dx1 = with_env("1", cap, lambda: run_dgrad(x, w, gout, pad))
    dx0 = with_env("0", None, lambda: run_dgrad(x, w, gout, pad))
    assert torch.equal(dx1, dx0)
    assert relerr(dx1, ref) < 0.04


# ------------------------------------------------------ convT forward
CONVT_SHAPES = [
    # cin, hi, cout, R, pad
    (256, 8, 128, 4, 1),
    (128, 16, 64, 4, 1),
]


@functools.lru_cache(maxsize=None)
def convt_case(cin, hi, cout, r, pad):
    x = mk((4, cin, hi, hi), 80, 0.5)
    w = mk((cin, cout, r, r), 81, 0.1)
    b = torch.randn(cout, generator=torch.Generator().manual_seed(84)).to(
        DEV, torch.bfloat16)
    ref = torch.tanh(F.conv_transpose2d(
        x.float().cpu(), w.float().cpu(), b.float().cpu(), stride=2,
        padding=pad))
    return x, w, b, ref


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,hi,cout,r,pad", CONVT_SHAPES)
def test_convt_persist_matches_oneshot(cin, hi, cout, r, pad, cap):
    from gan_deeplearning4j_amd.ops import gpu_ops

    assert p_eligible(2 * hi, cout, cin, r, pad) != 0
    x, w, b, ref = convt_case(cin, hi, cout, r, pad)

    def run():
        return gpu_ops.conv_transpose2d(x, w, b, 2, pad, "tanh")

    y1 = with_env("1", cap, run)
    y0 = with_env("0", None, run)
    assert torch.equal(y1, y0)
    assert relerr(y1, ref) < 0.04


@pytest.mark.parametrize("cap", CAPS)
def test_convt_persist_stats(cap):
    # fused BN statistics: deferred per-block reduction vs the one-shot
    # kernel's per-tile one, and vs direct fp32 sums over the output
    from gan_deeplearning4j_amd.ops import gpu_ops
    from gan_deeplearning4j_amd.ops.gpu_ops import take_bn_stats

    x = mk((4, 256, 8, 8), 82, 0.5)
    w = mk((256, 128, 4, 4), 83, 0.1)

    def run():
        y = gpu_ops.conv_transpose2d(x, w, None, 2, 1, "identity",
                                     emit_stats=True)
        stats = take_bn_stats(y)
        assert stats is not None
        return y, stats[0].float().cpu(), stats[1].float().cpu()

    y1, s1, q1 = with_env("1", cap, run)
    y0, s0, q0 = with_env("0", None, run)
    assert torch.equal(y1, y0)
    yf = y1.float()
    rsum = yf.sum(dim=(0, 2, 3)).cpu()
    rsq = (yf * yf).sum(dim=(0, 2, 3)).cpu()
    for got, want in ((s1, s0), (s1, rsum), (q1, q0), (q1, rsq)):
        assert (got - want).abs().max() / want.abs().max() < 0.02


# -------------------------------------------- producer act-backward + bias
@pytest.mark.parametrize("cap", CAPS)
def test_dgrad_persist_pact_leaf(cap):
    # act-backward epilogue + bias partials straight off the kernel: the
    # input is a leaf holding a leaky-relu output, the hook picks up the
    # bias gradient the dgrad deposits for its producer
    from gan_deeplearning4j_amd.ops import gpu_ops
    from gan_deeplearning4j_amd.ops.gpu_ops import take_act_fused

    xa = F.leaky_relu(mk((4, 64, 32, 32), 60, 0.5), 0.2)
    w = mk((128, 64, 4, 4), 61, 0.2)
    gout = mk((4, 128, 16, 16), 62)

    def run():
        got = []
        x = xa.detach().clone().requires_grad_(True)
        x.register_hook(lambda g: got.append(take_act_fused(g)))
        y = gpu_ops.conv2d(x, w, None, 2, 1, "identity",
                           prev_act=(3, 0.2, True))
        y.backward(gout)
        assert got and got[0] is not None and got[0][2] is not None
        return x.grad, got[0][2].float().cpu()

    dx1, db1 = with_env("1", cap, run)
    dx0, db0 = with_env("0", None, run)
    assert torch.equal(dx1, dx0)
    rdb = dx1.float().sum(dim=(0, 2, 3)).cpu()
    for want in (db0, rdb):
        assert (db1 - want).abs().max() / want.abs().max() < 0.02


@functools.lru_cache(maxsize=None)
def chain_reference():
    gout = torch.randn(4, 128, 16, 16,
                       generator=torch.Generator().manual_seed(72))
    x0 = mk((4, 64, 32, 32), 70, 0.5).float().cpu().requires_grad_(True)
    w1 = mk((64, 64, 3, 3), 71, 0.2).float().cpu().requires_grad_(True)
    b1 = mk((64,), 73).float().cpu().requires_grad_(True)
    w2 = mk((128, 64, 5, 5), 74, 0.2).float().cpu().requires_grad_(True)
    y = F.conv2d(F.leaky_relu(F.conv2d(x0, w1, b1, padding=1), 0.2),
                 w2, None, stride=2, padding=2)
    y.backward(gout)
    return gout, (x0.grad, w1.grad, b1.grad, w2.grad)


@pytest.mark.parametrize("cap", CAPS)
def test_dgrad_persist_pact_chain(cap):
    # the producer->consumer chain of test_conv_dgrad_direct_pact_fusion
    from gan_deeplearning4j_amd.ops import gpu_ops

    gout_cpu, ref = chain_reference()

    def run():
        x0 = mk((4, 64, 32, 32), 70, 0.5).requires_grad_(True)
        w1 = mk((64, 64, 3, 3), 71, 0.2).requires_grad_(True)
        b1 = mk((64,), 73).requires_grad_(True)
        w2 = mk((128, 64, 5, 5), 74, 0.2).requires_grad_(True)
        xh = gpu_ops.conv2d(x0, w1, b1, 1, 1, "lrelu", 0.2)
        y = gpu_ops.conv2d(xh, w2, None, 2, 2, "identity",
                           prev_act=(3, 0.2, True))
        y.backward(gout_cpu.to(DEV, torch.bfloat16))
        return x0.grad, w1.grad, b1.grad, w2.grad

    r1 = with_env("1", cap, run)
    r0 = with_env("0", None, run)
    for a, b in zip(r1, r0):
        assert relerr(a, b) < 0.02
    for a, b in zip(r1, ref):
        assert relerr(a, b) < 0.06


# ------------------------------------------------------------- eligibility
def test_dgrad_persist_refuses_lds_overflow():
    # Ko8=512 at a 16-wide class grid: no tile's union region + W double
    # buffer fits the two-blocks-per-CU LDS budget (and more than two
    # c-tiles are refused outright); the call must still be right through
    # the fallbacks
    assert p_eligible(32, 64, 512, 4, 1) == 0
    assert p_eligible(16, 256, 256, 4, 1) == 0
    nb, cin, h, cout, r, pad = 2, 64, 32, 512, 4, 1
    x, w, gout, ref = dgrad_case(nb, cin, h, cout, r, pad)
    dx = with_env("1", None, lambda: run_dgrad(x, w, gout, pad))
    assert relerr(dx, ref) < 0.04


# ----------------------------------------------------------------- capture
def test_dgrad_persist_graph_capture():
    # the kernel keeps no state between launches: capture one backward
    # with a 3-block grid, replay it on changed inputs
    from gan_deeplearning4j_amd.ops import gpu_ops

    nb, cin, h, cout, r, pad = DGRAD_SHAPES[0]
    x, w, gout, _ = dgrad_case(nb, cin, h, cout, r, pad)

    def body():
        xs = x.detach().clone().requires_grad_(True)
        gs = gout.clone()

        def step():
            gpu_ops.conv2d(xs, w, None, 2, pad, "identity").backward(gs)

        # warm-up on a side stream (packs the weights, sets attributes)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        xs.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        outs = []
        for seed in (90, 91):
            gs.copy_(mk(tuple(gout.shape), seed))
            graph.replay()
            torch.cuda.synchronize()
            outs.append((gs.clone(), xs.grad.clone()))
        return outs

    outs = with_env("1", 3, body)
    for gs, dx in outs:
        eager = with_env("0", None, lambda: run_dgrad(x, w, gs, pad))
        assert torch.equal(dx, eager)
