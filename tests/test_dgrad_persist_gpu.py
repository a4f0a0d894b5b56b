"""GPU numerics of the persistent class-fused direct dgrad / convT kernel
(conv_dgrad_direct_p in conv_dgrad_direct.hip).

Every case runs the default routing (GDLJ_DGRAD_PERSIST=1; the other gates
are left unset, so the 8x8-class-grid cases run the wide kernel
conv_dgrad_direct_w and the rest the persistent one; the persistent kernel
on the 8x8 grid, its qsplit path, is pinned by
test_dgrad_direct_golden_gpu.py and compared in test_dgrad_wide_gpu.py)
with the grid capped at 1 block (one block walks every tile), 3 blocks
(uneven split) and uncapped, and compares against the one-shot kernel
(GDLJ_DGRAD_PERSIST=0).  dx / y must be bit-identical: per output element
the accumulation sequence and the epilogue are the same; only the order
of the fp32 bias / BN partial sums differs.  Against an fp32 torch
reference the project's bounds for these paths apply.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import dgrad_direct_cases as D
from dgrad_direct_cases import (DEV, convt_case, dgrad_case, mk, p_eligible,
                                relerr, run_dgrad)

pytestmark = pytest.mark.gpu

CAPS = [1, 3, None]


def with_env(persist, cap, fn):
    """Run fn() with GDLJ_DGRAD_PERSIST = persist and the grid cap, every
    other routing gate unset: "1" is the default routing, i.e. the wide
    kernel where it takes the geometry, else the persistent one.
    Deliberately unlike this file's earlier helper, which left
    GDLJ_DGRAD_WIDE and GDLJ_DGRAD_DIRECT as the caller's environment had
    them: an exported gate no longer changes which kernels these tests
    compare."""
    return D.with_env({"GDLJ_DGRAD_PERSIST": persist}, cap, fn)


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


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,hi,cout,r,pad", CONVT_SHAPES)
def test_convt_persist_matches_oneshot(cin, hi, cout, r, pad, cap):
    from gan_deeplearning4j_amd.ops import gpu_ops

    assert p_eligible(2 * hi, cout, cin, r, pad) != 0
    x, w, b, ref = convt_case(4, cin, hi, cout, r, pad)

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


def test_dgrad_oneshot_refuses_unswizzlable_region():
    # Ko8 = 384 is 48 16-byte chunks per cell, not a power of two: the
    # stager's chunk swizzle slot ^ (cc & 47) stops being a permutation of
    # a cell's chunks at region column 32.  The plan refuses such Ko8 by the
    # simple sufficient condition "more columns than the lowest set bit of
    # 48", i.e. from 17 columns on.  This geometry (2x32 class grid, 2x2
    # taps: a 2x32 region of 48 KiB, which fits) has 32 columns: its staging
    # would still be right, but it is on the refused side of that condition,
    # so no direct kernel may take it and the empty result sends the caller
    # to dcol + col2im.  dpre is the head of a larger buffer.
    from gan_deeplearning4j_amd.ops import gpu_ops
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    n, h, w, c8, ko8, r = 1, 4, 64, 64, 384, 2
    ho, wo = h // 2, w // 2
    rows = n * ho * wo
    buf = mk((rows + 8, ko8), 95)
    dpre = buf[:rows]
    wt = mk((r * r * c8, ko8), 96, 0.2)
    zp = gpu_ops._zero_page(dpre.device)
    res = D.with_env(D.ONESHOT, None, lambda: hip_ext().conv_dgrad_direct(
        dpre, wt, None, zp, n, h, w, c8, ho, wo, r, r, 2, 0, 0, 0.0, False))
    assert len(res) == 0


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
