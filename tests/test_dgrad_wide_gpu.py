"""GPU numerics of the wide direct dgrad / convT kernel
(conv_dgrad_direct_w in conv_dgrad_direct.hip): one 8-wave block per CU,
tiles of two images' 8x8 class grids, three W buffers.  The 16x16 class
grid lost its A/B and stays on conv_dgrad_direct_p; its shapes (the 32x32
rows of DGRAD_SHAPES, the convT3 row, the class A leaf case) run here all
the same, but both arms are then conv_dgrad_direct_p: those rows only
guard the routing and the GDLJ_DGRAD_WIDE gate, the 16x16-input rows are
the ones that compare two kernels.

Batch 3 throughout, so that the image-pair tile runs one full tile and
one half tile.  Every case runs the default routing with the
grid capped at 1 block (one block walks every tile), 2 blocks and
uncapped, and once with GDLJ_DGRAD_WIDE=0 (the two-blocks-per-CU
persistent kernel).  dx / y must be bit-identical between the arms: per
output element the accumulation sequence and the epilogue are the same;
only the order of the fp32 bias / BN partial sums differs.  Against an
fp32 torch reference the project's bounds for these paths apply.
"""

import functools

import pytest
import torch

import dgrad_direct_cases as D
from dgrad_direct_cases import (DCOL, ONESHOT, WIDE, WIDE0, mk, p_eligible,
                                relerr, run_dgrad, run_pact, with_env)

gpu = pytest.mark.gpu

NB = 3
CAPS = [1, 2, None]


# ------------------------------------------------------------ conv2d dgrad
DGRAD_SHAPES = [
    # cin, h, cout, R, pad, taken by the older direct kernels
    (64, 32, 128, 4, 1, True),    # class A: 16x16 class grid
    (128, 16, 256, 4, 1, True),   # class B: image-pair tile, 2 c-tiles
    (128, 32, 128, 4, 1, True),   # 16x16 class grid with two c-tiles
    (64, 32, 128, 5, 2, True),    # asymmetric tap set
    (64, 32, 128, 7, 3, True),    # 19x19 union region
    (128, 16, 256, 5, 2, False),  # newly eligible: no direct predecessor
    (64, 16, 128, 4, 1, True),    # image-pair tile with one c-tile
]


def want_kind(h):
    """conv_dgrad_direct_p_eligible of the shapes here: 2 (wide) on the
    8x8 class grid, 1 (persistent) on the 16x16 one."""
    return 2 if h == 16 else 1


def dgrad_case(cin, h, cout, r, pad):
    return D.dgrad_case(NB, cin, h, cout, r, pad)


@functools.lru_cache(maxsize=None)
def dgrad_other_arms(cin, h, cout, r, pad, direct):
    """dx of the arms the wide kernel is compared with, once per shape."""
    x, w, gout, _ = dgrad_case(cin, h, cout, r, pad)
    arms = {"wide0": with_env(WIDE0, None, lambda: run_dgrad(x, w, gout, pad))}
    if direct:
        arms["oneshot"] = with_env(ONESHOT, None,
                                   lambda: run_dgrad(x, w, gout, pad))
    else:
        arms["dcol"] = with_env(DCOL, None,
                                lambda: run_dgrad(x, w, gout, pad))
    return arms


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,h,cout,r,pad,direct", DGRAD_SHAPES)
def test_dgrad_wide_matches_other_arms(cin, h, cout, r, pad, direct, cap):
    assert p_eligible(h, cin, cout, r, pad) == want_kind(h)
    x, w, gout, ref = dgrad_case(cin, h, cout, r, pad)
    arms = dgrad_other_arms(cin, h, cout, r, pad, direct)
    dx = with_env(WIDE, cap, lambda: run_dgrad(x, w, gout, pad))
    if direct:
        assert torch.equal(dx, arms["wide0"])
        assert torch.equal(dx, arms["oneshot"])
    else:
        # GDLJ_DGRAD_WIDE=0 leaves this geometry to dcol + col2im
        assert torch.equal(arms["wide0"], arms["dcol"])
        assert relerr(dx, arms["dcol"]) < 0.02
    assert relerr(dx, ref) < 0.04


# ------------------------------------------------------ convT forward
CONVT_SHAPES = [
    # cin, hi, cout, R, pad
    (256, 8, 128, 4, 1),     # convT2 class: image-pair tile
    (128, 16, 64, 4, 1),     # convT3 class: 16x16 class grid
]


@functools.lru_cache(maxsize=None)
def convt_case(cin, hi, cout, r, pad):
    x, w, b, ref = D.convt_case(NB, cin, hi, cout, r, pad)
    y0 = with_env(WIDE0, None, lambda: D.run_convt(x, w, b, pad))
    return x, w, b, ref, y0


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,hi,cout,r,pad", CONVT_SHAPES)
def test_convt_wide_matches_persistent(cin, hi, cout, r, pad, cap):
    from gan_deeplearning4j_amd.ops import gpu_ops

    assert p_eligible(2 * hi, cout, cin, r, pad) == want_kind(2 * hi)
    x, w, b, ref, y0 = convt_case(cin, hi, cout, r, pad)
    y1 = with_env(WIDE, cap,
                  lambda: gpu_ops.conv_transpose2d(x, w, b, 2, pad, "tanh"))
    assert torch.equal(y1, y0)
    assert relerr(y1, ref) < 0.04


@functools.lru_cache(maxsize=None)
def stats_case():
    x = mk((NB, 256, 8, 8), 82, 0.5)
    w = mk((256, 128, 4, 4), 83, 0.1)
    return x, w, with_env(WIDE0, None, lambda: run_stats(x, w))


def run_stats(x, w):
    from gan_deeplearning4j_amd.ops import gpu_ops
    from gan_deeplearning4j_amd.ops.gpu_ops import take_bn_stats

    y = gpu_ops.conv_transpose2d(x, w, None, 2, 1, "identity",
                                 emit_stats=True)
    stats = take_bn_stats(y)
    assert stats is not None
    return y, stats[0].float().cpu(), stats[1].float().cpu()


@gpu
@pytest.mark.parametrize("cap", CAPS)
def test_convt_wide_stats(cap):
    # fused BN statistics on the convT2 shape; the half tile's absent
    # image must add nothing to them
    x, w, (y0, s0, q0) = stats_case()
    y1, s1, q1 = with_env(WIDE, cap, lambda: run_stats(x, w))
    assert torch.equal(y1, y0)
    yf = y1.float()
    rsum = yf.sum(dim=(0, 2, 3)).cpu()
    rsq = (yf * yf).sum(dim=(0, 2, 3)).cpu()
    for got, want in ((s1, s0), (s1, rsum), (q1, q0), (q1, rsq)):
        assert (got - want).abs().max() / want.abs().max() < 0.02


# -------------------------------------------- producer act-backward + bias
PACT_SHAPES = [
    # cin, h, cout
    (64, 32, 128),     # the class A leaf case
    (128, 16, 256),    # the same on the image-pair tile (wide kernel)
    (64, 16, 128),     # image-pair tile with one c-tile
]


@functools.lru_cache(maxsize=None)
def pact_case(cin, h, cout):
    xa, w, gout = D.pact_inputs(NB, cin, h, cout)
    return xa, w, gout, with_env(WIDE0, None, lambda: run_pact(xa, w, gout))


@gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cin,h,cout", PACT_SHAPES)
def test_dgrad_wide_pact_leaf(cin, h, cout, cap):
    # act-backward epilogue + bias partials straight off the kernel
    xa, w, gout, (dx0, db0) = pact_case(cin, h, cout)
    dx1, db1 = with_env(WIDE, cap, lambda: run_pact(xa, w, gout))
    assert torch.equal(dx1, dx0)
    rdb = dx1.float().sum(dim=(0, 2, 3)).cpu()
    for want in (db0, rdb):
        assert (db1 - want).abs().max() / want.abs().max() < 0.02


# ----------------------------------------------------------------- capture
@gpu
def test_dgrad_wide_graph_capture():
    # the kernel keeps no state between launches: capture one backward
    # with a 2-block grid, replay it on changed inputs
    from gan_deeplearning4j_amd.ops import gpu_ops

    cin, h, cout, r, pad, _ = DGRAD_SHAPES[1]
    x, w, gout, _ = dgrad_case(cin, h, cout, r, pad)

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

    outs = with_env(WIDE, 2, body)
    for gs, dx in outs:
        eager = with_env(WIDE, None, lambda: run_dgrad(x, w, gs, pad))
        assert torch.equal(dx, eager)


# ------------------------------------------------------- eligibility (CPU)
def test_dgrad_wide_eligibility():
    # the plan needs no GPU: 2 = wide kernel, 1 = persistent, 0 = neither
    from gan_deeplearning4j_amd.ops.backend import has_hip_ext

    if not has_hip_ext():
        pytest.skip("extension not built")
    for cin, h, cout, r, pad, _ in DGRAD_SHAPES:
        assert p_eligible(h, cin, cout, r, pad) == want_kind(h)
    for cin, hi, cout, r, pad in CONVT_SHAPES:
        assert p_eligible(2 * hi, cout, cin, r, pad) == want_kind(2 * hi)
    # the tile is an image pair whatever the batch; C8 = 64 on that grid
    assert p_eligible(16, 64, 128, 4, 1) == 2
    # refused by every persistent kernel: Ko8=512 at a 16-wide class grid,
    # and more than two c-tiles
    assert p_eligible(32, 64, 512, 4, 1) == 0
    assert p_eligible(16, 256, 256, 4, 1) == 0
    # Ko8=256 at a 16-wide class grid: not wide.  The plan refuses every
    # class grid but 8x8 before it looks at LDS (the 18x18x512 B region
    # would not fit next to three W buffers either); the persistent
    # kernel keeps the geometry
    assert p_eligible(32, 64, 256, 4, 1) == 1
    # a non-square class grid of 64 pixels (4x16) is not wide either
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    assert hip_ext().conv_dgrad_direct_p_eligible(8, 32, 128, 256, 256, 4, 4,
                                                  2, 1) != 2
