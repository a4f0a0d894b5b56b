"""The class-GEMM route of the strided dgrad / convT forward (plan kind 3:
one gathered 8-phase GEMM per parity class, B read in place from the
[(r,s,c)][ko] pack; gemm8p.hip TAPB, launch_conv_dgrad_classgemm).

The small cases force the kind with GDLJ_DGRAD_CLASSGEMM_MINM=1 and assert a
non-empty result, and [] with GDLJ_DGRAD_CLASSGEMM=0: the pair shows the path
is taken (no direct kernel takes a class grid below 64 pixels).

Reference: float64 conv_transpose2d on the bf16-rounded inputs, compared per
element, never normalised by a tensor-wide maximum (the policy of
tests/membound_oracle.py).  With K = ntaps * Ko8 of the element's parity
class and S_e = (|dy| conv |w|)_e (+ |bias|) in float64:

    |got - ref| <= 2^-8 |ref| + K 2^-23 S_e

one bf16 rounding of the output plus fp32 accumulation, a factor 2 of margin
included.  lrelu is 1-Lipschitz, so the accumulation term holds after it.

That bound is for the route with one fp32 accumulation over all taps,
GDLJ_DGRAD_CLASSGEMM_FP32=1 (plan kind 4): the tests that carry it, the bit
equality with conv_parity_implicit, the statistics and the graph replay run
with that gate set.  The DEFAULT route (kind 3) reproduces dcol GEMM + col2im
instead, so that taking it does not change what a training step computes:
every tap's sum goes through bf16 before the taps add up.  It is held to
  * bit equality with gemm_tn + col2im where both run the 8p core, and
  * the bound above widened by exactly those roundings,
        + 2^-8 sum_taps |s_tap|,   s_tap the float64 sum of one tap,
    at the small shapes.
"""

import functools
import os

import pytest
import torch
import torch.nn.functional as F

import membound_oracle as mo

gpu = pytest.mark.gpu

COMPAT = {"GDLJ_DGRAD_CLASSGEMM_MINM": "1"}          # kind 3, the default
FORCE = {"GDLJ_DGRAD_CLASSGEMM_MINM": "1", "GDLJ_DGRAD_CLASSGEMM_FP32": "1"}
OFF = {"GDLJ_DGRAD_CLASSGEMM": "0", "GDLJ_DGRAD_CLASSGEMM_MINM": "1"}
DEFAULT = {}
FP32 = {"GDLJ_DGRAD_CLASSGEMM_FP32": "1"}
SLOPE = 0.2

CASES = [
    # Nb, H, W, C8, Ko8, R, pad
    (3, 8, 8, 256, 64, 4, 1),    # partial M-tile; K = 256; a tap per K-tile
    (3, 8, 8, 256, 128, 4, 1),   # two K-tiles per tap
    (3, 8, 8, 256, 192, 4, 1),   # Ko8 not a power of two
    (17, 8, 8, 256, 64, 4, 1),   # M = 272: a second, partial M-tile
    (3, 8, 8, 192, 64, 4, 1),    # N below one tile
    (3, 8, 8, 320, 64, 4, 1),    # a second, partial N-tile
    (3, 4, 8, 256, 64, 4, 1),    # 2x4 class grid
    (3, 8, 8, 256, 64, 5, 2),    # 3x3 / 3x2 / 2x3 / 2x2 taps: K per class
    (3, 8, 8, 256, 256, 3, 1),   # one class has a single tap, K = 256
]


def ext():
    from gan_deeplearning4j_amd.ops.backend import hip_ext
    return hip_ext()


def with_env(env, fn):
    keys = ("GDLJ_DGRAD_CLASSGEMM", "GDLJ_DGRAD_CLASSGEMM_MINM",
            "GDLJ_DGRAD_CLASSGEMM_FP32")
    old = {k: os.environ.pop(k, None) for k in keys}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def out_dim(h, r, pad):
    return (h + 2 * pad - r) // 2 + 1


@functools.lru_cache(maxsize=None)
def case(nb, h, w, c8, ko8, r, pad, seed=11):
    """CPU tensors: dy [Nb,Ho,Wo,Ko8], taps wc [C8,R,R,Ko8], bias [C8]."""
    g = torch.Generator().manual_seed(seed)
    ho, wo = out_dim(h, r, pad), out_dim(w, r, pad)
    dy = mo.bf(torch.randn(nb, ho, wo, ko8, generator=g) * 0.5)
    wc = mo.bf(torch.randn(c8, r, r, ko8, generator=g) * 0.1)
    bias = torch.randn(c8, generator=g) * 0.25
    return dy, wc, bias


def class_k(h, w, ko8, r, pad):
    """[H][W] K = ntaps * Ko8 of each output element's parity class."""
    def ntap(n):
        q = torch.arange(n) % 2
        return (r - (q + pad) % 2 + 1) // 2
    return (ntap(h)[:, None] * ntap(w)[None, :] * ko8).double()


def transposed(dy, wc, h, w, r, pad):
    """float64 conv_transpose2d, NHWC out: dx[n,h,w,c]."""
    ho, wo = dy.shape[1], dy.shape[2]
    op = (h - ((ho - 1) * 2 - 2 * pad + r), w - ((wo - 1) * 2 - 2 * pad + r))
    y = F.conv_transpose2d(dy.permute(0, 3, 1, 2), wc.permute(3, 0, 1, 2),
                           stride=2, padding=pad, output_padding=op)
    return y.permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def reference(nb, h, w, c8, ko8, r, pad):
    """(pre-activation float64 result, S_e, K map), shared by the tests."""
    dy, wc, _ = case(nb, h, w, c8, ko8, r, pad)
    ref = transposed(mo.d(dy), mo.d(wc), h, w, r, pad)
    s_e = transposed(mo.d(dy).abs(), mo.d(wc).abs(), h, w, r, pad)
    return ref, s_e, class_k(h, w, ko8, r, pad)[None, :, :, None]


def ratio(got, ref, s_e, kmap, taps=None):
    """worst |got - ref| / bound; <= 1 passes.  taps: sum_taps |s_tap| for
    the route that rounds every tap's sum to bf16."""
    bound = mo.BF16_ULP * ref.abs() + kmap * 2.0 ** -23 * s_e
    if taps is not None:
        bound = bound + mo.BF16_ULP * taps
    return mo._ratio(got, ref, bound)


@functools.lru_cache(maxsize=None)
def tap_abs_sum(nb, h, w, c8, ko8, r, pad):
    """sum over the taps of |float64 sum of that tap|, per output element."""
    dy, wc, _ = case(nb, h, w, c8, ko8, r, pad)
    dyd, wcd = mo.d(dy), mo.d(wc)
    tot = 0
    for i in range(r):
        for j in range(r):
            one = torch.zeros_like(wcd)
            one[:, i, j] = wcd[:, i, j]
            tot = tot + transposed(dyd, one, h, w, r, pad).abs()
    return tot


def wt_pack(wc):
    c8, r, s, ko8 = wc.shape
    return wc.permute(1, 2, 0, 3).reshape(r * s * c8, ko8).contiguous()


def zero_page():
    return torch.zeros(32, dtype=torch.uint8, device="cuda").view(
        torch.bfloat16)


def run_dgrad(geom, env, y0=None):
    nb, h, w, c8, ko8, r, pad = geom
    dy, wc, _ = case(*geom)
    ho, wo = dy.shape[1], dy.shape[2]
    return with_env(env, lambda: ext().conv_dgrad_direct(
        dy.cuda().view(-1, ko8), wt_pack(wc).cuda(), y0, zero_page(), nb, h,
        w, c8, ho, wo, r, r, 2, pad, 0, 0.0, False))


def run_convt(geom, env, act=3, want_stats=False):
    nb, h, w, c8, ko8, r, pad = geom
    dy, wc, bias = case(*geom)
    ho, wo = dy.shape[1], dy.shape[2]
    return with_env(env, lambda: ext().conv_transpose_fwd_direct(
        dy.cuda().view(-1, ko8), wt_pack(wc).cuda(), bias.cuda(), zero_page(),
        nb, ho, wo, h, w, c8, r, r, 2, pad, act, SLOPE, want_stats))


# ---------------------------------------------------------------- accuracy
@gpu
@pytest.mark.parametrize("geom", CASES, ids=lambda g: "x".join(map(str, g)))
def test_dgrad_classgemm_accuracy(geom):
    res = run_dgrad(geom, FORCE)
    assert len(res) == 1, "class GEMM not taken"
    assert run_dgrad(geom, OFF) == []
    assert run_dgrad(geom, DEFAULT) == []      # below the default floors
    ref, s_e, kmap = reference(*geom)
    r = ratio(res[0], ref, s_e, kmap)
    print(f"dgrad {geom}: worst error / bound = {r:.3f}")
    assert r <= 1.0


@gpu
@pytest.mark.parametrize("geom", CASES, ids=lambda g: "x".join(map(str, g)))
def test_convt_classgemm_accuracy(geom):
    res = run_convt(geom, FORCE)
    assert len(res) == 1, "class GEMM not taken"
    assert run_convt(geom, OFF) == []
    assert run_convt(geom, DEFAULT) == []
    pre, s_e, kmap = reference(*geom)
    bias = mo.d(case(*geom)[2])
    ref = mo.act_ref(pre + bias, "lrelu", SLOPE)
    r = ratio(res[0], ref, s_e + bias.abs(), kmap)
    print(f"convT {geom}: worst error / bound = {r:.3f}")
    assert r <= 1.0


@gpu
def test_convt_classgemm_stats():
    """want_stats: sum / sumsq are those of the returned y."""
    geom = CASES[3]
    y, ssum, ssq = run_convt(geom, FORCE, want_stats=True)
    y2 = mo.d(y).reshape(-1, geom[3])
    assert torch.equal(y.cpu(), run_convt(geom, FORCE)[0].cpu())
    assert mo.reduction(ssum, y2.sum(0), y2.abs().sum(0)) <= 1.0
    assert mo.reduction(ssq, (y2 * y2).sum(0), (y2 * y2).sum(0)) <= 1.0


@gpu
def test_dgrad_classgemm_refuses_y0():
    """No fused act backward in this kind: with y0 the caller falls back."""
    geom = CASES[0]
    nb, h, w, c8 = geom[:4]
    y0 = torch.ones(nb, h, w, c8, device="cuda", dtype=torch.bfloat16)
    assert run_dgrad(geom, FORCE, y0=y0) == []
    assert len(run_dgrad(geom, FORCE)) == 1


@gpu
def test_p_eligible_stays_zero():
    nb, h, w, c8, ko8, r, pad = CASES[0]
    assert with_env(FORCE, lambda: ext().conv_dgrad_direct_p_eligible(
        h, w, c8, ko8, ko8, r, r, 2, pad)) == 0


# ------------------------------------- the default route: dcol's roundings
@gpu
@pytest.mark.parametrize("geom", CASES, ids=lambda g: "x".join(map(str, g)))
def test_compat_classgemm_accuracy(geom):
    taps = tap_abs_sum(*geom)
    pre, s_e, kmap = reference(*geom)
    res = run_dgrad(geom, COMPAT)
    assert len(res) == 1, "class GEMM not taken"
    r = ratio(res[0], pre, s_e, kmap, taps)
    print(f"compat dgrad {geom}: worst error / bound = {r:.3f}")
    assert r <= 1.0
    bias = mo.d(case(*geom)[2])
    res = run_convt(geom, COMPAT)
    assert len(res) == 1, "class GEMM not taken"
    ref = mo.act_ref(pre + bias, "lrelu", SLOPE)
    r = ratio(res[0], ref, s_e + bias.abs(), kmap, taps)
    print(f"compat convT {geom}: worst error / bound = {r:.3f}")
    assert r <= 1.0
    # no statistics epilogue that could reproduce col2im_stats, no act bwd
    assert run_convt(geom, COMPAT, want_stats=True) == []
    nb, h, w, c8 = geom[:4]
    y0 = torch.ones(nb, h, w, c8, device="cuda", dtype=torch.bfloat16)
    assert run_dgrad(geom, COMPAT, y0=y0) == []


# The smallest shapes at which the dcol GEMM runs the 8p core as it does in
# training (M = Nb*Ho*Wo >= 32768 rows, K = Ko8 = 256), so that its tap sums
# are accumulated in the class GEMMs' order.  The first runs under the default
# gates (65536 rows per class); the others have 32768 rows per class, below the
# class route's block floor, and force it.
BIT_EQUAL = [
    ((4096, 8, 8, 256, 256, 4, 1), DEFAULT),
    ((2048, 8, 8, 256, 256, 5, 2), COMPAT),   # 3x3 / 3x2 / 2x3 / 2x2 taps
    ((2048, 8, 8, 320, 256, 3, 1), COMPAT),   # single-tap class, partial N
    ((4096, 4, 8, 192, 256, 4, 1), COMPAT),   # 2x4 class grid, N < 2 tiles
]


@gpu
@pytest.mark.parametrize("geom,env", BIT_EQUAL,
                         ids=lambda v: "x".join(map(str, v))
                         if isinstance(v, tuple) else "")
def test_compat_classgemm_bit_equal_to_dcol_col2im(geom, env):
    """dx / y of the default route are the bits of gemm_tn + col2im, so
    taking the route changes no training step."""
    nb, h, w, c8, ko8, r, pad = geom
    dy, wc, bias = case(*geom)
    ho, wo = dy.shape[1], dy.shape[2]
    wt = wt_pack(wc).cuda()
    dcol = ext().gemm_tn(dy.cuda().view(-1, ko8), wt, None, 0, 0.0, False)
    res = run_dgrad(geom, env)
    assert len(res) == 1, "class GEMM not taken"
    want = ext().col2im(dcol, nb, h, w, c8, ho, wo, r, r, 2, pad, r * r * c8,
                        None, 0, 0.0)
    assert torch.equal(res[0], want)
    res = run_convt(geom, env, act=4)
    assert len(res) == 1
    want = ext().col2im(dcol, nb, h, w, c8, ho, wo, r, r, 2, pad, r * r * c8,
                        bias.cuda(), 4, SLOPE)
    assert torch.equal(res[0], want)


# ------------------------------------------- bit equality with class packs
def parity_packs(wc, pad):
    from gan_deeplearning4j_amd.ops import gpu_ops
    return gpu_ops._parity_class_packs(wc, 2, pad)


@gpu
def test_classgemm_bit_equal_to_parity_implicit():
    """Smallest shape where both sides run the 8p core under the default
    floors (65536 rows per class = 256 blocks): same kernel, K order and
    data, only where B is read from differs."""
    geom = (4096, 8, 8, 256, 128, 4, 1)
    nb, h, w, c8, ko8, r, pad = geom
    dy, wc, bias = case(*geom)
    dyg, wcg, bg = dy.cuda(), wc.cuda(), bias.cuda()
    packs = parity_packs(wcg, pad)
    res = run_dgrad(geom, FP32)
    assert len(res) == 1, "class GEMM not taken under the default floors"
    want = ext().conv_parity_implicit(dyg, packs, None, zero_page(), nb, 4, 4,
                                      ko8, h, w, c8, r, r, 2, pad, 0, 0.0)
    assert torch.equal(res[0].view(-1, c8), want)
    res = run_convt(geom, FP32, act=1)
    assert len(res) == 1
    want = ext().conv_parity_implicit(dyg, packs, bg, zero_page(), nb, 4, 4,
                                      ko8, h, w, c8, r, r, 2, pad, 1, SLOPE)
    assert torch.equal(res[0].view(-1, c8), want)


# ----------------------------------------------------------- graph capture
@gpu
@pytest.mark.parametrize("env", [COMPAT, FORCE], ids=["default", "fp32"])
def test_classgemm_graph_replay_on_changed_inputs(env):
    geom = CASES[3]
    nb, h, w, c8, ko8, r, pad = geom
    dy, wc, _ = case(*geom)
    dy2 = case(*geom, seed=12)[0]
    ho, wo = dy.shape[1], dy.shape[2]
    sdy = dy.cuda().view(-1, ko8).clone()
    wt, zp = wt_pack(wc).cuda(), zero_page()

    def call():
        return ext().conv_dgrad_direct(sdy, wt, None, zp, nb, h, w, c8, ho,
                                       wo, r, r, 2, pad, 0, 0.0, False)[0]

    def body():
        eager1 = call().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = call()
        sdy.copy_(dy2.cuda().view(-1, ko8))
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager2 = call()
        return eager1, replayed, eager2

    eager1, replayed, eager2 = with_env(env, body)
    assert torch.equal(replayed, eager2)
    assert not torch.equal(replayed, eager1)


# ------------------------------------------------- the bound rejects mutants
def test_bound_rejects_wrong_tap_and_unwritten_class():
    """CPU: the comparator above accepts an fp32-accumulated, bf16-rounded
    result and rejects the two ways this route can go wrong: one tap's
    weights taken from another tap, and one parity class left unwritten."""
    for geom in (CASES[0], CASES[7], CASES[8]):
        nb, h, w, c8, ko8, r, pad = geom
        dy, wc, _ = case(*geom)
        ref, s_e, kmap = reference(*geom)
        good = mo.bf(transposed(dy.float(), wc.float(), h, w, r, pad))
        assert ratio(good, ref, s_e, kmap) <= 1.0
        wrong = wc.clone()
        wrong[:, r - 1, r - 1] = wc[:, 0, 0]           # one wrong tap
        bad = mo.bf(transposed(dy.float(), wrong.float(), h, w, r, pad))
        assert ratio(bad, ref, s_e, kmap) > 1.0
        for qh in (0, 1):
            for qw in (0, 1):
                bad = good.clone()
                bad[:, qh::2, qw::2] = 0                # class unwritten
                assert ratio(bad, ref, s_e, kmap) > 1.0
