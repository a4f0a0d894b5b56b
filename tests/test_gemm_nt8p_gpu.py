"""GPU numerics of the deep-pipelined NT weight-gradient core (gemm_nt_8p in
gemm8p_nt.hip) against gemm_nt_core, the kernel it replaces by default.

Every case runs through ext.gemm_nt / ext.gemm_nt_implicit twice: once with
GDLJ_NT8P=0 (old core) and once with the gate unset and GDLJ_NT8P_MINK=1, so
the new core takes shapes far below its default floors.

splitk == 1: per C element both kernels issue the same MFMA sequence (same
fragment mapping, K-tiles and kc ascending), so the results must be
bit-equal (torch.equal).
splitk > 1: the new core re-derives its own split, so the fp32 partial sums
associate differently.  Bounds: relerr < 0.02 against the fp32 torch product
(the bound of test_ops_gpu.py::test_gemm_nt), and elementwise
|new - old| <= 1e-5 * max|ref| * sqrt(splitk), or twice the measured
old-vs-old difference of two runs on the same inputs if that is larger.
Measured on MI355X (each case prints its figures): the largest |new - old|
is 1.07e-4 at (512, 1152, 4096) against a bound of 5.96e-3 and an old-vs-old
difference of 3.05e-5; in no case was twice the old-vs-old difference the
larger bound, so the 1e-5 rule is the one that applied everywhere.
"""

import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("GDLJ_NT8P", "GDLJ_NT8P_MINK")


def ext():
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    return hip_ext()


def zero_page():
    from gan_deeplearning4j_amd.ops import gpu_ops

    return gpu_ops._zero_page(torch.device(DEV))


def mk(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, torch.bfloat16)


def with_env(env, fn):
    """Run fn() with exactly `env` set among the two gates, then restore."""
    old = {k: os.environ.get(k) for k in KEYS}
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


OLD = {"GDLJ_NT8P": "0"}
NEW = {"GDLJ_NT8P_MINK": "1"}


def relerr(a, b):
    denom = b.abs().max().clamp_min(1e-6)
    return ((a.float() - b).abs().max() / denom).item()


def check(call, ref, splitk, tail=False):
    """call(splitk) -> C; the assertions of the module docstring."""
    old = with_env(OLD, lambda: call(splitk))
    new = with_env(NEW, lambda: call(splitk))
    torch.cuda.synchronize()
    assert new.shape == ref.shape
    if splitk == 1:
        assert torch.equal(new, old)
    else:
        old2 = with_env(OLD, lambda: call(splitk))
        floor = (old2 - old).abs().max().item()
        bound = max(1e-5 * ref.abs().max().item() * math.sqrt(splitk),
                    2.0 * floor)
        diff = (new - old).abs().max().item()
        print(f"splitk={splitk} |new-old|={diff:.3e} |old-old|={floor:.3e} "
              f"bound={bound:.3e} relerr={relerr(new, ref):.3e}")
        assert diff <= bound
    assert relerr(new, ref) < 0.02
    if tail:
        # rows >= M / columns >= N are never written, and the last valid
        # row and column carry the right values
        assert relerr(new[-1, :], ref[-1, :]) < 0.02
        assert relerr(new[:, -1], ref[:, -1]) < 0.02


# ------------------------------------------------------------------ plain
PLAIN = [
    # M, N, K
    (256, 256, 64),     # one K-chunk: prologue + tail only
    (256, 256, 128),    # two K-chunks
    (256, 256, 192),    # three K-chunks
    (128, 256, 1000),   # K not a multiple of 64; 128-wide M tile
    (264, 520, 640),    # M and N tails
    (64, 128, 512),     # smaller than a tile
    (512, 1152, 4096),  # the test_gemm_nt shape
]


@functools.lru_cache(maxsize=None)
def plain_case(m, n, k):
    a = mk((k, m), 1)
    b = mk((k, n), 2)
    return a, b, a.float().t() @ b.float()


@pytest.mark.parametrize("splitk", [1, 4])
@pytest.mark.parametrize("m,n,k", PLAIN)
def test_plain(m, n, k, splitk):
    a, b, ref = plain_case(m, n, k)
    zp = zero_page()
    check(lambda sk: ext().gemm_nt(a, b, sk, zp), ref, splitk,
          tail=(m, n) == (264, 520))


# ------------------------------------------------- gathered (implicit wgrad)
def im2col_rsc(img_nhwc, r, stride, pad):
    """fp32 im2col of an NHWC image, columns ordered (r, s, c)."""
    nb, h, w, c = img_nhwc.shape
    x = img_nhwc.float().permute(0, 3, 1, 2)
    cols = F.unfold(x, r, padding=pad, stride=stride)   # [N, C*R*R, L]
    l = cols.shape[-1]
    cols = cols.view(nb, c, r, r, l).permute(0, 4, 2, 3, 1)
    return cols.reshape(nb * l, r * r * c)


def rup(x, m):
    return (x + m - 1) // m * m


CONV = [
    # batch, H, C8, Ko8, R, stride, pad
    (3, 8, 64, 128, 4, 2, 1),    # conv2 class: M = 128, the 128x256 tile
    (2, 8, 128, 256, 4, 2, 1),   # conv3 class: 256x256 tile
    (5, 16, 8, 64, 4, 2, 1),     # conv1 class: C8 = 8, below a tile
    (3, 8, 64, 128, 5, 2, 2),    # R=5 pad=2: border taps on every side
    (2, 8, 64, 128, 3, 1, 1),    # stride 1, R=3
]


@functools.lru_cache(maxsize=None)
def conv_case(nb, h, c8, ko8, r, stride, pad):
    from gan_deeplearning4j_amd.ops import gpu_ops

    ho = (h + 2 * pad - r) // stride + 1
    x = mk((nb, h, h, c8), 3, 0.5)
    dy = mk((nb * ho * ho, ko8), 4, 0.5)
    kpad = rup(r * r * c8, 64)
    ref = torch.zeros(ko8, kpad, device=DEV)
    ref[:, :r * r * c8] = dy.float().t() @ im2col_rsc(x, r, stride, pad)
    dims = gpu_ops._dims(nb, h, h, c8, ho, ho, r, r, stride, pad)
    return x, dy, kpad, nb * ho * ho, dims, ref


def conv_call(case, ko8):
    x, dy, kpad, npq, dims, _ = case
    zp = zero_page()
    return lambda sk: ext().gemm_nt_implicit(dy, x, 2, ko8, kpad, npq, dims,
                                             sk, zp)


@pytest.mark.parametrize("splitk", [1, 4])
@pytest.mark.parametrize("geom", CONV)
def test_gathered_b(geom, splitk):
    case = conv_case(*geom)
    check(conv_call(case, geom[3]), case[-1], splitk)


CONVT = [
    # batch, Hi, Cin, Co8 (R=4, stride 2, pad 1; dy is [N, 2Hi, 2Hi, Co8])
    (3, 4, 256, 128),   # convT2 mirror: M = 2048, N = 256
    (3, 8, 128, 64),    # convT3 mirror: N = 128, the 256x128 tile
]


@functools.lru_cache(maxsize=None)
def convt_case(nb, hi, cin, co8):
    from gan_deeplearning4j_amd.ops import gpu_ops

    ho = 2 * hi
    dy = mk((nb, ho, ho, co8), 5, 0.5)
    x2d = mk((nb * hi * hi, rup(cin, 64)), 6, 0.5)
    m = rup(16 * co8, 64)
    ref = torch.zeros(m, x2d.shape[1], device=DEV)
    ref[:16 * co8] = im2col_rsc(dy, 4, 2, 1).t() @ x2d.float()
    dims = gpu_ops._dims(nb, ho, ho, co8, hi, hi, 4, 4, 2, 1)
    return dy, x2d, m, nb * hi * hi, dims, ref


@pytest.mark.parametrize("splitk", [1, 4])
@pytest.mark.parametrize("geom", CONVT)
def test_gathered_a(geom, splitk):
    dy, x2d, m, npq, dims, ref = convt_case(*geom)
    zp = zero_page()
    check(lambda sk: ext().gemm_nt_implicit(dy, x2d, 1, m, x2d.shape[1], npq,
                                            dims, sk, zp), ref, splitk)


# ---------------------------------------------------------------- routing
def test_ineligible_shape_takes_fallback():
    """K below the default floor, both gates unset: the old core runs.  With
    splitk == 2 the old core's two atomic addends commute, so its result is
    deterministic, while the new core would re-derive a different split."""
    a, b, _ = plain_case(256, 256, 1024)
    zp = zero_page()
    old = with_env(OLD, lambda: ext().gemm_nt(a, b, 2, zp))
    dflt = with_env({}, lambda: ext().gemm_nt(a, b, 2, zp))
    assert torch.equal(dflt, old)


@pytest.mark.parametrize("splitk", [1, 4])
def test_graph_capture_replay(splitk):
    case = conv_case(*CONV[0])
    call = conv_call(case, CONV[0][3])
    ref = case[-1]

    def run():
        eager = call(splitk)           # also warms the launcher's one-time init
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = call(splitk)
        g.replay()
        torch.cuda.synchronize()
        return eager, out.clone()

    eager, replay = with_env(NEW, run)
    if splitk == 1:
        assert torch.equal(replay, eager)
    else:
        bound = 1e-5 * ref.abs().max().item() * math.sqrt(splitk)
        assert (replay - eager).abs().max().item() <= bound
    assert relerr(replay, ref) < 0.02
