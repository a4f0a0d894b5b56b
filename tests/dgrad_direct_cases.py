"""Shared inputs, references and runners of the direct dgrad / convT tests
(conv_dgrad_direct.hip: the one-shot, persistent and wide kernels).

Not collected by pytest.  Used by test_dgrad_persist_gpu.py,
test_dgrad_wide_gpu.py and test_dgrad_direct_golden_gpu.py (and by the
latter's golden recorder), so that all of them run the same data through
the same calls.
"""

import functools
import os

import torch
import torch.nn.functional as F

DEV = "cuda:0"
GATES = ("GDLJ_DGRAD_DIRECT", "GDLJ_DGRAD_PERSIST", "GDLJ_DGRAD_WIDE",
         "GDLJ_DGRAD_PERSIST_BLOCKS")
# routing arms: the gates each one sets (all others are cleared)
WIDE = {}                                  # the default routing
WIDE0 = {"GDLJ_DGRAD_WIDE": "0"}           # two-blocks-per-CU persistent
ONESHOT = {"GDLJ_DGRAD_PERSIST": "0"}      # one-shot kernel
DCOL = {"GDLJ_DGRAD_DIRECT": "0"}          # dcol GEMM + col2im


def mk(shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return t.to(DEV, torch.bfloat16)


def relerr(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


def with_env(env, cap, fn):
    """Run fn() with exactly the given routing gates set (cap is
    GDLJ_DGRAD_PERSIST_BLOCKS, None = uncapped), then restore them."""
    old = {k: os.environ.get(k) for k in GATES}
    for k in GATES:
        os.environ.pop(k, None)
    os.environ.update(env)
    if cap is not None:
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
    """0 = no persistent kernel takes it, 1 = persistent, 2 = wide."""
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    return hip_ext().conv_dgrad_direct_p_eligible(h, h, c8, ko8, ko8, r, r,
                                                  2, pad)


# ------------------------------------------------------------ conv2d dgrad
@functools.lru_cache(maxsize=None)
def dgrad_case(nb, cin, h, cout, r, pad):
    """x, w, gout of a stride-2 conv and its fp32 torch dx."""
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


# ------------------------------------------------------ convT forward
@functools.lru_cache(maxsize=None)
def convt_case(nb, cin, hi, cout, r, pad):
    """x, w, b of a stride-2 tanh convT and its fp32 torch output."""
    x = mk((nb, cin, hi, hi), 80, 0.5)
    w = mk((cin, cout, r, r), 81, 0.1)
    b = torch.randn(cout, generator=torch.Generator().manual_seed(84)).to(
        DEV, torch.bfloat16)
    ref = torch.tanh(F.conv_transpose2d(
        x.float().cpu(), w.float().cpu(), b.float().cpu(), stride=2,
        padding=pad))
    return x, w, b, ref


def run_convt(x, w, b, pad):
    from gan_deeplearning4j_amd.ops import gpu_ops

    return gpu_ops.conv_transpose2d(x, w, b, 2, pad, "tanh")


# -------------------------------------------- producer act-backward + bias
@functools.lru_cache(maxsize=None)
def pact_inputs(nb, cin, h, cout, r=4, pad=1):
    """A leaf holding a leaky-relu output, the consumer's w and gout."""
    xa = F.leaky_relu(mk((nb, cin, h, h), 60, 0.5), 0.2)
    w = mk((cout, cin, r, r), 61, 0.2)
    ho = (h + 2 * pad - r) // 2 + 1
    gout = mk((nb, cout, ho, ho), 62)
    return xa, w, gout


def run_pact(xa, w, gout, pad=1):
    """dx with the act-backward epilogue, and the bias gradient the dgrad
    deposits for its producer (picked up by the hook)."""
    from gan_deeplearning4j_amd.ops import gpu_ops
    from gan_deeplearning4j_amd.ops.gpu_ops import take_act_fused

    got = []
    x = xa.detach().clone().requires_grad_(True)
    x.register_hook(lambda g: got.append(take_act_fused(g)))
    y = gpu_ops.conv2d(x, w, None, 2, pad, "identity",
                       prev_act=(3, 0.2, True))
    y.backward(gout)
    assert got and got[0] is not None and got[0][2] is not None
    return x.grad, got[0][2].float().cpu()
