"""Per-shape A/B of the NT weight-gradient GEMM: gemm_nt_core vs gemm_nt_8p.

Two arms: "old" (GDLJ_NT8P=0, the 128x128 core of gemm.hip) and "new"
(gemm8p_nt.hip, forced onto every shape with GDLJ_NT8P_MINK=0 so that
shapes the default eligibility leaves on the old core are measured too).
Both gates are re-read per call, so the arms run in one process on
identical data.  Shapes are the DCGAN-64 weight gradients at batch 16384
(plus the two K = 32768 shapes of DCGAN-128 at its batch 2048, which sit on
the default K floor), called through ext.gemm_nt_implicit / ext.gemm_nt
exactly as gpu_ops does (same operands, same caller split-K).  The old arm
is timed REPS times; its spread (max-min)/min is the bar a new-core win has
to clear.  The new core is also timed without its XCD block remap
(GDLJ_NT8P_XCD=0).

  python tools/ab_wgrad_nt.py                    # all shapes
  python tools/ab_wgrad_nt.py --only conv3 --arm new --iters 1   # PMC runs
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gan_deeplearning4j_amd.ops import gpu_ops  # noqa: E402
from gan_deeplearning4j_amd.ops.backend import hip_ext  # noqa: E402

ARMS = {
    "old": {"GDLJ_NT8P": "0"},
    "new": {"GDLJ_NT8P": "1", "GDLJ_NT8P_MINK": "0"},
}
REPS = 3

NB = 16384
# conv wgrad, gathered-B: name, Cin8, H, Cout8, batch (R=4, stride 2, pad 1)
CONVS = [
    ("conv1", 8, 64, 64, NB),
    ("conv2", 64, 32, 128, NB),
    ("conv3", 128, 16, 256, NB),
    ("conv4", 256, 8, 512, NB),
    ("dcgan128_conv5", 512, 8, 512, 2048),
]
# convT wgrad, gathered-A: name, Cin, Hi, Cout8, batch (R=4, stride 2, pad 1)
CONVTS = [
    ("convT1", 512, 4, 256, NB),
    ("convT2", 256, 8, 128, NB),
    ("convT3", 128, 16, 64, NB),
    ("g_out", 64, 32, 8, NB),
    ("dcgan128_convT1", 512, 4, 512, 2048),
]
# dense wgrad, plain: name, nout, nin, batch (= contraction rows)
DENSES = [
    ("d_dense_feat", 1024, 8192, NB),
    ("g_dense_0", 8192, 128, NB),
]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def rand_bf16(shape, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(
        torch.bfloat16)


def make_conv(cin8, h, cout8, nb):
    ho = h // 2
    x = rand_bf16((nb, h, h, cin8), 1, 0.5)
    dy = rand_bf16((nb * ho * ho, cout8), 2, 0.1)
    kpad = (16 * cin8 + 63) // 64 * 64
    npq = nb * ho * ho
    sk = gpu_ops._splitk_for((cout8 + 127) // 128, (kpad + 127) // 128,
                             (npq + 63) // 64)
    dims = gpu_ops._dims(nb, h, h, cin8, ho, ho, 4, 4, 2, 1)
    zp = gpu_ops._zero_page(x.device)
    flops = 2.0 * cout8 * kpad * npq
    return (lambda: hip_ext().gemm_nt_implicit(dy, x, 2, cout8, kpad, npq,
                                               dims, sk, zp)), flops


def make_convt(cin, hi, cout8, nb):
    ho = hi * 2
    dy = rand_bf16((nb, ho, ho, cout8), 3, 0.1)
    npq = nb * hi * hi
    x2d = rand_bf16((npq, (cin + 63) // 64 * 64), 4, 0.5)
    m = (16 * cout8 + 63) // 64 * 64
    sk = gpu_ops._splitk_for((m + 127) // 128, (x2d.shape[1] + 127) // 128,
                             (npq + 63) // 64)
    dims = gpu_ops._dims(nb, ho, ho, cout8, hi, hi, 4, 4, 2, 1)
    zp = gpu_ops._zero_page(dy.device)
    flops = 2.0 * m * x2d.shape[1] * npq
    return (lambda: hip_ext().gemm_nt_implicit(dy, x2d, 1, m, x2d.shape[1],
                                               npq, dims, sk, zp)), flops


def make_dense(nout, nin, nb):
    dy = rand_bf16((nb, nout), 5, 0.1)
    x = rand_bf16((nb, nin), 6, 0.5)
    sk = gpu_ops._splitk_for((nout + 127) // 128, (nin + 127) // 128,
                             (nb + 63) // 64)
    zp = gpu_ops._zero_page(x.device)
    return (lambda: hip_ext().gemm_nt(dy, x, sk, zp)), 2.0 * nout * nin * nb


def report(name, fn, flops, iters, arms):
    if arms != ["old", "new"]:
        for arm in arms:
            t = with_env(ARMS[arm], lambda: timed(fn, iters))
            print(f"{name}: {arm} {t:.3f} ms", flush=True)
        return
    olds = [with_env(ARMS["old"], lambda: timed(fn, iters))
            for _ in range(REPS)]
    new = with_env(ARMS["new"], lambda: timed(fn, iters))
    noxcd = with_env(dict(ARMS["new"], GDLJ_NT8P_XCD="0"),
                     lambda: timed(fn, iters))
    c_old = with_env(ARMS["old"], fn).double()
    c_new = with_env(ARMS["new"], fn).double()
    scale = c_old.abs().max().item()
    diff = (c_new - c_old).abs().max().item() / max(scale, 1e-30)
    lo, hi = min(olds), max(olds)
    spread = (hi - lo) / lo
    gain = lo / new - 1.0
    verdict = "WIN" if new < lo * (1.0 - spread) else "no win"
    print(f"{name}: old {lo:.3f}..{hi:.3f} ms (spread {spread * 100:.2f}%) "
          f"{flops / lo / 1e9:.0f} TF/s | new {new:.3f} ms "
          f"{flops / new / 1e9:.0f} TF/s (no XCD remap {noxcd:.3f} ms) | "
          f"{gain * 100:+.1f}% {verdict} | "
          f"sum old {c_old.sum().item():.6e} new {c_new.sum().item():.6e} "
          f"max|d|/max|c| {diff:.2e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="run one shape by name")
    ap.add_argument("--arm", default=None, choices=list(ARMS))
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    arms = [a.arm] if a.arm else ["old", "new"]
    jobs = ([(n, make_conv, r) for n, *r in CONVS] +
            [(n, make_convt, r) for n, *r in CONVTS] +
            [(n, make_dense, r) for n, *r in DENSES])
    for name, make, rest in jobs:
        if a.only and a.only != name:
            continue
        fn, flops = make(*rest)
        report(name, fn, flops, a.iters, arms)
        del fn
        torch.cuda.empty_cache()
