"""Per-shape A/B: dcol+col2im vs conv_dgrad_direct vs conv_dgrad_direct_p.

Three arms: "dcol" (GDLJ_DGRAD_DIRECT=0), "direct" (the one-shot direct
kernel, GDLJ_DGRAD_PERSIST=0) and "persist" (the persistent class-fused
kernel, the default).  Both gates are re-read per call, so all arms run
in one process on identical data; the checksum of the result is compared
across arms.  The dgrad rows time the full backward of a bias-free
identity conv (dgrad + wgrad; wgrad identical in all arms), the convT
rows time the forward alone.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gan_deeplearning4j_amd.ops import gpu_ops  # noqa: E402

ARMS = [
    ("dcol", {"GDLJ_DGRAD_DIRECT": "0"}),
    ("direct", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "0"}),
    ("persist", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "1"}),
]

SHAPES = [
    # name, Nb, Cin, H, Cout, R, stride, pad
    ("conv2_r4_b16384", 16384, 64, 32, 128, 4, 2, 1),
    ("conv3_r4_b16384", 16384, 128, 16, 256, 4, 2, 1),
    ("conv2_r5_b16384", 16384, 64, 32, 128, 5, 2, 2),
    ("conv3_r5_b16384", 16384, 128, 16, 256, 5, 2, 2),
]

CONVT_SHAPES = [
    # name, Nb, Cin, Hi, Cout, R, stride, pad
    ("convT2_r4_b16384", 16384, 256, 8, 128, 4, 2, 1),
    ("convT3_r4_b16384", 16384, 128, 16, 64, 4, 2, 1),
]


def timed(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


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


def bench_one(nb, cin, h, cout, r, stride, pad):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(nb, cin, h, h, generator=g) * 0.5).to(
        "cuda", torch.bfloat16).requires_grad_(True)
    w = (torch.randn(cout, cin, r, r, generator=g) * 0.2).to(
        "cuda", torch.bfloat16).requires_grad_(True)
    y = gpu_ops.conv2d(x, w, None, stride, pad, "identity")
    gout = torch.ones_like(y)

    def step():
        x.grad = None
        y.backward(gout, retain_graph=True)

    dt = timed(step)
    return dt, x.grad.float().abs().sum().item()


def bench_pact(nb, cin, h, cout, r, stride, pad, want_bias=True):
    # producer-act-fused variant (the bench's conv2 path): dgrad folds
    # lrelu' + bias partials for the producer
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(nb, cin, h, h, generator=g) * 0.5).to(
        "cuda", torch.bfloat16)
    x = torch.nn.functional.leaky_relu(x, 0.2).requires_grad_(True)
    w = (torch.randn(cout, cin, r, r, generator=g) * 0.2).to(
        "cuda", torch.bfloat16)
    y = gpu_ops.conv2d(x, w, None, stride, pad, "identity",
                       prev_act=(3, 0.2, want_bias))
    gout = torch.ones_like(y)

    def step():
        x.grad = None
        y.backward(gout, retain_graph=True)

    dt = timed(step)
    return dt, x.grad.float().abs().sum().item()


def bench_convt(nb, cin, hi, cout, r, stride, pad):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(nb, cin, hi, hi, generator=g) * 0.5).to(
        "cuda", torch.bfloat16)
    w = (torch.randn(cin, cout, r, r, generator=g) * 0.1).to(
        "cuda", torch.bfloat16)
    out = []

    def step():
        out[:] = [gpu_ops.conv_transpose2d(x, w, None, stride, pad,
                                           "identity", emit_stats=True)]
        gpu_ops.take_bn_stats(out[0])

    with torch.no_grad():
        dt = timed(step)
    return dt, out[0].float().abs().sum().item()


def report(name, fn):
    res = [(arm, *with_env(env, fn)) for arm, env in ARMS]
    c0 = res[0][2]
    ok = all(abs(c - c0) < 1e-3 * abs(c0) for _, _, c in res)
    match = "match" if ok else "MISMATCH " + " vs ".join(
        f"{c}" for _, _, c in res)
    times = " | ".join(f"{arm} {t:.3f} ms" for arm, t, _ in res)
    print(f"{name}: {times} (persist/direct "
          f"{res[2][1] / res[1][1]:.2f}x time) [{match}]", flush=True)


if __name__ == "__main__":
    for name, *args in SHAPES:
        report(name, lambda: bench_one(*args))
    # the bench's real conv2 geometry (R=4 pad=1) with pact fusion
    for name, args in [
        ("conv2_r4_pact_bias", (16384, 64, 32, 128, 4, 2, 1, True)),
        ("conv2_r4_pact_nobias", (16384, 64, 32, 128, 4, 2, 1, False)),
    ]:
        report(name, lambda: bench_pact(*args[:7], want_bias=args[7]))
    for name, *args in CONVT_SHAPES:
        report(name, lambda: bench_convt(*args))
