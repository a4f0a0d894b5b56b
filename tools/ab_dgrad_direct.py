"""Per-shape A/B of the strided dgrad / convT forward kernels.

Four arms: "dcol" (GDLJ_DGRAD_DIRECT=0), "direct" (the one-shot direct
kernel, GDLJ_DGRAD_PERSIST=0), "persist" (the two-blocks-per-CU persistent
kernel, GDLJ_DGRAD_WIDE=0) and "wide" (the one-block-per-CU wide kernel,
the default where eligible).  The gates are re-read per call, so all arms
run in one process on identical data; the checksum of the result is
compared across arms.  The persist arm is timed three times: the spread
of those is the noise figure a wide time has to beat.  The dgrad rows
time the full backward of a bias-free identity conv (dgrad + wgrad; wgrad
identical in all arms), the convT rows time the forward alone.  Next to
each row: the bytes the persist and wide kernels stage into LDS per call
(plan arithmetic), for the DMA-rate column of the write-up.
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
    ("persist", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "1",
                 "GDLJ_DGRAD_WIDE": "0"}),
    ("persist", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "1",
                 "GDLJ_DGRAD_WIDE": "0"}),
    ("persist", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "1",
                 "GDLJ_DGRAD_WIDE": "0"}),
    ("wide", {"GDLJ_DGRAD_DIRECT": "1", "GDLJ_DGRAD_PERSIST": "1",
              "GDLJ_DGRAD_WIDE": "1"}),
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


def bench_convt(nb, cin, hi, cout, r, stride, pad, act="identity",
                with_bias=False):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(nb, cin, hi, hi, generator=g) * 0.5).to(
        "cuda", torch.bfloat16)
    w = (torch.randn(cin, cout, r, r, generator=g) * 0.1).to(
        "cuda", torch.bfloat16)
    b = None
    if with_bias:
        b = (torch.randn(cout, generator=g) * 0.1).to("cuda", torch.bfloat16)
    out = []

    def step():
        out[:] = [gpu_ops.conv_transpose2d(x, w, b, stride, pad, act,
                                           emit_stats=True)]
        gpu_ops.take_bn_stats(out[0])

    with torch.no_grad():
        dt = timed(step)
    return dt, out[0].float().abs().sum().item()


def axis_window(pad, r, q):
    t0 = (q + pad) & 1
    nt = (r - t0 + 1) >> 1
    bo = (q + pad - t0) >> 1
    return bo - (nt - 1), bo


def axis_extent(length, pad, r, qsplit=False):
    (l0, h0), (l1, h1) = axis_window(pad, r, 0), axis_window(pad, r, 1)
    if qsplit:
        return length + max(h0 - l0, h1 - l1)
    return length + max(h0, h1) - min(l0, l1)


def staged_bytes(nb, h, c8, ko8, r, pad):
    """(persist, wide) bytes staged into LDS per call: regions + W slices,
    mirroring plan_persistent / plan_wide (None where not taken)."""
    hc = wc = h // 2
    nj = ko8 // 128
    nct = c8 // 64
    slices = sum(((r - ((qh + pad) & 1) + 1) >> 1) *
                 ((r - ((qw + pad) & 1) + 1) >> 1)
                 for qh in (0, 1) for qw in (0, 1)) * nj * nct
    persist = None
    for bm in (128, 64):
        if wc > bm or bm % wc or (hc * wc) % bm:
            continue
        for qsplit in (0, 1):
            rgn = (axis_extent(bm // wc, pad, r, bool(qsplit)) *
                   axis_extent(wc, pad, r) * ko8 * 2)
            if rgn + 32768 > 80 * 1024:
                continue
            tiles = nb * hc * wc // bm
            persist = tiles * (rgn * (2 if qsplit else 1) + slices * 16384)
            break
        if persist is not None:
            break
    wide = None
    if hc * wc == 64:
        imgs = 2
        rgn = imgs * axis_extent(hc, pad, r) * axis_extent(wc, pad, r) * ko8 * 2
        if rgn + 3 * 16384 <= 160 * 1024:
            tiles = (nb + imgs - 1) // imgs
            wide = tiles * (rgn + slices * 16384)
    return persist, wide


def report(name, fn, geom=None):
    res = [(arm, *with_env(env, fn)) for arm, env in ARMS]
    c0 = res[0][2]
    ok = all(abs(c - c0) < 1e-3 * abs(c0) for _, _, c in res)
    match = "match" if ok else "MISMATCH " + " vs ".join(
        f"{c}" for _, _, c in res)
    times = " | ".join(f"{arm} {t:.3f} ms" for arm, t, _ in res)
    pt = [t for arm, t, _ in res if arm == "persist"]
    wt = [t for arm, t, _ in res if arm == "wide"][0]
    verdict = "WIDE WINS" if min(pt) - wt > max(pt) - min(pt) else "no win"
    print(f"{name}: {times} (persist spread {max(pt) - min(pt):.3f} ms, "
          f"wide - fastest persist {wt - min(pt):+.3f} ms: {verdict}) "
          f"[{match}]", flush=True)
    if geom is not None:
        ps, ws = staged_bytes(*geom)
        print(f"    staged per call: persist "
              f"{'-' if ps is None else '%.2f GB' % (ps / 1e9)}, wide "
              f"{'-' if ws is None else '%.2f GB' % (ws / 1e9)}", flush=True)


# ---------------------------------------------------------------------------
# The 4x4 class grid (conv4 dgrad / convT1 forward of DCGAN-64, conv5 dgrad /
# convT1 forward of DCGAN-128): no direct kernel takes it.  Two modes:
#   step0     arm A = gemm_tn + col2im(_stats), arm B = conv_parity_implicit
#             on class packs built once, both through the raw extension
#             entry points (the go / no-go measurement, runs on any build);
#   classgemm arm A = GDLJ_DGRAD_CLASSGEMM=0 (dcol + col2im), arm B = default
#             (the class GEMMs behind the direct bindings, dcol's roundings),
#             arm C = GDLJ_DGRAD_CLASSGEMM_FP32=1 (one fp32 accumulation on
#             the 256-wide tile), through gpu_ops.  The convT rows ask for BN
#             statistics, which only arm C serves on this route.
# Arm A is timed three times; B wins if it beats the fastest A by more than
# A's spread.
CLASS4_SHAPES = [
    # name, Nb, H (= W, full-res side), C8, Ko8, R, pad   [dgrad naming]
    ("dcgan64_conv4_b16384", 16384, 8, 256, 512, 4, 1),
    ("dcgan128_conv5_b2048", 2048, 8, 512, 512, 4, 1),
]


def class4_data(nb, h, c8, ko8, r, pad):
    g = torch.Generator().manual_seed(6)
    hc = (h + 2 * pad - r) // 2 + 1
    dy = (torch.randn(nb, hc, hc, ko8, generator=g) * 0.5).to(
        "cuda", torch.bfloat16)
    wc = (torch.randn(c8, r, r, ko8, generator=g) * 0.05).to(
        "cuda", torch.bfloat16)                       # [c][R][S][ko]
    wt = wc.permute(1, 2, 0, 3).reshape(r * r * c8, ko8).contiguous()
    bias = (torch.randn(c8, generator=g) * 0.1).to("cuda")
    return hc, dy, wc, wt, bias


def step0_row(name, nb, h, c8, ko8, r, pad, convt):
    ext = gpu_ops.hip_ext()
    hc, dy, wc, wt, bias = class4_data(nb, h, c8, ko8, r, pad)
    zp = gpu_ops._zero_page(dy.device)
    packs = gpu_ops._parity_class_packs(wc, 2, pad)
    dy2d = dy.view(-1, ko8)
    gamma, beta = torch.ones_like(bias), torch.zeros_like(bias)
    none = torch.empty(0, device="cuda")
    out = []

    def arm_a():
        dcol = ext.gemm_tn(dy2d, wt, None, 0, 0.0, False)
        if convt:
            y, ssum, ssq = ext.col2im_stats(dcol, nb, h, h, c8, hc, hc, r, r,
                                            2, pad, r * r * c8, bias, 3, 0.2)
            ext.bn_fwd_train_pre(y, ssum, ssq, gamma, beta, none, none, 0.1,
                                 1e-5)
        else:
            y = ext.col2im(dcol, nb, h, h, c8, hc, hc, r, r, 2, pad,
                           r * r * c8, None, 0, 0.0)
        out[:] = [y]

    def arm_b():
        y = ext.conv_parity_implicit(dy, packs, bias if convt else None, zp,
                                     nb, hc, hc, ko8, h, h, c8, r, r, 2, pad,
                                     3 if convt else 0, 0.2)
        if convt:  # separate statistics pass, as the binding would run it
            ext.bn_fwd_train(y.view(nb, h, h, c8), gamma, beta, none, none,
                             0.1, 1e-5)
        out[:] = [y]

    res = []
    with torch.no_grad():
        for arm, fn in (("dcol", arm_a), ("dcol", arm_a), ("dcol", arm_a),
                        ("parity", arm_b)):
            res.append((arm, timed(fn), out[0].float().abs().sum().item()))
    print_verdict(name + ("_convT" if convt else "_dgrad"), res, "dcol",
                  "parity")


def classgemm_row(name, nb, h, c8, ko8, r, pad, convt):
    hc = (h + 2 * pad - r) // 2 + 1
    off = {"GDLJ_DGRAD_CLASSGEMM": "0"}
    on = {"GDLJ_DGRAD_CLASSGEMM": "1"}
    if convt:
        fn = lambda: bench_convt(nb, ko8, hc, c8, r, 2, pad,  # noqa: E731
                                 "lrelu", True)
    else:
        fn = lambda: bench_one(nb, c8, h, ko8, r, 2, pad)  # noqa: E731
    fp32 = dict(on, GDLJ_DGRAD_CLASSGEMM_FP32="1")
    res = [(arm, *with_env(env, fn)) for arm, env in (
        ("dcol", off), ("dcol", off), ("dcol", off), ("classgemm", on),
        ("classgemm_fp32", fp32))]
    for arm in ("classgemm", "classgemm_fp32"):
        print_verdict(name + ("_convT" if convt else "_dgrad+wgrad"),
                      [x for x in res if x[0] in ("dcol", arm)], "dcol", arm)


def print_verdict(name, res, a_name, b_name):
    at = [t for arm, t, _ in res if arm == a_name]
    bt = [t for arm, t, _ in res if arm == b_name][0]
    c0 = res[0][2]
    ok = all(abs(c - c0) < 1e-3 * abs(c0) for _, _, c in res)
    match = "match" if ok else "MISMATCH " + " vs ".join(
        f"{c}" for _, _, c in res)
    win = "WINS" if min(at) - bt > max(at) - min(at) else "no win"
    print(f"{name}: {a_name} " + " / ".join(f"{t:.3f}" for t in at) +
          f" ms (spread {max(at) - min(at):.3f}) | {b_name} {bt:.3f} ms | "
          f"{b_name} - fastest {a_name} {bt - min(at):+.3f} ms: "
          f"{b_name.upper()} {win} [{match}]", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode in ("step0", "classgemm"):
        row = step0_row if mode == "step0" else classgemm_row
        for name, *geom in CLASS4_SHAPES:
            row(name, *geom, convt=False)
            row(name, *geom, convt=True)
        if mode == "classgemm":  # unchanged controls
            report("conv2_r4_b16384 (control)",
                   lambda: bench_one(*SHAPES[0][1:]))
            report("conv3_r4_b16384 (control)",
                   lambda: bench_one(*SHAPES[1][1:]))
        sys.exit(0)
    # geom = (Nb, H, C8, Ko8, R, pad) in the kernel's dgrad naming
    for name, *args in SHAPES:
        nb, cin, h, cout, r, _, pad = args
        report(name, lambda: bench_one(*args), (nb, h, cin, cout, r, pad))
    # the bench's real conv2 geometry (R=4 pad=1) with pact fusion
    for name, args in [
        ("conv2_r4_pact_bias", (16384, 64, 32, 128, 4, 2, 1, True)),
        ("conv2_r4_pact_nobias", (16384, 64, 32, 128, 4, 2, 1, False)),
    ]:
        nb, cin, h, cout, r, _, pad = args[:7]
        report(name, lambda: bench_pact(*args[:7], want_bias=args[7]),
               (nb, h, cin, cout, r, pad))
    for name, *args in CONVT_SHAPES:
        nb, cin, hi, cout, r, _, pad = args
        report(name, lambda: bench_convt(*args),
               (nb, 2 * hi, cout, cin, r, pad))
