"""Spectral-norm kernel bandwidth and trainer cost
(profiles/spectral_norm_ab.md).

Part 1 (kernels): forward (power iteration + W / sigma) and backward time
and achieved GB/s for each D weight matrix of DCGAN-64, next to act_fwd -
the existing memory-bound yardstick - on its usual large tensor
(batch x 32 x 32 x 64 bf16, as tools/ab_dropout.py) and on a tensor of the
largest matrix's byte count, which separates launch latency from
bandwidth. Device-event timing, warm-up, interleaved rounds in one process,
median/min/max.

Bytes moved, B = 2 M K: forward 4 B (column pass and row pass read W, the
scale pass reads W and writes W_sn; the fp32 partials are under 1% of
that), backward 4 B (the reduction reads G and W_sn, the apply pass reads G
and writes dW).

Part 2 (trainer, --trainer): img/s of the captured fast trainer on DCGAN-64
with the hinge loss, three arms alternating: the default D, D with its
BatchNorm simply removed (isolates the recipe change), and
model.dis_spectral_norm (the third against the second is the feature's
per-step cost).

    python tools/ab_spectral_norm.py [--batch 16384] [--rounds 7] [--trainer]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gan_deeplearning4j_amd.ops.backend import hip_ext, spectral_ext  # noqa: E402

# (name, M, K) of DCGAN-64's D at base_width 64
D_MATRICES = [
    ("d_conv_0", 64, 3 * 16),
    ("d_conv_1", 128, 64 * 16),
    ("d_conv_2", 256, 128 * 16),
    ("d_conv_3", 512, 256 * 16),
    ("d_dense_feat", 1024, 512 * 16),
    ("d_out", 1, 1024),
]


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def kernels(batch, rounds, iters):
    ext, sx = hip_ext(), spectral_ext()
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    variants = {}
    big = rnd(batch * 32 * 32 * 64).to(torch.bfloat16)
    variants["act_fwd (lrelu), yardstick tensor"] = (
        lambda: ext.act_fwd(big, 3, 0.2), 4 * big.numel())
    m, k = D_MATRICES[4][1:]
    small = rnd(m * k).to(torch.bfloat16)
    variants[f"act_fwd (lrelu), {m}x{k}"] = (
        lambda: ext.act_fwd(small, 3, 0.2), 4 * small.numel())
    for name, m, k in D_MATRICES:
        w = rnd(m, k).to(torch.bfloat16)
        gr = (0.5 * w.float() + rnd(m, k)).to(torch.bfloat16)
        u = torch.nn.functional.normalize(rnd(m), dim=0)
        v = torch.nn.functional.normalize(rnd(k), dim=0)
        w_sn, u_c, v_c, sig = sx.sn_forward(w, u, v)[:4]
        nbytes = 2 * m * k
        variants[f"sn_forward {name} {m}x{k}"] = (
            lambda w=w, u=u, v=v: sx.sn_forward(w, u, v), 4 * nbytes)
        variants[f"sn_backward {name} {m}x{k}"] = (
            lambda a=(gr, w_sn, u_c, v_c, sig): sx.sn_backward(*a),
            4 * nbytes)
    for fn, _ in variants.values():          # warm-up every shape/kernel
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(rounds):                  # interleaved rounds
        for name, (fn, _) in variants.items():
            times[name].append(time_ms(fn, iters))
    print(f"{rounds} rounds x {iters} launches, device events; forward = 5 "
          "kernels, backward = 2")
    print("| pass | median us | min | max | bytes moved | GB/s (median) | "
          "of yardstick |")
    print("|---|---|---|---|---|---|---|")
    rate = {}
    for name, (_, moved) in variants.items():
        t = times[name]
        med = statistics.median(t)
        rate[name] = moved / med / 1e6
        yard = rate["act_fwd (lrelu), yardstick tensor"]
        print(f"| {name} | {med * 1e3:.1f} | {min(t) * 1e3:.1f} | "
              f"{max(t) * 1e3:.1f} | {moved / 1e6:.2f} MB | "
              f"{rate[name]:.0f} | {rate[name] / yard:.3f} |")
    fwd = sum(statistics.median(times[n]) for n in times if "sn_forward" in n)
    bwd = sum(statistics.median(times[n]) for n in times
              if "sn_backward" in n)
    print(f"all six matrices: forward {fwd * 1e3:.1f} us, backward "
          f"{bwd * 1e3:.1f} us; one trainer step runs 3 forwards and 2 "
          f"backwards of D: {(3 * fwd + 2 * bwd) * 1e3:.1f} us of kernels")


def trainer(batch, rounds, steps):
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan
    from gan_deeplearning4j_amd.train import GanTrainer

    g = torch.Generator().manual_seed(1234)
    real = (torch.rand(batch, 3, 64, 64, generator=g) * 2 - 1).to(
        "cuda", torch.bfloat16).contiguous(memory_format=torch.channels_last)
    trainers = {}
    for arm in ("default D", "D without BatchNorm", "dis_spectral_norm"):
        cfg = preset("dcgan64")
        cfg.train.loss_type = "hinge"
        cfg.model.dis_spectral_norm = arm != "default D"
        gen, dis = build_dcgan(cfg)
        if arm == "D without BatchNorm":
            # the spectral-norm vertex list with the normalization off
            for name in dis.layer_names():
                dis.layers[name].spectral_norm = False
        tr = GanTrainer(gen, dis, cfg, device=torch.device("cuda"),
                        dtype=torch.bfloat16, capture=True)
        for _ in range(4):                   # capture + warm-up
            tr.step(real)
        torch.cuda.synchronize()
        assert not tr._graph_failed
        trainers[arm] = tr
    rates = {a: [] for a in trainers}
    for _ in range(rounds):
        for a, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(real)
            torch.cuda.synchronize()
            rates[a].append(batch * steps / (time.perf_counter() - t0))
    print(f"DCGAN-64 captured trainer, hinge loss, batch {batch}, {rounds} "
          f"rounds x {steps} steps, alternating")
    print("| arm | median img/s | min | max | ms / step (median) |")
    print("|---|---|---|---|---|")
    ms = {}
    for a, r in rates.items():
        ms[a] = batch / statistics.median(r) * 1e3
        print(f"| {a} | {statistics.median(r):.0f} | {min(r):.0f} | "
              f"{max(r):.0f} | {ms[a]:.3f} |")
    print(f"recipe change (no BatchNorm - default): "
          f"{ms['D without BatchNorm'] - ms['default D']:+.3f} ms / step")
    print(f"feature cost (dis_spectral_norm - no BatchNorm): "
          f"{ms['dis_spectral_norm'] - ms['D without BatchNorm']:+.3f} "
          f"ms / step")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_spectral_norm.py needs a GPU")
    if args.trainer:
        trainer(args.batch, args.rounds, args.steps)
    else:
        kernels(args.batch, args.rounds, args.iters)
