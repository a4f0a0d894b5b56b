"""Dropout kernel bandwidth and trainer cost (profiles/dropout_ab.md).

Part 1 (kernels): achieved GB/s of dropout_fwd / dropout_bwd and of
gaussian_noise_fwd on the DCGAN-64 d_conv_0 output (16384x32x32x64 bf16),
next to act_fwd / act_bwd on the same tensor — the existing memory-bound
yardstick with the same traffic apart from the mask bytes. Device-event
timing, warm-up, interleaved rounds in one process, median/min/max.

Part 2 (trainer, --trainer): img/s of the captured fast trainer on
DCGAN-64 with model.dis_dropout=0.3 against 0.0, alternating.

    python tools/ab_dropout.py [--batch 16384] [--rounds 7] [--trainer]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gan_deeplearning4j_amd.ops.backend import hip_ext  # noqa: E402


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
    ext = hip_ext()
    n = batch * 32 * 32 * 64
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, device="cuda", dtype=torch.bfloat16, generator=g)
    dy = torch.randn(n, device="cuda", dtype=torch.bfloat16, generator=g)
    state = torch.tensor([666, 0], dtype=torch.int64, device="cuda")
    y, mask = ext.dropout_fwd(x, state, 0.7)
    ya = ext.act_fwd(x, 3, 0.2)
    nbytes = 2 * n
    variants = {
        # name: (callable, bytes moved)
        "act_fwd (lrelu)": (lambda: ext.act_fwd(x, 3, 0.2), 2 * nbytes),
        "dropout_fwd": (lambda: ext.dropout_fwd(x, state, 0.7),
                        2 * nbytes + n // 8),
        "act_bwd (lrelu)": (lambda: ext.act_bwd(dy, ya, 3, 0.2), 3 * nbytes),
        "dropout_bwd": (lambda: ext.dropout_bwd(dy, mask, 0.7),
                        2 * nbytes + n // 8),
        "gaussian_noise_fwd": (
            lambda: ext.gaussian_noise_fwd(x, state, 0.1), 2 * nbytes),
    }
    for fn, _ in variants.values():          # warm-up every shape/kernel
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                  # interleaved rounds
        for name, (fn, _) in variants.items():
            times[name].append(time_ms(fn, iters))
    print(f"tensor {batch}x32x32x64 bf16 = {nbytes / 2**30:.2f} GiB, "
          f"{rounds} rounds x {iters} launches, device events")
    print("| kernel | median ms | min | max | bytes moved | GB/s (median) |")
    print("|---|---|---|---|---|---|")
    med = {}
    for name, (_, moved) in variants.items():
        t = times[name]
        med[name] = statistics.median(t)
        print(f"| {name} | {med[name]:.3f} | {min(t):.3f} | {max(t):.3f} | "
              f"{moved / 1e9:.2f} GB | {moved / med[name] / 1e6:.0f} |")
    print(f"dropout_fwd / act_fwd time ratio: "
          f"{med['dropout_fwd'] / med['act_fwd (lrelu)']:.3f}")
    print(f"dropout_bwd / act_bwd time ratio: "
          f"{med['dropout_bwd'] / med['act_bwd (lrelu)']:.3f}")


def trainer(batch, rounds, steps):
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan
    from gan_deeplearning4j_amd.train import GanTrainer

    g = torch.Generator().manual_seed(1234)
    real = (torch.rand(batch, 3, 64, 64, generator=g) * 2 - 1).to(
        "cuda", torch.bfloat16).contiguous(memory_format=torch.channels_last)
    trainers = {}
    for p in (0.0, 0.3):
        cfg = preset("dcgan64")
        cfg.model.dis_dropout = p
        gen, dis = build_dcgan(cfg)
        tr = GanTrainer(gen, dis, cfg, device=torch.device("cuda"),
                        dtype=torch.bfloat16, capture=True)
        for _ in range(4):                   # capture + warm-up
            tr.step(real)
        torch.cuda.synchronize()
        assert not tr._graph_failed
        trainers[p] = tr
    rates = {p: [] for p in trainers}
    for _ in range(rounds):
        for p, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(real)
            torch.cuda.synchronize()
            rates[p].append(batch * steps / (time.perf_counter() - t0))
    print(f"DCGAN-64 captured trainer, batch {batch}, {rounds} rounds x "
          f"{steps} steps, alternating")
    print("| model.dis_dropout | median img/s | min | max |")
    print("|---|---|---|---|")
    for p, r in rates.items():
        print(f"| {p} | {statistics.median(r):.0f} | {min(r):.0f} | "
              f"{max(r):.0f} |")
    print(f"ratio 0.3 / 0.0: "
          f"{statistics.median(rates[0.3]) / statistics.median(rates[0.0]):.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--trainer", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_dropout.py needs a GPU")
    if args.trainer:
        trainer(args.batch, args.rounds, args.steps)
    else:
        kernels(args.batch, args.rounds, args.iters)
