"""Flagship benchmark: DCGAN 64x64 bf16 images/sec (whole node).

Driver contract:
    python bench.py --gpus N --steps K --warmup W
launched for N>1 as one rank per GPU via torch.distributed.run; reads
RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from env. One "step" = one full
alternating GAN iteration (D update on real+fake and G update) on the
per-rank batch; value = whole-job real images consumed per second
(global_batch * steps / elapsed), weak scaling.

Prints exactly one JSON line from rank 0.

A plain run sets up, warms up, times the K steps and prints the line.
    --dump-outputs DIR  additionally writes what the last timed step
                        produced (losses, updated G/D weights and BN
                        statistics) as DIR/<name>.npy. Inputs, weights and
                        noise are seeded, and the trainer is rewound to its
                        seeded start state (clock stopped) before that last
                        step, so the dump is one step of the timed path from
                        a known state: equal from run to run up to the
                        rounding of the GPU's atomic reductions, whatever K
                        and W are (see StartState).
    --full              gate for secondary measurements (baselines, other
                        precisions, per-kernel figures). The benchmark has
                        none of its own today, so it changes nothing yet;
                        anything of that kind added later goes behind it.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gan_deeplearning4j_amd.config import preset  # noqa: E402
from gan_deeplearning4j_amd.models import build_dcgan, build_mlp_gan  # noqa: E402
from gan_deeplearning4j_amd.parallel.launch import init_distributed  # noqa: E402
from gan_deeplearning4j_amd.train import GanTrainer  # noqa: E402


DUMP_CAP_BYTES = 64 * 1000 * 1000


def dump_outputs(out_dir: str, step_out: dict, tr: GanTrainer) -> None:
    """Write what the last timed step produced as <out_dir>/<name>.npy.

    A caller of `GanTrainer.step` receives the two losses and holds the
    trainer whose G/D weights and BatchNorm statistics the step updated,
    so those are the arrays written (float32). If they exceed the 64 MB
    cap, every array is reduced to a fixed seeded sample of its elements
    (same indices in every run, so two builds stay comparable).
    """
    import numpy as np

    arrays = {
        "loss_d": step_out["loss_d"].detach().float().reshape(1).cpu().numpy(),
        "loss_g": step_out["loss_g"].detach().float().reshape(1).cpu().numpy(),
    }
    for prefix, graph in (("gen", tr.gen), ("dis", tr.dis)):
        tensors = list(graph.named_parameters()) + list(graph.named_buffers())
        for name, t in tensors:
            if not t.is_floating_point():
                continue
            arrays[f"{prefix}_{name.replace('.', '_')}"] = (
                t.detach().float().cpu().contiguous().numpy())
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_CAP_BYTES:
        keep = 0.95 * DUMP_CAP_BYTES / total  # headroom for .npy headers
        rng = np.random.default_rng(20240607)
        for name in sorted(arrays):
            flat = arrays[name].reshape(-1)
            n = max(1, int(flat.size * keep))
            idx = np.sort(rng.choice(flat.size, size=n, replace=False))
            arrays[name] = flat[idx]
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"),
                np.ascontiguousarray(a, dtype=np.float32))


class StartState:
    """The trainer's seeded start state, restorable in place.

    Several GPU reductions accumulate with float atomics, so a step's
    gradients differ between runs in their last bits, and the normalized
    Adam/RMSProp updates turn that into full-size differences within a few
    steps. What a run leaves after many steps is therefore not comparable
    between runs or builds; one step from the seeded start is, to rounding.
    `--dump-outputs` rewinds to this state before the last timed step.

    Taken before the first step; `restore()` copies weights and BatchNorm
    statistics back, resets the updater to its freshly-initialized state
    (zero moments, step count 0, fp32 masters re-derived from the weights,
    exactly as the lazy init does) and rewinds the noise generators. All
    of it in place, so a captured step graph stays valid.
    """

    def __init__(self, tr: GanTrainer):
        self.tr = tr
        self.tensors = [t for g in (tr.gen, tr.dis)
                        for t in list(g.parameters()) + list(g.buffers())]
        self.saved = [t.detach().clone() for t in self.tensors]
        self.host_rng = tr._g.get_state()
        self.dev_rng = (torch.cuda.get_rng_state(tr.device)
                        if tr.device.type == "cuda" else None)

    @torch.no_grad()
    def restore(self) -> None:
        tr = self.tr
        for t, s in zip(self.tensors, self.saved):
            t.copy_(s)
        for g in (tr.gen, tr.dis):
            u = g.updater
            u.t = 0
            if u._t_dev is not None:
                u._t_dev.zero_()
            for s in u.slots:
                if s.master is not None:
                    s.master.copy_(s.param.detach().float())
                for moment in (s.m, s.v):
                    if moment is not None:
                        moment.zero_()
        tr.it = 0
        tr._g.set_state(self.host_rng)
        if self.dev_rng is not None:
            torch.cuda.set_rng_state(self.dev_rng, tr.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0,
                    help="per-GPU batch (0 = arch default)")
    ap.add_argument("--arch", type=str, default="dcgan64")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write the last step's "
                         "losses and the updated G/D state as DIR/<name>.npy "
                         "(that step runs from the seeded start state)")
    ap.add_argument("--full", action="store_true",
                    help="also run the benchmark's secondary measurements "
                         "(none today: a plain run already does only what "
                         "the headline figure needs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    rank, world, local_rank, device = init_distributed()
    use_gpu = device.type == "cuda"

    cfg = preset(args.arch) if args.arch != "mlp" else preset("mlp_tabular_cpu")
    per_gpu_batch = args.batch
    if per_gpu_batch == 0:
        # sized for 288 GB HBM3E: bigger batches amortize fixed kernel
        # costs (measured +13% at 4096 vs 1024 on dcgan64)
        per_gpu_batch = {"dcgan28": 8192, "dcgan64": 16384,
                         "dcgan128": 2048}.get(args.arch, 512)
        if not use_gpu:
            per_gpu_batch = 16
    cfg.train.use_gpu = use_gpu

    if args.arch == "mlp":
        gen, dis = build_mlp_gan(cfg)
    else:
        gen, dis = build_dcgan(cfg)
    dtype = torch.bfloat16 if use_gpu else torch.float32
    # hipGraph capture only at world_size==1: capturing RCCL collectives is
    # not validated on this stack (a capture hang would be worse than the
    # ~0 measured gain; eager == captured throughput at these batch sizes)
    capture = (use_gpu and world == 1
               and os.environ.get("GDLJ_NO_CAPTURE") != "1")
    tr = GanTrainer(gen, dis, cfg, device=device, dtype=dtype,
                    capture=capture)

    m = cfg.model
    # synthetic pixel-lattice-shaped data, random-init weights (no-network
    # environment; BASELINE.json data contract)
    g = torch.Generator().manual_seed(1234 + rank)
    real = (torch.rand(per_gpu_batch, m.image_channels, m.image_height,
                       m.image_width, generator=g) * 2 - 1).to(device, dtype)
    if use_gpu and args.arch != "mlp":
        # channels-last once up front: the NHWC conv path then consumes
        # the batch copy-free every step (a user pipeline would store
        # images channels-last for the same reason)
        real = real.contiguous(memory_format=torch.channels_last)
    if args.arch == "mlp":
        real = torch.rand(per_gpu_batch, cfg.data.num_features,
                          generator=g).to(device, dtype)

    def barrier_sync():
        if torch.distributed.is_initialized():
            torch.distributed.barrier()
        if use_gpu:
            torch.cuda.synchronize(device)

    def timed(n):
        out = None
        barrier_sync()
        t0 = time.perf_counter()
        for _ in range(n):
            out = tr.step(real)
        barrier_sync()
        return time.perf_counter() - t0, out

    start = StartState(tr) if args.dump_outputs else None

    for _ in range(args.warmup):
        tr.step(real)

    if start is None:
        elapsed, out = timed(args.steps)
    else:
        if tr.it == 0:
            # --warmup 0: the first step also draws the soft labels and,
            # on the GPU, captures the step graph (which runs eager steps
            # of its own); both have to precede the rewind (untimed)
            tr.step(real)
        # the clock stops for the rewind: K steps are timed either way
        head, _ = timed(args.steps - 1)
        start.restore()
        tail, out = timed(1)
        elapsed = head + tail
        if rank == 0:
            dump_outputs(args.dump_outputs, out, tr)

    # MAX over ranks
    if torch.distributed.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_gpu else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world  # == --gpus under the driver contract (CPU dry-runs incl.)
    global_batch = per_gpu_batch * world
    images_per_sec = global_batch * args.steps / elapsed
    size = m.image_height
    if use_gpu and cfg.model.dtype == "fp8":
        # fwd convs (incl. convT) run e4m3 MFMA; backward defaults to
        # bf16 — fp8 dgrad exists (GDLJ_FP8_BWD=1) but measured 4-6%
        # slower at these K-thin memory-bound dgrad shapes
        # (profiles/fp8_bwd_ab.md), and wgrad has no fp8 transpose-read
        # path. The label states exactly what is measured.
        dt = ("fp8-fwd+dgrad/bf16-wgrad"
              if os.environ.get("GDLJ_FP8_BWD") == "1"
              else "fp8-fwd/bf16-bwd")
    else:
        dt = "bf16" if use_gpu else "fp32"
    metric = (f"images/sec (whole node) DCGAN {size}x{size} "
              f"{'bf16' if cfg.model.dtype != 'fp8' else 'fp8'}"
              if args.arch != "mlp" else "samples/sec MLP GAN")
    if rank == 0:
        print(json.dumps({
            "metric": metric,
            "value": round(images_per_sec, 2),
            "unit": "images/s" if args.arch != "mlp" else "samples/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": dt,
            "data": "synthetic",
            "config": {
                "model": args.arch,
                "global_batch": global_batch,
                "image": [m.image_channels, m.image_height, m.image_width],
                "z_size": m.z_size,
                "parallelism": f"dp{world}",
            },
        }))


if __name__ == "__main__":
    main()
