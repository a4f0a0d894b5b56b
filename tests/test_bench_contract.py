"""Driver-contract tests for bench.py.

Runs the EXACT launch shapes the driver uses: single-process, and
torchrun --nnodes=1 --nproc-per-node 2 with gloo on CPU (world_size>1
rendezvous on 127.0.0.1).
"""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


def _check_json_line(out: str, n_gpus_expected: int):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, f"no JSON line in output:\n{out[-2000:]}"
    d = json.loads(lines[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, f"missing {key}"
    assert d["value"] > 0
    assert d["n_gpus"] == n_gpus_expected
    assert d["data"] == "synthetic"
    assert d["scaling"] == "weak"
    assert "global_batch" in d["config"]
    return d


def test_bench_single_process_cpu():
    env = dict(os.environ)
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--batch", "8", "--arch", "dcgan28"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    d = _check_json_line(r.stdout, 1)
    assert d["config"]["parallelism"] == "dp1"


def _run_dump(out_dir, steps, warmup=1):
    # CPU on every machine: the fp32 CPU path is bit-reproducible
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
         "--warmup", str(warmup), "--batch", "8", "--arch", "dcgan28",
         "--full", "--dump-outputs", str(out_dir)],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=600,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    d = _check_json_line(r.stdout, 1)
    assert d["steps"] == steps
    assert d["dtype"] == "fp32"
    return {p.stem: np.load(p) for p in sorted(Path(out_dir).glob("*.npy"))}


def test_bench_dump_outputs_reproducible_cpu(tmp_path):
    """--dump-outputs writes the last timed step's losses and the updated
    G/D state as float32 .npy under the size cap; equal arguments give
    bit-equal dumps on CPU. The last step runs from the seeded start
    state, so the dump is one real update of it (weights moved) and does
    not depend on how many steps or warmup steps came before."""
    a = _run_dump(tmp_path / "a", 2)
    b = _run_dump(tmp_path / "b", 2)
    c = _run_dump(tmp_path / "c", 1, warmup=0)
    assert {"loss_d", "loss_g"} <= set(a)
    assert any(k.startswith("gen_") for k in a)
    assert any(k.startswith("dis_") for k in a)
    assert set(a) == set(b) == set(c)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for k in a:
        assert a[k].dtype == np.float32
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan

    gen, dis = build_dcgan(preset("dcgan28"))
    for prefix, graph in (("gen", gen), ("dis", dis)):
        init = {f"{prefix}_{n.replace('.', '_')}": p.detach().numpy()
                for n, p in graph.named_parameters()}
        assert set(init) <= set(a)
        assert any(not np.array_equal(init[k], a[k]) for k in init), prefix


@pytest.mark.gpu
def test_bench_rewound_step_reproducible_gpu():
    """On the GPU one step from bench.StartState gives the same losses,
    weights and BatchNorm statistics however many (noisy, atomically
    reduced) steps ran before the rewind, through the captured graph.

    Bound per array: max|a-b| <= 2*lr + 2**-7 * max|a|. bf16 weights and
    activations carry an 8-bit significand, so atomic-order noise shows as
    one or two spacings of 2**-8 relative; and the first Adam update of a
    weight is lr*sign(g), so a gradient within that noise of zero may flip
    it, which moves the weight by 2*lr at most.
    """
    import bench
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan
    from gan_deeplearning4j_amd.train import GanTrainer

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234)
    real = (torch.rand(64, 1, 28, 28, generator=g) * 2 - 1).to(
        dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def run(steps_before):
        cfg = preset("dcgan28")
        gen, dis = build_dcgan(cfg)
        tr = GanTrainer(gen, dis, cfg, device=dev, dtype=torch.bfloat16,
                        capture=True)
        start = bench.StartState(tr)
        for _ in range(steps_before):
            tr.step(real)
        start.restore()
        out = tr.step(real)
        torch.cuda.synchronize()
        assert tr._graph is not None, "step graph was not captured"
        arrays = {"loss_d": out["loss_d"].float().reshape(1).cpu(),
                  "loss_g": out["loss_g"].float().reshape(1).cpu()}
        for prefix, graph in (("gen", tr.gen), ("dis", tr.dis)):
            for n, t in (list(graph.named_parameters())
                         + list(graph.named_buffers())):
                if t.is_floating_point():
                    arrays[f"{prefix}_{n}"] = t.detach().float().cpu()
        lr = max(s.lr for gr in (tr.gen, tr.dis) for s in gr.updater.slots)
        return arrays, lr

    a, lr = run(1)
    b, _ = run(4)
    assert set(a) == set(b)
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        bound = 2 * lr + 2 ** -7 * float(a[k].abs().max())
        diff = float((a[k] - b[k]).abs().max())
        assert diff <= bound, (k, diff, bound)
    # the rewound step is a real update, not a no-op
    gen0, _ = build_dcgan(preset("dcgan28"))
    assert any(
        not torch.equal(p.detach().to(torch.bfloat16).float(),
                        a[f"gen_{n}"])
        for n, p in gen0.named_parameters())


def test_bench_dump_outputs_sampled_under_cap(tmp_path, monkeypatch):
    """Above the cap every array shrinks to the same seeded sample."""
    import bench

    class _Graph(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(
                torch.arange(4000, dtype=torch.float32).reshape(40, 100))
            self.register_buffer("steps", torch.zeros(1, dtype=torch.long))

    class _Trainer:
        gen, dis = _Graph(), _Graph()

    out = {"loss_d": torch.tensor(0.5), "loss_g": torch.tensor(1.5)}
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 8000)
    for name in ("x", "y"):
        bench.dump_outputs(str(tmp_path / name), out, _Trainer())
    x = {p.stem: np.load(p) for p in (tmp_path / "x").glob("*.npy")}
    y = {p.stem: np.load(p) for p in (tmp_path / "y").glob("*.npy")}
    assert set(x) == {"loss_d", "loss_g", "gen_w", "dis_w"}
    assert sum(v.nbytes for v in x.values()) <= 8000
    assert 0 < x["gen_w"].size < 4000
    # the sample is a subset of the source values, in order, and stable
    assert np.all(np.diff(x["gen_w"]) > 0)
    assert float(x["loss_g"][0]) == 1.5
    for k in x:
        np.testing.assert_array_equal(x[k], y[k])


def test_bench_torchrun_2proc_cpu():
    env = dict(os.environ)
    env["MASTER_ADDR"] = "127.0.0.1"
    # the CPU/gloo launch shape on every machine: with GPUs visible both
    # ranks would land on the first one and RCCL refuses a duplicate device
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29571", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--batch", "8", "--arch", "dcgan28"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=900,
    )
    assert r.returncode == 0, r.stderr[-3000:]
    d = _check_json_line(r.stdout, 2)
    # whole-job value over both ranks; weak scaling => global batch 16
    assert d["config"]["global_batch"] == 16
    assert d["config"]["parallelism"] == "dp2"
