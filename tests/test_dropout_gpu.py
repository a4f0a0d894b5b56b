"""GPU dropout / Gaussian-noise kernels against the CPU Philox oracle
(ops/philox_ref.py): bit-exact masks and outputs, storage-order layout,
saved-mask backward, hipGraph replay with an on-device counter, graph
chains around the fusion pass, and the captured trainer."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ext():
    from gan_deeplearning4j_amd.ops.backend import hip_ext

    return hip_ext()


def _state(seed=666, calls=0):
    from gan_deeplearning4j_amd.ops import functional as OF

    st = OF.new_rng_state(seed, device=DEV)
    st[1] = calls
    return st


def _ramp(n, mod=251):
    """Fixed non-zero bf16 ramp; (1..mod)/32 is exact in bf16."""
    v = (torch.arange(n, dtype=torch.float32) % mod + 1.0) / 32.0
    return v.to(DEV, torch.bfloat16)


def _scaled(t, keep):
    """bf16(float(t) * fp32(1/keep)) — the kernel's arithmetic."""
    s = torch.tensor(1.0 / keep, dtype=torch.float32)
    return (t.float().cpu() * s).to(torch.bfloat16)


def _sizes():
    # the launcher caps the grid at DROPOUT_GRID_CAP blocks of DROPOUT_BLOCK
    # lanes, one 8-element vector per lane per trip: one vector more than
    # cap x block makes the grid-stride loop take a second trip
    e = ext()
    cap_vectors = e.DROPOUT_GRID_CAP * e.DROPOUT_BLOCK
    return [7, 8, 8 * 64 + 3, 8 * 256 * 5 + 5, 8 * (cap_vectors + 1) + 3]


SIZE_IDS = ["tail_only", "one_vector", "wave_plus_tail", "several_blocks",
            "second_grid_trip"]


@pytest.fixture(scope="module", params=range(5), ids=SIZE_IDS)
def n(request):
    return _sizes()[request.param]


def test_launcher_constants():
    e = ext()
    assert e.DROPOUT_BLOCK % 64 == 0
    assert e.DROPOUT_GRID_CAP * e.DROPOUT_BLOCK * 8 < 2 ** 31


@pytest.mark.parametrize("keep", [0.5, 0.8])
def test_dropout_forward_bit_exact(n, keep):
    from gan_deeplearning4j_amd.ops import philox_ref

    st = _state(seed=(1 << 40) + 7, calls=3)
    seed, calls = st.tolist()                 # read BEFORE the call
    x = _ramp(n)
    y, mask = ext().dropout_fwd(x, st, keep)
    assert st.tolist() == [seed, calls]       # the kernel only reads it
    keep_ref = philox_ref.dropout_keep_mask(n, seed, calls, keep)
    assert mask.dtype == torch.uint8 and mask.numel() == (n + 7) // 8
    assert (mask.cpu().numpy() == philox_ref.pack_mask_bytes(keep_ref)).all()
    m = torch.from_numpy(keep_ref)
    expect = torch.where(m, _scaled(x, keep),
                         torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(y.cpu(), expect)


@pytest.mark.parametrize("keep", [0.5, 0.8])
def test_dropout_backward_uses_saved_mask(n, keep):
    from gan_deeplearning4j_amd.ops import gpu_ops

    st = _state(seed=11, calls=0)
    x = _ramp(n).requires_grad_(True)
    y = gpu_ops.dropout(x, st, keep)
    assert st.tolist() == [11, 1]
    # a second forward in between must not disturb the first one's backward
    y_other = gpu_ops.dropout(x.detach(), st, keep)
    assert st.tolist() == [11, 2]
    assert not torch.equal(y_other, y.detach()) or n < 64
    dy = _ramp(n, mod=127)
    y.backward(dy)
    kept = (y.detach() != 0).cpu()
    expect = torch.where(kept, _scaled(dy, keep),
                         torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(x.grad.cpu(), expect)


def test_dropout_channels_last_view():
    from gan_deeplearning4j_amd.ops import gpu_ops, philox_ref

    base = _ramp(2 * 4 * 4 * 8).reshape(2, 4, 4, 8)
    x = base.permute(0, 3, 1, 2)                       # (2, 8, 4, 4) view
    assert not x.is_contiguous()
    st = _state(seed=5, calls=9)
    y = gpu_ops.dropout(x, st, 0.5)
    assert y.shape == x.shape and y.stride() == x.stride()
    keep_ref = philox_ref.dropout_keep_mask(x.numel(), 5, 9, 0.5)
    y_storage = y.permute(0, 2, 3, 1).reshape(-1).cpu()
    x_storage = base.reshape(-1)
    expect = torch.where(torch.from_numpy(keep_ref), _scaled(x_storage, 0.5),
                         torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(y_storage, expect)
    # CPU functional path draws the very same elements
    from gan_deeplearning4j_amd.ops import functional as OF

    st_cpu = torch.tensor([5, 9])
    y_cpu = OF.dropout(x.float().cpu(), st_cpu, 0.5, training=True)
    assert torch.equal((y_cpu != 0), (y.cpu() != 0))


def test_binding_checks():
    e = ext()
    x = _ramp(64)
    st = _state()
    with pytest.raises(RuntimeError, match="bf16"):
        e.dropout_fwd(x.float(), st, 0.5)
    with pytest.raises(RuntimeError, match="state"):
        e.dropout_fwd(x, st.cpu(), 0.5)
    with pytest.raises(RuntimeError, match="state"):
        e.dropout_fwd(x, st.to(torch.int32), 0.5)
    with pytest.raises(RuntimeError, match="keep"):
        e.dropout_fwd(x, st, 0.0)
    with pytest.raises(RuntimeError, match="keep"):
        e.dropout_bwd(x, torch.zeros(8, dtype=torch.uint8, device=DEV), 1.5)
    with pytest.raises(RuntimeError, match="mask"):
        e.dropout_bwd(x, torch.zeros(7, dtype=torch.uint8, device=DEV), 0.5)
    with pytest.raises(RuntimeError, match="stddev"):
        e.gaussian_noise_fwd(x, st, -1.0)
    with pytest.raises(RuntimeError, match="dense"):
        e.dropout_fwd(_ramp(128).reshape(8, 16)[:, :8], st, 0.5)


# -------------------------------------------------------- gaussian noise
def test_gaussian_noise_matches_reference():
    from gan_deeplearning4j_amd.ops import functional as OF
    from gan_deeplearning4j_amd.ops import philox_ref

    n = 8 * 1024 + 5
    st = _state(seed=(1 << 40) + 7, calls=2)
    seed, calls = st.tolist()
    x = torch.zeros(n, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = OF.gaussian_noise(x, st, 1.0, training=True)
    assert st.tolist() == [seed, calls + 1]
    ref = philox_ref.gaussian_noise_ref(n, seed, calls)
    err = np.abs(y.detach().float().cpu().numpy().astype(np.float64) - ref)
    # two bf16 ulps (from the format) + fp32 log/sincos slack at |n| <= 6.7
    bound = 2.0 ** -7 * np.abs(ref) + 1e-4
    print("gaussian noise: worst err/bound", float((err / bound).max()))
    assert (err <= bound).all()
    dy = _ramp(n, mod=127)
    y.backward(dy)
    assert torch.equal(x.grad, dy)
    xs = _ramp(n)
    assert OF.gaussian_noise(xs, st, 0.0, training=True) is xs
    assert OF.gaussian_noise(xs, st, 0.5, training=False) is xs
    assert st.tolist() == [seed, calls + 1]
    # x + stddev * n with a non-zero x
    st2 = _state(seed=seed, calls=calls)
    y2 = OF.gaussian_noise(xs, st2, 0.25, training=True)
    expect = (xs.float().cpu() + 0.25 * y.detach().float().cpu())
    assert (y2.float().cpu() - expect).abs().max() <= 2.0 ** -7 * 8.0


# ---------------------------------------------------------------- capture
def test_dropout_capture_replays_fresh_masks():
    from gan_deeplearning4j_amd.ops import gpu_ops, philox_ref

    n, keep, seed = 8 * 256 * 5 + 5, 0.5, 4242
    st = _state(seed=seed, calls=0)
    x = _ramp(n).requires_grad_(True)

    def run():
        y = gpu_ops.dropout(x, st, keep)
        (g,) = torch.autograd.grad(y.float().sum(), x)
        return y, g

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    c0 = int(st[1])
    assert c0 == 2
    state_ptr = st.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static, g_static = run()
    outs, grads = [], []
    for _ in range(3):
        graph.replay()
        outs.append(y_static.clone())
        grads.append(g_static.clone())
    torch.cuda.synchronize()
    assert st.data_ptr() == state_ptr
    assert st.tolist() == [seed, c0 + 3]
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(outs[a], outs[b])
    one = torch.tensor(1.0 / keep, dtype=torch.float32).to(torch.bfloat16)
    for r in range(3):
        m = torch.from_numpy(
            philox_ref.dropout_keep_mask(n, seed, c0 + r, keep))
        expect = torch.where(m, _scaled(x.detach(), keep),
                             torch.zeros((), dtype=torch.bfloat16))
        assert torch.equal(outs[r].cpu(), expect)
        g_expect = torch.where(m, one, torch.zeros((), dtype=torch.bfloat16))
        assert torch.equal(grads[r].cpu(), g_expect)


# ----------------------------------------------------------- graph chains
def relerr(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


def _chain_graph(kind, keep):
    from gan_deeplearning4j_amd.graph import (
        BatchNormLayer, CnnToFeedForwardPreProcessor, Conv2dLayer,
        DenseLayer, DropoutLayer, GraphBuilder, InputType)

    gb = GraphBuilder(seed=7)
    gb.add_inputs("in")
    gb.set_input_types(InputType.convolutional(8, 8, 64))
    gb.add_layer("conv", Conv2dLayer(64, 64, 3, 1, 1, activation="lrelu"),
                 "in")
    gb.add_layer("drop", DropoutLayer(keep), "conv")
    if kind == "bn_dense":
        gb.add_layer("bn", BatchNormLayer(64), "drop")
        gb.add_layer("dense", DenseLayer(64 * 8 * 8, 16, "identity"), "bn",
                     preprocessor=CnnToFeedForwardPreProcessor())
        gb.set_outputs("dense")
    else:
        gb.add_layer("conv2", Conv2dLayer(64, 64, 4, 2, 1,
                                          activation="identity"), "drop")
        gb.set_outputs("conv2")
    return gb.build().init()


@pytest.mark.parametrize("kind", ["bn_dense", "conv"])
def test_graph_chain_around_dropout(kind):
    """conv(lrelu) -> dropout -> BN -> dense and conv(lrelu) -> dropout ->
    conv: the fusion pass must not reach across the dropout vertex. The
    mask is recovered from the dropout output; loss and every parameter
    gradient are recomputed in fp32 torch on the CPU with that mask.
    Tolerances are those of test_ops_gpu.py for the same layers (conv /
    dense 0.03 fwd, 0.04 grads; BN 0.05 params, 0.08 input grad — which
    also bounds everything upstream of the BN)."""
    keep = 0.7
    g = _chain_graph(kind, keep).to_device(torch.device(DEV), torch.bfloat16)
    g.train()
    assert not hasattr(g.get_layer("conv"), "emit_bn_stats") or \
        not g.get_layer("conv").emit_bn_stats
    assert not hasattr(g.get_layer("bn" if kind == "bn_dense" else "conv2"),
                       "bwd_act" if kind == "bn_dense" else "prev_act")
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(4, 64, 8, 8, generator=gen) * 0.5).to(
        DEV, torch.bfloat16).requires_grad_(True)
    seen = {}
    hook = g.get_layer("drop").register_forward_hook(
        lambda mod, inp, out: seen.update(conv=inp[0].detach(),
                                          drop=out.detach()))
    y = g(x)
    hook.remove()
    gout = (torch.randn(*y.shape, generator=gen)).to(DEV, torch.bfloat16)
    loss = (y.float() * gout.float()).sum()
    loss.backward()

    mask = (seen["drop"] != 0).cpu()
    frac = mask.float().mean().item()
    assert abs(frac - keep) < 0.03          # lrelu output is never exactly 0
    # the recovered mask is the oracle's, in storage (NHWC) order
    from gan_deeplearning4j_amd.ops import philox_ref

    drop = g.get_layer("drop")
    oracle = philox_ref.dropout_keep_mask(mask.numel(), drop.seed, 0, keep)
    storage = seen["drop"].permute(0, 2, 3, 1) \
        if seen["drop"].stride(1) == 1 else seen["drop"]
    assert ((storage.reshape(-1) != 0).cpu().numpy() == oracle).all()
    assert drop.calls == 1

    def f32(t):
        return t.detach().float().cpu().requires_grad_(True)

    conv = g.get_layer("conv")
    xr, wr, br = f32(x), f32(conv.weight), f32(conv.bias)
    h = F.leaky_relu(F.conv2d(xr, wr, br, stride=1, padding=1), 0.2)
    h = h * mask / keep
    if kind == "bn_dense":
        bn, dense = g.get_layer("bn"), g.get_layer("dense")
        gr, ber = f32(bn.weight), f32(bn.bias)
        dw, db = f32(dense.weight), f32(dense.bias)
        h = F.batch_norm(h, torch.zeros(64), torch.ones(64), gr, ber, True,
                         0.1, 1e-5)
        yr = F.linear(h.reshape(4, -1), dw, db)
        pairs = [("bn.gamma", bn.weight.grad, gr, 0.05),
                 ("bn.beta", bn.bias.grad, ber, 0.05),
                 ("dense.W", dense.weight.grad, dw, 0.04),
                 ("dense.b", dense.bias.grad, db, 0.04)]
        upstream = 0.08
    else:
        conv2 = g.get_layer("conv2")
        w2, b2 = f32(conv2.weight), f32(conv2.bias)
        yr = F.conv2d(h, w2, b2, stride=2, padding=1)
        pairs = [("conv2.W", conv2.weight.grad, w2, 0.04),
                 ("conv2.b", conv2.bias.grad, b2, 0.04)]
        upstream = 0.04
    loss_r = (yr * gout.float().cpu()).sum()
    loss_r.backward()
    pairs += [("conv.W", conv.weight.grad, wr, upstream),
              ("conv.b", conv.bias.grad, br, upstream),
              ("x", x.grad, xr, upstream)]
    assert relerr(y, yr) < (0.05 if kind == "bn_dense" else 0.03)
    scale = (yr.detach().abs() * gout.float().cpu().abs()).sum().item()
    assert abs(loss.item() - loss_r.item()) < 0.03 * scale
    for name, got, ref, tol in pairs:
        err = relerr(got, ref.grad)
        print(f"{kind}: {name} relerr {err:.4f} (tol {tol})")
        assert err < tol, name


# ---------------------------------------------------------------- trainer
def test_trainer_capture_with_dropout_and_noise():
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan
    from gan_deeplearning4j_amd.train import GanTrainer

    def make(capture):
        cfg = preset("dcgan28")
        cfg.model.dis_dropout = 0.3
        cfg.model.dis_input_noise_std = 0.1
        gen, dis = build_dcgan(cfg)
        tr = GanTrainer(gen, dis, cfg, device=torch.device(DEV),
                        dtype=torch.bfloat16, capture=capture)
        return tr, cfg

    real = (torch.rand(64, 1, 28, 28, generator=torch.Generator()
                       .manual_seed(0)) * 2 - 1).to(DEV, torch.bfloat16)
    tr, cfg = make(True)
    steps = 4
    for _ in range(steps):
        out = tr.step(real)
        assert math.isfinite(float(out["loss_d"]))
        assert math.isfinite(float(out["loss_g"]))
    assert not tr._graph_failed and tr._graph is not None
    # D runs 2 forwards (real, fake) per D pass and 1 in the G pass. The
    # first step() also runs the two eager warm-up steps before capturing;
    # recording itself executes nothing, every replay is one step.
    per_step = 2 * max(1, cfg.train.d_steps_per_g) + 1
    executed = 2 + steps
    counters = {k: layer.calls for k, layer in tr._stochastic_layers()}
    assert sorted(counters) == ["dis/d_drop_0", "dis/d_drop_1",
                                "dis/d_drop_feat", "dis/d_noise_in"]
    assert set(counters.values()) == {executed * per_step}

    eager, _ = make(False)
    for _ in range(executed):
        eager.step(real)
    assert {k: layer.calls for k, layer in eager._stochastic_layers()} \
        == counters
    # eval paths see the identity and leave the counters alone
    tr.sample_grid(4)
    tr.dis.output(real)
    assert {k: layer.calls for k, layer in tr._stochastic_layers()} \
        == counters
