"""The spectral-norm HIP kernels held to spectral_oracle's comparators, plus
reproducibility, graph capture, the layers and the captured trainer.  That
the comparators can fail is proven on the CPU by test_spectral_norm_cpu.py
(every mutant rejected)."""

import math

import pytest
import torch

import spectral_oracle as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(m, k, False) for m, k in S.ALL_SHAPES] + \
        [(m, k, True) for m, k in S.BASE_SHAPES]


def sx():
    from gan_deeplearning4j_amd.ops.backend import spectral_ext

    return spectral_ext()


def relerr(a, b):
    a = a.float().cpu()
    b = b.float().cpu()
    denom = b.abs().max().clamp_min(1e-6)
    return ((a - b).abs().max() / denom).item()


def _fwd(inp):
    """One training forward on the kernels from a clone of the state."""
    u, v = inp["u0"].to(DEV), inp["v0"].to(DEV)
    w_sn, u_c, v_c, sig, t, s = sx().sn_forward(inp["w"].to(DEV), u, v)
    return {"t": t, "s": s, "v": v_c, "u": u_c, "sig": sig, "w_sn": w_sn,
            "u_copy": u_c, "v_copy": v_c, "u_state": u, "v_state": v}


def _report(name, r):
    print(f"{name}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert S.worst(r) <= 1.0, r


# --------------------------------------------------------------- 8. surface
PUBLIC_NAMES = [
    "SN_BLOCK",
    "SN_CHUNK_ROWS",
    "SN_GRID_CAP",
    "SN_MAX_CHUNKS",
    "sn_backward",
    "sn_forward",
    "sn_forward_eval",
]


def test_spectral_ext_public_names_frozen():
    names = {n for n in dir(sx()) if not n.startswith("_")}
    assert names == set(PUBLIC_NAMES)


def test_launcher_constants_match_the_oracle():
    e = sx()
    assert (e.SN_BLOCK, e.SN_GRID_CAP, e.SN_CHUNK_ROWS, e.SN_MAX_CHUNKS) == \
        (S.SN_BLOCK, S.SN_GRID_CAP, S.SN_CHUNK_ROWS, S.SN_MAX_CHUNKS)


def test_binding_checks():
    e = sx()
    w = torch.zeros(4, 8, device=DEV, dtype=torch.bfloat16)
    u, v = torch.zeros(4, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="bf16"):
        e.sn_forward(w.float(), u, v)
    with pytest.raises(RuntimeError, match="GPU"):
        e.sn_forward(w.cpu(), u, v)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.sn_forward(w.t(), v, u)
    with pytest.raises(RuntimeError, match="elements"):
        e.sn_forward(w, v, u)
    with pytest.raises(RuntimeError, match="fp32"):
        e.sn_forward_eval(w, u.double(), v)
    with pytest.raises(RuntimeError, match="same shape"):
        e.sn_backward(w, w[:2].contiguous(), u, v,
                      torch.ones(2, device=DEV))


# ------------------------------------------------- 1. the oracle's comparators
@pytest.mark.parametrize("m,k,tiny", CASES)
def test_forward_against_the_oracle(m, k, tiny):
    inp = S.inputs(m, k, 10 + m + k, tiny)
    _report(f"fwd {m}x{k}", S.fwd_check(inp, _fwd(inp)))


@pytest.mark.parametrize("m,k,tiny", CASES)
def test_eval_against_the_oracle(m, k, tiny):
    # 3. eval leaves u and v bit-unchanged: u_unchanged / v_unchanged
    inp = S.inputs(m, k, 20 + m + k, tiny)
    u, v = inp["u0"].to(DEV), inp["v0"].to(DEV)
    w_sn, sig, s = sx().sn_forward_eval(inp["w"].to(DEV), u, v)
    out = {"s": s, "sig": sig, "w_sn": w_sn, "u_state": u, "v_state": v}
    _report(f"eval {m}x{k}", S.eval_check(inp, out))


@pytest.mark.parametrize("m,k,tiny", CASES)
def test_backward_against_the_oracle(m, k, tiny):
    inp = S.inputs(m, k, 30 + m + k, tiny)
    f1 = _fwd(inp)
    # a later forward moves the live state; backward gets the first's copies
    sx().sn_forward(inp["w"].to(DEV), f1["u_state"], f1["v_state"])
    binp = {**inp, "w_sn": f1["w_sn"], "u": f1["u_copy"], "v": f1["v_copy"],
            "sig": f1["sig"]}
    dw, part = sx().sn_backward(inp["g"].to(DEV), f1["w_sn"], f1["u_copy"],
                                f1["v_copy"], f1["sig"])
    _report(f"bwd {m}x{k}", S.bwd_check(binp, {"dw": dw, "dot_part": part}))


def test_autograd_backward_uses_the_first_forwards_state():
    from gan_deeplearning4j_amd.ops import gpu_ops

    inp = S.inputs(130, 72, 77)
    w = inp["w"].to(DEV).requires_grad_(True)
    u, v = inp["u0"].to(DEV), inp["v0"].to(DEV)
    first = gpu_ops.spectral_normalize(w, u, v, True)
    f1 = _fwd(inp)                                   # the same first call
    assert torch.equal(first, f1["w_sn"]) and torch.equal(u, f1["u_state"])
    gpu_ops.spectral_normalize(w, u, v, True)        # moves u, v again
    assert not torch.equal(u, f1["u_state"])
    first.backward(inp["g"].to(DEV))
    dw = sx().sn_backward(inp["g"].to(DEV), f1["w_sn"], f1["u_copy"],
                          f1["v_copy"], f1["sig"])[0]
    assert torch.equal(w.grad, dw)


# --------------------------------------------------------- 2. reproducibility
@pytest.mark.parametrize("m,k", [(130, 72), (5, 19), S.BIG_SHAPE])
def test_same_call_twice_is_bit_identical(m, k):
    inp = S.inputs(m, k, 5)
    a, b = _fwd(inp), _fwd(inp)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    g = inp["g"].to(DEV)
    da = sx().sn_backward(g, a["w_sn"], a["u"], a["v"], a["sig"])
    db = sx().sn_backward(g, b["w_sn"], b["u"], b["v"], b["sig"])
    assert torch.equal(da[0], db[0]) and torch.equal(da[1], db[1])


# ----------------------------------------------------------------- 4. capture
def test_capture_replays_the_power_iteration():
    inp = S.inputs(130, 72, 9)
    w = inp["w"].to(DEV)
    u, v = inp["u0"].to(DEV), inp["v0"].to(DEV)
    eu, ev = u.clone(), v.clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        wu, wv = u.clone(), v.clone()
        for _ in range(2):
            sx().sn_forward(w, wu, wv)               # warm the allocator
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                    # one stream, no branch
        w_static = sx().sn_forward(w, u, v)[0]
    torch.cuda.synchronize()
    assert torch.equal(u, eu) and torch.equal(v, ev)  # recording runs nothing
    for _ in range(3):
        graph.replay()
        got = (w_static.clone(), u.clone(), v.clone())
        want_w = sx().sn_forward(w, eu, ev)[0]
        torch.cuda.synchronize()
        assert torch.equal(got[0], want_w)
        assert torch.equal(got[1], eu) and torch.equal(got[2], ev)


# ------------------------------------------------------------- 5. convergence
def test_planted_gap_convergence_on_the_kernels():
    w, u, v = S.planted_gap_weight()
    w, u, v = w.to(DEV), u.to(DEV), v.to(DEV)
    for _ in range(8):
        w_sn = sx().sn_forward(w, u, v)[0]
    err, bound = S.planted_gap_check(w_sn)
    print(f"planted gap: |sigma1 - 1| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_zero_matrix_gives_zeros():
    w = torch.zeros(6, 10, device=DEV, dtype=torch.bfloat16)
    u = torch.full((6,), 6 ** -0.5, device=DEV)
    v = torch.full((10,), 10 ** -0.5, device=DEV)
    w_sn = sx().sn_forward(w, u, v)[0]
    assert torch.equal(w_sn, w)


# ------------------------------------------------------------------ 6. layers
@pytest.mark.parametrize("kind", ["conv", "dense"])
def test_layer_with_the_flag_against_the_cpu_path(kind):
    from gan_deeplearning4j_amd.graph import Conv2dLayer, DenseLayer
    from gan_deeplearning4j_amd.ops import functional as OF

    gen = torch.Generator().manual_seed(11)
    if kind == "conv":
        layer = Conv2dLayer(16, 32, 4, 2, 1, "lrelu", spectral_norm=True)
        x = torch.randn(4, 16, 16, 16, generator=gen) * 0.5
    else:
        layer = DenseLayer(200, 48, "lrelu", spectral_norm=True)
        x = torch.randn(4, 200, generator=gen)
    layer.reset_parameters(gen)
    with torch.no_grad():
        layer.bias.normal_(0.0, 0.1, generator=gen)
    layer.to(DEV)
    for p in layer.parameters():
        p.data = p.data.to(torch.bfloat16)
    assert layer.sn_u.dtype == torch.float32 and layer.sn_u.is_cuda
    u0, v0 = layer.sn_u.cpu().clone(), layer.sn_v.cpu().clone()
    xg = x.to(DEV, torch.bfloat16).requires_grad_(True)
    layer.train()
    y = layer(xg)
    gout = torch.randn(y.shape, generator=gen).to(torch.bfloat16)
    y.backward(gout.to(DEV))

    # the same layer, without the flag, fed the CPU path's W_sn as a plain
    # weight (in bf16, as the layer holds it: the reference then sees the
    # weights the kernels see, and no lrelu mask flips on a rounding)
    wr = layer.weight.detach().float().cpu().requires_grad_(True)
    w_sn = OF.spectral_normalize(wr, u0, v0, True)
    plain = Conv2dLayer(16, 32, 4, 2, 1, "lrelu") if kind == "conv" \
        else DenseLayer(200, 48, "lrelu")
    plain.to(DEV)
    plain.weight.data = w_sn.detach().to(DEV, torch.bfloat16)
    plain.bias.data = layer.bias.detach().clone()
    xp = xg.detach().clone().requires_grad_(True)
    plain.train()
    yp = plain(xp)
    yp.backward(gout.to(DEV))
    assert relerr(y, yp) < 0.03
    assert relerr(xg.grad, xp.grad) < 0.04
    assert relerr(layer.bias.grad, plain.bias.grad) < 0.04
    # dL/dW_sn of the plain layer, pulled back through the CPU path
    (dw_ref,) = torch.autograd.grad(w_sn, wr,
                                    plain.weight.grad.float().cpu())
    assert relerr(layer.weight.grad, dw_ref) < 0.04
    assert (layer.sn_u.cpu() - u0).abs().max() < 1e-5
    assert (layer.sn_v.cpu() - v0).abs().max() < 1e-5


def test_eval_caches_w_sn_until_the_state_moves():
    from gan_deeplearning4j_amd.graph import DenseLayer

    layer = DenseLayer(64, 16, spectral_norm=True)
    layer.reset_parameters(torch.Generator().manual_seed(2))
    layer.to(DEV)
    layer.weight.data = layer.weight.data.to(torch.bfloat16)
    layer.bias.data = layer.bias.data.to(torch.bfloat16)
    x = torch.randn(4, 64, device=DEV, dtype=torch.bfloat16)
    layer.eval()
    with torch.no_grad():
        y1 = layer(x)
        cached = layer.weight._gdlj_cache[1]["sn_eval"]
        y2 = layer(x)
        assert layer.weight._gdlj_cache[1]["sn_eval"] is cached
        assert torch.equal(y1, y2)
        layer.train()
        layer(x)                    # moves u, v: the cached W_sn is stale
        layer.eval()
        assert "sn_eval" not in layer.weight._gdlj_cache[1]
        y3 = layer(x)
    assert not torch.equal(y1, y3)


# ----------------------------------------------------------------- 7. trainer
def test_captured_trainer_with_spectral_norm():
    from gan_deeplearning4j_amd.config import preset
    from gan_deeplearning4j_amd.models import build_dcgan
    from gan_deeplearning4j_amd.train import GanTrainer

    cfg = preset("dcgan28")
    cfg.model.dis_spectral_norm = True
    cfg.train.loss_type = "hinge"
    gen, dis = build_dcgan(cfg)
    tr = GanTrainer(gen, dis, cfg, device=torch.device(DEV),
                    dtype=torch.bfloat16, capture=True)
    real = (torch.rand(16, 1, 28, 28, generator=torch.Generator()
                       .manual_seed(0)) * 2 - 1).to(DEV, torch.bfloat16)
    names = [n for n in tr.dis.layer_names()
             if tr.dis.layers[n].spectral_norm]
    assert names == ["d_conv_0", "d_conv_1", "d_dense_feat", "d_out"]
    prev = None
    for _ in range(5):
        out = tr.step(real)
        assert math.isfinite(float(out["loss_d"]))
        assert math.isfinite(float(out["loss_g"]))
        state = {n: (tr.dis.layers[n].sn_u.clone(),
                     tr.dis.layers[n].sn_v.clone()) for n in names}
        for n, (u, v) in state.items():
            assert abs(float(u.norm()) - 1.0) <= 1e-5, n
            assert abs(float(v.norm()) - 1.0) <= 1e-5, n
            if prev is not None:
                # W moved, so the iteration moved v (d_out's u is 1 x 1:
                # a sign, nothing to move)
                assert not torch.equal(v, prev[n][1]), n
                if u.numel() > 1:
                    assert not torch.equal(u, prev[n][0]), n
        prev = state
    assert not tr._graph_failed and tr._graph is not None
