"""Spectral normalization without a GPU: the oracle's own gate (emulation
accepted, every mutant rejected), the CPU path against
torch.nn.utils.spectral_norm bit for bit, and the layer / model / config /
persistence / trainer plumbing.  No tolerance lives here except the planted-
gap bound, which is derived in spectral_oracle.planted_gap_check."""

import io
import json
import zipfile

import pytest
import torch

import spectral_oracle as S
from gan_deeplearning4j_amd.config import GanConfig, preset
from gan_deeplearning4j_amd.graph import (
    Conv2dLayer,
    ConvTranspose2dLayer,
    DenseLayer,
    OutputLayer,
)
from gan_deeplearning4j_amd.graph.serialization import ModelSerializer
from gan_deeplearning4j_amd.models import build_dcgan, build_mlp_gan
from gan_deeplearning4j_amd.ops import functional as OF
from gan_deeplearning4j_amd.train import GanTrainer

KILLED = {}
CASES = [(m, k, False) for m, k in S.ALL_SHAPES] + \
        [(m, k, True) for m, k in S.BASE_SHAPES]


def _gate(table, inp, emulate, check, mutants):
    r = check(emulate(None))
    assert S.worst(r) <= 1.0, f"emulation rejected: {r}"
    for name, applies in mutants.items():
        if not applies(inp):
            continue
        rm = check(emulate(name))
        assert S.worst(rm) > 1.0, f"mutant {name} survived: {rm}"
        KILLED[(table, name)] = KILLED.get((table, name), 0) + 1


# ------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("m,k,tiny", CASES)
def test_oracle_forward(m, k, tiny):
    inp = S.inputs(m, k, 10 + m + k, tiny)
    _gate("fwd", inp, lambda mu: S.fwd_emulate(inp, mu),
          lambda o: S.fwd_check(inp, o), S.FWD_MUTANTS)


@pytest.mark.parametrize("m,k,tiny", CASES)
def test_oracle_eval(m, k, tiny):
    inp = S.inputs(m, k, 20 + m + k, tiny)
    _gate("eval", inp, lambda mu: S.eval_emulate(inp, mu),
          lambda o: S.eval_check(inp, o), S.EVAL_MUTANTS)


@pytest.mark.parametrize("m,k,tiny", CASES)
def test_oracle_backward(m, k, tiny):
    binp = S.bwd_inputs(S.inputs(m, k, 30 + m + k, tiny))
    _gate("bwd", binp, lambda mu: S.bwd_emulate(binp, mu),
          lambda o: S.bwd_check(binp, o), S.BWD_MUTANTS)


def test_every_mutant_is_exercised():
    listed = {("fwd", n) for n in S.FWD_MUTANTS} | \
        {("eval", n) for n in S.EVAL_MUTANTS} | \
        {("bwd", n) for n in S.BWD_MUTANTS}
    assert len(listed) == S.MUTANT_COUNT == 10
    KILLED.clear()
    for m, k, tiny in [(64, 48, False), (64, 48, True), (1, 1024, False)]:
        test_oracle_forward(m, k, tiny)
        test_oracle_eval(m, k, tiny)
        test_oracle_backward(m, k, tiny)
    assert not sorted(listed - set(KILLED))


# ------------------------------------------- 2. CPU path == torch, float64
def _torch_sn(m, k, seed):
    torch.manual_seed(seed)
    lin = torch.nn.Linear(k, m, bias=False).double()
    w = lin.weight.detach().clone()
    sn = torch.nn.utils.spectral_norm(lin, n_power_iterations=1, eps=1e-12,
                                      dim=0)
    return sn, w, sn.weight_u.detach().clone(), sn.weight_v.detach().clone()


@pytest.mark.parametrize("m,k", S.BASE_SHAPES)
def test_cpu_path_matches_torch_bit_for_bit(m, k):
    sn, w, u, v = _torch_sn(m, k, m * 1000 + k)
    x = torch.randn(3, k, dtype=torch.float64)
    sn.train()
    for step in range(3):
        sn(x)
        w_sn = OF.spectral_normalize(w, u, v, True)
        if step in (0, 2):
            assert torch.equal(w_sn, sn.weight.detach())
            assert torch.equal(u, sn.weight_u)
            assert torch.equal(v, sn.weight_v)
    sn.eval()
    sn(x)
    u_before, v_before = u.clone(), v.clone()
    w_eval = OF.spectral_normalize(w, u, v, False)
    assert torch.equal(w_eval, sn.weight.detach())
    assert torch.equal(u, u_before) and torch.equal(v, v_before)


@pytest.mark.parametrize("m,k", [(5, 19), (64, 48)])
def test_cpu_path_gradcheck_with_state_held_fixed(m, k):
    gen = torch.Generator().manual_seed(m)
    w = torch.randn(m, k, generator=gen, dtype=torch.float64,
                    requires_grad=True)
    u = S.unit(m, gen).double()
    v = S.unit(k, gen).double()
    # eval mode reads (u, v) and writes nothing: the state is held fixed
    assert torch.autograd.gradcheck(
        lambda t: OF.spectral_normalize(t, u, v, False), (w,))


def test_zero_matrix_gives_zeros_not_nan():
    w = torch.zeros(4, 6)
    u, v = torch.ones(4) / 2.0, torch.ones(6) / 6 ** 0.5
    out = OF.spectral_normalize(w, u, v, True)
    assert torch.equal(out, torch.zeros(4, 6))


# ------------------------------------- 3. two forwards, then one backward
def test_first_forwards_backward_uses_first_forwards_state():
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(7, 11, generator=gen, dtype=torch.float64,
                    requires_grad=True)
    g = torch.randn(7, 11, generator=gen, dtype=torch.float64)
    u, v = S.unit(7, gen).double(), S.unit(11, gen).double()
    first = OF.spectral_normalize(w, u, v, True)
    u1, v1 = u.clone(), v.clone()
    OF.spectral_normalize(w, u, v, True)          # moves u, v again
    assert not torch.equal(u, u1)
    (dw,) = torch.autograd.grad((first * g).sum(), w)
    wd = w.detach()
    sigma1 = torch.dot(u1, wd.mv(v1))
    expect = (g - (g * (wd / sigma1)).sum() * torch.outer(u1, v1)) / sigma1
    assert (dw - expect).abs().max() <= 1e-14 * expect.abs().max()
    sigma2 = torch.dot(u, wd.mv(v))
    wrong = (g - (g * (wd / sigma2)).sum() * torch.outer(u, v)) / sigma2
    assert (dw - wrong).abs().max() > 1e-3 * expect.abs().max()


# ------------------------------------------------------------ 4. convergence
def test_planted_gap_convergence():
    w, u, v = S.planted_gap_weight()
    err0, bound = S.planted_gap_check(w)          # no iteration: far off
    assert err0 > 0.5
    w32 = w.float()
    for _ in range(8):
        w_sn = OF.spectral_normalize(w32, u, v, True)
    err, bound = S.planted_gap_check(w_sn.to(torch.bfloat16))
    print(f"planted gap: |sigma1 - 1| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------ 5. layers and models
def _drawn(layer):
    gen = torch.Generator().manual_seed(5)
    layer.reset_parameters(gen)
    return gen.get_state()


@pytest.mark.parametrize("make", [
    lambda sn: DenseLayer(12, 7, "lrelu", spectral_norm=sn),
    lambda sn: OutputLayer(12, 1, "sigmoid", "xent", spectral_norm=sn),
    lambda sn: Conv2dLayer(3, 5, 4, 2, 1, "lrelu", spectral_norm=sn),
])
def test_layer_without_the_flag_is_the_parent_layer(make):
    plain, flagged = make(False), make(True)
    st_plain, st_flag = _drawn(plain), _drawn(flagged)
    # the same weights either way; only the flagged layer draws more
    assert torch.equal(plain.weight, flagged.weight)
    assert not torch.equal(st_plain, st_flag)
    gen = torch.Generator().manual_seed(5)
    torch.empty_like(plain.weight).normal_(0.0, 1.0, generator=gen)
    assert torch.equal(gen.get_state(), st_plain)   # W only, nothing else
    assert plain.sn_u is None and plain.sn_v is None
    assert plain.n_params() == flagged.n_params()
    assert abs(float(flagged.sn_u.norm()) - 1) < 1e-6
    assert abs(float(flagged.sn_v.norm()) - 1) < 1e-6
    assert flagged.sn_v.numel() == flagged.weight[0].numel()
    x = torch.randn(2, 3, 8, 8) if plain.weight.dim() == 4 \
        else torch.randn(2, 12)
    ref = plain(x)
    u0, v0 = flagged.sn_u.clone(), flagged.sn_v.clone()
    w_sn = OF.spectral_normalize(flagged.weight.detach(), u0, v0, True)
    plain.weight.data.copy_(w_sn)
    assert torch.equal(flagged(x), plain(x))
    assert not torch.equal(flagged(x), ref)
    # get_param / set_param address the raw W
    assert torch.equal(flagged.get_param("W"), flagged.weight.detach())


def test_state_follows_the_module_and_stays_fp32():
    layer = DenseLayer(6, 4, spectral_norm=True)
    layer.reset_parameters(torch.Generator().manual_seed(1))
    u = layer.sn_u.clone()
    layer.double()
    assert layer.weight.dtype == torch.float64
    assert layer.sn_u.dtype == torch.float32
    assert torch.equal(layer.sn_u, u)
    layer(torch.randn(3, 6, dtype=torch.float64))     # mixed dtypes run
    assert not list(layer.buffers())


def test_transposed_conv_flag_raises():
    with pytest.raises(ValueError, match="spectral_norm"):
        ConvTranspose2dLayer(4, 4, 4, 2, 1, spectral_norm=True)
    ConvTranspose2dLayer(4, 4, 4, 2, 1, spectral_norm=False)


def _cfg(arch, sn=True, width=8):
    cfg = preset(arch)
    cfg.model.base_width = width
    cfg.model.dis_spectral_norm = sn
    cfg.train.use_gpu = False
    cfg.train.loss_type = "hinge"
    return cfg


@pytest.mark.parametrize("arch,n_conv", [("dcgan28", 2), ("dcgan64", 4),
                                         ("dcgan128", 5)])
def test_dis_spectral_norm_vertex_list(arch, n_conv):
    _, dis = build_dcgan(_cfg(arch))
    expect = [f"d_conv_{i}" for i in range(n_conv)] + ["d_dense_feat",
                                                       "d_out"]
    assert dis.layer_names() == expect
    assert all(dis.layers[n].spectral_norm for n in expect)
    _, plain = build_dcgan(_cfg(arch, sn=False))
    assert [n for n in plain.layer_names() if n.startswith("d_bn_")] == \
        [f"d_bn_{i}" for i in range(1, n_conv)]
    assert not any(getattr(plain.layers[n], "spectral_norm")
                   for n in plain.layer_names())
    # the generator never carries the flag
    gen, _ = build_dcgan(_cfg(arch))
    assert not any(gen.layers[n].spectral_norm for n in gen.layer_names())


def test_default_off_changes_no_initialisation():
    cfg = _cfg("dcgan28", sn=False)
    g1, d1 = build_dcgan(cfg)
    cfg2 = preset("dcgan28")
    cfg2.model.base_width = 8
    g2, d2 = build_dcgan(cfg2)
    assert torch.equal(d1.params_flat(), d2.params_flat())
    assert torch.equal(g1.params_flat(), g2.params_flat())


def test_mlp_gan_flag():
    cfg = preset("mlp_tabular_cpu")
    cfg.model.dis_spectral_norm = True
    _, dis = build_mlp_gan(cfg, hidden=16)
    assert all(dis.layers[n].spectral_norm
               for n in ("d_dense_1", "d_dense_feat", "d_out"))
    cfg.model.dis_spectral_norm = False
    _, plain = build_mlp_gan(cfg, hidden=16)
    assert plain.layer_names() == dis.layer_names()


def test_config_round_trip_and_cli_override(tmp_path):
    cfg = GanConfig()
    assert cfg.model.dis_spectral_norm is False
    cfg2 = cfg.apply_overrides(["model.dis_spectral_norm=true"])
    assert cfg2.model.dis_spectral_norm is True
    cfg2.to_yaml(tmp_path / "c.yaml")
    assert GanConfig.from_yaml(tmp_path / "c.yaml").model.dis_spectral_norm \
        is True
    assert GanConfig.from_cli(["model.dis_spectral_norm=1"]) \
        .model.dis_spectral_norm is True


# ----------------------------------------------------------- 6. persistence
def _sn_state(graph):
    return [(n, graph.layers[n].sn_u.clone(), graph.layers[n].sn_v.clone())
            for n in graph.layer_names() if graph.layers[n].spectral_norm]


def test_write_restore_keeps_u_v_and_eval_outputs(tmp_path):
    _, dis = build_dcgan(_cfg("dcgan28"))
    x = torch.randn(4, 1, 28, 28)
    dis.train()
    dis(x)                                  # move u, v off their init
    before = _sn_state(dis)
    out = dis.output(x)
    path = ModelSerializer.write_model(dis, tmp_path / "d.zip")
    back = ModelSerializer.restore_computation_graph(path)
    for (n, u, v), (n2, u2, v2) in zip(before, _sn_state(back)):
        assert n == n2 and torch.equal(u, u2) and torch.equal(v, v2)
    assert torch.equal(back.output(x), out)
    with zipfile.ZipFile(path) as zf:
        assert "spectralNorm.bin" in zf.namelist()
        dl4j = json.loads(zf.read("configuration.json"))
        zf_bytes = {n: zf.read(n) for n in zf.namelist()}
    conv0 = dl4j["vertices"]["d_conv_0"]["layerConf"]["layer"]
    assert conv0["spectralNorm"] is True
    # the DL4J-layout JSON alone restores the flag through the parser
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for n in ("configuration.json", "coefficients.bin",
                  "spectralNorm.bin"):
            zf.writestr(n, zf_bytes[n])
    (tmp_path / "dl4j_only.zip").write_bytes(buf.getvalue())
    back2 = ModelSerializer.restore_computation_graph(
        tmp_path / "dl4j_only.zip", load_updater=False)
    assert [n for n, _, _ in _sn_state(back2)] == [n for n, _, _ in before]
    assert torch.equal(back2.layers["d_out"].sn_u, dis.layers["d_out"].sn_u)
    # native format too
    nat = ModelSerializer.load_native(
        ModelSerializer.save_native(dis, tmp_path / "d.pt"))
    assert torch.equal(nat.output(x), out)


def test_model_without_the_flag_writes_no_new_entry(tmp_path):
    _, dis = build_dcgan(_cfg("dcgan28", sn=False))
    path = ModelSerializer.write_model(dis, tmp_path / "d.zip")
    with zipfile.ZipFile(path) as zf:
        assert "spectralNorm.bin" not in zf.namelist()
        for name in ("configuration.json", "configuration.native.json"):
            text = zf.read(name).decode()
            assert "spectral" not in text.lower()


# --------------------------------------------------------------- 7. trainer
def _trainer():
    cfg = _cfg("dcgan28")
    gen, dis = build_dcgan(cfg)
    return GanTrainer(gen, dis, cfg, device=torch.device("cpu"))


def test_trainer_three_steps_equal_two_plus_resume_plus_one(tmp_path):
    x = torch.rand(8, 1, 28, 28) * 2 - 1
    tr = _trainer()
    init = _sn_state(tr.dis)
    for _ in range(2):
        tr.step(x)
    tr.save(tmp_path)
    z_stream = tr._g.get_state()     # the z generator is not checkpointed
    ref = tr.step(x)                 # step 3, uninterrupted
    assert all(not torch.equal(v, v2) for (_, _, v), (_, _, v2)
               in zip(init, _sn_state(tr.dis)))     # (d_out's u is 1 x 1)

    tr2 = _trainer()
    ident = [(id(u), id(v)) for _, u, v in
             [(n, tr2.dis.layers[n].sn_u, tr2.dis.layers[n].sn_v)
              for n in tr2.dis.layer_names()]]
    assert tr2.resume(tmp_path)
    assert ident == [(id(tr2.dis.layers[n].sn_u), id(tr2.dis.layers[n].sn_v))
                     for n in tr2.dis.layer_names()]    # restored in place
    tr2._labels(8)       # drawn once from the same generator, before z
    tr2._g.set_state(z_stream)
    out = tr2.step(x)
    assert float(out["loss_d"]) == float(ref["loss_d"])
    assert float(out["loss_g"]) == float(ref["loss_g"])
    assert torch.equal(tr2.dis.params_flat(), tr.dis.params_flat())
    assert torch.equal(tr2.gen.params_flat(), tr.gen.params_flat())
    for (n, u, v), (_, u2, v2) in zip(_sn_state(tr.dis), _sn_state(tr2.dis)):
        assert torch.equal(u, u2) and torch.equal(v, v2), n


# ------------------------------------------------------------ loud failure
def test_missing_spectral_module_is_an_error(monkeypatch):
    from gan_deeplearning4j_amd.ops import backend

    monkeypatch.setattr(backend, "_spectral", None)
    monkeypatch.setattr(backend, "_spectral_tried", False)
    monkeypatch.setattr(backend, "_find_spectral_path", lambda: None)
    assert not backend.has_spectral_ext()
    with pytest.raises(RuntimeError, match="_spectral"):
        backend.spectral_ext()


def test_spectral_module_is_not_seen_by_the_c_glob():
    # backend._find_ext_path globs _C*.so: the second module must not match
    from gan_deeplearning4j_amd.ops import backend

    path = backend._find_ext_path()
    assert path is None or "_spectral" not in path
