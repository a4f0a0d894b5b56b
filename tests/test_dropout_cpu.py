"""Dropout / GaussianNoise layers: the Philox reference stream, the CPU
functional path, the layers, serialization, model wiring and the trainer's
counter checkpointing. Everything here runs without a GPU; the GPU kernels
are checked against the same reference in test_dropout_gpu.py."""

import json
import math

import numpy as np
import pytest
import torch

from gan_deeplearning4j_amd.config import GanConfig, preset
from gan_deeplearning4j_amd.graph import (
    DenseLayer,
    DropoutLayer,
    GaussianNoiseLayer,
    GraphBuilder,
    InputType,
    ModelSerializer,
    OutputLayer,
)
from gan_deeplearning4j_amd.graph.dl4j_json import from_dl4j_json, to_dl4j_json
from gan_deeplearning4j_amd.models import build_dcgan, build_mlp_gan
from gan_deeplearning4j_amd.ops import functional as OF
from gan_deeplearning4j_amd.ops import philox_ref
from gan_deeplearning4j_amd.train import GanTrainer


# --------------------------------------------------------------- philox
@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, expect):
    out = philox_ref.philox4x32_10(counter, key).reshape(-1)
    assert tuple(int(v) for v in out) == expect


def test_philox_vectorised_matches_scalar():
    c0 = np.arange(5, dtype=np.uint64)
    batch = philox_ref.philox4x32_10((c0, 7, 3, 0), (11, 13))
    for i in range(5):
        one = philox_ref.philox4x32_10((i, 7, 3, 0), (11, 13))
        assert (batch[i] == one[0]).all()


def test_block_index_above_32_bits_changes_counter_word_1():
    seed, calls, keep = 666, 2, 0.5
    i = (1 << 32) + 5
    m = philox_ref.dropout_keep_mask(8, seed, calls, keep, first_block=i)
    w = philox_ref.philox4x32_10((5, 1, calls, 0), (seed, 0)).reshape(-1)
    h = []
    for word in w:
        h += [int(word) & 0xFFFF, int(word) >> 16]
    assert m.tolist() == [v < 32768 for v in h]
    # ...and it is NOT the stream of block 5 (counter word 1 == 0)
    w_low = philox_ref.philox4x32_10((5, 0, calls, 0), (seed, 0))
    assert (w_low.reshape(-1) != w).all()
    # gaussian noise: block i uses Philox blocks 2i and 2i+1 of the same
    # counter space, also past 2^32
    g = philox_ref.gaussian_noise_ref(8, seed, calls, first_block=i)
    wa = philox_ref.philox4x32_10(((2 * i) & 0xFFFFFFFF, (2 * i) >> 32,
                                   calls, 0), (seed, 0)).reshape(-1)
    u1 = (float(wa[0]) + 1.0) * 2.0 ** -32
    u2 = float(wa[1]) * 2.0 ** -32
    r = math.sqrt(-2.0 * math.log(u1))
    assert g[0] == pytest.approx(r * math.cos(2 * math.pi * u2), abs=1e-12)
    assert g[1] == pytest.approx(r * math.sin(2 * math.pi * u2), abs=1e-12)


def test_seed_above_32_bits_uses_key_word_1():
    seed = (1 << 40) + 7
    m = philox_ref.dropout_keep_mask(8, seed, 0, 0.5)
    w = philox_ref.philox4x32_10((0, 0, 0, 0), (7, 1 << 8)).reshape(-1)
    h = []
    for word in w:
        h += [int(word) & 0xFFFF, int(word) >> 16]
    assert m.tolist() == [v < 32768 for v in h]


@pytest.mark.parametrize("keep", [0.25, 0.5, 0.8])
@pytest.mark.parametrize("seed", [666, 1, (1 << 40) + 7])
def test_mask_keep_fraction(keep, seed):
    n = 65536
    sigma = math.sqrt(keep * (1 - keep) / n)
    for calls in range(4):
        frac = philox_ref.dropout_keep_mask(n, seed, calls, keep).mean()
        assert abs(frac - keep) <= 5 * sigma, (keep, seed, calls, frac)


@pytest.mark.parametrize("seed", [666, 1, (1 << 40) + 7])
def test_masks_of_consecutive_calls_are_independent(seed):
    n = 65536
    masks = [philox_ref.dropout_keep_mask(n, seed, c, 0.5) for c in range(4)]
    for a, b in zip(masks, masks[1:]):
        agree = (a == b).mean()
        assert 0.45 <= agree <= 0.55, agree


def test_gaussian_ref_moments():
    g = philox_ref.gaussian_noise_ref(65536, 666, 0)
    # mean of n standard normals: sigma = 1/sqrt(n); 5 sigma
    assert abs(g.mean()) <= 5 / math.sqrt(g.size)
    # variance of the sample variance: 2/n; 5 sigma
    assert abs(g.var() - 1.0) <= 5 * math.sqrt(2.0 / g.size)


# ----------------------------------------------------------- functional
def _state(seed=666, calls=0):
    st = OF.new_rng_state(seed)
    st[1] = calls
    return st


@pytest.mark.parametrize("keep", [0.25, 0.5, 0.8])
def test_functional_dropout_cpu_exact(keep):
    torch.manual_seed(0)
    x = torch.randn(5, 13, requires_grad=True)
    st = _state(666, 3)
    y = OF.dropout(x, st, keep, training=True)
    mask = torch.from_numpy(
        philox_ref.dropout_keep_mask(x.numel(), 666, 3, keep)).reshape(5, 13)
    scale = torch.tensor(1.0 / keep, dtype=torch.float32)
    expect = torch.where(mask, x.detach() * scale, torch.zeros(()))
    assert torch.equal(y.detach(), expect)
    assert st.tolist() == [666, 4]
    dy = torch.randn(5, 13)
    y.backward(dy)
    assert torch.equal(x.grad, torch.where(mask, dy * scale, torch.zeros(())))


def test_functional_counter_rules():
    x = torch.randn(4, 8)
    st = _state(1, 0)
    assert OF.dropout(x, st, 0.5, training=False) is x
    assert OF.dropout(x, st, 1.0, training=True) is x
    assert OF.gaussian_noise(x, st, 0.0, training=True) is x
    assert OF.gaussian_noise(x, st, 0.3, training=False) is x
    assert st.tolist() == [1, 0]
    OF.dropout(x, st, 0.5, training=True)
    assert st.tolist() == [1, 1]
    OF.gaussian_noise(x, st, 0.3, training=True)
    assert st.tolist() == [1, 2]
    with pytest.raises(ValueError):
        OF.dropout(x, st, 0.0)
    with pytest.raises(ValueError):
        OF.dropout(x, st, 1.5)
    with pytest.raises(ValueError):
        OF.gaussian_noise(x, st, -1.0)


def test_functional_gaussian_noise_cpu():
    x = torch.randn(3, 11, requires_grad=True)
    st = _state(9, 5)
    y = OF.gaussian_noise(x, st, 0.25, training=True)
    nz = torch.from_numpy(philox_ref.gaussian_noise_ref(33, 9, 5)).float()
    assert torch.equal(y.detach(), x.detach() + 0.25 * nz.reshape(3, 11))
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad, torch.ones(3, 11))
    assert st.tolist() == [9, 6]


def test_functional_mask_follows_storage_order():
    # channels-last view: block/element indices walk the STORAGE
    base = torch.arange(1, 2 * 4 * 4 * 8 + 1, dtype=torch.float32)
    x = base.reshape(2, 4, 4, 8).permute(0, 3, 1, 2)     # NCHW view of NHWC
    y = OF.dropout(x, _state(3, 0), 0.5, training=True)
    kept_storage = (y.permute(0, 2, 3, 1).reshape(-1) != 0).numpy()
    expect = philox_ref.dropout_keep_mask(x.numel(), 3, 0, 0.5)
    assert (kept_storage == expect).all()


# --------------------------------------------------------------- layers
def _two_dropout_graph(seed=666, keep=0.5, with_dropout=True):
    gb = GraphBuilder(seed=seed)
    gb.add_inputs("in")
    gb.set_input_types(InputType.feed_forward(8))
    gb.add_layer("d1", DenseLayer(8, 16, "lrelu"), "in")
    prev = "d1"
    if with_dropout:
        gb.add_layer("drop1", DropoutLayer(keep), prev)
        prev = "drop1"
    gb.add_layer("d2", DenseLayer(16, 16, "lrelu"), prev)
    prev = "d2"
    if with_dropout:
        gb.add_layer("drop2", DropoutLayer(keep), prev)
        gb.add_layer("noise", GaussianNoiseLayer(0.2), "drop2")
        prev = "noise"
    gb.add_layer("out", OutputLayer(16, 1, "sigmoid", "xent"), prev)
    gb.set_outputs("out")
    return gb.build().init()


def test_layers_have_no_params_and_state_is_not_a_buffer():
    g = _two_dropout_graph()
    for name in ("drop1", "drop2", "noise"):
        layer = g.get_layer(name)
        assert layer.n_params() == 0
        assert list(layer.parameters()) == []
        assert list(layer.buffers()) == []
        assert layer.out_shape((4, 16)) == (4, 16)
        assert layer.calls == 0
    ids = {id(b) for b in g.buffers()} | {id(p) for p in g.parameters()}
    assert id(g.get_layer("drop1").rng_state) not in ids
    assert not any("rng_state" in k for k in g.state_dict())
    plain = _two_dropout_graph(with_dropout=False)
    assert g.n_params() == plain.n_params()
    assert "drop1" in g.summary()


def test_layer_state_follows_to():
    layer = DropoutLayer(0.5)
    layer.reset_parameters(torch.Generator().manual_seed(1))
    seed = layer.seed
    layer.to(torch.float64)               # dtype moves leave the state int64
    assert layer.rng_state.dtype == torch.int64 and layer.seed == seed
    layer.to("meta")                      # device moves take the state along
    assert layer.rng_state.device.type == "meta"


def test_layer_seeds_distinct_and_reproducible():
    a = _two_dropout_graph(seed=666)
    b = _two_dropout_graph(seed=666)
    c = _two_dropout_graph(seed=667)
    seeds_a = [a.get_layer(n).seed for n in ("drop1", "drop2", "noise")]
    seeds_b = [b.get_layer(n).seed for n in ("drop1", "drop2", "noise")]
    seeds_c = [c.get_layer(n).seed for n in ("drop1", "drop2", "noise")]
    assert len(set(seeds_a)) == 3
    assert seeds_a == seeds_b
    assert seeds_a != seeds_c


def test_graph_output_is_identity_through_stochastic_layers():
    g = _two_dropout_graph()
    plain = _two_dropout_graph(with_dropout=False)
    for name in ("d1", "d2", "out"):
        for key in ("W", "b"):
            plain.get_layer(name).set_param(key, g.get_layer(name).get_param(key))
    x = torch.randn(6, 8)
    o1, o2 = g.output(x), g.output(x)
    assert torch.equal(o1, o2)
    assert torch.equal(o1, plain.output(x))
    assert g.get_layer("drop1").calls == 0
    # training mode is stochastic and advances the counters
    g.train()
    t1, t2 = g(x), g(x)
    assert not torch.equal(t1, t2)
    assert g.get_layer("drop1").calls == 2
    assert g.get_layer("noise").calls == 2


def test_layer_ctor_validation():
    with pytest.raises(ValueError):
        DropoutLayer(0.0)
    with pytest.raises(ValueError):
        DropoutLayer(1.1)
    with pytest.raises(ValueError):
        GaussianNoiseLayer(-0.1)


# ------------------------------------------------------------ DL4J JSON
def test_dl4j_json_roundtrip_keeps_keep_and_stddev():
    g = _two_dropout_graph(keep=0.7)
    conf = json.loads(json.dumps(to_dl4j_json(g)))
    ld = conf["vertices"]["drop1"]["layerConf"]["layer"]
    assert ld["@class"] == "org.deeplearning4j.nn.conf.layers.DropoutLayer"
    assert ld["idropout"] == {
        "@class": "org.deeplearning4j.nn.conf.dropout.Dropout", "p": 0.7}
    nd = conf["vertices"]["noise"]["layerConf"]["layer"]
    assert nd["@class"] == "org.deeplearning4j.nn.conf.layers.DropoutLayer"
    assert nd["idropout"] == {
        "@class": "org.deeplearning4j.nn.conf.dropout.GaussianNoise",
        "stddev": 0.2}
    g2 = from_dl4j_json(conf)
    assert g2.layer_names() == g.layer_names()
    assert isinstance(g2.get_layer("drop1"), DropoutLayer)
    assert g2.get_layer("drop1").keep == 0.7
    assert isinstance(g2.get_layer("noise"), GaussianNoiseLayer)
    assert g2.get_layer("noise").stddev == 0.2
    assert g2.get_layer("drop1").seed != g2.get_layer("drop2").seed


def _handwritten_conf(idropout):
    """The way DL4J writes `.layer(new DenseLayer.Builder()...dropOut(p))`:
    the IDropout sits on the layer that owns it."""
    ns_l = "org.deeplearning4j.nn.conf.layers."

    def vertex(layer, preproc=None):
        return {"@class": "org.deeplearning4j.nn.conf.graph.LayerVertex",
                "layerConf": {"layer": layer, "seed": 42},
                "preProcessor": preproc}

    act = {"@class": "org.nd4j.linalg.activations.impl.ActivationLReLU"}
    return {
        "networkInputs": ["in"],
        "networkInputTypes": [{
            "@class": "org.deeplearning4j.nn.conf.inputs."
                      "InputType$InputTypeConvolutional",
            "height": 2, "width": 2, "channels": 2}],
        "networkOutputs": ["out"],
        "vertexInputs": {"dense": ["in"], "out": ["dense"]},
        "vertices": {
            "dense": vertex(
                {"@class": ns_l + "DenseLayer", "layerName": "dense",
                 "activationFn": act, "nin": 8, "nout": 4,
                 "idropout": idropout},
                {"@class": "org.deeplearning4j.nn.conf.preprocessor."
                           "CnnToFeedForwardPreProcessor"}),
            "out": vertex(
                {"@class": ns_l + "OutputLayer", "layerName": "out",
                 "activationFn": {"@class": "org.nd4j.linalg.activations."
                                            "impl.ActivationSigmoid"},
                 "lossFn": {"@class": "org.nd4j.linalg.lossfunctions.impl."
                                      "LossBinaryXENT"},
                 "nin": 4, "nout": 1, "idropout": None}),
        },
    }


@pytest.mark.parametrize("idropout,cls,field,value", [
    ({"@class": "org.deeplearning4j.nn.conf.dropout.Dropout", "p": 0.6},
     DropoutLayer, "keep", 0.6),
    ({"@class": "org.deeplearning4j.nn.conf.dropout.GaussianNoise",
      "stddev": 0.3}, GaussianNoiseLayer, "stddev", 0.3),
])
def test_dl4j_per_layer_idropout_becomes_vertex_and_folds_back(
        idropout, cls, field, value):
    g = from_dl4j_json(_handwritten_conf(idropout))
    assert g.layer_names() == ["dense__idropout", "dense", "out"]
    drop = g.get_layer("dense__idropout")
    assert isinstance(drop, cls) and getattr(drop, field) == value
    # in front of the layer, AFTER its preprocessor
    assert g._vertex_inputs["dense"] == ["dense__idropout"]
    assert g._vertex_inputs["dense__idropout"] == ["in"]
    assert "dense__idropout" in g.preprocessors
    assert "dense" not in g.preprocessors
    g.init()
    assert g.output(torch.randn(3, 2, 2, 2)).shape == (3, 1)
    g.train()
    assert g(torch.randn(3, 2, 2, 2)).shape == (3, 1)
    # written back folded into the owning layer
    conf = json.loads(json.dumps(to_dl4j_json(g)))
    assert sorted(conf["vertices"]) == ["dense", "out"]
    assert conf["vertexInputs"]["dense"] == ["in"]
    assert conf["vertices"]["dense"]["layerConf"]["layer"]["idropout"] == \
        idropout
    assert conf["vertices"]["dense"]["preProcessor"]["@class"].endswith(
        "CnnToFeedForwardPreProcessor")
    assert conf["vertices"]["out"]["layerConf"]["layer"]["idropout"] is None
    # the folded form parses back into the same graph
    g3 = from_dl4j_json(conf)
    assert g3.layer_names() == g.layer_names()
    assert g3.get_layer("dense__idropout").folded_into == "dense"


def test_dl4j_unknown_idropout_class_raises():
    bad = {"@class": "org.deeplearning4j.nn.conf.dropout.AlphaDropout",
           "p": 0.5}
    with pytest.raises(TypeError, match="AlphaDropout"):
        from_dl4j_json(_handwritten_conf(bad))


def test_native_zip_roundtrip(tmp_path):
    g = from_dl4j_json(_handwritten_conf(
        {"@class": "org.deeplearning4j.nn.conf.dropout.Dropout", "p": 0.6}))
    g.init()
    g2 = _two_dropout_graph(keep=0.7)
    for graph, fname in ((g, "a.zip"), (g2, "b.zip")):
        path = ModelSerializer.write_model(graph, tmp_path / fname)
        back = ModelSerializer.restore_computation_graph(path)
        assert back.layer_names() == graph.layer_names()
        assert torch.equal(back.params_flat(), graph.params_flat())
        for name in graph.layer_names():
            a, b = graph.get_layer(name), back.get_layer(name)
            assert type(a) is type(b)
            for field in ("keep", "stddev", "folded_into", "seed"):
                assert getattr(a, field, None) == getattr(b, field, None)
    # coefficients.bin carries parameters only
    import zipfile

    with zipfile.ZipFile(tmp_path / "b.zip") as zf:
        assert len(zf.read("coefficients.bin")) == 4 * g2.params_flat().numel()


# ------------------------------------------------------- model wiring
def test_build_dcgan_default_graph_is_unchanged():
    gen, dis = build_dcgan(preset("dcgan64"))
    assert dis.layer_names() == [
        "d_conv_0", "d_conv_1", "d_bn_1", "d_conv_2", "d_bn_2", "d_conv_3",
        "d_bn_3", "d_dense_feat", "d_out"]
    assert gen.layer_names() == [
        "g_dense_0", "g_bn_0", "g_deconv_1", "g_bn_1", "g_deconv_2", "g_bn_2",
        "g_deconv_3", "g_bn_3", "g_out"]
    _, dis28 = build_dcgan(preset("dcgan28"))
    assert dis28.layer_names() == [
        "d_conv_0", "d_conv_1", "d_bn_1", "d_dense_feat", "d_out"]


def test_build_dcgan_with_regularisers():
    cfg = preset("dcgan64")
    cfg.model.dis_dropout = 0.3
    cfg.model.dis_input_noise_std = 0.1
    gen, dis = build_dcgan(cfg)
    assert dis.layer_names() == [
        "d_noise_in", "d_conv_0", "d_drop_0", "d_conv_1", "d_bn_1",
        "d_drop_1", "d_conv_2", "d_bn_2", "d_drop_2", "d_conv_3", "d_bn_3",
        "d_drop_3", "d_dense_feat", "d_drop_feat", "d_out"]
    assert dis.get_layer("d_drop_0").keep == pytest.approx(0.7)
    assert dis.get_layer("d_noise_in").stddev == 0.1
    assert dis._vertex_inputs["d_dense_feat"] == ["d_drop_3"]
    assert dis._vertex_inputs["d_out"] == ["d_drop_feat"]
    assert "d_dense_feat" in dis.preprocessors
    # G is untouched, parameters are the same count as without the knobs
    _, plain = build_dcgan(preset("dcgan64"))
    assert dis.n_params() == plain.n_params()
    assert gen.layer_names()[0] == "g_dense_0"
    # no producer<->consumer fusion reaches across a dropout vertex
    assert hasattr(plain.get_layer("d_conv_1"), "prev_act")
    assert not hasattr(dis.get_layer("d_conv_1"), "prev_act")


def test_build_mlp_with_regularisers():
    cfg = preset("mlp_tabular_cpu")
    _, plain = build_mlp_gan(cfg, hidden=16)
    assert plain.layer_names() == ["d_dense_1", "d_dense_feat", "d_out"]
    cfg.model.dis_dropout = 0.3
    cfg.model.dis_input_noise_std = 0.05
    _, dis = build_mlp_gan(cfg, hidden=16)
    assert dis.layer_names() == ["d_noise_in", "d_dense_1", "d_drop_1",
                                 "d_dense_feat", "d_drop_feat", "d_out"]


@pytest.mark.parametrize("field,value", [
    ("dis_dropout", 1.0), ("dis_dropout", -0.1),
    ("dis_input_noise_std", -0.5)])
def test_trainer_rejects_bad_knobs(field, value):
    cfg = preset("mlp_tabular_cpu")
    gen, dis = build_mlp_gan(cfg, hidden=16)
    setattr(cfg.model, field, value)
    with pytest.raises(ValueError, match=field):
        GanTrainer(gen, dis, cfg, device=torch.device("cpu"))


def test_cli_override_reaches_the_knobs():
    cfg = GanConfig().apply_overrides(
        ["model.dis_dropout=0.25", "model.dis_input_noise_std=0.1"])
    assert cfg.model.dis_dropout == 0.25
    assert cfg.model.dis_input_noise_std == 0.1


# -------------------------------------------------------------- trainer
def _mlp_trainer():
    cfg = preset("mlp_tabular_cpu")
    cfg.train.use_gpu = False
    cfg.model.dis_dropout = 0.3
    cfg.model.dis_input_noise_std = 0.05
    gen, dis = build_mlp_gan(cfg, hidden=16)
    return GanTrainer(gen, dis, cfg, device=torch.device("cpu")), cfg


def test_trainer_same_seed_same_losses():
    x = torch.rand(8, 64)
    runs = []
    for _ in range(2):
        tr, _ = _mlp_trainer()
        runs.append([tr.step(x) for _ in range(3)])
    for a, b in zip(*runs):
        assert float(a["loss_d"]) == float(b["loss_d"])
        assert float(a["loss_g"]) == float(b["loss_g"])
    # 2 D forwards per D pass + 1 per G pass, per step
    assert tr.dis.get_layer("d_drop_feat").calls == 3 * 3


def test_trainer_save_resume_carries_the_counters(tmp_path):
    x = torch.rand(8, 64)
    tr, _ = _mlp_trainer()
    for _ in range(2):
        tr.step(x)
    tr.save(tmp_path)
    z_stream = tr._g.get_state()     # the z generator is not checkpointed
    ref = tr.step(x)                 # step 3, uninterrupted

    state = torch.load(tmp_path / "trainer_state.pt", weights_only=True)
    assert state["rng"] == {"dis/d_noise_in": 6, "dis/d_drop_1": 6,
                            "dis/d_drop_feat": 6}

    tr2, _ = _mlp_trainer()
    ident = [id(layer.rng_state) for _, layer in tr2._stochastic_layers()]
    assert tr2.resume(tmp_path)
    assert [id(layer.rng_state) for _, layer in tr2._stochastic_layers()] \
        == ident                     # written back in place
    assert tr2.dis.get_layer("d_drop_1").calls == 6
    tr2._labels(8)                   # same seed -> same one-shot soft labels
    tr2._g.set_state(z_stream)
    out = tr2.step(x)
    assert float(out["loss_d"]) == float(ref["loss_d"])
    assert float(out["loss_g"]) == float(ref["loss_g"])
    assert torch.equal(tr2.dis.params_flat(), tr.dis.params_flat())

    # without the counters the masks of step 3 differ and so does the loss
    tr3, _ = _mlp_trainer()
    assert tr3.resume(tmp_path)
    for _, layer in tr3._stochastic_layers():
        layer.set_calls(0)
    tr3._labels(8)
    tr3._g.set_state(z_stream)
    assert float(tr3.step(x)["loss_d"]) != float(ref["loss_d"])


def test_resume_without_rng_key_or_layers(tmp_path):
    # a model without stochastic layers writes no key and resumes as before
    cfg = preset("mlp_tabular_cpu")
    cfg.train.use_gpu = False
    gen, dis = build_mlp_gan(cfg, hidden=16)
    tr = GanTrainer(gen, dis, cfg, device=torch.device("cpu"))
    tr.step(torch.rand(8, 64))
    tr.save(tmp_path)
    state = torch.load(tmp_path / "trainer_state.pt", weights_only=True)
    assert "rng" not in state
    # a checkpoint without the key resumes into a model that has the layers
    tr2, _ = _mlp_trainer()
    tr2.step(torch.rand(8, 64))
    tr2.save(tmp_path / "b")
    st = torch.load(tmp_path / "b" / "trainer_state.pt", weights_only=True)
    del st["rng"]
    torch.save(st, tmp_path / "b" / "trainer_state.pt")
    tr3, _ = _mlp_trainer()
    assert tr3.resume(tmp_path / "b")
    assert tr3.dis.get_layer("d_drop_1").calls == 0
