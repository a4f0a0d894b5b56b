"""CPU call trace of the gpu_ops router.

gpu_ops decides which extension entry points run for every conv, convT,
dense and BN call, and with which packs, pads and fused epilogues.  This
module pins that routing without a GPU: a recording stub stands in for the
_C extension (each method returns zero tensors of the shape, dtype and list
length the real binding returns), gpu_ops is driven with CPU tensors, and
the recorded call sequence is compared with tests/golden/gpu_ops_routing.json.

Every case runs its op twice on the same parameters; the second pass must
not rebuild a weight pack (no second fp8_quantize of a weight).

Regenerate the golden file (only for a deliberate routing change) with
    GDLJ_ROUTING_REGEN=1 pytest tests/test_gpu_ops_routing.py
"""

import json
import os
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from gan_deeplearning4j_amd.ops import backend, gpu_ops
from test_ext_surface import PUBLIC_NAMES

GOLDEN = Path(__file__).parent / "golden" / "gpu_ops_routing.json"
REGEN = os.environ.get("GDLJ_ROUTING_REGEN") == "1"

ROUTING_GATES = ("GDLJ_DGRAD_DIRECT", "GDLJ_NO_ACT_FUSE", "GDLJ_SMALLC_COL",
                 "GDLJ_FP8_BWD", "GDLJ_FP8_DELAYED", "GDLJ_FP8_CONVT")

REQUIRED_NAMES = [
    "conv_fwd_implicit", "conv_fwd_implicit_fp8", "im2col", "gemm_tn",
    "gemm_tn_stats", "gemm_tn_fp8", "gemm_nt", "gemm_nt_implicit",
    "conv_parity_implicit", "conv_dgrad_direct", "conv_transpose_fwd_direct",
    "col2im", "col2im_dact", "col2im_stats", "act_bwd", "act_bwd_bias",
    "col_sum", "fp8_quantize", "fp8_quantize_delayed", "bn_fwd_train",
    "bn_fwd_train_pre", "bn_fwd_eval", "bn_bwd", "bn_bwd_act",
]

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.uint8: "u8",
       torch.int64: "i64", torch.int32: "i32"}


def _desc(a):
    """Tensor -> 'dtype[shape]', list -> 'listN[...]', scalar/None as is."""
    if isinstance(a, torch.Tensor):
        s = _DT[a.dtype] + json.dumps(list(a.shape), separators=(",", ":"))
        if a.dtype == torch.int64:      # conv gather dims: values matter
            s += "=" + json.dumps(a.tolist(), separators=(",", ":"))
        return s
    if isinstance(a, (list, tuple)):    # length and what it holds
        return "list%d[%s]" % (len(a), ",".join(_desc(e) for e in a))
    return a


def _out_desc(t):
    if t is None:
        return None
    return "%s%s/%s" % (_DT[t.dtype],
                        json.dumps(list(t.shape), separators=(",", ":")),
                        json.dumps(list(t.stride()), separators=(",", ":")))


def _z(shape, dtype):
    return torch.zeros([int(s) for s in shape], dtype=dtype)


def _bf16c(*ts):
    for t in ts:
        assert t.dtype == BF16 and t.is_contiguous(), (t.dtype, t.stride())


def _f32c(*ts):
    for t in ts:
        assert t is None or (t.dtype == F32 and t.is_contiguous())


class StubExt:
    """Recording stand-in for _C.  Shapes, dtypes and list lengths follow
    ext.cpp; the cheap argument checks of the bindings are kept so a wrong
    route fails here as it would on the device."""

    def __init__(self):
        self.trace = []
        self.direct_eligible = True

    def _rec(self, name, *args):
        self.trace.append(json.dumps([name] + [_desc(a) for a in args],
                                     separators=(",", ":")))

    # ------------------------------------------------------------- GEMM
    def gemm_tn(self, A, B, bias, act, slope, out_f32):
        self._rec("gemm_tn", A, B, bias, act, slope, out_f32)
        _bf16c(A, B)
        _f32c(bias)
        assert B.shape[1] == A.shape[1] and A.shape[1] % 64 == 0
        assert bias is None or bias.numel() == B.shape[0]
        return _z((A.shape[0], B.shape[0]), F32 if out_f32 else BF16)

    def gemm_tn_stats(self, A, B, bias, act, slope):
        self._rec("gemm_tn_stats", A, B, bias, act, slope)
        _bf16c(A, B)
        _f32c(bias)
        n = B.shape[0]
        assert B.shape[1] == A.shape[1] and A.shape[1] % 64 == 0
        assert n % 8 == 0
        return [_z((A.shape[0], n), BF16), _z((n,), F32), _z((n,), F32)]

    def gemm_nt(self, A, B, splitk, zero_page):
        self._rec("gemm_nt", A, B, splitk, zero_page)
        _bf16c(A, B)
        assert A.shape[0] == B.shape[0]
        assert A.shape[1] % 8 == 0 and B.shape[1] % 8 == 0
        return _z((A.shape[1], B.shape[1]), F32)

    def gemm_nt_implicit(self, A, B, gmode, Mdim, Ndim, Kdim, img_dims,
                         splitk, zero_page):
        self._rec("gemm_nt_implicit", A, B, gmode, Mdim, Ndim, Kdim,
                  img_dims, splitk, zero_page)
        _bf16c(A, B)
        assert img_dims.numel() in (10, 11)
        return _z((Mdim, Ndim), F32)

    def gemm_tn_fp8(self, Aq, Bq, inv_qa, inv_qb, bias, act, slope):
        self._rec("gemm_tn_fp8", Aq, Bq, inv_qa, inv_qb, bias, act, slope)
        assert Aq.dtype == U8 and Aq.is_contiguous()
        assert Bq.dtype == U8 and Bq.is_contiguous()
        assert Aq.shape[1] == Bq.shape[1] and Aq.shape[1] % 128 == 0
        _f32c(inv_qa, inv_qb, bias)
        return _z((Aq.shape[0], Bq.shape[0]), BF16)

    # ------------------------------------------------------------- conv
    def conv_fwd_implicit(self, x, Wp, bias, zero_page, Nb, H, W, C, Ho, Wo,
                          R, S, stride, pad, act, slope, mode, want_stats):
        self._rec("conv_fwd_implicit", x, Wp, bias, zero_page, Nb, H, W, C,
                  Ho, Wo, R, S, stride, pad, act, slope, mode, want_stats)
        _bf16c(x, Wp)
        _f32c(bias)
        assert C % 8 == 0 and x.numel() == Nb * H * W * C
        kout = Wp.shape[0]
        y = _z((Nb * Ho * Wo, kout), BF16)
        if want_stats and kout % 8 == 0:
            return [y, _z((kout,), F32), _z((kout,), F32)]
        return [y]

    def conv_fwd_implicit_fp8(self, xq, wq, bias, inv_qx, inv_qw, zero_page,
                              Nb, H, W, C, Ho, Wo, R, S, stride, pad, act,
                              slope, mode):
        self._rec("conv_fwd_implicit_fp8", xq, wq, bias, inv_qx, inv_qw,
                  zero_page, Nb, H, W, C, Ho, Wo, R, S, stride, pad, act,
                  slope, mode)
        assert xq.dtype == U8 and xq.is_contiguous()
        assert wq.dtype == U8 and wq.is_contiguous()
        assert C % 16 == 0 and wq.shape[1] % 128 == 0
        assert zero_page.dtype == U8 and zero_page.numel() == 32
        _f32c(inv_qx, inv_qw, bias)
        return _z((Nb * Ho * Wo, wq.shape[0]), BF16)

    def conv_parity_implicit(self, img, wcls, bias, zero_page, Nb, Hs, Ws,
                             Cs, oHd, oWd, Nout, R, S, stride, pad, act,
                             slope):
        self._rec("conv_parity_implicit", img, wcls, bias, zero_page, Nb,
                  Hs, Ws, Cs, oHd, oWd, Nout, R, S, stride, pad, act, slope)
        _bf16c(img, *wcls)
        _f32c(bias)
        assert Cs % 8 == 0 and len(wcls) == stride * stride
        assert all(w.shape[0] == Nout for w in wcls)
        return _z((Nb * oHd * oWd, Nout), BF16)

    def im2col(self, x, N, H, W, C, Ho, Wo, R, S, stride, pad, kpad):
        self._rec("im2col", x, N, H, W, C, Ho, Wo, R, S, stride, pad, kpad)
        _bf16c(x)
        return _z((N * Ho * Wo, kpad), BF16)

    def col2im(self, dcol, N, H, W, C, Ho, Wo, R, S, stride, pad, kpad,
               bias, act, slope):
        self._rec("col2im", dcol, N, H, W, C, Ho, Wo, R, S, stride, pad,
                  kpad, bias, act, slope)
        _bf16c(dcol)
        _f32c(bias)
        return _z((N, H, W, C), BF16)

    def col2im_dact(self, dcol, N, H, W, C, Ho, Wo, R, S, stride, pad, kpad,
                    y0, act, slope, want_bias):
        self._rec("col2im_dact", dcol, N, H, W, C, Ho, Wo, R, S, stride,
                  pad, kpad, y0, act, slope, want_bias)
        _bf16c(dcol, y0)
        assert C % 8 == 0 and kpad % 8 == 0 and y0.numel() == N * H * W * C
        return [_z((N, H, W, C), BF16), _z((C if want_bias else 0,), F32)]

    def col2im_stats(self, dcol, N, H, W, C, Ho, Wo, R, S, stride, pad,
                     kpad, bias, act, slope):
        self._rec("col2im_stats", dcol, N, H, W, C, Ho, Wo, R, S, stride,
                  pad, kpad, bias, act, slope)
        _bf16c(dcol)
        _f32c(bias)
        assert C % 8 == 0 and kpad % 8 == 0
        return [_z((N, H, W, C), BF16), _z((C,), F32), _z((C,), F32)]

    def conv_dgrad_direct(self, dpre, wt, y0, zero_page, N, H, W, C8, Ho,
                          Wo, R, S, stride, pad, act, slope, want_bias):
        self._rec("conv_dgrad_direct", dpre, wt, y0, zero_page, N, H, W, C8,
                  Ho, Wo, R, S, stride, pad, act, slope, want_bias)
        _bf16c(dpre, wt)
        if not self.direct_eligible:
            return []
        assert dpre.shape[0] == N * Ho * Wo and wt.shape[0] >= R * S * C8
        out = [_z((N, H, W, C8), BF16)]
        if y0 is not None:
            _bf16c(y0)
            assert y0.numel() == N * H * W * C8
            if want_bias:
                out.append(_z((C8,), F32))
        return out

    def conv_transpose_fwd_direct(self, x2d, w2a, bias, zero_page, N, Hi,
                                  Wi, Ho, Wo, Co8, R, S, stride, pad, act,
                                  slope, want_stats):
        self._rec("conv_transpose_fwd_direct", x2d, w2a, bias, zero_page, N,
                  Hi, Wi, Ho, Wo, Co8, R, S, stride, pad, act, slope,
                  want_stats)
        _bf16c(x2d, w2a)
        if not self.direct_eligible:
            return []
        assert x2d.shape[0] == N * Hi * Wi and w2a.shape[0] >= R * S * Co8
        _f32c(bias)
        assert bias is None or bias.numel() >= Co8
        out = [_z((N, Ho, Wo, Co8), BF16)]
        if want_stats:
            out += [_z((Co8,), F32), _z((Co8,), F32)]
        return out

    # ------------------------------------------------------ elementwise
    def act_bwd(self, dy, y, act, slope):
        self._rec("act_bwd", dy, y, act, slope)
        _bf16c(dy, y)
        return torch.zeros_like(dy)

    def act_bwd_bias(self, dy, y, act, slope):
        self._rec("act_bwd_bias", dy, y, act, slope)
        _bf16c(dy)
        assert dy.shape[1] % 8 == 0
        if act != 0:
            _bf16c(y)
        return [torch.zeros_like(dy), _z((dy.shape[1],), F32)]

    def col_sum(self, a):
        self._rec("col_sum", a)
        _bf16c(a)
        return _z((a.shape[1],), F32)

    # --------------------------------------------------------------- BN
    def bn_fwd_train(self, x, gamma, beta, rm, rv, momentum, eps):
        self._rec("bn_fwd_train", x, gamma, beta, rm, rv, momentum, eps)
        _bf16c(x)
        _f32c(gamma)
        c = x.shape[-1]
        return [torch.zeros_like(x), _z((c,), F32), _z((c,), F32)]

    def bn_fwd_train_pre(self, x, ssum, ssq, gamma, beta, rm, rv, momentum,
                         eps):
        self._rec("bn_fwd_train_pre", x, ssum, ssq, gamma, beta, rm, rv,
                  momentum, eps)
        _bf16c(x)
        _f32c(ssum, ssq)
        c = x.shape[-1]
        return [torch.zeros_like(x), _z((c,), F32), _z((c,), F32)]

    def bn_fwd_eval(self, x, gamma, beta, rm, rv, eps):
        self._rec("bn_fwd_eval", x, gamma, beta, rm, rv, eps)
        _bf16c(x)
        return torch.zeros_like(x)

    def bn_bwd(self, x, dy, mean, istd, gamma):
        self._rec("bn_bwd", x, dy, mean, istd, gamma)
        _bf16c(x, dy)
        c = x.shape[-1]
        return [torch.zeros_like(x), _z((c,), F32), _z((c,), F32)]

    def bn_bwd_act(self, x, dy, mean, istd, gamma, act, slope, want_bias):
        self._rec("bn_bwd_act", x, dy, mean, istd, gamma, act, slope,
                  want_bias)
        _bf16c(x, dy)
        c = x.shape[-1]
        assert c % 8 == 0
        return [torch.zeros_like(x), _z((c,), F32), _z((c,), F32),
                _z((c if want_bias else 0,), F32)]

    # -------------------------------------------------------------- fp8
    def fp8_quantize(self, x):
        self._rec("fp8_quantize", x)
        _bf16c(x)
        assert x.numel() % 8 == 0
        return [_z(x.shape, U8), _z((1,), F32), _z((1,), F32)]

    def fp8_quantize_delayed(self, x, scale, inv, amax, first):
        self._rec("fp8_quantize_delayed", x, scale, inv, amax, first)
        _bf16c(x)
        assert x.numel() % 8 == 0
        return _z(x.shape, U8)


def test_stub_is_a_subset_of_the_extension_surface():
    names = {n for n in vars(StubExt) if not n.startswith("_")}
    assert names <= set(PUBLIC_NAMES), names - set(PUBLIC_NAMES)
    assert set(REQUIRED_NAMES) <= names


# --------------------------------------------------------------- the cases
def _t(*shape, grad=True, dtype=F32, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    t = (torch.randn(*shape, generator=g) * 0.5).to(dtype)
    return t.requires_grad_(grad)


class Case:
    """setup() -> params (built once); run(params) -> named outputs.  The
    runner calls run twice and collects the params' gradients after each."""

    def __init__(self, setup, run, env=None, fp8=False, parity=False,
                 direct=True):
        self.setup, self.run = setup, run
        self.env, self.fp8, self.parity, self.direct = (env or {}, fp8,
                                                        parity, direct)


CASES = {}


def _conv(C=16, Kout=16, k=4, stride=2, pad=1, act="identity", bias=True,
          dtype=F32, x_grad=True, w_grad=True, emit_stats=False,
          prev_act=None, H=8):
    def setup():
        return SimpleNamespace(
            x=_t(2, C, H, H, grad=x_grad, dtype=dtype),
            w=_t(Kout, C, k, k, grad=w_grad, dtype=dtype),
            b=_t(Kout, dtype=dtype) if bias else None)

    def run(p):
        y = gpu_ops.conv2d(p.x, p.w, p.b, stride, pad, act, 0.2, emit_stats,
                           prev_act)
        y.sum().backward()
        return {"y": y}

    return setup, run


def _convt(Cin=16, Cout=16, k=4, stride=2, pad=1, act="identity", bias=True,
           dtype=F32, emit_stats=False, H=4, backward=True):
    def setup():
        return SimpleNamespace(
            x=_t(2, Cin, H, H, dtype=dtype),
            w=_t(Cin, Cout, k, k, dtype=dtype),
            b=_t(Cout, dtype=dtype) if bias else None)

    def run(p):
        y = gpu_ops.conv_transpose2d(p.x, p.w, p.b, stride, pad, act, 0.2,
                                     emit_stats)
        if backward:
            y.sum().backward()
        return {"y": y}

    return setup, run


def _add(name, setup_run, **kw):
    assert name not in CASES, name
    CASES[name] = Case(*setup_run, **kw)


def _add_strided(name, **conv_kw):
    """Each strided conv: direct eligible / ineligible / gated off, and
    with the act-fusion kill switch."""
    _add(name + "-direct", _conv(**conv_kw))
    _add(name + "-ineligible", _conv(**conv_kw), direct=False)
    _add(name + "-gate0", _conv(**conv_kw), env={"GDLJ_DGRAD_DIRECT": "0"})
    _add(name + "-noactfuse", _conv(**conv_kw),
         env={"GDLJ_NO_ACT_FUSE": "1"})
    if conv_kw.get("prev_act") is not None:
        _add(name + "-noactfuse-ineligible", _conv(**conv_kw),
             env={"GDLJ_NO_ACT_FUSE": "1"}, direct=False)


# conv2d
_add("conv-s1-3x3-c16-k32-lrelu",
     _conv(C=16, Kout=32, k=3, stride=1, pad=1, act="lrelu"))
_add("conv-s1-3x3-c16-k32-stats",
     _conv(C=16, Kout=32, k=3, stride=1, pad=1, act="lrelu",
           emit_stats=True))
_add("conv-s1-k3-tanh", _conv(C=16, Kout=3, k=3, stride=1, pad=1,
                              act="tanh"))
_add("conv-s1-c3-bf16", _conv(C=3, Kout=16, k=3, stride=1, pad=1,
                              dtype=BF16))
_add_strided("conv-s2-c3-k16-bf16", C=3, Kout=16, dtype=BF16)
_add("conv-s2-c3-k16-f32-direct", _conv(C=3, Kout=16, act="lrelu"))
_add("conv-s2-c3-k16-f32-ineligible", _conv(C=3, Kout=16, act="lrelu"),
     direct=False)
_add_strided("conv-s2-c16-k24", C=16, Kout=24, act="lrelu")
_add_strided("conv-s2-c16-k3", C=16, Kout=3, act="tanh")
_add_strided("conv-s2-nobias", bias=False, act="lrelu")
_add("conv-s2-stats", _conv(emit_stats=True))
_add_strided("conv-s2-x-nograd", x_grad=False, act="lrelu")
_add_strided("conv-s2-w-nograd", w_grad=False, act="lrelu")
_add_strided("conv-s2-prevact-bias", prev_act=(3, 0.2, True))
_add_strided("conv-s2-prevact-nobias", prev_act=(3, 0.2, False))
_add_strided("conv-s2-c3-prevact-dropped", C=3, dtype=BF16,
             prev_act=(3, 0.2, True))


# chains
def _chain_convt_conv(dtype=BF16):
    def setup():
        return SimpleNamespace(
            z=_t(2, 16, 4, 4, dtype=dtype),
            wt=_t(16, 3, 4, 4, dtype=dtype), bt=_t(3, dtype=dtype),
            wc=_t(16, 3, 4, 4, dtype=dtype, seed=1),
            bc=_t(16, dtype=dtype, seed=1))

    def run(p):
        img = gpu_ops.conv_transpose2d(p.z, p.wt, p.bt, 2, 1, "tanh")
        y = gpu_ops.conv2d(img, p.wc, p.bc, 2, 1, "lrelu")
        y.sum().backward()
        return {"img": img, "y": y}

    return setup, run


def _chain_conv_conv():
    def setup():
        return SimpleNamespace(
            x=_t(2, 16, 8, 8), w1=_t(16, 16, 4, 4), b1=_t(16),
            w2=_t(24, 16, 4, 4, seed=1), b2=_t(24, seed=1))

    def run(p):
        h = gpu_ops.conv2d(p.x, p.w1, p.b1, 2, 1, "lrelu")
        y = gpu_ops.conv2d(h, p.w2, p.b2, 2, 1, "lrelu",
                           prev_act=(3, 0.2, True))
        y.sum().backward()
        return {"h": h, "y": y}

    return setup, run


def _chain_bn(producer, emit_stats=False):
    def setup():
        p = SimpleNamespace(g=_t(16, seed=2), be=_t(16, seed=3),
                            rm=torch.zeros(16), rv=torch.ones(16))
        if producer == "conv":
            p.x, p.w, p.b = _t(2, 16, 8, 8), _t(16, 16, 4, 4), _t(16)
        else:
            p.x, p.w, p.b = _t(4, 64), _t(16, 64), _t(16)
        return p

    def run(p):
        if producer == "conv":
            h = gpu_ops.conv2d(p.x, p.w, p.b, 2, 1, "lrelu", 0.2,
                               emit_stats)
            bwd_act = (3, 0.2, True)
        else:
            h = gpu_ops.linear(p.x, p.w, p.b, "tanh", 0.2, emit_stats)
            bwd_act = (1, 0.2, True)
        y = gpu_ops.batch_norm(h, p.g, p.be, p.rm, p.rv, True,
                               bwd_act=bwd_act)
        y.sum().backward()
        return {"h": h, "y": y}

    return setup, run


for _v, _kw in (("direct", {}), ("ineligible", {"direct": False}),
                ("gate0", {"env": {"GDLJ_DGRAD_DIRECT": "0"}}),
                ("noactfuse", {"env": {"GDLJ_NO_ACT_FUSE": "1"}})):
    _add("chain-convt-conv-bf16-" + _v, _chain_convt_conv(), **_kw)
    if _v in ("direct", "ineligible"):
        _add("chain-conv-conv-prevact-" + _v, _chain_conv_conv(), **_kw)
_add("chain-convt-conv-f32", _chain_convt_conv(F32))
_add("chain-conv-bn-bwdact", _chain_bn("conv"))
_add("chain-conv-bn-bwdact-noactfuse", _chain_bn("conv"),
     env={"GDLJ_NO_ACT_FUSE": "1"})
_add("chain-conv-stats-bn-bwdact", _chain_bn("conv", emit_stats=True))
_add("chain-linear-bn-bwdact", _chain_bn("linear"))
_add("chain-linear-stats-bn-bwdact", _chain_bn("linear", emit_stats=True))
_add("chain-linear-bn-bwdact-noactfuse", _chain_bn("linear"),
     env={"GDLJ_NO_ACT_FUSE": "1"})

# conv_transpose2d
_add("convt-s1", _convt(k=3, stride=1, pad=1, act="lrelu"))
_add("convt-s1-stats", _convt(k=3, stride=1, pad=1, emit_stats=True))
for _act in ("identity", "tanh", "lrelu"):
    for _co in (16, 3):
        _n = "convt-s2-co%d-%s" % (_co, _act)
        _add(_n + "-direct", _convt(Cout=_co, act=_act))
        _add(_n + "-ineligible", _convt(Cout=_co, act=_act), direct=False)
_add("convt-s2-co3-tanh-bf16", _convt(Cout=3, act="tanh", dtype=BF16))
_add("convt-s2-gate0", _convt(act="lrelu"),
     env={"GDLJ_DGRAD_DIRECT": "0"})
_add("convt-s2-stats-direct", _convt(emit_stats=True))
_add("convt-s2-stats-ineligible", _convt(emit_stats=True), direct=False)
_add("convt-s2-co3-stats-direct", _convt(Cout=3, emit_stats=True))
_add("convt-s2-co3-stats-ineligible", _convt(Cout=3, emit_stats=True),
     direct=False)
_add("convt-s2-nobias", _convt(bias=False, act="lrelu"))
_add("convt-s2-nobias-ineligible", _convt(bias=False, act="lrelu"),
     direct=False)
_add("convt-s2-co3-nobias", _convt(Cout=3, bias=False, act="tanh"))
_add("convt-s2-fwd-only", _convt(backward=False))

# gates
_add("parity-conv", _conv(C=16, Kout=24, act="lrelu"), parity=True)
_add("parity-conv-c3-k3", _conv(C=3, Kout=3, dtype=BF16), parity=True)
_add("parity-convt", _convt(act="lrelu"), parity=True)
_add("parity-convt-co3", _convt(Cout=3, act="tanh"), parity=True)
_add("smallc-col-c16", _conv(C=16, Kout=16), env={"GDLJ_SMALLC_COL": "1"})
_add("smallc-col-c3-stats", _conv(C=3, Kout=16, emit_stats=True),
     env={"GDLJ_SMALLC_COL": "1"})
_add("smallc-col-c3-k3-stats", _conv(C=3, Kout=3, emit_stats=True),
     env={"GDLJ_SMALLC_COL": "1"})
_add("smallc-col-c32-not-taken", _conv(C=32, Kout=16),
     env={"GDLJ_SMALLC_COL": "1"})
_add("fp8-conv-c16", _conv(C=16, Kout=32, act="lrelu"), fp8=True)
_add("fp8-conv-c8-not-taken", _conv(C=8, Kout=32, act="lrelu"), fp8=True)
_add("fp8-conv-s1-c32", _conv(C=32, Kout=16, k=3, stride=1, pad=1),
     fp8=True)
for _s in (1, 2):
    _geo = (dict(k=3, stride=1, pad=1) if _s == 1
            else dict(k=4, stride=2, pad=1))
    _add("fp8-bwd-conv-s%d" % _s, _conv(C=16, Kout=32, act="lrelu", **_geo),
         fp8=True, env={"GDLJ_FP8_BWD": "1"})
    _add("fp8-bwd-conv-s%d-k24-bf16-only" % _s,
         _conv(C=16, Kout=24, **_geo), fp8=True, env={"GDLJ_FP8_BWD": "1"})
    _add("fp8-bwd-convt-s%d" % _s, _convt(Cin=16, Cout=32, **_geo),
         fp8=True, env={"GDLJ_FP8_BWD": "1"})
    if _s == 2:
        _add("fp8-bwd-without-fp8-conv", _conv(C=16, Kout=32, **_geo),
             env={"GDLJ_FP8_BWD": "1"})
    for _g in (None, "0", "1"):
        _env = {} if _g is None else {"GDLJ_FP8_CONVT": _g}
        _n = "fp8-convt-s%d-gate-%s" % (_s, "unset" if _g is None else _g)
        _add(_n, _convt(Cin=16, Cout=16, act="lrelu", **_geo), fp8=True,
             env=_env)
        if _g == "1":
            _add(_n + "-fp8-conv-off", _convt(Cin=16, Cout=16, **_geo),
                 env=_env)
_add("fp8-convt-s1-stats-stays-bf16",
     _convt(k=3, stride=1, pad=1, emit_stats=True), fp8=True)
_add("fp8-convt-s2-gate-1-ineligible", _convt(act="lrelu"), fp8=True,
     env={"GDLJ_FP8_CONVT": "1"}, direct=False)
_add("fp8-delayed-0-conv", _conv(C=16, Kout=32, act="lrelu"), fp8=True,
     env={"GDLJ_FP8_DELAYED": "0"})
_add("fp8-delayed-0-bwd-s1", _conv(C=16, Kout=32, k=3, stride=1, pad=1),
     fp8=True, env={"GDLJ_FP8_DELAYED": "0", "GDLJ_FP8_BWD": "1"})
_add("fp8-delayed-0-bwd-s2", _conv(C=16, Kout=32), fp8=True,
     env={"GDLJ_FP8_DELAYED": "0", "GDLJ_FP8_BWD": "1"})


# linear
def _linear(nin, nout, act="identity", emit_stats=False, lead=(4,),
            bias=True, x_grad=True):
    def setup():
        return SimpleNamespace(x=_t(*lead, nin, grad=x_grad),
                               w=_t(nout, nin),
                               b=_t(nout) if bias else None)

    def run(p):
        y = gpu_ops.linear(p.x, p.w, p.b, act, 0.2, emit_stats)
        y.sum().backward()
        return {"y": y}

    return setup, run


_add("linear-100-20-lrelu", _linear(100, 20, "lrelu"))
_add("linear-100-20-identity", _linear(100, 20))
_add("linear-64-32-stats", _linear(64, 32, "tanh", emit_stats=True))
_add("linear-100-20-stats-not-fused", _linear(100, 20, emit_stats=True))
_add("linear-3d", _linear(64, 32, "lrelu", lead=(2, 3)))
_add("linear-nobias-x-nograd", _linear(64, 32, "lrelu", bias=False,
                                       x_grad=False))


# batch_norm
def _bn(shape, training=True, bwd_act=None, deposit=False):
    c = shape[1]

    def setup():
        return SimpleNamespace(x=_t(*shape), g=_t(c, seed=2),
                               be=_t(c, seed=3), rm=torch.zeros(c),
                               rv=torch.ones(c))

    def run(p):
        x = p.x
        if deposit:
            x = x.to(BF16)
            gpu_ops.deposit_bn_stats(x, (torch.zeros(c), torch.ones(c)))
        y = gpu_ops.batch_norm(x, p.g, p.be, p.rm, p.rv, training,
                               bwd_act=bwd_act)
        if training:
            y.sum().backward()
        return {"y": y}

    return setup, run


_add("bn-2d", _bn((4, 16)))
_add("bn-4d", _bn((2, 16, 4, 4)))
_add("bn-4d-c12", _bn((2, 12, 4, 4)))
_add("bn-deposited-stats", _bn((4, 16), deposit=True))
_add("bn-bwdact-c12-dropped", _bn((4, 12), bwd_act=(3, 0.2, True)))
_add("bn-bwdact-c16-nobias", _bn((4, 16), bwd_act=(3, 0.2, False)))
_add("bn-eval-2d", _bn((4, 16), training=False))
_add("bn-eval-4d", _bn((2, 16, 4, 4), training=False))


# -------------------------------------------------------------- the runner
def run_case(case):
    """Trace of one case: {"pass1": [...], "pass2": [...] | "same",
    "out": {...}, "chan": [side channels left holding entries]}."""
    stub = StubExt()
    stub.direct_eligible = case.direct
    saved = (backend._ext, backend._tried, gpu_ops.FP8_CONV)
    with pytest.MonkeyPatch.context() as mp:
        for k in ROUTING_GATES:
            mp.delenv(k, raising=False)
        for k, v in case.env.items():
            mp.setenv(k, v)
        mp.setattr(gpu_ops, "PARITY_STRIDED", case.parity)
        mp.setattr(backend, "_ext", stub)
        mp.setattr(backend, "_tried", True)
        chans = (gpu_ops._bn_stats_chan, gpu_ops._act_fused_chan,
                 gpu_ops._chan_pad)
        for d in chans + (gpu_ops._dims_cache,):
            d.clear()
        try:
            gpu_ops.set_fp8_conv(case.fp8)
            params = case.setup()
            passes = []
            for _ in range(2):
                stub.trace = []
                outs = case.run(params)
                rec = {k: _out_desc(v) for k, v in outs.items()}
                for k, v in vars(params).items():
                    if isinstance(v, torch.Tensor) and v.requires_grad:
                        rec["d" + k] = _out_desc(v.grad)
                        v.grad = None
                passes.append((stub.trace, rec))
            # presence, not counts: entries are keyed by data_ptr, so how
            # many survive two passes depends on allocator reuse
            names = ("bn_stats", "act_fused", "chan_pad")
            chan = [n for n, d in zip(names, chans) if d]
        finally:
            gpu_ops.set_fp8_conv(saved[2])
            for d in chans + (gpu_ops._dims_cache,):
                d.clear()
    assert (backend._ext, backend._tried) == saved[:2]
    (t1, o1), (t2, o2) = passes
    assert o1 == o2, "outputs differ between the two passes"
    return {"pass1": t1, "pass2": "same" if t2 == t1 else t2, "out": o1,
            "chan": chan}


def _name(line):
    return json.loads(line)[0]


def _lines(golden_pass):
    """Golden calls are JSON arrays; compare as text so that true and 1,
    or 0 and 0.0, stay distinct."""
    if isinstance(golden_pass, str):
        return golden_pass
    return [json.dumps(c, separators=(",", ":")) for c in golden_pass]


def _count(trace, *names):
    return sum(_name(line) in names for line in trace)


def _dump(traces):
    """One call per line; the rest of the layout is fixed so the file
    diffs line by line."""
    out = ["{"]
    for i, (name, t) in enumerate(traces.items()):
        out.append(json.dumps(name) + ": {")
        for key in ("pass1", "pass2"):
            if isinstance(t[key], str):
                out.append(json.dumps(key) + ": " + json.dumps(t[key]) + ",")
                continue
            out.append(json.dumps(key) + ": [")
            out += [line + ("," if j + 1 < len(t[key]) else "")
                    for j, line in enumerate(t[key])]
            out.append("],")
        out.append('"out": ' + json.dumps(t["out"], separators=(",", ":"))
                   + ",")
        out.append('"chan": ' + json.dumps(t["chan"], separators=(",", ":")))
        out.append("}" + ("," if i + 1 < len(traces) else ""))
    out.append("}")
    return "\n".join(out) + "\n"


_golden_cache = None


def _golden():
    global _golden_cache
    if _golden_cache is None:
        if REGEN:
            GOLDEN.write_text(_dump({n: run_case(c)
                                     for n, c in CASES.items()}))
        _golden_cache = json.loads(GOLDEN.read_text())
    return _golden_cache


@pytest.mark.parametrize("name", list(CASES))
def test_routing_matches_golden(name):
    got = run_case(CASES[name])
    p1 = got["pass1"]
    p2 = p1 if got["pass2"] == "same" else got["pass2"]
    assert p1 and p2, "empty trace"
    # the second pass rebuilds no pack: every quantize left in it is the
    # single activation operand of an fp8 GEMM, none is a weight's
    quant = ("fp8_quantize", "fp8_quantize_delayed")
    fp8_gemm = ("conv_fwd_implicit_fp8", "gemm_tn_fp8")
    assert _count(p2, *quant) == _count(p2, *fp8_gemm)
    assert _count(p1, "fp8_quantize") >= _count(p2, "fp8_quantize")
    if _count(p1, *fp8_gemm):
        assert _count(p1, "fp8_quantize") > _count(p2, "fp8_quantize")
    if CASES[name].env.get("GDLJ_FP8_DELAYED") != "0":
        assert _count(p2, "fp8_quantize") == 0
    want = _golden()[name]
    assert got["pass1"] == _lines(want["pass1"])
    assert got["pass2"] == _lines(want["pass2"])
    assert got["out"] == want["out"]
    assert got["chan"] == want["chan"]


def test_golden_has_exactly_the_cases():
    assert list(_golden()) == list(CASES)
    assert GOLDEN.stat().st_size < 100 * 1024


def test_golden_reaches_every_required_entry_point():
    seen = set()
    for t in _golden().values():
        assert t["pass1"], "empty trace"
        for key in ("pass1", "pass2"):
            if not isinstance(t[key], str):
                seen.update(call[0] for call in t[key])
    missing = [n for n in REQUIRED_NAMES if n not in seen]
    assert not missing, missing
