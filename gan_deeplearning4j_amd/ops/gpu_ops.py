"""GPU op layer: custom autograd Functions over the gfx950 HIP kernels.

Layout strategy (MI355X-first): convolution activations live in NHWC
physical layout (channels innermost) — the natural layout for MFMA
implicit-GEMM convs. Tensors stay logically NCHW; outputs are returned as
channels-last VIEWS of our NHWC buffers, so chains of conv/BN/pool ops
pass layout through with zero copies (only graph edges that leave the conv
world pay one permute-copy).

Contraction (K) dims are zero-padded to multiples of 64 to match the MFMA
GEMM tile (TN_BK); im2col emits padded K directly, dense inputs/weights are
padded with one small copy.

Every Function here raises if the _C extension is missing — on a GPU box
the HIP path is the only path (no silent eager fallback).

Which extension entry points a call reaches is pinned, without a GPU, by
tests/test_gpu_ops_routing.py.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from .backend import hip_ext, spectral_ext

ACT_CODES = {"identity": 0, None: 0, "tanh": 1, "sigmoid": 2, "lrelu": 3,
             "relu": 4}


# ===================================================================== gates
# Every GDLJ_* switch this module routes on, one predicate each. Defaults,
# when each is read and the measurement behind it: docs/KERNELS.md,
# "Environment gates".
def _gate(name: str) -> Optional[str]:
    return os.environ.get(name)


# Strided dgrad/convT-fwd algorithm choice: parity-decomposed gathered
# GEMMs vs dcol+col2im. Measured on DCGAN-64: dcol wins by ~4% (the
# parity gather re-reads the source once per tap, so traffic is a wash
# and the 4 launches add overhead); parity kept selectable for other
# shapes. Read at import; the routes read the attribute per call.
PARITY_STRIDED = _gate("GDLJ_PARITY") == "1"

# FP8 conv-forward mode (BASELINE config 4: DCGAN-128 fp8 MFMA path).
# When enabled, conv forwards with C % 16 == 0 quantize activations and
# weights to e4m3 (per-tensor dynamic scale) and run the fp8 MFMA implicit
# GEMM; backward stays bf16.
FP8_CONV = False


def set_fp8_conv(enabled: bool) -> None:
    global FP8_CONV
    FP8_CONV = bool(enabled)


def _dgrad_direct_on() -> bool:
    """Fused direct strided dgrad / convT forward (conv_dgrad_direct.hip),
    default on."""
    return _gate("GDLJ_DGRAD_DIRECT") != "0"


def _act_fuse_on() -> bool:
    """Producer act-backward fusion into the consumer's BN backward or
    col2im; GDLJ_NO_ACT_FUSE=1 is the kill switch."""
    return _gate("GDLJ_NO_ACT_FUSE") != "1"


def _smallc_col_on() -> bool:
    """Explicit im2col for C8 <= 16 conv forwards. MEASURED NEGATIVE,
    opt-in only (dcgan64 117.0k -> 114.4k, dcgan28 791k -> 765k): the
    hypothesis was that small-C gathers are TA-address-bound (a gathered
    16B chunk spans 2+ taps -> 64 scattered addresses per glds) and an
    explicit coalesced im2col + plain-TN GEMM would win; the col round
    trip costs more than the scattered addressing does."""
    return _gate("GDLJ_SMALLC_COL") == "1"


# fp8 backward (dgrad family) is implemented and numerics-tested but OFF
# by default (GDLJ_FP8_BWD=1 opts in): measured on DCGAN-128 at batches
# 512-2048, fp8 dgrad is 4-6% SLOWER end-to-end than bf16 dgrad — the
# dgrad GEMMs are K-thin (K = Cout <= 1024) and memory-bound on the
# C-write/A-read stream, so halving the A bytes saves less than the
# extra quantize pass (a full dy read + fp8 write) costs
# (profiles/fp8_bwd_ab.md). fp8 pays where MFMA rate is the bound: the
# K-deep forward gathers (on by default). wgrad stays bf16: the NT
# contraction reads both operands k(=np)-major, and glds cannot build
# the transposed fp8 LDS image (lane-linear dest; no tr16-style
# transpose read exists for 8-bit fragments at the 16x16x128 layout).
def _fp8_bwd_on() -> bool:
    return FP8_CONV and _gate("GDLJ_FP8_BWD") == "1"


def _fp8_delayed_on() -> bool:
    """Delayed fp8 scaling; GDLJ_FP8_DELAYED=0 falls back to exact
    per-call scaling."""
    return _gate("GDLJ_FP8_DELAYED") != "0"


# GDLJ_FP8_CONVT has three states. Unset: only the stride-1 convT forward
# runs fp8 (K = rsc, deep — fp8 pays). "0": no convT runs fp8. "1": the
# strided convT also takes the fp8 dcol GEMM, and for that skips the
# direct kernel (K = Cin <= 1024, thin and memory-bound: measured -2%
# end-to-end at dcgan128 b2048, profiles/fp8_bwd_ab.md).
def _fp8_convt_s1_on() -> bool:
    return FP8_CONV and _gate("GDLJ_FP8_CONVT") != "0"


def _fp8_convt_strided_on() -> bool:
    return FP8_CONV and _gate("GDLJ_FP8_CONVT") == "1"


# =================================================================== helpers
def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).contiguous()


def _pad_last(t: torch.Tensor, m: int) -> torch.Tensor:
    """Zero-pad the last dim to a multiple of m (contiguous result)."""
    k = t.shape[-1]
    kp = _rup(k, m)
    if kp == k:
        return t.contiguous()
    out = t.new_zeros(*t.shape[:-1], kp)
    out[..., :k] = t
    return out


def _pad_k(t: torch.Tensor) -> torch.Tensor:
    """Zero-pad the contraction (last) dim to the 64-deep MFMA tile."""
    return _pad_last(t, 64)


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    """[N,C,H,W] logical -> [N,H,W,C] bf16 contiguous (free if x is already
    a channels-last view from an upstream op). The cast happens BEFORE the
    permute-contiguous so a channels-last input never takes an NCHW
    round-trip copy."""
    return x.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()


def _as_nchw_view(y_nhwc: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] buffer -> logical [N,C,H,W] channels-last view (no copy)."""
    return y_nhwc.permute(0, 3, 1, 2)


def _splitk_for(m_tiles: int, n_tiles: int, kchunks: int) -> int:
    tiles = max(1, m_tiles * n_tiles)
    want = max(1, 512 // tiles)  # ~2 blocks per CU target (512-thread blocks)
    return int(min(want, kchunks, 512))


_zero_pages: dict = {}
_dims_cache: dict = {}

# side-channel for producer-fused BN statistics: the producing Function
# deposits (sum, sumsq) here keyed by the output tensor's data_ptr; the
# BatchNorm wrapper consumes (and clears) them. Entries are overwritten
# every producer call, so the dict stays O(#fused layers).
_bn_stats_chan: dict = {}


def deposit_bn_stats(t: torch.Tensor, stats) -> None:
    _bn_stats_chan[t.data_ptr()] = stats


def take_bn_stats(t: torch.Tensor):
    return _bn_stats_chan.pop(t.data_ptr(), None)


# Backward act-fusion side channel (consumer BatchNorm -> producer conv/
# dense): when BN is the sole consumer of a producer's activation output,
# BN's backward applies the activation backward INSIDE its apply kernel
# (the activation output is already in registers there) and reduces the
# producer's bias gradient on the way out, then deposits
# (act_code, n_cols, db) keyed by the grad tensor it returns. The
# producer's backward pops the entry by data_ptr (grads flow through
# view-only nodes, so the storage pointer is preserved) and skips its own
# act_bwd_bias pass — removing 3 full tensor streams per fused layer.
_act_fused_chan: dict = {}


def deposit_act_fused(t: torch.Tensor, payload) -> None:
    _act_fused_chan[t.data_ptr()] = payload


def take_act_fused(t: torch.Tensor):
    return _act_fused_chan.pop(t.data_ptr(), None)


# Channel-pad pass-through side channel: NHWC producers whose true channel
# count C is below the pad C8 (the 3-channel image boundary) return a
# trimmed [..., :C] VIEW and deposit the PADDED buffer here (pad channels
# provably zero: zero weight columns + tanh/identity epilogue). The next
# conv consumer takes the padded buffer directly instead of re-padding —
# removing a slow strided trim-copy AND a re-pad per boundary crossing.
# Entries hold the padded tensor (keeps its storage from allocator reuse,
# so a data_ptr key can never go stale); FIFO-capped so at most a few
# boundary buffers stay pinned. Peek semantics: the same fake batch is
# consumed by both the D-step and the G-step forward.
_chan_pad: dict = {}


def deposit_chan_pad(trimmed: torch.Tensor, padded: torch.Tensor) -> None:
    if len(_chan_pad) >= 4:
        _chan_pad.pop(next(iter(_chan_pad)))
    _chan_pad[trimmed.data_ptr()] = (padded, trimmed.numel())


def take_chan_pad(t: torch.Tensor, c8: int):
    ent = _chan_pad.get(t.data_ptr())
    if ent is None:
        return None
    p, numel = ent
    # the key (a base data_ptr) can also belong to a DIFFERENT view of
    # the same storage: require the consumer's logical element count and
    # batch to match the deposited trim exactly
    if (p.shape[-1] == c8 and p.shape[0] == t.shape[0]
            and t.numel() == numel):
        return p
    return None


def _trim_channels(th: torch.Tensor, c: int, as_view: bool) -> torch.Tensor:
    """NHWC [..., c8] buffer -> its first c channels (th itself when
    c8 == c). as_view: a [..., :c] view, with the padded buffer deposited
    for the next conv to take whole — the caller vouches that the pad
    channels are exact zeros; otherwise one contiguous trim-copy."""
    if th.shape[-1] != c:
        if as_view:
            padded, th = th, th[..., :c]
            deposit_chan_pad(th, padded)
        else:
            th = th[..., :c].contiguous()
    return th


def _fp8_state(w: torch.Tensor, role: str, device) -> list:
    """Per-layer persistent delayed-scaling state (scale, inv, amax,
    first) attached to the layer's weight tensor (stable identity across
    steps, unlike activations)."""
    st = getattr(w, "_gdlj_fp8st", None)
    if st is None:
        st = {}
        w._gdlj_fp8st = st
    if role not in st:
        st[role] = [
            torch.ones(1, dtype=torch.float32, device=device),
            torch.ones(1, dtype=torch.float32, device=device),
            torch.zeros(1, dtype=torch.int32, device=device),
            True,
        ]
    return st[role]


def _quant_delayed(x: torch.Tensor, w: torch.Tensor, role: str):
    """Quantize x to e4m3 with the previous step's scale (fused amax
    accumulation; exact two-pass on first use). Returns (q, inv_scale)."""
    ext = hip_ext()
    if not _fp8_delayed_on():
        q, _, inv = ext.fp8_quantize(x.contiguous())
        return q, inv
    st = _fp8_state(w, role, x.device)
    y = ext.fp8_quantize_delayed(x.contiguous(), st[0], st[1], st[2], st[3])
    st[3] = False
    return y, st[1]


def _zero_page(device, dtype=torch.bfloat16) -> torch.Tensor:
    """32 zero bytes, viewed as dtype, for gathered global_load_lds
    (OOB/pad chunks redirect there). One per (device, dtype)."""
    key = (device, dtype)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(32, dtype=torch.uint8,
                                       device=device).view(dtype)
    return _zero_pages[key]


def _dims(*vals) -> torch.Tensor:
    """Cached CPU int64 tensor of conv gather dims."""
    if vals not in _dims_cache:
        _dims_cache[vals] = torch.tensor(vals, dtype=torch.int64)
    return _dims_cache[vals]


def _packed(w: torch.Tensor, key: str, builder):
    """Per-parameter cache of derived weight layouts (padded/transposed/
    permuted copies), invalidated by the tensor's in-place version counter.
    Saves a handful of aten copies per layer per forward/backward."""
    cache = getattr(w, "_gdlj_cache", None)
    ver = w._version
    if cache is None or cache[0] != ver:
        cache = (ver, {})
        try:
            w._gdlj_cache = cache
        except AttributeError:  # non-leaf / view tensors: skip caching
            return builder()
    d = cache[1]
    if key not in d:
        d[key] = builder()
    return d[key]


def _fp8_pack(owner: torch.Tensor, key: str, pack: torch.Tensor):
    """(q, scale, inv_scale) e4m3 image of a bf16 weight pack, cached on
    owner. The double-rate fp8 MFMA consumes K in 128-deep tiles."""
    return _packed(owner, key, lambda: tuple(
        hip_ext().fp8_quantize(_pad_last(pack, 128))))


def _bias_f32(b):
    return (None if b is None else
            _packed(b, "f32", lambda: b.detach().float().contiguous()))


def _act_bwd(ctx, dy, y, n: int, c: int, fused, want_bias: bool):
    """Gradient at the producer's pre-activation, n channels wide of which
    the first c are real: (dpre [M, n], bias grad [c] or None when it is
    still to be reduced). `fused` is what a consumer left in the act-fusion
    side channel; when it matches, dy already IS dpre."""
    ext = hip_ext()
    dy2d = dy.reshape(-1, n)
    db = None
    if fused is not None and fused[0] == ctx.act and fused[1] == n:
        # the consumer already applied act backward + bias reduction
        dpre = dy2d
        if want_bias and fused[2] is not None:
            db = fused[2].to(ctx.dtypes[2])
    elif ctx.act and want_bias and n % 8 == 0:
        dpre, db_f = ext.act_bwd_bias(dy2d, y.reshape(-1, n).contiguous(),
                                      ctx.act, ctx.slope)
        db = db_f[:c].to(ctx.dtypes[2])
    elif ctx.act:
        dpre = ext.act_bwd(dy2d, y.reshape(-1, n).contiguous(), ctx.act,
                           ctx.slope)
    else:
        dpre = dy2d
    return dpre, db


# ===================================================================== linear
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, act: int, slope: float, emit_stats: bool):
        ext = hip_ext()
        xp = _pad_k(_bf(x))
        wp = _packed(w, "wp", lambda: _pad_k(_bf(w.detach())))
        bias = _bias_f32(b)
        if emit_stats and w.shape[0] % 8 == 0:
            y, ssum, ssq = ext.gemm_tn_stats(xp, wp, bias, act, slope)
            deposit_bn_stats(y, (ssum, ssq))
        else:
            y = ext.gemm_tn(xp, wp, bias, act, slope, False)
        ctx.save_for_backward(xp, wp, y)
        ctx.act, ctx.slope = act, slope
        ctx.nin = x.shape[-1]
        ctx.has_bias = b is not None
        ctx.dtypes = (x.dtype, w.dtype, b.dtype if b is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = hip_ext()
        xp, wp, y = ctx.saved_tensors
        fused = take_act_fused(dy)
        dy = _bf(dy)
        dx = dw = None
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        nout = dy.shape[1]
        dpre, db = _act_bwd(ctx, dy, y, nout, nout, fused, want_bias)
        if ctx.needs_input_grad[0]:
            # dgrad: dx = dpre @ w ;  B = w^T padded over nout
            nin = ctx.nin
            wt = _packed(wp, "wt",
                         lambda: _pad_k(wp[:, :nin].t().contiguous()))
            dx = ext.gemm_tn(_pad_k(dpre), wt, None, 0, 0.0, False)
            if dx.shape[1] != ctx.nin:
                dx = dx[:, : ctx.nin].contiguous()
        if ctx.needs_input_grad[1]:
            # wgrad: dw = dpre^T-contracted-with-x (rows = batch); padded
            # x cols are zero so the sliced grad region is exact
            kchunks = (xp.shape[0] + 63) // 64
            sk = _splitk_for((nout + 127) // 128, (ctx.nin + 127) // 128, kchunks)
            dw = ext.gemm_nt(_pad_last(dpre, 8), xp, sk, _zero_page(xp.device))
            dw = dw[: nout, : ctx.nin].contiguous().to(ctx.dtypes[1])
        if want_bias and db is None:
            db = ext.col_sum(dpre).to(ctx.dtypes[2])
        if dx is not None:
            dx = dx.to(ctx.dtypes[0])
        return dx, dw, db, None, None, None


def linear(x, w, b=None, act="identity", slope=0.2, emit_stats=False):
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() > 2 else x
    y = _Linear.apply(_bf(x2), w, b, ACT_CODES[act], slope, emit_stats)
    if x.dim() > 2:
        y = y.reshape(*x.shape[:-1], y.shape[-1])
    return y


# ====================================================================== conv
def _conv_out(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def _pad_channels(xh: torch.Tensor, c8: int) -> torch.Tensor:
    """[N,H,W,C] -> [N,H,W,c8] zero-padded channels (gather needs C%8==0).
    new_empty + two slice writes beats new_zeros + copy (the full-buffer
    zero fill re-wrote the data region for nothing)."""
    n, h, w, c = xh.shape
    out = xh
    if c != c8:
        out = xh.new_empty(n, h, w, c8)
        out[..., :c] = xh
        out[..., c:] = 0
    return out


def _weight_taps(w: torch.Tensor, perm, c8: int) -> torch.Tensor:
    """Weight permuted to [out, R, S, c] in bf16, c zero-padded to c8."""
    wc = _bf(w.detach().permute(*perm))
    o, r, s, c = wc.shape
    return _pad_channels(wc.reshape(o * r * s, 1, 1, c),
                         c8).reshape(o, r, s, c8)


def _parity_class_packs(wc: torch.Tensor, stride: int, pad: int) -> list:
    """[out, R, S, c] taps -> one K-padded [out, taps_q * c] pack per
    output parity class (qh-major), each over the class's valid taps."""
    packs = []
    for qh in range(stride):
        for qw in range(stride):
            prh = (qh + pad) % stride
            prw = (qw + pad) % stride
            sub = wc[:, prh::stride, prw::stride, :]
            packs.append(_pad_k(sub.reshape(wc.shape[0], -1).contiguous()))
    return packs


def _conv_wgrad(ctx, dpre8, xh):
    """dw as one implicit gathered-B NT GEMM (rows = N*Ho*Wo)."""
    N, C, H, W, Kout, R, S, Ho, Wo, stride, pad, kpad, C8 = ctx.geom
    npq, Ko8 = dpre8.shape
    sk = _splitk_for((Ko8 + 127) // 128, (kpad + 127) // 128,
                     (npq + 63) // 64)
    dw = hip_ext().gemm_nt_implicit(
        dpre8, xh, 2, Ko8, kpad, npq,
        _dims(N, H, W, C8, Ho, Wo, R, S, stride, pad), sk,
        _zero_page(xh.device))
    return (dw[:Kout, :R * S * C8].reshape(Kout, R, S, C8)[..., :C]
            .permute(0, 3, 1, 2).contiguous().to(ctx.dtypes[1]))


def _conv_dgrad_s1(ctx, dpre8):
    """Stride 1: dgrad as ONE transposed-gather GEMM (no dcol/col2im;
    every tap valid at stride 1)."""
    ext = hip_ext()
    N, C, H, W, Kout, R, S, Ho, Wo, stride, pad, kpad, C8 = ctx.geom
    w = ctx.wref
    Ko8 = dpre8.shape[1]
    wd = _packed(w, "dgrad_w", lambda: _pad_k(
        _weight_taps(w, (1, 2, 3, 0), Ko8).reshape(C, R * S * Ko8)))
    dpre_img = dpre8.view(N, Ho, Wo, Ko8)
    if _fp8_bwd_on() and Ko8 % 16 == 0:
        wdq, _, iwd = _fp8_pack(w, "dgrad_w_fp8", wd)
        dq, idy = _quant_delayed(dpre_img, w, "dy")
        dx2d = ext.conv_fwd_implicit_fp8(
            dq, wdq, None, idy, iwd, _zero_page(dpre8.device, torch.uint8),
            N, Ho, Wo, Ko8, H, W, R, S, stride, pad, 0, 0.0, 1)
    else:
        dx2d = ext.conv_fwd_implicit(
            dpre_img, wd, None, _zero_page(dpre8.device), N, Ho, Wo, Ko8, H,
            W, R, S, stride, pad, 0, 0.0, 1, 0)[0]
    return _as_nchw_view(dx2d.view(N, H, W, C)).to(ctx.dtypes[0])


def _conv_dgrad_parity(ctx, dpre8):
    """Strided, GDLJ_PARITY: parity-decomposed gather (each output parity
    class is a dense GEMM over its valid taps only)."""
    N, C, H, W, Kout, R, S, Ho, Wo, stride, pad, kpad, C8 = ctx.geom
    w = ctx.wref
    Ko8 = dpre8.shape[1]
    wd_cls = _packed(w, "dgrad_wcls", lambda: _parity_class_packs(
        _weight_taps(w, (1, 2, 3, 0), Ko8), stride, pad))
    dx2d = hip_ext().conv_parity_implicit(
        dpre8.view(N, Ho, Wo, Ko8), wd_cls, None, _zero_page(dpre8.device),
        N, Ho, Wo, Ko8, H, W, C, R, S, stride, pad, 0, 0.0)
    return _as_nchw_view(dx2d.view(N, H, W, C)).to(ctx.dtypes[0])


def _conv_dgrad_strided(ctx, dpre, dpre8, xh, wp):
    """Strided default: the fused direct kernel (conv_dgrad_direct.hip)
    when the geometry qualifies, else dcol GEMM + col2im gather. With
    prev_act the producer's act backward folds into either (xh IS the
    producer's activation output) along with its bias-grad column sums;
    both go to the producer through the side channel so it skips its own
    pass."""
    ext = hip_ext()
    N, C, H, W, Kout, R, S, Ho, Wo, stride, pad, kpad, C8 = ctx.geom
    rsc8 = R * S * C8
    wt = _packed(wp, "wt", lambda: _pad_k(
        wp[:, :rsc8].t().contiguous()))   # [rsc8, kout_pad]
    pact = ctx.prev_act if C8 == C and _act_fuse_on() else None
    p_code, p_slope, p_bias = pact if pact is not None else (0, 0.0, None)
    fp8 = _fp8_bwd_on()
    res = None
    if not fp8 and _dgrad_direct_on():
        res = ext.conv_dgrad_direct(
            dpre8, wt, xh if pact is not None else None,
            _zero_page(dpre.device), N, H, W, C8, Ho, Wo, R, S, stride, pad,
            p_code, p_slope, p_bias is not False and p_bias is not None)
    if res:
        dxh, pdb = res[0], res[1] if len(res) > 1 else None
    else:
        if fp8:
            wtq, _, iwt = _fp8_pack(wp, "wt_fp8", wt)
            dq, idy = _quant_delayed(_pad_last(dpre, 128), ctx.wref, "dy")
            dcol = ext.gemm_tn_fp8(dq, wtq, idy, iwt, None, 0, 0.0)
        else:
            dcol = ext.gemm_tn(_pad_k(dpre), wt, None, 0, 0.0, False)
        if pact is not None:
            dxh, pdb = ext.col2im_dact(
                dcol, N, H, W, C8, Ho, Wo, R, S, stride, pad, rsc8, xh,
                p_code, p_slope, p_bias)
            pdb = pdb if p_bias else None
        else:
            dxh, pdb = ext.col2im(dcol, N, H, W, C8, Ho, Wo, R, S, stride,
                                  pad, rsc8, None, 0, 0.0), None
    # at the channel-pad boundary the padded dx (pad lanes: zero weight
    # rows) passes through to a convT producer when no cast intervenes
    dx = _as_nchw_view(_trim_channels(
        dxh, C, dxh.dtype == ctx.dtypes[0])).to(ctx.dtypes[0])
    if pact is not None:
        deposit_act_fused(dx, (p_code, C, pdb))
    return dx


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride: int, pad: int, act: int, slope: float,
                emit_stats: bool, prev_act):
        ext = hip_ext()
        N, C, H, W = x.shape
        Kout, _, R, S = w.shape
        Ho, Wo = _conv_out(H, R, stride, pad), _conv_out(W, S, stride, pad)
        # channel dim padded to 8 so every conv runs the implicit path
        C8 = _rup(C, 8)
        xh = take_chan_pad(x, C8)
        if xh is None:
            xh = _pad_channels(_nhwc(x), C8)
        kpad = _rup(R * S * C8, 64)
        wp = _packed(w, "conv_wp", lambda: _pad_k(
            _weight_taps(w, (0, 2, 3, 1), C8).reshape(Kout, R * S * C8)))
        bias = _bias_f32(b)
        stats = None
        if FP8_CONV and C8 % 16 == 0:
            xq, ix = _quant_delayed(xh, w, "x")
            wq, _, iw = _fp8_pack(w, "fp8", wp)
            y2d = ext.conv_fwd_implicit_fp8(
                xq, wq, bias, ix, iw, _zero_page(x.device, torch.uint8), N,
                H, W, C8, Ho, Wo, R, S, stride, pad, act, slope, 0)
        elif C8 <= 16 and _smallc_col_on():
            col = ext.im2col(xh, N, H, W, C8, Ho, Wo, R, S, stride, pad,
                             kpad)
            if emit_stats and Kout % 8 == 0:
                y2d, ssum, ssq = ext.gemm_tn_stats(col, wp, bias, act,
                                                   slope)
                stats = (ssum, ssq)
            else:
                y2d = ext.gemm_tn(col, wp, bias, act, slope, False)
        else:
            # implicit GEMM: im2col gather fused into the MFMA staging
            # (optionally also emitting the consumer BN's batch statistics)
            res = ext.conv_fwd_implicit(
                xh, wp, bias, _zero_page(x.device), N, H, W, C8, Ho, Wo, R,
                S, stride, pad, act, slope, 0, 1 if emit_stats else 0)
            y2d = res[0]
            if len(res) == 3:
                stats = (res[1], res[2])
        ctx.save_for_backward(xh, wp, y2d)
        ctx.geom = (N, C, H, W, Kout, R, S, Ho, Wo, stride, pad, kpad, C8)
        ctx.act, ctx.slope = act, slope
        ctx.has_bias = b is not None
        ctx.dtypes = (x.dtype, w.dtype, b.dtype if b is not None else None)
        ctx.wref = w
        ctx.prev_act = prev_act
        out = _as_nchw_view(y2d.view(N, Ho, Wo, Kout))
        if stats is not None:
            deposit_bn_stats(out, stats)
        return out

    @staticmethod
    def backward(ctx, dy):
        xh, wp, y2d = ctx.saved_tensors
        Kout, stride = ctx.geom[4], ctx.geom[9]
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        fused = take_act_fused(dy)
        dy2d = _bf(dy.permute(0, 2, 3, 1)).reshape(-1, Kout)
        dpre, db = _act_bwd(ctx, dy2d, y2d, Kout, Kout, fused, want_bias)
        dpre8 = _pad_last(dpre, 8)
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = _conv_wgrad(ctx, dpre8, xh)
        if ctx.needs_input_grad[0]:
            if stride == 1:
                dx = _conv_dgrad_s1(ctx, dpre8)
            elif PARITY_STRIDED:
                dx = _conv_dgrad_parity(ctx, dpre8)
            else:
                dx = _conv_dgrad_strided(ctx, dpre, dpre8, xh, wp)
        if want_bias and db is None:
            db = hip_ext().col_sum(dpre).to(ctx.dtypes[2])
        return dx, dw, db, None, None, None, None, None, None


def conv2d(x, w, b=None, stride=1, padding=0, act="identity", slope=0.2,
           emit_stats=False, prev_act=None):
    return _Conv2d.apply(x, w, b, stride, padding, ACT_CODES[act], slope,
                         emit_stats, prev_act)


# ============================================================ conv transpose
# The three forward routes of _ConvTranspose2d; each returns (yh, stats):
# the NHWC output (trimmed to Cout) and the fused BN (sum, sumsq) or None.
def _convt_fwd_s1(geom, xh, w, bias, act, slope, emit_stats):
    """Stride 1: ONE transposed-gather GEMM with fused bias+activation:
    y[ho,wo,cout] = act( sum_{r,s,cin}[valid hi=ho+pad-r]
                         x[hi,wi,cin] * W[cin][cout][r][s] + b )"""
    ext = hip_ext()
    N, Cin, Hi, Wi, Cout, R, S, Ho, Wo, stride, pad = geom
    wt = _packed(w, "convt_fwd_w", lambda: _pad_k(
        _bf(w.detach().permute(1, 2, 3, 0))      # [Cout,R,S,Cin]
        .reshape(Cout, R * S * Cin)))
    stats = None
    if _fp8_convt_s1_on() and Cin % 16 == 0 and not emit_stats:
        wtq, _, iw = _fp8_pack(w, "convt_fwd_w_fp8", wt)
        xq, ix = _quant_delayed(xh, w, "x")
        y2d = ext.conv_fwd_implicit_fp8(
            xq, wtq, bias, ix, iw, _zero_page(xh.device, torch.uint8), N,
            Hi, Wi, Cin, Ho, Wo, R, S, stride, pad, act, slope, 1)
    else:
        res = ext.conv_fwd_implicit(
            xh, wt, bias, _zero_page(xh.device), N, Hi, Wi, Cin, Ho, Wo, R,
            S, stride, pad, act, slope, 1, 1 if emit_stats else 0)  # mode 1
        y2d = res[0]
        if len(res) == 3:
            stats = (res[1], res[2])
    return y2d.view(N, Ho, Wo, Cout), stats


def _convt_fwd_parity(geom, xh, w, bias, act, slope):
    """Strided, GDLJ_PARITY: parity-decomposed gathered GEMMs with fused
    bias+activation (each output parity class reads only its valid taps;
    no col buffer / col2im pass)."""
    N, Cin, Hi, Wi, Cout, R, S, Ho, Wo, stride, pad = geom
    wcls = _packed(w, "convt_fwd_wcls", lambda: _parity_class_packs(
        _bf(w.detach().permute(1, 2, 3, 0)), stride, pad))  # [Cout,R,S,Cin]
    y2d = hip_ext().conv_parity_implicit(
        xh, wcls, bias, _zero_page(xh.device), N, Hi, Wi, Cin, Ho, Wo, Cout,
        R, S, stride, pad, act, slope)
    return y2d.view(N, Ho, Wo, Cout), None


def _convt_fwd_strided(geom, xh, w, b, bias, act, slope, emit_stats):
    """Strided default: the parity-direct kernel (conv_dgrad_direct.hip,
    the strided dgrad's kernel with a bias+act-fwd epilogue and fused BN
    stats) when the geometry qualifies, else GEMM over Cin + col2im with
    the same epilogue. Cout is padded to 8 so col2im stays on the
    vectorized path (scalar col2im for the Cout=3 generator head measured
    745us vs ~100us vectorized; the wider col write is ~170us)."""
    ext = hip_ext()
    N, Cin, Hi, Wi, Cout, R, S, Ho, Wo, stride, pad = geom
    x2d = _pad_k(xh.reshape(-1, Cin))
    Co8 = _rup(Cout, 8)
    def build_w2a():
        wr = _bf(w.detach().permute(2, 3, 1, 0))        # [R,S,Cout,Cin]
        if Co8 != Cout:
            wr = torch.nn.functional.pad(wr, (0, 0, 0, Co8 - Cout))
        return _pad_k(wr.reshape(R * S * Co8, Cin))

    w2a = _packed(w, "w2a8" if Co8 != Cout else "w2a", build_w2a)
    if Co8 != Cout and bias is not None:
        bias = _packed(b, "f32p8", lambda: torch.nn.functional.pad(
            b.detach().float(), (0, Co8 - Cout)).contiguous())
    want_stats = bool(emit_stats and Cout % 8 == 0)
    fp8 = _fp8_convt_strided_on()
    res = None
    if _dgrad_direct_on() and not fp8:
        res = ext.conv_transpose_fwd_direct(
            x2d, w2a, bias, _zero_page(xh.device), N, Hi, Wi, Ho, Wo, Co8, R,
            S, stride, pad, act, slope, want_stats)
    if res:
        yh, stats = res[0], (res[1], res[2]) if len(res) > 1 else None
    else:
        if fp8:
            w2aq, _, iw2 = _fp8_pack(w, "w2a_fp8", w2a)
            xq2, ix2 = _quant_delayed(_pad_last(x2d, 128), w, "xT")
            col = ext.gemm_tn_fp8(xq2, w2aq, ix2, iw2, None, 0, 0.0)
        else:
            col = ext.gemm_tn(x2d, w2a, None, 0, 0.0,
                              False)  # [NPin, RSCo8]
        if want_stats:
            yh, ssum, ssq = ext.col2im_stats(
                col, N, Ho, Wo, Cout, Hi, Wi, R, S, stride, pad,
                R * S * Cout, bias, act, slope)
            stats = (ssum, ssq)
        else:
            yh, stats = ext.col2im(col, N, Ho, Wo, Co8, Hi, Wi, R, S, stride,
                                   pad, R * S * Co8, bias, act, slope), None
    # identity/tanh keep the pad channels zero: act(0 + 0-bias) == 0
    return _trim_channels(yh, Cout, act in (0, 1)), stats


class _ConvTranspose2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride: int, pad: int, act: int, slope: float,
                emit_stats: bool):
        N, Cin, Hi, Wi = x.shape
        _, Cout, R, S = w.shape
        Ho = (Hi - 1) * stride - 2 * pad + R
        Wo = (Wi - 1) * stride - 2 * pad + S
        geom = (N, Cin, Hi, Wi, Cout, R, S, Ho, Wo, stride, pad)
        xh = _nhwc(x)                       # [N,Hi,Wi,Cin]; Cin % 8 == 0
        bias = _bias_f32(b)
        if stride == 1:
            yh, stats = _convt_fwd_s1(geom, xh, w, bias, act, slope,
                                      emit_stats)
        elif PARITY_STRIDED:
            yh, stats = _convt_fwd_parity(geom, xh, w, bias, act, slope)
        else:
            yh, stats = _convt_fwd_strided(geom, xh, w, b, bias, act, slope,
                                           emit_stats)
        ctx.save_for_backward(xh, yh)
        ctx.geom = geom
        ctx.act, ctx.slope = act, slope
        ctx.has_bias = b is not None
        ctx.dtypes = (x.dtype, w.dtype, b.dtype if b is not None else None)
        ctx.wref = w
        out = _as_nchw_view(yh)
        if stats is not None:
            deposit_bn_stats(out, stats)
        return out

    @staticmethod
    def backward(ctx, dy):
        ext = hip_ext()
        xh, yh = ctx.saved_tensors
        w = ctx.wref
        N, Cin, Hi, Wi, Cout, R, S, Ho, Wo, stride, pad = ctx.geom
        fused = take_act_fused(dy)
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        Co8 = _rup(Cout, 8)
        # 3-channel image boundary pass-through: when the downstream
        # conv's dgrad deposited the PADDED dy and the forward deposited
        # the padded y, act backward runs at Co8 width (the pad lanes are
        # exact zeros through tanh/identity) and no trim/re-pad copies
        # are paid on either side of the boundary.
        dy_pad = y_pad = None
        if fused is None and Co8 != Cout:
            dy_pad = take_chan_pad(dy, Co8)
            y_pad = take_chan_pad(yh, Co8) if dy_pad is not None else None
        if dy_pad is not None and (y_pad is not None or ctx.act == 0):
            dpre, db = _act_bwd(ctx, dy_pad, y_pad, Co8, Cout, None,
                                want_bias)
            dpre8 = dpre.view(N, Ho, Wo, Co8)
        else:
            dpre, db = _act_bwd(ctx, _nhwc(dy), yh, Cout, Cout, fused,
                                want_bias)
            dpre8 = _pad_channels(dpre.view(N, Ho, Wo, Cout), Co8)
        npq = N * Hi * Wi
        dx = dw = None
        if ctx.needs_input_grad[0]:
            # dx[np_in][cin] = sum_{r,s,cout} dpre[ho=hi*s-p+r..][cout]
            #                  * W[cin][cout][r][s]  (forward-gather, mode 0)
            w2b = _packed(w, "convt_dgrad_w", lambda: _pad_k(
                _weight_taps(w, (0, 2, 3, 1), Co8)     # [Cin,R,S,Co8]
                .reshape(Cin, R * S * Co8)))
            if _fp8_bwd_on() and Co8 % 16 == 0:
                w2bq, _, iw2b = _fp8_pack(w, "convt_dgrad_w_fp8", w2b)
                dq, idy = _quant_delayed(dpre8, w, "dy")
                dx2d = ext.conv_fwd_implicit_fp8(
                    dq, w2bq, None, idy, iw2b,
                    _zero_page(dpre8.device, torch.uint8), N, Ho, Wo, Co8,
                    Hi, Wi, R, S, stride, pad, 0, 0.0, 0)
            else:
                dx2d = ext.conv_fwd_implicit(
                    dpre8, w2b, None, _zero_page(dpre8.device), N, Ho, Wo,
                    Co8, Hi, Wi, R, S, stride, pad, 0, 0.0, 0, 0)[0]
            dx = _as_nchw_view(dx2d.view(N, Hi, Wi, Cin)).to(ctx.dtypes[0])
        if ctx.needs_input_grad[1]:
            # wgrad: dW[(r,s,cout)][cin] = sum_np im2col(dpre)[np][rs*cout]
            #        * x[np][cin]  (gathered-A NT over dOut)
            rsco8 = R * S * Co8
            rscop8 = _rup(rsco8, 64)
            x2d = _pad_k(xh.reshape(-1, Cin))
            sk = _splitk_for((rscop8 + 127) // 128,
                             (x2d.shape[1] + 127) // 128, (npq + 63) // 64)
            dw2a = ext.gemm_nt_implicit(
                dpre8, x2d, 1, rscop8, x2d.shape[1], npq,
                _dims(N, Ho, Wo, Co8, Hi, Wi, R, S, stride, pad),
                sk, _zero_page(x2d.device))
            dw = (dw2a[:rsco8, :Cin].reshape(R, S, Co8, Cin)[:, :, :Cout]
                  .permute(3, 2, 0, 1).contiguous().to(ctx.dtypes[1]))
        if want_bias and db is None:
            db = ext.col_sum(dpre8.reshape(-1, Co8))[:Cout].to(
                ctx.dtypes[2])
        return dx, dw, db, None, None, None, None, None


def conv_transpose2d(x, w, b=None, stride=1, padding=0, act="identity",
                     slope=0.2, emit_stats=False):
    return _ConvTranspose2d.apply(x, w, b, stride, padding, ACT_CODES[act],
                                  slope, emit_stats)


# ================================================================ batch norm
class _BatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2, gamma, beta, rm, rv, momentum, eps, pre_stats,
                bwd_act):
        ext = hip_ext()
        if pre_stats is not None:
            # producer-fused statistics (conv/dense epilogue): skip the
            # stats pass entirely
            y, mean, istd = ext.bn_fwd_train_pre(
                x2, pre_stats[0], pre_stats[1], gamma.detach().float(),
                beta.detach().float(), rm, rv, momentum, eps)
        else:
            y, mean, istd = ext.bn_fwd_train(x2, gamma.detach().float(),
                                             beta.detach().float(), rm, rv,
                                             momentum, eps)
        ctx.save_for_backward(x2, mean, istd, gamma)
        ctx.bwd_act = bwd_act
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = hip_ext()
        x2, mean, istd, gamma = ctx.saved_tensors
        if ctx.bwd_act is not None:
            # x2 is the producer's activation output: fold the activation
            # backward + producer bias-grad into the BN apply kernel and
            # hand the result to the producer via the side channel
            act, slope, want_bias = ctx.bwd_act
            dx, dgamma, dbeta, db = ext.bn_bwd_act(
                x2, _bf(dy), mean, istd, gamma.detach().float(), act, slope,
                want_bias)
            deposit_act_fused(
                dx, (act, x2.shape[-1], db if want_bias else None))
        else:
            dx, dgamma, dbeta = ext.bn_bwd(x2, _bf(dy), mean, istd,
                                           gamma.detach().float())
        return dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None, \
            None, None, None, None, None


def batch_norm(x, weight, bias, running_mean, running_var, training,
               momentum=0.1, eps=1e-5, bwd_act=None):
    is4d = x.dim() == 4
    pre_stats = take_bn_stats(x)
    if is4d:
        xh = _nhwc(x)
        x2 = xh.reshape(-1, xh.shape[-1])
    else:
        x2 = _bf(x)
    if bwd_act is not None and (x2.shape[-1] % 8 != 0
                                or not _act_fuse_on()):
        bwd_act = None
    if training:
        y2 = _BatchNorm.apply(x2, weight, bias, running_mean, running_var,
                              momentum, eps, pre_stats, bwd_act)
    else:
        y2 = hip_ext().bn_fwd_eval(x2, weight.detach().float(),
                                   bias.detach().float(), running_mean,
                                   running_var, eps)
    if is4d:
        return _as_nchw_view(y2.view(*xh.shape))
    return y2


# ================================================================== pooling
class _MaxPool2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel: int, stride: int):
        ext = hip_ext()
        N, C, H, W = x.shape
        xh = _nhwc(x)
        out, argmax = ext.maxpool_fwd(xh, N, H, W, C, kernel, stride)
        ctx.save_for_backward(argmax)
        ctx.geom = (N, C, H, W, kernel, stride)
        ctx.x_dtype = x.dtype
        return _as_nchw_view(out)

    @staticmethod
    def backward(ctx, dy):
        ext = hip_ext()
        (argmax,) = ctx.saved_tensors
        N, C, H, W, kernel, stride = ctx.geom
        dyh = _nhwc(dy)
        din = ext.maxpool_bwd(dyh, argmax, N, H, W, C, kernel, stride)
        return _as_nchw_view(din).to(ctx.x_dtype), None, None


def max_pool2d(x, kernel, stride):
    return _MaxPool2d.apply(x, kernel, stride)


class _Upsample2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale: int):
        ext = hip_ext()
        N, C, H, W = x.shape
        xh = _nhwc(x)
        out = ext.upsample_fwd(xh, N, H, W, C, scale)
        ctx.geom = (N, C, H, W, scale)
        ctx.x_dtype = x.dtype
        return _as_nchw_view(out)

    @staticmethod
    def backward(ctx, dy):
        ext = hip_ext()
        N, C, H, W, scale = ctx.geom
        dyh = _nhwc(dy)
        din = ext.upsample_bwd(dyh, N, H, W, C, scale)
        return _as_nchw_view(din).to(ctx.x_dtype), None


def upsample_nearest2d(x, scale):
    return _Upsample2d.apply(x, scale)


# =============================================================== activations
class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act: int, slope: float):
        y = hip_ext().act_fwd(_bf(x), act, slope)
        ctx.save_for_backward(y)
        ctx.act, ctx.slope = act, slope
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = hip_ext().act_bwd(_bf(dy), y, ctx.act, ctx.slope)
        return dx.to(ctx.x_dtype), None, None


def activation(x, act, slope=0.2):
    code = ACT_CODES[act]
    if code == 0:
        return x
    return _Act.apply(x, code, slope)


# ========================================================= dropout / noise
def _bf_dense(t: torch.Tensor) -> torch.Tensor:
    """bf16 cast that keeps any dense stride order (channels-last views
    pass through with zero copies; the kernels walk storage order). Only a
    genuinely strided tensor (e.g. a channel-trimmed view) is copied, into
    channels-last when that is its innermost axis."""
    from .functional import _storage_order

    t = t.to(torch.bfloat16)
    if _storage_order(t) is not None:
        return t
    if t.dim() == 4 and t.stride(1) == 1:
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous()


class _Dropout(torch.autograd.Function):
    """Inverted dropout on the Philox kernel. The kernel reads
    [seed, calls] from `state` on the device; the counter is advanced by a
    stream-ordered in-place add AFTER the launch (captured with the step,
    like Updater._t_dev). Backward uses only the saved mask bytes."""

    @staticmethod
    def forward(ctx, x, state, keep: float):
        xb = _bf_dense(x)
        y, mask = hip_ext().dropout_fwd(xb, state, keep)
        state[1:2].add_(1)
        ctx.save_for_backward(mask)
        ctx.keep = keep
        ctx.x_dtype = x.dtype
        ctx.strides = y.stride()
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dyb = dy.to(torch.bfloat16)
        if dyb.stride() != ctx.strides:
            # the mask is in the forward's storage order
            dyb = torch.empty_strided(dy.shape, ctx.strides, dtype=dyb.dtype,
                                      device=dyb.device).copy_(dyb)
        dx = hip_ext().dropout_bwd(dyb, mask, ctx.keep)
        return dx.to(ctx.x_dtype), None, None


class _GaussianNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, state, stddev: float):
        y = hip_ext().gaussian_noise_fwd(_bf_dense(x), state, stddev)
        state[1:2].add_(1)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy.to(ctx.x_dtype), None, None


def dropout(x, state, keep):
    return _Dropout.apply(x, state, keep)


def gaussian_noise(x, state, stddev):
    return _GaussianNoise.apply(x, state, stddev)


# ============================================================ spectral norm
class _SpectralNorm(torch.autograd.Function):
    """W / sigma on the _spectral kernels (ops/hip/spectral/). Training
    mode runs one power iteration and overwrites u, v on the device; the
    kernels also hand back this call's OWN copies of u, v and sigma, which
    is what backward uses: loss_d runs D twice before one backward, and
    the second forward's state update must not reach the first's
    gradient. Nothing crosses to the host, so a captured step replays."""

    @staticmethod
    def forward(ctx, w, u, v, training: bool):
        ext = spectral_ext()
        wb = _bf(w.detach())
        if training:
            w_sn, u_c, v_c, sig = ext.sn_forward(wb, u, v)[:4]
        else:
            w_sn, sig = ext.sn_forward_eval(wb, u, v)[:2]
            u_c, v_c = u, v
            if ctx.needs_input_grad[0]:
                u_c, v_c = u.clone(), v.clone()
        ctx.save_for_backward(w_sn, u_c, v_c, sig)
        ctx.w_dtype = w.dtype
        return w_sn

    @staticmethod
    def backward(ctx, g):
        w_sn, u_c, v_c, sig = ctx.saved_tensors
        dw = spectral_ext().sn_backward(_bf(g), w_sn, u_c, v_c, sig)[0]
        return dw.to(ctx.w_dtype), None, None, None


def spectral_normalize(w, u, v, training):
    """GPU path of functional.spectral_normalize. Training: a fresh W_sn
    per forward (its conv/linear packs are rebuilt per forward). Eval
    without autograd: W_sn is cached on w like any other derived layout,
    so serving keeps its packs across requests; a training forward drops
    that entry because it moves u and v without touching w's version."""
    if training:
        cache = getattr(w, "_gdlj_cache", None)
        if cache is not None:
            cache[1].pop("sn_eval", None)
    elif not (torch.is_grad_enabled() and w.requires_grad):
        return _packed(w, "sn_eval", lambda: _SpectralNorm.apply(
            w.detach(), u, v, False))
    return _SpectralNorm.apply(w, u, v, training)


# ==================================================================== losses
class _BceWithLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        ext = hip_ext()
        lb = _bf(logits)
        yb = _bf(labels)
        s = ext.bce_fwd(lb, yb)
        ctx.save_for_backward(lb, yb)
        ctx.x_dtype = logits.dtype
        return (s / lb.numel()).squeeze(0)

    @staticmethod
    def backward(ctx, grad):
        ext = hip_ext()
        lb, yb = ctx.saved_tensors
        d = ext.bce_bwd(lb, yb, 1.0 / lb.numel())
        return (d * grad).to(ctx.x_dtype), None


def bce_with_logits(logits, labels):
    return _BceWithLogits.apply(logits, labels)


class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, onehot):
        ext = hip_ext()
        lb = _bf(logits)
        ob = _bf(onehot)
        s, probs = ext.softmax_xent_fwd(lb, ob)
        ctx.save_for_backward(probs, ob)
        ctx.x_dtype = logits.dtype
        return (s / lb.shape[0]).squeeze(0)

    @staticmethod
    def backward(ctx, grad):
        ext = hip_ext()
        probs, ob = ctx.saved_tensors
        d = ext.softmax_xent_bwd(probs, ob, 1.0 / probs.shape[0])
        return (d * grad).to(ctx.x_dtype), None


def softmax_cross_entropy(logits, onehot):
    return _SoftmaxXent.apply(logits, onehot)


# =================================================================== updater
def fused_update(kind, param, grad, master, m, v, lr, beta1, beta2, rms_decay,
                 eps, clip, l2, t, t_dev=None):
    ext = hip_ext()
    g = grad.contiguous()
    if kind == "adam":
        ext.fused_adam(param.view(-1), g.view(-1),
                       None if master is None else master.view(-1),
                       m.view(-1), v.view(-1), lr, beta1, beta2, eps, clip,
                       l2, t, t_dev)
    elif kind == "rmsprop":
        ext.fused_rmsprop(param.view(-1), g.view(-1),
                          None if master is None else master.view(-1),
                          v.view(-1), lr, rms_decay, eps, clip, l2)
    else:
        raise KeyError(kind)
