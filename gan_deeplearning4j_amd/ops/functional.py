"""Functional op API with per-device dispatch.

The op surface is the reference's exercised GPU-op worklist:
dense/conv/conv-transpose (im2col-MFMA-GEMM on gfx950), batchnorm, maxpool,
nearest-upsample, tanh/sigmoid/leaky-relu, BCE-with-logits, softmax-CE.

CPU tensors run plain PyTorch (fp32 reference); CUDA tensors run the HIP
kernels via `gpu_ops` (loudly failing if the extension is missing).
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

ACTIVATIONS = ("identity", "tanh", "sigmoid", "lrelu", "relu")


def _apply_act(x: torch.Tensor, act: Optional[str], slope: float = 0.2):
    if act is None or act == "identity":
        return x
    if act == "tanh":
        return torch.tanh(x)
    if act == "sigmoid":
        return torch.sigmoid(x)
    if act == "lrelu":
        return F.leaky_relu(x, slope)
    if act == "relu":
        return F.relu(x)
    raise KeyError(f"unknown activation {act!r}")


def linear(
    x: torch.Tensor,
    w: torch.Tensor,
    b: Optional[torch.Tensor] = None,
    act: Optional[str] = None,
    slope: float = 0.2,
    emit_stats: bool = False,
) -> torch.Tensor:
    """y = act(x @ w.T + b); w is [out, in] (torch convention).
    emit_stats: fuse the consumer BatchNorm's batch statistics into the
    GEMM epilogue (GPU; no-op on CPU)."""
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.linear(x, w, b, act or "identity", slope, emit_stats)
    return _apply_act(F.linear(x, w, b), act, slope)


def conv2d(
    x: torch.Tensor,
    w: torch.Tensor,
    b: Optional[torch.Tensor] = None,
    stride: int = 1,
    padding: int = 0,
    act: Optional[str] = None,
    slope: float = 0.2,
    emit_stats: bool = False,
    prev_act=None,
) -> torch.Tensor:
    """NCHW-logical conv; on GPU runs NHWC im2col-MFMA-GEMM kernels.

    prev_act: optional (act_code, slope, has_bias) of the sole producer
    feeding x — the strided dgrad folds that activation's backward into
    its col2im pass (see gpu_ops deposit_act_fused).
    """
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.conv2d(x, w, b, stride, padding, act or "identity",
                              slope, emit_stats, prev_act)
    return _apply_act(F.conv2d(x, w, b, stride=stride, padding=padding), act, slope)


def conv_transpose2d(
    x: torch.Tensor,
    w: torch.Tensor,
    b: Optional[torch.Tensor] = None,
    stride: int = 1,
    padding: int = 0,
    act: Optional[str] = None,
    slope: float = 0.2,
    emit_stats: bool = False,
) -> torch.Tensor:
    """True transposed conv (the reference emulates it as upsample+conv,
    Java:201-219; the north-star names a real transposed-conv kernel)."""
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.conv_transpose2d(
            x, w, b, stride, padding, act or "identity", slope, emit_stats
        )
    return _apply_act(
        F.conv_transpose2d(x, w, b, stride=stride, padding=padding), act, slope
    )


def batch_norm(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    running_mean: torch.Tensor,
    running_var: torch.Tensor,
    training: bool,
    momentum: float = 0.1,
    eps: float = 1e-5,
    bwd_act=None,
) -> torch.Tensor:
    """BatchNorm over dim 1 (2D) or channel dim (4D). Stats kept fp32.

    bwd_act: optional (act_code, slope, want_bias) describing the sole
    producer's fused output activation — GPU path folds that activation's
    backward into the BN backward kernel (see gpu_ops deposit_act_fused).
    """
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.batch_norm(
            x, weight, bias, running_mean, running_var, training, momentum,
            eps, bwd_act
        )
    return F.batch_norm(
        x, running_mean, running_var, weight, bias, training, momentum, eps
    )


def max_pool2d(x: torch.Tensor, kernel: int, stride: int) -> torch.Tensor:
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.max_pool2d(x, kernel, stride)
    return F.max_pool2d(x, kernel_size=kernel, stride=stride)


def upsample_nearest2d(x: torch.Tensor, scale: int) -> torch.Tensor:
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.upsample_nearest2d(x, scale)
    return F.interpolate(x, scale_factor=scale, mode="nearest")


def activation(x: torch.Tensor, act: str, slope: float = 0.2) -> torch.Tensor:
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.activation(x, act, slope)
    return _apply_act(x, act, slope)


def new_rng_state(seed: int = 0, device=None) -> torch.Tensor:
    """Per-layer random state int64[2] = [seed, calls] (ops/philox_ref.py).
    It lives on the layer's device so a captured step reads and advances
    it there; it is only ever mutated in place."""
    return torch.tensor([int(seed), 0], dtype=torch.int64, device=device)


def _storage_order(x: torch.Tensor):
    """Permutation that sorts x's dims by decreasing stride, or None when
    x is not a dense permutation of a contiguous block."""
    dims = sorted(range(x.dim()), key=lambda d: (-x.stride(d), d))
    expect = 1
    for d in reversed(dims):
        if x.shape[d] != 1 and x.stride(d) != expect:
            return None
        expect *= x.shape[d]
    return dims


def _storage_flat_like(vals: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Lay a flat storage-order vector out with x's shape and strides."""
    dims = _storage_order(x)
    if dims is None:
        return vals.reshape(x.shape)
    inv = [0] * len(dims)
    for pos, d in enumerate(dims):
        inv[d] = pos
    return vals.reshape([x.shape[d] for d in dims]).permute(inv)


class _DropoutRef(torch.autograd.Function):
    """x * mask / keep with the multiply done in fp32 (the kernel's order
    of operations), gradient dy * mask / keep."""

    @staticmethod
    def _masked_scale(t, mask, keep):
        wide = torch.float64 if t.dtype == torch.float64 else torch.float32
        scale = torch.tensor(1.0 / keep, dtype=wide)
        out = torch.where(mask, t.to(wide) * scale,
                          torch.zeros((), dtype=wide))
        return out.to(t.dtype)

    @staticmethod
    def forward(ctx, x, mask, keep):
        ctx.save_for_backward(mask)
        ctx.keep = keep
        return _DropoutRef._masked_scale(x, mask, keep)

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        return _DropoutRef._masked_scale(dy, mask, ctx.keep), None, None


def dropout(x: torch.Tensor, state: torch.Tensor, keep: float,
            training: bool = True) -> torch.Tensor:
    """Inverted dropout (DL4J Dropout(p): p = keep = retain probability).

    state is the layer's int64 [seed, calls]; one training call consumes
    the current `calls` value and advances it by 1 in place. Eval mode and
    keep == 1 return x itself and leave the counter alone. CPU and GPU
    draw the same Philox stream (ops/philox_ref.py)."""
    if not 0.0 < keep <= 1.0:
        raise ValueError(f"dropout keep must be in (0, 1], got {keep}")
    if not training or keep == 1.0:
        return x
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.dropout(x, state, keep)
    from . import philox_ref

    seed, calls = (int(v) for v in state.tolist())
    m = philox_ref.dropout_keep_mask(x.numel(), seed, calls, keep)
    mask = _storage_flat_like(torch.from_numpy(m), x)
    state[1] += 1
    return _DropoutRef.apply(x, mask, keep)


def gaussian_noise(x: torch.Tensor, state: torch.Tensor, stddev: float,
                   training: bool = True) -> torch.Tensor:
    """y = x + stddev * N(0, 1) (DL4J GaussianNoise); identity gradient.
    Same state/counter contract as dropout()."""
    if stddev < 0.0:
        raise ValueError(f"gaussian noise stddev must be >= 0, got {stddev}")
    if not training or stddev == 0.0:
        return x
    if x.is_cuda:
        from . import gpu_ops

        return gpu_ops.gaussian_noise(x, state, stddev)
    from . import philox_ref

    seed, calls = (int(v) for v in state.tolist())
    nz = philox_ref.gaussian_noise_ref(x.numel(), seed, calls)
    noise = _storage_flat_like(torch.from_numpy(nz), x)
    state[1] += 1
    if x.dtype == torch.float64:
        return x + stddev * noise
    return (x.float() + stddev * noise.float()).to(x.dtype)


SPECTRAL_EPS = 1e-12


def spectral_normalize(w: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                       training: bool = True) -> torch.Tensor:
    """Spectral normalization W / sigma with the semantics of
    torch.nn.utils.spectral_norm (n_power_iterations=1, eps=1e-12, dim=0).

    w is viewed as the matrix [w.shape[0], -1]; u [rows] and v [cols] are
    the layer's persistent vectors. A training call does one power
    iteration and overwrites u and v IN PLACE:

        t = W^T u;  v = t / max(|t|, eps)
        s = W v;    u = s / max(|s|, eps)
        sigma = u . s;  W_sn = W / max(sigma, eps)

    An eval call takes sigma = u . (W v) from the stored vectors and
    writes nothing. The gradient treats u and v as constants, as torch
    does: dW = (G - <G, W_sn> u v^T) / sigma, with the u, v and sigma of
    the SAME forward (each call keeps its own copies, so a later forward
    does not reach an earlier forward's backward).

    One deliberate deviation from torch: the last division is guarded by
    max(sigma, eps), so a zero matrix gives zeros, not NaN.

    CPU: plain torch in any float dtype (computed in the wider of w's and
    u's dtype). GPU: the _spectral HIP kernels (bf16 W, fp32 u/v)."""
    if w.is_cuda:
        from . import gpu_ops

        return gpu_ops.spectral_normalize(w, u, v, training)
    ct = torch.promote_types(w.dtype, u.dtype)
    wm = w.reshape(w.shape[0], -1).to(ct)
    if training:
        with torch.no_grad():
            wd = wm.detach()
            v_c = F.normalize(torch.mv(wd.t(), u.to(ct)), dim=0,
                              eps=SPECTRAL_EPS)
            u_c = F.normalize(torch.mv(wd, v_c), dim=0, eps=SPECTRAL_EPS)
            v.copy_(v_c)
            u.copy_(u_c)
    else:
        u_c, v_c = u.detach().to(ct, copy=True), v.detach().to(ct, copy=True)
    sigma = torch.dot(u_c, torch.mv(wm, v_c))
    return (wm / sigma.clamp_min(SPECTRAL_EPS)).reshape(w.shape).to(w.dtype)


def bce_with_logits_loss(
    logits: torch.Tensor, labels: torch.Tensor
) -> torch.Tensor:
    """Fused sigmoid+XENT (reference D7: sigmoid + LossFunction.XENT,
    Java:159-164)."""
    if logits.is_cuda:
        from . import gpu_ops

        return gpu_ops.bce_with_logits(logits, labels)
    if logits.dtype != torch.float64:
        logits = logits.float()
    return F.binary_cross_entropy_with_logits(
        logits, labels.to(logits.dtype))


def softmax_cross_entropy(
    logits: torch.Tensor, onehot: torch.Tensor
) -> torch.Tensor:
    """MCXENT with softmax head (reference classifier output, Java:357-363)."""
    if logits.is_cuda:
        from . import gpu_ops

        return gpu_ops.softmax_cross_entropy(logits, onehot)
    if logits.dtype != torch.float64:
        logits = logits.float()
    logp = F.log_softmax(logits, dim=1)
    return -(onehot.to(logits.dtype) * logp).sum(dim=1).mean()


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return F.mse_loss(pred.float(), target.float())


LOSSES = {
    "xent": bce_with_logits_loss,
    "mcxent": softmax_cross_entropy,
    "mse": mse_loss,
}
