"""The Python-visible surface of the _C extension is frozen.

Refactors of the binding layer (ext.cpp / launch_abi.h) must not add, drop
or rename anything gpu_ops.py and the tests can reach.  Importing _C needs
no GPU.  A deliberate change to the surface edits the list below.
"""

import pytest

PUBLIC_NAMES = [
    "DROPOUT_BLOCK",
    "DROPOUT_GRID_CAP",
    "act_bwd",
    "act_bwd_bias",
    "act_fwd",
    "arch",
    "bce_bwd",
    "bce_fwd",
    "bn_bwd",
    "bn_bwd_act",
    "bn_fwd_eval",
    "bn_fwd_train",
    "bn_fwd_train_pre",
    "col2im",
    "col2im_dact",
    "col2im_stats",
    "col_sum",
    "conv_dgrad_direct",
    "conv_dgrad_direct_p_eligible",
    "conv_fwd_implicit",
    "conv_fwd_implicit_fp8",
    "conv_parity_implicit",
    "conv_transpose_fwd_direct",
    "csv_load",
    "dropout_bwd",
    "dropout_fwd",
    "fp8_quantize",
    "fp8_quantize_delayed",
    "fused_adam",
    "fused_rmsprop",
    "gaussian_noise_fwd",
    "gemm_nt",
    "gemm_nt_implicit",
    "gemm_tn",
    "gemm_tn_8p_tweak",
    "gemm_tn_fp8",
    "gemm_tn_stats",
    "im2col",
    "maxpool_bwd",
    "maxpool_fwd",
    "softmax_xent_bwd",
    "softmax_xent_fwd",
    "upsample_bwd",
    "upsample_fwd",
]


def test_ext_public_names_frozen():
    from gan_deeplearning4j_amd.ops.backend import has_hip_ext, hip_ext

    if not has_hip_ext():
        pytest.skip("extension not built")
    ext = hip_ext()
    names = {n for n in dir(ext) if not n.startswith("_")}
    assert names == set(PUBLIC_NAMES)
    assert len(PUBLIC_NAMES) == len(set(PUBLIC_NAMES))
