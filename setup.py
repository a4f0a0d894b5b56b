"""In-tree build of the gfx950 HIP extension.

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

Kernels (.hip) are compiled directly by hipcc for gfx950; ext.cpp (torch
bindings) goes through torch.utils.cpp_extension so it links against the
running PyTorch. The resulting _C*.so lives inside the package directory
(it travels with repo snapshots; no JIT cache involvement).

A second module, _spectral (ops/hip/spectral/), is built the same way; the
*.hip glob of _C is not recursive, so _C's sources are what they were.
"""

import os
import subprocess
import sys
from pathlib import Path

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from setuptools import setup  # noqa: E402
from torch.utils import cpp_extension  # noqa: E402

ROOT = Path(__file__).resolve().parent
HIP_DIR = ROOT / "gan_deeplearning4j_amd" / "ops" / "hip"
OBJ_DIR = ROOT / "build" / "hip_obj"

HIP_SOURCES = sorted(HIP_DIR.glob("*.hip"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIP_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-fgpu-rdc" if False else "-fno-gpu-rdc",
    "-c",
]


HIP_HEADERS = sorted(HIP_DIR.glob("*.h"))

SPECTRAL_DIR = HIP_DIR / "spectral"
SPECTRAL_SOURCES = sorted(SPECTRAL_DIR.glob("*.hip"))
# the spectral kernels include ../common.h (and through it launch_abi.h)
SPECTRAL_HEADERS = sorted(SPECTRAL_DIR.glob("*.h")) + HIP_HEADERS


def compile_hip_objects(sources=HIP_SOURCES, headers=HIP_HEADERS,
                        obj_dir=OBJ_DIR) -> list[str]:
    obj_dir.mkdir(parents=True, exist_ok=True)
    objs = []
    for src in sources:
        obj = obj_dir / (src.stem + ".o")
        # stale when older than its source or than ANY header it can see
        if not obj.exists() or obj.stat().st_mtime < max(
                f.stat().st_mtime for f in [src, *headers]):
            cmd = [HIPCC, *HIP_FLAGS, str(src), "-o", str(obj)]
            print("[hipcc]", " ".join(cmd))
            subprocess.run(cmd, check=True)
        objs.append(str(obj))
    return objs


ext = cpp_extension.CUDAExtension(
    name="gan_deeplearning4j_amd._C",
    sources=[str(HIP_DIR / "ext.cpp"), str(HIP_DIR / "csv_loader.cpp")],
    extra_objects=compile_hip_objects(),
    depends=[str(h) for h in HIP_HEADERS],
    extra_compile_args={"cxx": ["-O2"], "nvcc": ["-O2"]},
)

spectral_ext = cpp_extension.CUDAExtension(
    name="gan_deeplearning4j_amd._spectral",
    sources=[str(SPECTRAL_DIR / "spectral_ext.cpp")],
    extra_objects=compile_hip_objects(SPECTRAL_SOURCES, SPECTRAL_HEADERS,
                                      OBJ_DIR / "spectral"),
    depends=[str(h) for h in SPECTRAL_HEADERS],
    extra_compile_args={"cxx": ["-O2"], "nvcc": ["-O2"]},
)

setup(
    name="gan_deeplearning4j_amd",
    version="0.1.0",
    packages=["gan_deeplearning4j_amd"],
    ext_modules=[ext, spectral_ext],
    cmdclass={"build_ext": cpp_extension.BuildExtension},
)
