"""Bitwise pin of the direct dgrad / convT kernels (conv_dgrad_direct.hip).

For every case dx (conv2d dgrad) or y (convT forward) is computed through
gpu_ops and its SHA-256 over the raw bf16 bytes is compared with
tests/golden/dgrad_direct_digests.json.  The digests were recorded from the
build that preceded the sharing of the three kernels' building blocks, so a
change of any of them that moves a single output bit shows here.  A digest
of the inputs is stored and checked first: a changed input generator is
reported as such and not as a kernel difference.

Only dx / y are pinned.  The bias-gradient and BN-statistics outputs go
through fp32 atomics, whose order is free; the tolerance tests of
test_dgrad_persist_gpu.py and test_dgrad_wide_gpu.py hold them.

Batch 3 throughout: an odd image count, so the wide kernel's image-pair
tile ends in a half tile.  Every instantiation of the three kernels and
both qsplit values appear; the plan of each case is noted next to it
(plan_oneshot / plan_persistent / plan_wide arithmetic; "rgn" is the dy
region in cells, each Ko8 * 2 bytes, which has to fit 48 KiB next to the
two W buffers of the 256-thread kernels).

Running this module as a script writes the JSON (optionally to the path
given as its argument) and is its only writer.
"""

import hashlib
import json
import sys
from pathlib import Path

import pytest
import torch

import dgrad_direct_cases as D

GOLDEN = Path(__file__).resolve().parent / "golden" / \
    "dgrad_direct_digests.json"
NB = 3
P_CAPS = [1, 3, None]      # persistent arm: GDLJ_DGRAD_PERSIST_BLOCKS
W_CAPS = [1, 2, None]      # default arm
ARMS = {"oneshot": (D.ONESHOT, [None]), "persist": (D.WIDE0, P_CAPS),
        "default": (D.WIDE, W_CAPS)}

# (kind, arm, geometry).  dgrad / pact: cin, h, cout, R, pad (the kernel's
# C8 = cin, Ko8 = cout, class grid (h/2)^2); convt: cin, hi, cout, R, pad
# (the kernel's C8 = cout, Ko8 = cin, class grid hi^2).
CASES = [
    # ---- one-shot kernel, grid (tiles, C8/64, 4 classes)
    ("dgrad", "oneshot", (64, 32, 128, 4, 1)),    # <2>: bm 128, rgn 9x17
    ("dgrad", "oneshot", (64, 32, 128, 7, 3)),    # <1>: bm 64, rgn 7x19 (11x19 at bm 128 is too large)
    ("dgrad", "oneshot", (128, 16, 256, 4, 1)),   # <1>: bm 64 = the 8x8 grid, rgn 9x9, 2 c-tiles
    ("pact", "oneshot", (64, 32, 128, 4, 1)),     # <2>, y0 given
    ("convt", "oneshot", (256, 8, 128, 4, 1)),    # <1>: as (128,16,256,4,1), bias + tanh
    ("convt", "oneshot", (128, 16, 64, 4, 1)),    # <2>: as (64,32,128,4,1), bias + tanh
    # ---- persistent kernel <MI,NCT,PACT>, bm = 64 MI, NCT = C8/64
    ("dgrad", "persist", (64, 32, 128, 4, 1)),    # <2,1,F>: bm 128, qsplit 0, rgn 10x18
    ("dgrad", "persist", (128, 32, 128, 4, 1)),   # <2,2,F>: bm 128, qsplit 0, rgn 10x18
    ("dgrad", "persist", (64, 32, 128, 7, 3)),    # <1,1,F>: bm 64, qsplit 0, rgn 7x19
    ("dgrad", "persist", (128, 16, 256, 4, 1)),   # <1,2,F>: bm 64, qsplit 1, rgn 9x10 (10x10x512 B is too large)
    ("dgrad", "persist", (64, 32, 128, 5, 2)),    # <2,1,F>: bm 128, qsplit 0, rgn 10x18, 3+2 taps
    ("convt", "persist", (256, 8, 128, 4, 1)),    # <1,2,F>: bm 64, qsplit 1, bias + tanh
    ("convt", "persist", (128, 16, 64, 4, 1)),    # <2,1,F>: bm 128, qsplit 0, bias + tanh
    ("pact", "persist", (64, 32, 128, 4, 1)),     # <2,1,T>
    ("pact", "persist", (128, 32, 128, 4, 1)),    # <2,2,T>
    ("pact", "persist", (64, 32, 128, 7, 3)),     # <1,1,T>
    ("pact", "persist", (128, 16, 256, 4, 1)),    # <1,2,T>: qsplit 1
    # ---- default routing: wide kernel <NCT,PACT> on the 8x8 class grid
    # (bm 128 = two images, rgn 2 x 10x10, three W buffers)
    ("dgrad", "default", (64, 16, 128, 4, 1)),    # w<1,F>
    ("dgrad", "default", (128, 16, 256, 4, 1)),   # w<2,F>
    ("dgrad", "default", (128, 16, 256, 5, 2)),   # w<2,F>: 3+2 taps, no persistent / one-shot plan
    ("convt", "default", (256, 8, 128, 4, 1)),    # w<2,F>: bias + tanh
    ("convt", "default", (128, 16, 64, 4, 1)),    # not wide (16x16 grid): p<2,1,F>
    ("pact", "default", (64, 16, 128, 4, 1)),     # w<1,T>
    ("pact", "default", (128, 16, 256, 4, 1)),    # w<2,T>
]


def case_id(kind, arm, geom, cap):
    return "%s-%s-%s-cap%s" % (kind, arm, "x".join(map(str, geom)),
                               "none" if cap is None else cap)


PARAMS = [pytest.param(kind, arm, geom, cap,
                       id=case_id(kind, arm, geom, cap))
          for kind, arm, geom in CASES for cap in ARMS[arm][1]]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        assert t.dtype == torch.bfloat16
        h.update(t.contiguous().view(torch.int16).cpu().numpy().tobytes())
    return h.hexdigest()


def want_kind(kind, arm, geom):
    """conv_dgrad_direct_p_eligible of the case's geometry, which does not
    look at the gates: what the persistent / default arm must be able to
    take for the case to run the kernel its comment names."""
    c_in, h, c_out, r, pad = geom
    hk, c8, ko8 = (2 * h, c_out, c_in) if kind == "convt" else (h, c_in,
                                                               c_out)
    return D.p_eligible(hk, c8, ko8, r, pad), hk


def compute(kind, arm, geom, cap):
    """(digest of the inputs, digest of dx / y) of one case."""
    env = ARMS[arm][0]
    c_in, h, c_out, r, pad = geom
    if kind == "dgrad":
        x, w, gout, _ = D.dgrad_case(NB, c_in, h, c_out, r, pad)
        out = D.with_env(env, cap, lambda: D.run_dgrad(x, w, gout, pad))
        ins = (x, w, gout)
    elif kind == "pact":
        ins = D.pact_inputs(NB, c_in, h, c_out, r, pad)
        out = D.with_env(env, cap, lambda: D.run_pact(*ins, pad))[0]
    else:
        x, w, b, _ = D.convt_case(NB, c_in, h, c_out, r, pad)
        out = D.with_env(env, cap, lambda: D.run_convt(x, w, b, pad))
        ins = (x, w, b)
    return digest(*ins), digest(out)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,arm,geom,cap", PARAMS)
def test_dgrad_direct_digest(kind, arm, geom, cap, golden):
    elig, hk = want_kind(kind, arm, geom)
    if arm == "persist":
        assert elig != 0
    elif arm == "default":
        assert elig == (2 if hk == 16 else 1)
    want = golden[case_id(kind, arm, geom, cap)]
    ins, out = compute(kind, arm, geom, cap)
    assert ins == want["inputs"], "the input generator changed"
    assert out == want["output"]


def test_golden_covers_exactly_the_cases(golden):
    # needs no GPU: a case added without its digest fails here already
    assert sorted(golden) == sorted(p.id for p in PARAMS)


if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    rec = {}
    for p in PARAMS:
        ins, out = compute(*p.values)
        rec[p.id] = {"inputs": ins, "output": out}
    path = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(rec, indent=0, sort_keys=True) + "\n")
    print("recorded %d digests -> %s" % (len(rec), path))
