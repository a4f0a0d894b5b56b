"""Reference Philox4x32-10 stream of the stochastic layers (numpy).

This is the contract `ops/hip/dropout.hip` implements and is tested
against, and it IS the CPU behaviour of `functional.dropout` /
`functional.gaussian_noise`.

Per layer: state int64[2] = [seed, calls]. For the flattened
storage-order tensor, block i covers elements 8i..8i+7:

    counter = (i & 0xffffffff, i >> 32, calls & 0xffffffff, calls >> 32)
    key     = (seed & 0xffffffff, seed >> 32)

Dropout: output word j (0..3) serves element 2j with its low 16 bits and
element 2j+1 with its high 16 bits; kept iff that 16-bit value h < T,
T = round(keep * 65536).

Gaussian noise: block i uses Philox blocks 2i and 2i+1 (same counter
space); each block's words form the Box-Muller pairs (w0,w1), (w2,w3)
with u1 = (wa + 1) * 2^-32 in (0,1], u2 = wb * 2^-32, giving
r*cos(2*pi*u2), r*sin(2*pi*u2), r = sqrt(-2 ln u1) — eight normals for
the eight elements, in that order.
"""

from __future__ import annotations

import math

import numpy as np

M0 = 0xD2511F53
M1 = 0xCD9E8D57
W0 = 0x9E3779B9
W1 = 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10. counter: 4 words (scalars or equal-length uint
    arrays), key: 2 words. Returns uint32 array [..., 4]."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK32
         for w in counter]
    k = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK32
         for w in key]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = k
    m0, m1 = np.uint64(M0), np.uint64(M1)
    sh = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c0            # 32x32 -> 64 bit, exact in uint64
        p1 = m1 * c2
        hi0, lo0 = p0 >> sh, p0 & _MASK32
        hi1, lo1 = p1 >> sh, p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & _MASK32
        k1 = (k1 + np.uint64(W1)) & _MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _blocks(first: int, count: int, seed: int, calls: int) -> np.ndarray:
    """Philox outputs of blocks first .. first+count-1 -> uint32 [count,4]."""
    seed &= 0xFFFFFFFFFFFFFFFF
    calls &= 0xFFFFFFFFFFFFFFFF
    i = np.arange(count, dtype=np.uint64) + np.uint64(first)
    return philox4x32_10(
        (i & _MASK32, i >> np.uint64(32), calls & 0xFFFFFFFF, calls >> 32),
        (seed & 0xFFFFFFFF, seed >> 32))


def keep_threshold(keep: float) -> int:
    return int(math.floor(keep * 65536.0 + 0.5))


def dropout_keep_mask(n: int, seed: int, calls: int, keep: float,
                      first_block: int = 0) -> np.ndarray:
    """bool[n] keep mask of storage-order elements (element e lives in
    block first_block + e // 8)."""
    nb = (n + 7) // 8
    w = _blocks(first_block, nb, seed, calls)              # [nb, 4]
    h = np.empty((nb, 8), dtype=np.uint32)
    h[:, 0::2] = w & np.uint32(0xFFFF)
    h[:, 1::2] = w >> np.uint32(16)
    return (h.reshape(-1)[:n] < keep_threshold(keep))


def pack_mask_bytes(mask: np.ndarray) -> np.ndarray:
    """bool[n] -> uint8[ceil(n/8)], bit j of byte i = element 8i+j."""
    return np.packbits(mask.astype(np.uint8), bitorder="little")


def gaussian_noise_ref(n: int, seed: int, calls: int,
                       first_block: int = 0) -> np.ndarray:
    """float64[n] standard normals of storage-order elements."""
    nb = (n + 7) // 8
    w = _blocks(2 * first_block, 2 * nb, seed, calls).astype(np.float64)
    wa = w[:, 0::2]                                        # [2nb, 2]
    wb = w[:, 1::2]
    u1 = (wa + 1.0) * 2.0 ** -32
    u2 = wb * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty((2 * nb, 4), dtype=np.float64)
    out[:, 0::2] = r * np.cos(2.0 * np.pi * u2)
    out[:, 1::2] = r * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:n]
