"""Oracle for the spectral-norm kernels (ops/hip/spectral/spectral_norm.hip):
float64 references taken from the same bf16 inputs, an fp32 emulation of the
kernel formulas, per-element comparators and a named list of wrong
implementations (mutants).

Not collected by pytest.  tests/test_spectral_norm_cpu.py proves on the CPU
that every comparator accepts the fp32 emulation and rejects every mutant;
tests/test_spectral_norm_gpu.py holds the HIP kernels to the same
comparators.  The comparator forms and their policy are those of
tests/membound_oracle.py (imported, not copied): per element, a check
returns the worst error / bound, it passes at <= 1.

Downstream quantities are referenced from the kernel's OWN upstream outputs:
v from its t, s from its v, u' and sigma from its s, 1/sigma and W_sn from
its sigma, dW from its own summed partials and 1/sigma.  Reduction error and
apply error then never hide in each other.

Reduction chains
----------------
The ``reduction`` form allows k 2^-24 sum|term|, k = the number of roundings
a term can pass through.  Each k below is read off the kernel's reduction
tree (SN_* are the launcher constants, asserted equal to the exported ones
by the GPU test), plus 2: one for the reference being rounded to fp32 when
it is compared, one for the term's own product where it is not fused.

* t[k] = sum_m W[m,k] u[m]   (sn_col_partial + sn_col_finish)
    rows of one chunk are accumulated serially with fma (rows_per_chunk
    roundings), then the chunks are added serially (n_chunks roundings).
* s[m] = sum_k W[m,k] v[k]   (sn_row_pass, one wave per row)
    a lane runs 8 independent fma chains over its column groups
    (ceil(K8 / 64) roundings), sum8 adds them in 3 levels, the wave
    shuffle tree adds 6.
* block sums (|t|^2 per 256 columns, |s|^2, u.s, <G, W_sn> per block)
    serial per-thread part, 6 shuffle steps, then the 4 waves in order.
* sum_partials (|t|^2 and <G, W_sn> across blocks)
    ceil(n / 64) serial per lane, then 6 shuffle steps.

A norm enters its consumer as x / max(sqrt(sum), eps): half the relative
error of the sum, one rounding for sqrtf, one for the division, one spare
for the reference's own rounding: (k_sum / 2 + 3) 2^-24 relative.

Inputs
------
* u0 and v0 are random unit vectors, not singular vectors of W; W is dense
  Gaussian noise so |W^T u| and |W v| are far from 1 and from each other.
* G = 0.5 W + noise: with an independent G the u v^T term of the backward
  is 0.5 to 3% of dW and a mutant dropping it could pass.
* the ``tiny`` variant scales W by 2^-30, so |t| ~ 1e-8 and eps = 1e-12
  added to it (instead of max) moves v by ~1e-4 relative; at unit scale that
  mutant is mathematically invisible and is skipped (``applies``).
* at M = 1 the matrix has rank 1: |W^T u| IS sigma and one iteration
  converges, so the two mutants that rely on a difference there are skipped
  at M = 1.  Every mutant is live at one shape at least (asserted by the
  CPU gate).
Rule, as in the membound suite: if a mutant survives, change the inputs,
never the comparator.
"""

import math

import torch

import membound_oracle as O

EPS = 1e-12

# launcher constants of spectral_norm.hip (the GPU test asserts them)
SN_BLOCK = 256
SN_WAVES = SN_BLOCK // 64
SN_GRID_CAP = 1024
SN_CHUNK_ROWS = 16
SN_MAX_CHUNKS = 64

BASE_SHAPES = [(1, 1024), (64, 48), (5, 19), (130, 72)]
# one element past what one block / one grid trip covers
BOUNDARY_SHAPES = [
    (SN_CHUNK_ROWS + 1, 24),                   # second row chunk
    (SN_CHUNK_ROWS * SN_MAX_CHUNKS + 1, 16),   # chunk cap: 17 rows / chunk;
    #                                            also one past grid.y = 1024
    (SN_GRID_CAP * SN_WAVES + 1, 8),           # row pass: second grid trip
    (3, SN_BLOCK * 8 + 1),                     # second column block
    (2, 64 * 8 + 1),                           # row pass: second lane trip
    (1, SN_GRID_CAP * SN_BLOCK * 8 + 1),       # 2-D passes: second x trip
]
BIG_SHAPE = (1024, 8192)
ALL_SHAPES = BASE_SHAPES + BOUNDARY_SHAPES + [BIG_SHAPE]
TINY_SCALE = 2.0 ** -30


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------ chain lengths
def n_chunks(m):
    return min(cdiv(m, SN_CHUNK_ROWS), SN_MAX_CHUNKS)


def k_t(m):
    return cdiv(m, n_chunks(m)) + n_chunks(m) + 2


def k_s(k):
    return cdiv(cdiv(k, 8), 64) + 3 + 6 + 2


def k_block(per_thread):
    return per_thread + 6 + SN_WAVES + 2


def k_partials(n):
    return cdiv(n, 64) + 6


def k_nsq(k):
    # t^2 (1 rounding), block tree per 256 columns, partials across blocks
    return 1 + k_block(0) + k_partials(cdiv(k, SN_BLOCK))


def k_ssq(m):
    return k_block(cdiv(m, SN_BLOCK))


def grid2d(m, k):
    gx = min(cdiv(cdiv(k, 8), SN_BLOCK), SN_GRID_CAP)
    gy = max(1, min(SN_GRID_CAP // gx, m))
    return gx, gy


def k_dot_block(m, k):
    gx, gy = grid2d(m, k)
    trips = cdiv(m, gy) * cdiv(cdiv(k, 8), gx * SN_BLOCK)
    return trips + 3 + k_block(0)


def norm_rel(k_sum):
    return (0.5 * k_sum + 3) * O.U32


# ------------------------------------------------------------------ inputs
def unit(n, gen):
    x = torch.randn(n, generator=gen, dtype=torch.float64)
    return (x / x.norm()).float()


def inputs(m, k, seed, tiny=False):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(m, k, generator=gen)
    noise = torch.randn(m, k, generator=gen)
    g = O.bf(0.5 * w + noise)
    if tiny:
        w = w * TINY_SCALE
    return {"m": m, "k": k, "tiny": tiny, "w": O.bf(w), "g": g,
            "u0": unit(m, gen), "v0": unit(k, gen)}


def planted_gap_weight():
    """W = bf16(4 a b^T + 0.05 N) at 96 x 200, generator seed 666."""
    gen = torch.Generator().manual_seed(666)
    a = torch.randn(96, generator=gen, dtype=torch.float64)
    b = torch.randn(200, generator=gen, dtype=torch.float64)
    a, b = a / a.norm(), b / b.norm()
    noise = torch.randn(96, 200, generator=gen, dtype=torch.float64)
    w = O.bf((4.0 * torch.outer(a, b) + 0.05 * noise).float())
    return w, unit(96, gen), unit(200, gen)


def planted_gap_check(w_sn):
    """|sigma_1(W_sn) - 1| against the spectral-norm perturbation of one
    bf16 rounding per element: 2^-9 |W_sn|_F + 1e-5.  Returns (err, bound)."""
    wd = O.d(w_sn)
    s1 = float(torch.linalg.svdvals(wd)[0])
    return abs(s1 - 1.0), 2.0 ** -9 * float(wd.norm()) + 1e-5


# ------------------------------------------------------------ fp32 emulation
def _norm32(x):
    return torch.sqrt((x * x).sum())


def fwd_emulate(inp, mutant=None):
    """One training forward in fp32, the kernel's formulas.  Returns the
    kernel's outputs plus the state after the call (u_state, v_state)."""
    w = inp["w"].float()
    u0, v0 = inp["u0"], inp["v0"]
    eps = torch.tensor(EPS, dtype=torch.float32)
    t = w.t().mv(u0)
    nt = _norm32(t)
    if mutant == "v_unnormalised":
        v = t.clone()
    elif mutant == "eps_added":
        v = t / (nt + eps)
    else:
        v = t / torch.maximum(nt, eps)
    s = w.mv(v0 if mutant == "stale_v" else v)
    ns = _norm32(s)
    if mutant == "u_unnormalised":
        u = s.clone()
    elif mutant == "eps_added":
        u = s / (ns + eps)
    else:
        u = s / torch.maximum(ns, eps)
    sigma = nt.clone() if mutant == "sigma_is_norm_t" else torch.dot(u, s)
    if mutant == "eps_added":
        inv = 1.0 / (sigma + eps)
    else:
        inv = 1.0 / torch.maximum(sigma, eps)
    w_sn = O.bf(w * sigma) if mutant == "times_sigma" else O.bf(w * inv)
    return {"t": t, "s": s, "v": v, "u": u,
            "sig": torch.stack([sigma, inv]), "w_sn": w_sn,
            "u_copy": u.clone(), "v_copy": v.clone(),
            "u_state": u.clone(), "v_state": v.clone()}


def eval_emulate(inp, mutant=None):
    """Eval forward from the stored (u0, v0); writes no state."""
    w = inp["w"].float()
    u0, v0 = inp["u0"], inp["v0"]
    eps = torch.tensor(EPS, dtype=torch.float32)
    s = w.mv(v0)
    sigma = torch.dot(u0, s)
    inv = 1.0 / torch.maximum(sigma, eps)
    out = {"s": s, "sig": torch.stack([sigma, inv]), "w_sn": O.bf(w * inv),
           "u_state": u0.clone(), "v_state": v0.clone()}
    if mutant == "eval_writes_state":
        out["u_state"] = s / torch.maximum(_norm32(s), eps)
    return out


def bwd_inputs(inp):
    """State of a first forward (what backward must use) and of a second
    forward run after it (what it must not)."""
    f1 = fwd_emulate(inp)
    f2 = fwd_emulate({**inp, "u0": f1["u_state"], "v0": f1["v_state"]})
    return {**inp, "w_sn": f1["w_sn"], "u": f1["u_copy"], "v": f1["v_copy"],
            "sig": f1["sig"], "u_later": f2["u_copy"],
            "v_later": f2["v_copy"], "sig_later": f2["sig"]}


def bwd_emulate(binp, mutant=None):
    g = binp["g"].float()
    u, v, sig = binp["u"], binp["v"], binp["sig"]
    if mutant == "later_state":
        u, v, sig = binp["u_later"], binp["v_later"], binp["sig_later"]
    other = binp["w"].float() if mutant == "dot_with_w" else \
        binp["w_sn"].float()
    dot = (g * other).sum()
    if mutant == "no_uv_term":
        dw = g * sig[1]
    else:
        dw = (g - (dot * u)[:, None] * v[None, :]) * sig[1]
    # dot_part: the per-block partials; their fp64 sum is "the kernel's dot"
    return {"dw": O.bf(dw), "dot_part": dot.reshape(1)}


# -------------------------------------------------------------- comparators
def _rel(got, ref, rel):
    return O._ratio(got, ref, rel * ref.abs())


def fwd_check(inp, out):
    m, k = inp["m"], inp["k"]
    w, u0 = O.d(inp["w"]), O.d(inp["u0"])
    t, s, v, u = (O.d(out[n]) for n in ("t", "s", "v", "u"))
    sigma, inv = O.d(out["sig"])
    r = {}
    r["t"] = O.reduction(out["t"], w.t().mv(u0), w.abs().t().mv(u0.abs()),
                         k_t(m))
    r["v"] = _rel(out["v"], t / t.norm().clamp_min(EPS), norm_rel(k_nsq(k)))
    r["s"] = O.reduction(out["s"], w.mv(v), w.abs().mv(v.abs()), k_s(k))
    rel_u = norm_rel(k_ssq(m))
    u_ref = s / s.norm().clamp_min(EPS)
    r["u"] = _rel(out["u"], u_ref, rel_u)
    # sigma = sum u_m s_m with each u_m known to rel_u
    r["sigma"] = O.reduction(
        out["sig"][0:1], torch.dot(u_ref, s).reshape(1),
        (u_ref * s).abs().sum().reshape(1), k_ssq(m) + rel_u / O.U32)
    r["inv_sigma"] = _rel(out["sig"][1:2],
                          (1.0 / sigma.clamp_min(EPS)).reshape(1), 2 * O.U32)
    ref_w = w / sigma.clamp_min(EPS)
    # floor: the rounding of 1/sigma and of the product, in output units
    r["w_sn"] = O.pointwise(out["w_sn"], ref_w, O.ulp32(ref_w))
    r["u_copy"] = O.exact(out["u_copy"], out["u"])
    r["v_copy"] = O.exact(out["v_copy"], out["v"])
    r["u_state"] = O.exact(out["u_state"], out["u"])
    r["v_state"] = O.exact(out["v_state"], out["v"])
    return r


def eval_check(inp, out):
    k = inp["k"]
    w, u0, v0 = O.d(inp["w"]), O.d(inp["u0"]), O.d(inp["v0"])
    s = O.d(out["s"])
    sigma = O.d(out["sig"])[0]
    r = {}
    r["s"] = O.reduction(out["s"], w.mv(v0), w.abs().mv(v0.abs()), k_s(k))
    r["sigma"] = O.reduction(
        out["sig"][0:1], torch.dot(u0, s).reshape(1),
        (u0 * s).abs().sum().reshape(1), k_ssq(inp["m"]))
    r["inv_sigma"] = _rel(out["sig"][1:2],
                          (1.0 / sigma.clamp_min(EPS)).reshape(1), 2 * O.U32)
    ref_w = w / sigma.clamp_min(EPS)
    r["w_sn"] = O.pointwise(out["w_sn"], ref_w, O.ulp32(ref_w))
    r["u_unchanged"] = O.exact(out["u_state"], inp["u0"])
    r["v_unchanged"] = O.exact(out["v_state"], inp["v0"])
    return r


def bwd_check(binp, out):
    m, k = binp["m"], binp["k"]
    g, w_sn = O.d(binp["g"]), O.d(binp["w_sn"])
    u, v = O.d(binp["u"]), O.d(binp["v"])
    inv = O.d(binp["sig"])[1]
    part = O.d(out["dot_part"])
    dot = part.sum()
    abs_dot = (g * w_sn).abs().sum()
    r = {}
    # the partials, summed exactly: only the in-block chain is in play
    r["dot"] = O.reduction(dot.reshape(1), (g * w_sn).sum().reshape(1),
                           abs_dot.reshape(1), k_dot_block(m, k))
    uv = torch.outer(u, v)
    ref = (g - dot * uv) * inv
    # floor: one fp32 ulp of the addends' magnitudes (the subtraction can
    # cancel) plus what sum_partials can add to dot, both in output units
    k_sp = k_partials(part.numel())
    floor = (O.ulp32(g.abs() + 2 * (dot * uv).abs())
             + k_sp * O.U32 * abs_dot * uv.abs()) * inv.abs() \
        + O.ulp32(ref)
    r["dw"] = O.pointwise(out["dw"], ref, floor)
    return r


# ------------------------------------------------------------------ mutants
def _always(inp):
    return True


def _rank_above_1(inp):
    return inp["m"] > 1


def _tiny(inp):
    return inp["tiny"]


FWD_MUTANTS = {
    "sigma_is_norm_t": _rank_above_1,   # sigma taken as |W^T u|
    "u_unnormalised": _always,
    "v_unnormalised": _always,
    "stale_v": _always,                 # row pass on the previous call's v
    "times_sigma": _always,             # W * sigma instead of W / sigma
    "eps_added": _tiny,                 # x / (|x| + eps), not max
}
EVAL_MUTANTS = {
    "eval_writes_state": _always,
}
BWD_MUTANTS = {
    "no_uv_term": _always,
    "dot_with_w": _always,              # <G, W> instead of <G, W_sn>
    "later_state": _rank_above_1,       # u, v, sigma of a later forward
}
MUTANT_COUNT = len(FWD_MUTANTS) + len(EVAL_MUTANTS) + len(BWD_MUTANTS)

worst = O.worst
