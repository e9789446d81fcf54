"""The transformer row kernels (csrc/sp_transformer.hip, csrc/sp_bf16_rows.hip) in fp64 closed
form, the value cases that separate a careful fp32 row kernel from a fragile one, the bounds the
kernels are held to, a plain fp32 torch emulation of each kernel's arithmetic (the yardstick
that keeps every bound possible), and the tables of widths the GPU tests run.

LayerNorm.  A row of c channels is a GroupNorm group with groups = 1, h = w = 1, so the
reference is ``gn_ref.gn_fp64`` on the 2-D rows and the inputs are ``gn_ref.make_case`` at
shape (rows, c, 1, 1, 1) with its chan_bias ignored; ``rstd_error``, ``mean_excess``,
``forward_excess``, ``vjp_error`` and FWD_TOL / STAT_TOL / VJP_TOL / ULP apply as they stand.
The gn cases kept are 1, 2, 3, 4, 5, 6, 8, 9 (3 only above c = 8, where it does not make the row
constant), plus ``mean_30_std_1`` (randn + 30).  gn case 7 (mean 1e3, spread 1e-2) is left out:
the row kernels are two-pass in fp32 — mean = fl(sum x / c), then deviations from that rounded
mean — and one rounding of a mean of 1e3 is 6e-5, 6e-3 of that spread, so the emulation of this
arithmetic is 1.5x outside the gn bounds there and torch's own fp32 LayerNorm sits at 0.75 of
them.  The case asks for more than a two-pass fp32 row kernel gives, and token rows of a
transformer do not look like that; randn + 1e3 is marginal for the same reason (0.96 / 0.90 of
the bounds) and is left out too.  A shifted-mean row kernel would be a kernel change.

bf16 LayerNorm reads bf16 x / dy / add (the cases above, rounded to bf16; the reference is fp64
of the rounded inputs), computes in fp32, writes fp32 ``mean`` / ``rstd`` (held to the fp32
STAT_TOL forms) and rounds y and dx once to bf16 (2^-8 relative at the most):

    |y - ref| <= 2^-8 |ref| + FWD_TOL max(1, |ref|) + ULP |mean| rstd |gamma_c|     per element
    max |dx - ref| / max |ref| <= 2^-8 + VJP_TOL                                      per row

GEGLU.  y = a gelu(g), da = dy gelu(g), dgate = dy a gelu'(g) with gelu(g) = g Phi(g),
gelu'(g) = Phi(g) + g phi(g).  The reference takes Phi(g) = erfc(-g / sqrt 2) / 2, so its own
tail does not cancel (1 + erf(x) loses every digit below x = -5.9 in fp32 and below -8.3 in
fp64).  Gates: GATE_TABLE (specials first, then the band -6.5 .. -5 where the fp32 1 + erff()
cancels to 0, then a ramp over [-12, 12]); all finite (at -inf torch and the kernels both give
NaN, which is not tested).  Per element, K = GEGLU_K = 12:

    |y - ref|     <= K ULP |a|  max(1, |g|) + 2^-126
    |da - ref|    <= K ULP |dy| max(1, |g|) + 2^-126
    |dgate - ref| <= K ULP |dy a|           + 2^-126

(bf16: + 2^-8 |ref| each, against fp64 of the bf16-rounded inputs).  In these units the fp32
emulation of the kernels' formula measures 1.3 / 1.3 / 1.8 and torch's own fp32 ``F.gelu`` 1.6
on these inputs (tests/test_rows_ref.py prints them; 2.9 has been seen from ``F.gelu`` on other
builds, and K was set as 4x that), which leaves room for a device erff / expf of a few ulp.
2^-126: flush-to-zero is allowed.

Row softmax.  p = exp(s - max) / sum, lse = max + log(sum); VJP ds = scale p (dp - sum(p dp)).
With gap = max - s (0 where s = -inf), K = SOFTMAX_K = 8:

    |p - ref|         <= K ULP ref (1 + gap) + 2^-126      (s - max is rounded before exp)
    |lse - ref|       <= K ULP max(1, |ref|)
    |sum_row(p) - 1|  <= K ULP
    |ds - ref|        <= K ULP scale p max_row|dp| + 2^-126

and a -inf score gives exactly 0.  The VJP is judged on its own: its ``p`` is the fp64 softmax
rounded to fp32.  The fp32 emulation measures at most 1.9 / 0.6 / 1.9 / 1.6 of these units (the
device sums in another order and its expf is not torch's, hence about 4x).

1x1 conv over 4 / 8 channels.  Integer cases (weights in [-8, 8], bias and x in [-64, 64]):
every partial sum is an integer below 2^24, so the result must equal the int64 einsum bit for
bit, forward with and without bias and with trans = 1.  One randn case per channel count:
|err| <= (C + 1) ULP (sum_c |w||x| + |b|), the bound of a length-C fma chain.

Everything here runs on the CPU.
"""

from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

import gn_ref
from gn_ref import FWD_TOL, STAT_TOL, ULP, VJP_TOL  # noqa: F401  (re-exported to the tests)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TINY = 2.0 ** -126            # the smallest normal fp32: what flush-to-zero may cost
BF16_EPS = 2.0 ** -8          # one rounding to bf16 (8 significant bits), relative
ROWS = 9                      # two full workgroups (4 rows each) plus one wave
TAIL = 64                     # NaN elements the GPU tests keep behind every output buffer


def _gen(*key: int) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rb(t: torch.Tensor) -> torch.Tensor:
    """``t`` rounded to bf16, as fp32."""
    return t.to(BF16).to(F32)


# =============================================================================================
# LayerNorm
# =============================================================================================
MEAN_30 = 11
LN_CASES = {k: gn_ref.CASES[k] for k in (1, 2, 3, 4, 5, 6, 8, 9)} | {MEAN_30: "mean_30_std_1"}
LN_ALL = tuple(LN_CASES)
LN_FEW = (1, 2, 5, MEAN_30)

# width -> the cases run there (fp32: csrc/sp_transformer.hip; NV = ceil(c / 4 / 64))
LN_WIDTHS = (4, 252, 256, 260, 320, 768, 1024, 1280, 1536, 1540, 1792, 2044, 2048)
LN_ALL_AT = (260, 320)
# bf16: csrc/sp_bf16_rows.hip; NV = ceil(c / 8 / 64)
LN_BF16_WIDTHS = (8, 504, 512, 520, 1024, 1536, 1544, 2040, 2048)
LN_BF16_ALL_AT = (520,)
LN_EPS_ONCE = (320, 1e-5)     # the one (width, eps) besides EPS = 1e-6 (bf16: 520)
LN_BF16_EPS_ONCE = (520, 1e-5)


def ln_nv(c: int) -> int:
    """NV of k_layernorm_fwd/bwd<NV> that sp_layernorm_* dispatches c to (supported: <= 8)."""
    return (c // 4 + 63) // 64


def ln_bf16_nv(c: int) -> int:
    """NV of k_layernorm_bf16_fwd/bwd<NV> (supported: <= 4)."""
    return (c // 8 + 63) // 64


def ln_cases_at(c: int, bf16: bool = False) -> tuple:
    cases = LN_ALL if c in (LN_BF16_ALL_AT if bf16 else LN_ALL_AT) else LN_FEW
    return tuple(k for k in cases if not (k == 3 and c <= 8))


class LnCase(NamedTuple):
    x: torch.Tensor       # [rows][c] fp32 (bf16: bf16-representable)
    gamma: torch.Tensor   # [c] fp32 in [0.5, 1.5]
    beta: torch.Tensor    # [c] fp32
    dz: torch.Tensor      # [rows][c]
    add: torch.Tensor     # [rows][c] addend of the input VJP


@functools.lru_cache(maxsize=4)
def ln_case(case: int, rows: int, c: int, bf16: bool = False) -> LnCase:
    """LayerNorm value case ``case`` (a key of LN_CASES) on [rows][c]."""
    base = gn_ref.make_case(1 if case == MEAN_30 else case, (rows, c, 1, 1, 1))
    x = base.x.reshape(rows, c).clone()
    if case == MEAN_30:
        x += 30.0
    dz, add = base.dz.reshape(rows, c).clone(), base.add.reshape(rows, c).clone()
    if bf16:
        x, dz, add = rb(x), rb(dz), rb(add)
    return LnCase(x, base.gamma.clone(), base.beta.clone(), dz, add)


@functools.lru_cache(maxsize=4)
def ln_reference(case: int, rows: int, c: int, eps: float = gn_ref.EPS, with_add: bool = False,
                 bf16: bool = False) -> gn_ref.GnRef:
    """fp64 mean / rstd [rows], y and dx [rows][c] of ``ln_case`` (the tests leave it unchanged)."""
    t = ln_case(case, rows, c, bf16)
    return ln_fp64(t.x, t.gamma, t.beta, eps, t.dz, t.add if with_add else None)


def ln_fp64(x, gamma, beta, eps: float, dz=None, add=None) -> gn_ref.GnRef:
    return gn_ref.gn_fp64(x, 1, gamma, beta, eps, False, None, dz, add)


def ln_bf16_forward_excess(y, ref: gn_ref.GnRef, gamma) -> float:
    """max over elements of |y - ref| / (2^-8 |ref| + FWD_TOL max(1, |ref|) + ULP |mean| rstd |gamma_c|)"""
    y = y.double().cpu()
    assert torch.isfinite(y).all()
    rep = (ULP * ref.mean.abs() * ref.rstd)[:, None] * gamma.double().cpu().abs()[None, :]
    bound = BF16_EPS * ref.z.abs() + FWD_TOL * ref.z.abs().clamp_min(1.0) + rep
    return float(((y - ref.z).abs() / bound).max())


LN_BF16_VJP_TOL = BF16_EPS + VJP_TOL


def ln_figures(mean, rstd, y, dx, ref: gn_ref.GnRef, gamma, bf16: bool = False) -> dict:
    """{metric: (value, bound)} of one LayerNorm forward + VJP; every value must be <= its bound."""
    fwd = ln_bf16_forward_excess(y, ref, gamma) if bf16 else gn_ref.forward_excess(y, ref, gamma, 1)
    return {
        "rstd_rel": (gn_ref.rstd_error(rstd, ref), STAT_TOL),
        "mean_of_bound": (gn_ref.mean_excess(mean, ref), 1.0),
        "fwd_of_bound": (fwd, 1.0),
        "vjp_per_row": (gn_ref.vjp_error(dx, ref, 1), LN_BF16_VJP_TOL if bf16 else VJP_TOL),
    }


def ln_emulate(t: LnCase, eps: float, with_add: bool, bf16: bool = False):
    """(mean, rstd, y, dx) of the kernels' arithmetic in torch fp32 on the CPU: the two-pass
    statistics about the rounded mean, rstd = 1 / sqrt, the VJP from xhat = (x - mean) rstd and
    the saved statistics; bf16: y and dx rounded once."""
    x, c = t.x, t.x.shape[1]
    mu = x.sum(1, keepdim=True) / c
    d = x - mu
    rs = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / c + torch.tensor(eps, dtype=F32))
    y = d * rs * t.gamma + t.beta
    g, h = t.dz * t.gamma, d * rs
    m1, m2 = (g * h).sum(1, keepdim=True) * (1.0 / c), g.sum(1, keepdim=True) * (1.0 / c)
    dx = rs * (g - m2 - h * m1)
    if with_add:
        dx = dx + t.add
    assert y.dtype == F32 and dx.dtype == F32
    if bf16:
        y, dx = rb(y), rb(dx)
    return mu.reshape(-1), rs.reshape(-1), y, dx


# =============================================================================================
# GEGLU
# =============================================================================================
GEGLU_K = 12.0
GEGLU_SHAPES = ((1, 4), (7, 12), (9, 1280))          # fp32 (rows, f); bf16 doubles f below 1280
GEGLU_BF16_SHAPES = ((1, 8), (7, 24), (9, 1280))
GEGLU_TRIP = (6560, 1280)                            # 8,396,800 elements: 2048 past one trip
GEGLU_GRID_CAP, GEGLU_VEC = 8192, 4                  # stream_grid (sp_transformer.hip), float4
GEGLU_BF16_GRID_CAP, GEGLU_BF16_VEC = 4096, 8        # stream_blocks (sp_bf16.h), 8 x bf16
BLOCK = 256


def trip_elements(grid_cap: int, vec: int) -> int:
    """Output elements one trip of a capped grid-stride loop covers."""
    return grid_cap * BLOCK * vec


def _gate_table() -> torch.Tensor:
    special = [0.0, 1e-30, -1e-30, 1e-40, -1e-40, 38.0, -38.0, 1e4, -1e4, 3e19, -3e19]
    band = torch.linspace(-6.5, -5.0, 601, dtype=F64)
    ramp = torch.linspace(-12.0, 12.0, 2049, dtype=F64)
    return torch.cat([torch.tensor(special, dtype=F64), band, ramp]).to(F32)


GATE_TABLE = _gate_table()    # 2661 values: odd against every f, so a value meets every lane


def _sprinkle(t: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    """randn with about 1/16 of the entries exactly 0 and 1/16 at +-1e4."""
    u = torch.rand(t.shape, generator=gen)
    t = torch.where(u < 1 / 16, torch.zeros_like(t), t)
    t = torch.where((u >= 1 / 16) & (u < 3 / 32), torch.full_like(t, 1e4), t)
    return torch.where((u >= 3 / 32) & (u < 1 / 8), torch.full_like(t, -1e4), t)


def geglu_case(rows: int, f: int, bf16: bool = False):
    """(h [rows][2 f] = [a | gate], dy [rows][f]) fp32 (bf16: bf16-representable): the gate table
    tiled over the gates in memory order, a and dy randn with exact zeros and +-1e4."""
    gen = _gen(rows, f, 7)
    a = _sprinkle(torch.randn(rows, f, generator=gen), gen)
    dy = _sprinkle(torch.randn(rows, f, generator=gen), gen)
    reps = (rows * f + GATE_TABLE.numel() - 1) // GATE_TABLE.numel()
    gate = GATE_TABLE.repeat(reps)[:rows * f].reshape(rows, f)
    h = torch.cat([a, gate], 1).contiguous()
    return (rb(h), rb(dy)) if bf16 else (h, dy)


class GegluRef(NamedTuple):
    y: torch.Tensor       # [rows][f] fp64
    da: torch.Tensor
    dgate: torch.Tensor


def geglu_fp64(h: torch.Tensor, dy: torch.Tensor) -> GegluRef:
    a, g = h.double().chunk(2, -1)
    d = dy.double()
    cdf = 0.5 * torch.special.erfc(-g / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)
    gelu = g * cdf
    return GegluRef(a * gelu, d * gelu, d * a * (cdf + g * pdf))


def geglu_figures(y, dh, h, dy, ref: GegluRef, bf16: bool = False) -> dict:
    """{metric: (value, bound, flat index of the worst element)}: the largest
    |err| / (ULP scale + 2^-126 / K) per output in units of ULP (fp32: bound K), or, for bf16,
    |err| / (K ULP scale + 2^-126 + 2^-8 |ref|) (bound 1)."""
    a, g = h.cpu().double().chunk(2, -1)
    d = dy.cpu().double()
    y, dh = y.cpu().double(), dh.cpu().double()
    assert torch.isfinite(y).all() and torch.isfinite(dh).all()
    da, dg = dh.chunk(2, -1)
    gm = g.abs().clamp_min(1.0)
    out = {}
    for name, got, want, scale in (("y", y, ref.y, a.abs() * gm), ("da", da, ref.da, d.abs() * gm),
                                   ("dgate", dg, ref.dgate, (d * a).abs())):
        err = (got - want).abs()
        if bf16:
            q, bound = err / (GEGLU_K * ULP * scale + TINY + BF16_EPS * want.abs()), 1.0
        else:
            q, bound = err / (ULP * scale + TINY / GEGLU_K), GEGLU_K
        i = int(q.argmax())
        out[f"geglu_{name}"] = (float(q.reshape(-1)[i]), bound, i)
    return out


def geglu_emulate(h: torch.Tensor, dy: torch.Tensor, bf16: bool = False):
    """(y, dh) of the kernels' formula in torch fp32 on the CPU: gelu = 0.5 g (1 + erf(g sqrt 1/2)),
    gelu' = 0.5 (1 + erf) + g exp(-g^2 / 2) / sqrt(2 pi); bf16: outputs rounded once."""
    a, g = h.chunk(2, -1)
    r = torch.tensor(0.70710678118654752, dtype=F32)
    e = 1.0 + torch.erf(g * r)
    gelu = 0.5 * g * e
    # the kernel's g * g overflows to inf at 3e19 and exp(-inf) = 0; torch does the same
    grad = 0.5 * e + g * (torch.exp(-0.5 * g * g) * torch.tensor(0.39894228040143268, dtype=F32))
    y, dh = a * gelu, torch.cat([dy * gelu, dy * a * grad], 1)
    assert y.dtype == F32 and dh.dtype == F32
    return (rb(y), rb(dh)) if bf16 else (y, dh)


# =============================================================================================
# Row softmax
# =============================================================================================
SOFTMAX_K = 8.0
SM_CASES = ("randn_x4", "all_equal", "peak_first", "peak_middle", "peak_last", "randn_plus_3e4",
            "randn_x30_minus_1e4", "randn_x60", "masked")
SM_FEW = ("randn_x4", "peak_last", "masked")
SM_WIDTHS = (4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4092, 4096)
SM_ALL_AT = (260, 516, 1028, 2052)
SM_DP = ("randn", "randn_plus_1e3")
SM_SCALES = (0.5, 512 ** -0.5)


def sm_nv(n: int) -> int:
    """NV of k_softmax_rows / k_softmax_bwd_rows<NV> that n scores dispatch to (n <= 4096)."""
    nv = (n // 4 + 63) // 64
    return 1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8 if nv <= 8 else 16


def sm_cases_at(n: int) -> tuple:
    return SM_CASES if n in SM_ALL_AT else SM_FEW


def softmax_case(case: str, rows: int, n: int) -> torch.Tensor:
    """Scores [rows][n] fp32 of one value case (every row its own draw)."""
    r = torch.randn(rows, n, generator=_gen(rows, n, SM_CASES.index(case)))
    if case == "randn_x4":
        return r * 4
    if case == "all_equal":
        return torch.full((rows, n), 0.75)
    if case in ("peak_first", "peak_middle", "peak_last"):
        i = {"peak_first": 0, "peak_middle": n // 2, "peak_last": n - 1}[case]
        r[:, i] += 80.0
        return r
    if case == "randn_plus_3e4":
        return r + 3e4
    if case == "randn_x30_minus_1e4":
        return 30 * r - 1e4
    if case == "randn_x60":
        return 60 * r
    if case == "masked":
        r = r * 4
        last = r[:, n - 1].clone()
        r[:, 0::3] = -math.inf
        r[:, n - 1] = last  # the last active lane's last element stays finite
        return r
    raise ValueError(case)


class SoftmaxRef(NamedTuple):
    p: torch.Tensor       # [rows][n] fp64
    lse: torch.Tensor     # [rows]
    gap: torch.Tensor     # [rows][n] max - s, 0 where s = -inf


def softmax_fp64(s: torch.Tensor) -> SoftmaxRef:
    s = s.double()
    m = s.amax(1, keepdim=True)
    e = torch.exp(s - m)
    z = e.sum(1, keepdim=True)
    gap = torch.where(torch.isinf(s), torch.zeros_like(s), m - s)
    return SoftmaxRef(e / z, (m + torch.log(z)).reshape(-1), gap)


def softmax_figures(p, lse, ref: SoftmaxRef, s: torch.Tensor) -> dict:
    """{metric: (value in units of ULP, K, flat index or (row,))}; ``lse`` may be None.  Also asserts that
    the -inf scores came out exactly 0."""
    p = p.double().cpu()
    assert torch.isfinite(p).all()
    masked = torch.isinf(s)
    assert bool((p[masked] == 0).all()), "a -inf score did not give exactly 0"
    out = {}
    q = (p - ref.p).abs() / (ULP * ref.p * (1 + ref.gap) + TINY / SOFTMAX_K)
    i = int(q.argmax())
    out["softmax_p"] = (float(q.reshape(-1)[i]), SOFTMAX_K, i)
    q = (p.sum(1) - 1).abs() / ULP
    i = int(q.argmax())
    out["softmax_rowsum"] = (float(q[i]), SOFTMAX_K, (i,))
    if lse is not None:
        lse = lse.double().cpu()
        assert torch.isfinite(lse).all()
        q = (lse - ref.lse).abs() / (ULP * ref.lse.abs().clamp_min(1.0))
        i = int(q.argmax())
        out["softmax_lse"] = (float(q[i]), SOFTMAX_K, (i,))
    return out


def softmax_emulate(s: torch.Tensor):
    """(p, lse) of the kernel's arithmetic in torch fp32 on the CPU."""
    m = s.amax(1, keepdim=True)
    e = torch.exp(s - m)
    z = e.sum(1, keepdim=True)
    return e * (1.0 / z), (m + torch.log(z)).reshape(-1)


def softmax_vjp_case(kind: str, rows: int, n: int) -> torch.Tensor:
    r = torch.randn(rows, n, generator=_gen(rows, n, 100 + SM_DP.index(kind)))
    return r + 1e3 if kind == "randn_plus_1e3" else r


def softmax_vjp_fp64(p32: torch.Tensor, dp: torch.Tensor, scale: float) -> torch.Tensor:
    """ds = scale p (dp - sum(p dp)) in fp64 of the fp32 operands; ``scale`` as the kernel gets
    it (a C float)."""
    p, d = p32.double(), dp.double()
    sc = float(torch.tensor(scale, dtype=F32))
    return sc * p * (d - (p * d).sum(1, keepdim=True))


def softmax_vjp_figures(ds, ref: torch.Tensor, p32: torch.Tensor, dp: torch.Tensor, scale: float) -> dict:
    ds = ds.double().cpu()
    assert torch.isfinite(ds).all()
    unit = ULP * scale * p32.double() * dp.double().abs().amax(1, keepdim=True) + TINY / SOFTMAX_K
    q = (ds - ref).abs() / unit
    i = int(q.argmax())
    return {"softmax_vjp": (float(q.reshape(-1)[i]), SOFTMAX_K, i)}


def softmax_vjp_emulate(p32: torch.Tensor, dp: torch.Tensor, scale: float) -> torch.Tensor:
    d = (p32 * dp).sum(1, keepdim=True)
    return torch.tensor(scale, dtype=F32) * p32 * (dp - d)


# =============================================================================================
# 1x1 conv over 4 / 8 channels
# =============================================================================================
CONV_C = (4, 8)
CONV_HW = (4, 8, 1028)
CONV_N = (1, 3)
CONV_TRIP = (4, 1, 2 ** 22 + 1024)    # (c, n, hw): 1,048,832 float4 pixels, 256 past one trip
CONV_GRID_CAP, CONV_VEC = 4096, 4


def conv_int_case(c: int, n: int, hw: int):
    """(x [n][c][hw], w [c][c], b [c]) fp32 holding integers: |w| <= 8, |x|, |b| <= 64, so
    sum_c |w||x| + |b| <= 8 * 8 * 64 + 64 < 2^24 and every partial sum is exact."""
    gen = _gen(c, n, hw % 100003, 3)
    x = torch.randint(-64, 65, (n, c, hw), generator=gen).to(F32)
    w = torch.randint(-8, 9, (c, c), generator=gen).to(F32)
    b = torch.randint(-64, 65, (c,), generator=gen).to(F32)
    return x, w, b


def conv_randn_case(c: int, n: int, hw: int):
    gen = _gen(c, n, hw, 4)
    return (torch.randn(n, c, hw, generator=gen), torch.randn(c, c, generator=gen) * c ** -0.5,
            torch.randn(c, generator=gen))


def conv_exact(x, w, b, trans: bool) -> torch.Tensor:
    """The int64 result of an integer case: y[n][o][p] = sum_c w[o][c] x[n][c][p] + b[o], or with
    ``trans`` sum_c w[c][o] x[n][c][p]."""
    xi, wi = x.long(), w.long()
    y = torch.einsum("co,ncp->nop" if trans else "oc,ncp->nop", wi, xi)
    return y if b is None else y + b.long()[None, :, None]


def conv_fp64(x, w, b, trans: bool = False):
    """(y, bound) in fp64: bound = (C + 1) ULP (sum_c |w||x| + |b|) per element."""
    eq = "co,ncp->nop" if trans else "oc,ncp->nop"
    y = torch.einsum(eq, w.double(), x.double())
    env = torch.einsum(eq, w.double().abs(), x.double().abs())
    if b is not None:
        y, env = y + b.double()[None, :, None], env + b.double().abs()[None, :, None]
    return y, (w.shape[0] + 1) * ULP * env


def conv_emulate(x, w, b) -> torch.Tensor:
    """The kernel's chain acc = b; acc = w[o][c] x[c] + acc over c in fp32 (two roundings per
    step where the kernel's fmaf has one: the bound holds for either)."""
    n, c, hw = x.shape
    acc = (torch.zeros(c) if b is None else b)[None, :, None].expand(n, c, hw).clone()
    for ci in range(c):
        acc = w[None, :, ci, None] * x[:, ci:ci + 1, :] + acc
    return acc


def flat_index(i: int, shape) -> tuple:
    """Flat index -> index tuple (for naming the worst element)."""
    out = []
    for s in reversed(tuple(shape)):
        out.append(i % s)
        i //= s
    return tuple(reversed(out))
