"""GroupNorm (+ per-(sample, channel) input bias) (+ SiLU) in fp64 closed form, the value cases
that separate a robust fp32 variance from a fragile one, and the bounds the kernels are held to.

The op over x = cat(x1, x2) (+ chan_bias), per group of n elements (sample, Cg channels, h x w):

    mean = sum(x) / n,  var = sum((x - mean)^2) / n,  rstd = (var + eps)^-1/2,
    xhat = (x - mean) rstd,  y = xhat gamma_c + beta_c,  z = silu(y) or y,
    g = dz silu'(y) gamma_c,  A = sum(g),  B = sum(g xhat),
    dx = rstd (g - A / n - xhat B / n)  (+ addends)

written out without autograd, so the reference of the input VJP does not share code with what it
judges (tests/test_gn_ref.py holds it to fp64 ``F.group_norm`` + autograd at 1e-12).

A kernel that accumulates shifted sums S1 = sum(x - K), S2 = sum((x - K)^2) in fp32 and forms
var = S2 / n - (S1 / n)^2 is as good as a two-pass variance while (K - mean)^2 <~ var and loses
(K - mean)^2 / var times the rounding of the sums otherwise.  ``randn`` inputs never show which
of the two a kernel is: the value cases below put a group's first element, first vector, first
image row, last element, one channel, or the first channel's bias far from the group mean, make
the mean large against the spread, the spread small against eps, and the group constant but for
one element.  Every test file takes its inputs from ``make_case``.

The *yardstick* (``yardstick``) is torch's fp32 CPU ``native_group_norm`` and its autograd: a
correct fp32 implementation that shares nothing with the kernels.  It is inside every bound on
every case (tests/test_gn_ref.py), so no case asks for more than fp32 can give — with one
exception that is measured there: on case 7 torch's own fp32 moments are 1e-5 .. 2e-4 off in
rstd, and plain fp32 moments about the fp32 mean (``shifted_fp32_stats``) stand in for them.
Where the fp32 mean itself is coarse against the spread (cases 7 and 9) the input VJP is held to
a multiple of the yardstick's own error instead of VJP_TOL (``vjp_bound``).

Everything here runs on the CPU.
"""

from __future__ import annotations

import functools
from typing import NamedTuple

import torch

EPS = 1e-6
ULP = 2.0 ** -23          # spacing of fp32 numbers relative to their magnitude

# ---- bounds -----------------------------------------------------------------------------------
FWD_TOL = 2e-5            # |z - ref| <= FWD_TOL max(1, |ref|) + ULP |mean| rstd |gamma_c|
STAT_TOL = 5e-6           # |rstd - ref| / ref;  |mean - ref| rstd <= STAT_TOL + ULP |mean| rstd
VJP_TOL = 2e-5            # per group: max |dx - ref| / max |ref|
VJP_YARD_LIMIT = 2.5e-6   # above this value of the yardstick's own VJP metric on the case ...
VJP_YARD_FACTOR = 8.0     # ... the bound is this many times the yardstick's value instead

CASES = {
    1: "randn",
    2: "first_element_1000",
    3: "first_float4_300",
    4: "first_row_100",
    5: "last_element_1000",
    6: "one_channel_plus_50",
    7: "mean_1e3_std_1e-2",
    8: "std_1e-4",
    9: "constant_3_one_3.5",
    10: "bias_first_channel_500",
}
ALL_CASES = tuple(CASES)
FEW_CASES = (1, 2, 7)


class GnCase(NamedTuple):
    x: torch.Tensor       # [n][c][h][w] fp32 (the concatenation; tests split it into parts)
    cb: torch.Tensor      # [n][c] fp32 chan_bias
    gamma: torch.Tensor   # [c] fp32 in [0.5, 1.5]
    beta: torch.Tensor    # [c] fp32
    dz: torch.Tensor      # [n][c][h][w] fp32
    add: torch.Tensor     # [n][c][h][w] fp32 addend of the input VJP
    groups: int
    eps: float


def apply_case(case: int, x: torch.Tensor, cb: torch.Tensor, groups: int) -> None:
    """Turn N(0, 1)-like x [n][c][h][w] (contiguous) and chan_bias cb [n][c] into value case
    ``case``, in place."""
    n, c, h, w = x.shape
    cg = c // groups
    gs = cg * h * w
    flat = x.view(n, groups, gs)
    if case == 2:
        flat[:, :, 0] = 1000.0
    elif case == 3:
        flat[:, :, :4] = 300.0
    elif case == 4:
        x.view(n, groups, cg, h, w)[:, :, 0, 0, :] = 100.0
    elif case == 5:
        flat[:, :, -1] = 1000.0
    elif case == 6:
        x.view(n, groups, cg, h, w)[:, :, cg - 1] += 50.0
    elif case == 7:
        x.mul_(1e-2).add_(1e3)
        # a bias on the fp32 grid at 1e3 (2^-14): x + chan_bias, which every fp32 implementation
        # forms first, is then exact; off the grid each channel's bias is rounded by up to 3e-5,
        # a per-channel offset that moves rstd by 1e-4 before any kernel arithmetic
        cb.mul_(1e-3 * 2 ** 14).round_().mul_(2.0 ** -14)
    elif case == 8:
        x.mul_(1e-4)
        cb.mul_(1e-5)
    elif case == 9:
        x.fill_(2.75)
        cb.fill_(0.25)
        flat[:, :, gs // 3] = 3.25
    elif case == 10:
        cb.view(n, groups, cg)[:, :, 0] = 500.0
    elif case != 1:
        raise ValueError(case)


@functools.lru_cache(maxsize=2)
def make_case(case: int, shape: tuple, seed: int = 0) -> GnCase:
    """Value case ``case`` (a key of CASES) at shape (n, c, h, w, groups).  What the case names
    holds for x + chan_bias, per group; the outliers sit in x except in case 10."""
    n, c, h, w, groups = shape
    gen = torch.Generator().manual_seed(1000 * seed + 17 * case + sum(shape))
    x = torch.randn(n, c, h, w, generator=gen)
    cb = 0.5 * torch.randn(n, c, generator=gen)
    gamma = torch.rand(c, generator=gen) + 0.5
    beta = 0.4 * torch.rand(c, generator=gen) - 0.2
    dz = torch.randn(n, c, h, w, generator=gen)
    add = torch.randn(n, c, h, w, generator=gen)
    apply_case(case, x, cb, groups)
    return GnCase(x, cb, gamma, beta, dz, add, groups, EPS)


class GnRef(NamedTuple):
    mean: torch.Tensor    # [n * groups] fp64
    rstd: torch.Tensor    # [n * groups]
    z: torch.Tensor       # [n][c][h][w]
    dx: torch.Tensor | None


def _cat(t):
    if isinstance(t, (tuple, list)):
        return torch.cat([p for p in t if p is not None], 1)
    return t


def gn_fp64(x, groups: int, gamma, beta, eps: float, act: bool, chan_bias=None, dz=None, add=None) -> GnRef:
    """The op on the given operands (any dtype, read as fp64).  ``x`` / ``add``: one tensor or
    the parts (x1, x2) of a channel concatenation; ``dz``: None for the forward alone."""
    x = _cat(x).double()
    n, c = x.shape[:2]
    per = (1, c) + (1,) * (x.ndim - 2)
    ga = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    # Deviations from the group's first element (and the first channel's bias) first: differences
    # of fp32 operands are exact in fp64, so a mean of 1e3 over a spread of 1e-2 costs the
    # deviations nothing (x + chan_bias and x - mean formed directly each round at 1e-13, 1e-11
    # of that spread).
    v = x.reshape(n, groups, -1)
    k = v[:, :, :1]
    v = v - k
    if chan_bias is not None:
        cb = chan_bias.double().reshape(n, groups, c // groups)
        k = k + cb[:, :, :1]
        hw = v.shape[-1] // (c // groups)
        v = v + (cb - cb[:, :, :1]).repeat_interleave(hw, dim=-1)
    cnt = v.shape[-1]
    m0 = v.sum(-1, keepdim=True) / cnt
    mean = k + m0
    d = v - m0
    rstd = ((d * d).sum(-1, keepdim=True) / cnt + eps) ** -0.5
    xhat = (d * rstd).reshape(x.shape)
    y = xhat * ga.view(per) + be.view(per)
    s = torch.sigmoid(y)
    z = y * s if act else y
    dx = None
    if dz is not None:
        g = dz.double() * ga.view(per)
        if act:
            g = g * s * (1 + y * (1 - s))
        gv, xv = g.reshape(n, groups, -1), xhat.reshape(n, groups, -1)
        a = gv.sum(-1, keepdim=True) / cnt
        b = (gv * xv).sum(-1, keepdim=True) / cnt
        dx = (rstd * (gv - a - xv * b)).reshape(x.shape)
        if add is not None:
            dx = dx + _cat(add).double()
    return GnRef(mean.reshape(-1), rstd.reshape(-1), z, dx)


@functools.lru_cache(maxsize=4)
def reference(case: int, shape: tuple, act: bool, seed: int = 0, with_add: bool = False) -> GnRef:
    """``gn_fp64`` of ``make_case`` (computed once per case; the tests leave it unchanged)."""
    t = make_case(case, shape, seed)
    return gn_fp64(t.x, t.groups, t.gamma, t.beta, t.eps, act, t.cb, t.dz, t.add if with_add else None)


def yardstick(case: int, shape: tuple, act: bool, seed: int = 0, with_add: bool = False):
    """(mean, rstd, z, dx) of torch's fp32 CPU ``native_group_norm`` (+ SiLU) and its autograd."""
    t = make_case(case, shape, seed)
    n, c, h, w, groups = shape
    x = t.x.clone().requires_grad_(True)
    xb = x + t.cb[:, :, None, None]
    y, mean, rstd = torch.native_group_norm(xb, t.gamma, t.beta, n, c, h * w, groups, t.eps)
    z = torch.nn.functional.silu(y) if act else y
    (dx,) = torch.autograd.grad(z, x, t.dz)
    if with_add:
        dx = dx + t.add
    return mean.detach().reshape(-1), rstd.detach().reshape(-1), z.detach(), dx


def shifted_fp32_stats(case: int, shape: tuple, seed: int = 0):
    """(mean, rstd) in fp32 from moments about the fp32 mean K: var = mean((x - K)^2) - mean(x - K)^2.
    On case 7 (mean 1e3, spread 1e-2) torch's fp32 moments are themselves 1e-4 off in rstd; this
    is the plain fp32 formulation that is not, so the statistics bound is not impossible there."""
    t = make_case(case, shape, seed)
    n, c, h, w, groups = shape
    xb = (t.x + t.cb[:, :, None, None]).view(n, groups, -1)
    k = xb.mean(-1, keepdim=True)
    d = xb - k
    m1 = d.mean(-1, keepdim=True)
    var = (d * d).mean(-1, keepdim=True) - m1 * m1
    return (k + m1).reshape(-1), (var + t.eps).rsqrt().reshape(-1)


@functools.lru_cache(maxsize=None)
def yardstick_vjp_error(case: int, shape: tuple, act: bool, seed: int = 0, with_add: bool = False) -> float:
    ref = reference(case, shape, act, seed, with_add)
    return vjp_error(yardstick(case, shape, act, seed, with_add)[3], ref, shape[4])


# ---- the measured quantities (each over every group / element: nothing is left out) -------------
def rstd_error(rstd, ref: GnRef) -> float:
    """max over groups of |rstd - ref| / ref"""
    return float(((rstd.double().cpu().reshape(-1) - ref.rstd).abs() / ref.rstd).max())


def mean_excess(mean, ref: GnRef) -> float:
    """max over groups of |mean - ref| rstd / (STAT_TOL + ULP |mean| rstd)  (<= 1 passes)"""
    err = (mean.double().cpu().reshape(-1) - ref.mean).abs() * ref.rstd
    return float((err / (STAT_TOL + ULP * ref.mean.abs() * ref.rstd)).max())


def forward_excess(z, ref: GnRef, gamma, groups: int) -> float:
    """max over elements of |z - ref| / (FWD_TOL max(1, |ref|) + ULP |mean| rstd |gamma_c|)"""
    z = _cat(z).double().cpu()
    assert torch.isfinite(z).all()
    n, c = z.shape[:2]
    ga = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double().cpu()
    rep = (ULP * ref.mean.abs() * ref.rstd).view(n, groups, 1) * ga.abs().view(1, groups, c // groups)
    bound = FWD_TOL * ref.z.abs().clamp_min(1.0) + rep.reshape(n, c, *(1,) * (z.ndim - 2))
    return float(((z - ref.z).abs() / bound).max())


def forward_error(z, ref: GnRef) -> float:
    """max over elements of |z - ref| / max(1, |ref|) (the figure without the representability term)"""
    return float(((_cat(z).double().cpu() - ref.z).abs() / ref.z.abs().clamp_min(1.0)).max())


def vjp_error(dx, ref: GnRef, groups: int) -> float:
    """max over groups of max |dx - ref| / max |ref|"""
    dx = _cat(dx).double().cpu()
    assert torch.isfinite(dx).all()
    n = dx.shape[0]
    err = (dx - ref.dx).abs().reshape(n, groups, -1).amax(-1)
    return float((err / ref.dx.abs().reshape(n, groups, -1).amax(-1)).max())


def mean_ulp_in_spreads(ref: GnRef) -> float:
    """max over groups of ULP |mean| rstd: what one fp32 rounding of the mean is in units of the
    group's spread (an fp32 ``mean`` output cannot carry xhat more exactly than that)."""
    return float((ULP * ref.mean.abs() * ref.rstd).max())


# The cases whose mean is not representable in fp32 to VJP_YARD_LIMIT of the spread (7: 1.2e-2;
# 9: up to 2e-4 = 2^-23 * 3 / sqrt(0.25 / n + eps)): only they may take the relaxed VJP bound.
RELAXED_VJP_CASES = (7, 9)


def vjp_bound(yard: float, ref: GnRef, case: int) -> tuple[float, bool]:
    """(bound, relaxed) for a case whose yardstick VJP metric is ``yard``: VJP_TOL, or
    VJP_YARD_FACTOR times the yardstick's own value where that exceeds VJP_YARD_LIMIT — which is
    accepted only where the fp32 mean itself explains it."""
    if yard > VJP_YARD_LIMIT:
        assert case in RELAXED_VJP_CASES and mean_ulp_in_spreads(ref) > VJP_YARD_LIMIT, (case, yard)
        return VJP_YARD_FACTOR * yard, True
    return VJP_TOL, False


# ---- shapes of the GPU edge tests: (n, c, h, w, groups), c1 (0: one part), the cases run -------
SHAPES = [
    ((2, 8, 32, 32, 4), 0, ALL_CASES),        # gs 2048: one partial chunk
    ((1, 16, 32, 32, 2), 0, FEW_CASES),       # gs 8192: exactly one chunk
    ((2, 2, 4, 2049, 2), 0, FEW_CASES),       # gs 8196: the second chunk is one float4
    ((1, 2, 4, 32767, 2), 0, FEW_CASES),      # gs 2^17 - 4: 16 chunks, the last one short
    ((1, 8, 128, 128, 1), 0, ALL_CASES),      # gs 2^17: forward chunk 16384, backward 8192
    ((2, 64, 17, 17, 2), 0, ALL_CASES),       # gs 9248, scalar kernels, two chunks
    ((2, 64, 17, 17, 2), 24, FEW_CASES),      # ... as two parts
    ((1, 256, 8, 8, 2), 0, FEW_CASES),        # Cg = 128: the LDS table's last slot
    ((1, 258, 8, 8, 2), 0, FEW_CASES),        # Cg = 129: two-pass
    ((1, 8, 512, 520, 1), 0, FEW_CASES),      # 260 backward chunks (two-pass), 130 forward
    ((1, 8, 512, 1032, 1), 0, (1, 2)),        # 258 forward chunks: both two-pass
    ((3, 96, 12, 20, 8), 40, FEW_CASES),      # two parts, straddling, not chunk-aligned
    ((1, 256, 64, 64, 2), 128, FEW_CASES),    # two parts, group 1 starts at the split
    ((2, 8, 64, 64, 2), 2, ALL_CASES),        # two parts, chunk-aligned split inside group 0
]


def shape_id(entry) -> str:
    shape, c1, _ = entry
    return "x".join(map(str, shape)) + (f"-c1_{c1}" if c1 else "")


# (V, forward single-pass, backward single-pass) each entry must take with the single-pass kernels
# enabled (V: 4 float4 kernels, 1 scalar); with them disabled both directions are two-pass.
PATHS = {
    "2x8x32x32x4": (4, True, True), "1x16x32x32x2": (4, True, True), "2x2x4x2049x2": (4, True, True),
    "1x2x4x32767x2": (4, True, True), "1x8x128x128x1": (4, True, True), "2x64x17x17x2": (1, False, False),
    "2x64x17x17x2-c1_24": (1, False, False), "1x256x8x8x2": (4, True, True), "1x258x8x8x2": (4, False, False),
    "1x8x512x520x1": (4, True, False), "1x8x512x1032x1": (4, False, False),
    "3x96x12x20x8-c1_40": (4, False, False), "1x256x64x64x2-c1_128": (4, True, True),
    "2x8x64x64x2-c1_2": (4, True, True),
}


def expected_paths(entry) -> tuple:
    return PATHS[shape_id(entry)]
