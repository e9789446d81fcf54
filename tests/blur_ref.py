"""A second, independent statement of the reflect-padded separable blur and of the fused DPS
residual pass over it: dense fp64 matrices built by index arithmetic (numpy only, no torch op, no
fold formula), the per-element envelopes that bound an fp32 evaluation, cases no fp32 evaluation
can round, and fp32 emulations of the two algorithm shapes csrc/sp_blur.hip uses.

The map.  ``A1 = reflect_matrix(n, t)`` is the 1-D correlation with single-reflection padding,
``A1[i, reflect(i + d)] += t[d + R]``.  On a plane ``A X = A_H X A_W^T`` and
``A^T S = A_H^T S A_W``.  oracle/blur.py (F.pad + conv2d + autograd) states the same map a different
way; tests/test_blur_ref.py holds the two together to 1e-12.

The pass.  With the coefficients as the fp32 numbers the library receives,
``x0 = (x - k eps) / a``, ``r = y - A x0``, ``v = A^T (gs r)``, ``rsq = sum r^2`` per sample.

The envelopes bound every partial sum of any fp32 evaluation order (``|A|`` is built from ``|t|``,
so taps that land on one column after reflection do not cancel in it):
``x0env = (|x| + |k||eps|) / |a|``, ``E_r = |y| + |A| x0env``, ``E_v = |gs| |A|^T E_r``.

The rounding count.  ``rounding_count(R) = 6 K + 12`` with ``K = 2R + 1`` is the number of fp32
roundings on the longest path to one element of ``v``: x0 4 (k eps, the difference, 1/a, the
product); two forward passes, K each (one fused multiply-add per tap); the residual and its scale
2; two adjoint passes, at most 2K each (K taps of the zero-extended correlation and up to K fold
terms); the fold-corrected tap sums of the streaming kernels, at most 2 per pass.  Each rounding
perturbs the result by at most ``2^-24`` of the magnitude it acts on, which the envelope bounds, so
``|v - v64| <= rounding_count(R) 2^-24 E_v`` per element, to first order.  Apply alone is two
passes of K fused multiply-adds (``2K``), the adjoint alone two passes of at most 2K (``4K``).

The exact cases.  ``exact_taps(R)`` are eighths, asymmetric, sparse and reach both ends of the
support; ``exact_inputs`` are integers in [-4, 4]; with ``a = k = 1/2``, ``gs = 4``, x0 = 2x - eps
is an integer and every intermediate of the four 1-D passes is a multiple of 2^-12 bounded by
``E_v < 2^12``: 24 bits, no rounding anywhere, whatever the order, fused or not, in
zero-extended + fold form or with fold-corrected taps.  A correct kernel returns ``v64`` bit for bit.
"""

from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

U32 = 2.0 ** -24  # fp32 unit roundoff
EXACT_COEFS = (0.5, 0.5, 4.0)      # a, k, gs of the exact cases
RANDOM_COEFS = (0.3, math.sqrt(1 - 0.09), 400.0)


def f32(v: float) -> float:
    """The fp32 number the library receives for a coefficient, as a Python float."""
    return float(np.float32(v))


def reflect_index(i: int, n: int) -> int:
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    assert 0 <= i < n, "single reflection needs R < n"
    return i


def reflect_matrix(n: int, taps) -> np.ndarray:
    """Dense n x n matrix of the 1-D reflect-padded correlation with ``taps`` (t[-R..R])."""
    t = np.asarray(taps, dtype=np.float64)
    r = (t.size - 1) // 2
    assert t.size == 2 * r + 1 and r < n
    a = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for d in range(-r, r + 1):
            a[i, reflect_index(i + d, n)] += t[d + r]
    return a


def apply64(x, taps, shape) -> np.ndarray:
    """A x on (..., C, H, W) planes (any leading layout with C*H*W trailing elements), fp64."""
    c, h, w = shape
    p = np.asarray(x, dtype=np.float64).reshape(-1, h, w)
    out = reflect_matrix(h, taps) @ p @ reflect_matrix(w, taps).T
    return out.reshape(np.shape(x))


def adjoint64(s, taps, shape) -> np.ndarray:
    """A^T s: the transposed matrices, fp64."""
    c, h, w = shape
    p = np.asarray(s, dtype=np.float64).reshape(-1, h, w)
    out = reflect_matrix(h, taps).T @ p @ reflect_matrix(w, taps)
    return out.reshape(np.shape(s))


def dps_pass64(x, eps, y, ydiv, a, k, gs, taps, shape) -> SimpleNamespace:
    """The fused residual pass on (B, n) arrays (y: (B // ydiv, n)) in fp64, with its envelopes.
    Returns v, rsq (B,), r, x0, x0env, E_r, E_v."""
    a, k, gs = f32(a), f32(k), f32(gs)
    x = np.asarray(x, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    rows = np.arange(x.shape[0]) // ydiv
    yb = np.asarray(y, dtype=np.float64)[rows]
    t = np.asarray(taps, dtype=np.float64)
    x0 = (x - k * eps) / a
    r = yb - apply64(x0, t, shape)
    v = adjoint64(gs * r, t, shape)
    x0env = (np.abs(x) + abs(k) * np.abs(eps)) / abs(a)
    e_r = np.abs(yb) + apply64(x0env, np.abs(t), shape)
    e_v = abs(gs) * adjoint64(e_r, np.abs(t), shape)
    return SimpleNamespace(v=v, rsq=(r * r).sum(axis=1), r=r, x0=x0, x0env=x0env, E_r=e_r, E_v=e_v)


def rounding_count(radius: int) -> int:
    return 6 * (2 * radius + 1) + 12


def apply_count(radius: int) -> int:
    return 2 * (2 * radius + 1)


def adjoint_count(radius: int) -> int:
    return 4 * (2 * radius + 1)


# --- taps and inputs -------------------------------------------------------------------------------

def exact_taps(radius: int) -> np.ndarray:
    t = np.zeros(2 * radius + 1, dtype=np.float32)
    t[0], t[radius], t[2 * radius] = 2 / 8, 4 / 8, 1 / 8
    if radius >= 2:
        t[radius + 1] = -1 / 8
    return t


def gaussian_taps(radius: int, sigma: float = 3.0) -> np.ndarray:
    """The operator's own taps for kernel_size = 2R + 1 (exp in fp64, normalised, cast to fp32)."""
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    k = np.exp(-(i ** 2) / (2.0 * sigma ** 2))
    return (k / k.sum()).astype(np.float32)


def asym_taps(radius: int) -> np.ndarray:
    k = np.random.default_rng(100 + radius).uniform(0.05, 1.0, 2 * radius + 1)
    return (k / k.sum()).astype(np.float32)


def taps_of(name: str, radius: int) -> np.ndarray:
    return {"exact": exact_taps, "gauss": gaussian_taps, "asym": asym_taps}[name](radius)


def case_seed(radius: int, shape, batch: int) -> int:
    """One seed per (radius, plane, batch): the CPU pins and the GPU tests draw the same inputs."""
    return 10_000 * radius + 100 * shape[1] + shape[2] + batch


def exact_inputs(seed: int, batch: int, ydiv: int, shape):
    """x, eps (batch, n) and y (batch // ydiv, n): integers in [-4, 4] as fp32."""
    n = math.prod(shape)
    g = np.random.default_rng(seed)
    draw = lambda b: g.integers(-4, 5, size=(b, n)).astype(np.float32)  # noqa: E731
    return draw(batch), draw(batch), draw(batch // ydiv)


def random_inputs(seed: int, batch: int, ydiv: int, shape):
    n = math.prod(shape)
    g = np.random.default_rng(seed)
    draw = lambda b: g.standard_normal((b, n)).astype(np.float32)  # noqa: E731
    return draw(batch), draw(batch), draw(batch // ydiv)


def near_consistent_inputs(seed: int, batch: int, ydiv: int, shape, taps, a, k):
    """x = 30 + randn, eps = randn and y = fp32(A x0) + 1e-3 randn (x0 of each y row's first
    sample; ydiv = 1 makes every sample near-consistent): the residual lies four orders below
    its operands, as in the last steps of a run."""
    n = math.prod(shape)
    g = np.random.default_rng(seed)
    x = (30.0 + g.standard_normal((batch, n))).astype(np.float32)
    eps = g.standard_normal((batch, n)).astype(np.float32)
    x0 = (x.astype(np.float64) - f32(k) * eps.astype(np.float64)) / f32(a)
    ax0 = apply64(x0[::ydiv], np.asarray(taps, dtype=np.float64), shape).astype(np.float32)
    y = (ax0 + np.float32(1e-3) * g.standard_normal(ax0.shape).astype(np.float32)).astype(np.float32)
    return x, eps, y


# --- the planes the CPU and GPU tests share: (shape, batch, ydiv) ---------------------------------

def tile_cases(radius: int):
    """Tile kernel k_blur<R, MODE>.  Block counts 2, 8, 12 and 18: below 8, a multiple of 8, and
    8 q + r in the XCD-ordered decode."""
    h = -(-radius // 2)
    return [((1, 2 * radius + 1, 2 * radius + 1), 2, 2),   # both fold bands overlap on row / column R
            ((2, 33 + h, 65 + h), 1, 1),                   # the bands cross row 32 and column 64
            ((1, 33, 65), 3, 1),                           # second tiles of one row and one column
            ((3, 40, 36), 3, 3)]


REG_CASES = [((1, 64, 256), 2, 1), ((2, 128, 256), 3, 3)]   # even H / 32: k_blur_dps_reg<R>
DMA_CASES = [((1, 32, 256), 3, 3), ((2, 96, 256), 2, 1)]    # odd H / 32: k_blur_dps_dma<R>


def tile_partials(shape) -> int:
    c, h, w = shape
    return c * (-(-h // 32)) * (-(-w // 64))


def stream_partials(shape) -> int:
    c, h, w = shape
    assert w == 256 and h % 32 == 0
    return c * (h // 32)


def fold_band_mask(shape, radius: int) -> np.ndarray:
    """(C, H, W) bool: rows [1, R] and [H-1-R, H-2], columns [1, R] and [W-1-R, W-2]."""
    c, h, w = shape
    rows = np.zeros(h, dtype=bool)
    cols = np.zeros(w, dtype=bool)
    rows[1:radius + 1] = rows[h - 1 - radius:h - 1] = True
    cols[1:radius + 1] = cols[w - 1 - radius:w - 1] = True
    return np.broadcast_to(rows[:, None] | cols[None, :], (c, h, w)).copy()


def describe_mismatch(got, want, shape, radius: int, limit: int = 6) -> str:
    """The first mismatching (sample, plane, row, column), and whether each lies in a fold band or
    on a tile seam (row 31 / 32, column 63 / 64)."""
    c, h, w = shape
    g = np.asarray(got).reshape(-1, c, h, w)
    r = np.asarray(want).reshape(-1, c, h, w)
    bad = np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))
    band = fold_band_mask(shape, radius)
    out = [f"{len(bad)} of {g.size} differ"]
    for b, p, i, j in bad[:limit]:
        where = []
        if band[p, i, j]:
            where.append("fold band")
        if i % 32 in (0, 31) and 0 < i < h - 1 or j % 64 in (0, 63) and 0 < j < w - 1:
            where.append("seam")
        out.append(f"(b{b} c{p} r{i} c{j}: got {g[b, p, i, j]!r} want {r[b, p, i, j]!r}"
                   f"{' ' + '+'.join(where) if where else ''})")
    return "; ".join(out)


# --- fp32 emulations of the two algorithm shapes ---------------------------------------------------
# Every array is fp32 and every product and sum rounds to fp32 (no fused multiply-add): on the exact
# cases nothing rounds, so this is the kernel's result whatever its order.

def _order(radius: int, reverse: bool):
    ds = list(range(-radius, radius + 1))
    return ds[::-1] if reverse else ds


def _corr_reflect32(x, t, reverse):
    """Correlation along the last axis with reflected indices."""
    n, r = x.shape[-1], (t.size - 1) // 2
    acc = np.zeros_like(x)
    for d in _order(r, reverse):
        idx = [reflect_index(i + d, n) for i in range(n)]
        acc = acc + t[d + r] * x[..., idx]
    return acc


def _adj_fold32(s, t, reverse, drop_far_fold):
    """Zero-extended correlation U(p) = sum_d t[d] s(p - d) on p in [-R, n-1+R], then the halo
    folded back: v(j) = U(j) + [0 < j <= R] U(-j) + [n-1-R <= j < n-1] U(2n-2-j)."""
    n, r = s.shape[-1], (t.size - 1) // 2
    pad = np.zeros(s.shape[:-1] + (2 * r,), dtype=np.float32)
    sp = np.concatenate([pad, s, pad], axis=-1)  # s(q) at q + 2R
    u = np.zeros(s.shape[:-1] + (n + 2 * r,), dtype=np.float32)  # U(p) at p + R
    for d in _order(r, reverse):
        u = u + t[d + r] * sp[..., r - d:r - d + n + 2 * r]
    v = u[..., r:r + n].copy()
    for j in range(1, r + 1):
        v[..., j] = v[..., j] + u[..., r - j]
    if not drop_far_fold:
        for j in range(n - 1 - r, n - 1):
            v[..., j] = v[..., j] + u[..., 2 * n - 2 - j + r]
    return v


def _adj_taps32(s, t, reverse, drop_far_fold):
    """Fold-corrected taps: v(j) = sum_o T_j[o] s(j + o), T_j[o] = t[R-o] + t[R-2j-o] (1 <= j <= R)
    + t[2n-2-2j+R-o] (n-1-R <= j <= n-2), each index taken only inside [0, 2R]."""
    n, r = s.shape[-1], (t.size - 1) // 2
    pad = np.zeros(s.shape[:-1] + (r,), dtype=np.float32)
    sp = np.concatenate([pad, s, pad], axis=-1)  # s(q) at q + R
    v = np.zeros_like(s)
    for o in _order(r, reverse):
        tj = np.full(n, t[r - o], dtype=np.float32)
        for j in range(n):
            if 1 <= j <= r and 0 <= r - 2 * j - o <= 2 * r:
                tj[j] = tj[j] + t[r - 2 * j - o]
            i = 2 * n - 2 - 2 * j + r - o
            if not drop_far_fold and n - 1 - r <= j <= n - 2 and 0 <= i <= 2 * r:
                tj[j] = tj[j] + t[i]
        v = v + tj * sp[..., r + o:r + o + n]
    return v


FORMS = {"fold": _adj_fold32, "taps": _adj_taps32}
WRONG = ("vertical_taps_reversed", "bottom_fold_dropped")


def emulate_pass32(x, eps, y, ydiv, a, k, gs, taps, shape, form="fold", reverse=False, wrong=None):
    """v of the fused pass evaluated in fp32 in one of the two algorithm shapes (``form``), summing
    taps forward or reversed.  ``wrong`` breaks it on purpose: the vertical adjoint with reversed
    taps, or without its bottom fold."""
    assert wrong is None or wrong in WRONG
    c, h, w = shape
    t = np.asarray(taps, dtype=np.float32)
    a, k, gs = np.float32(a), np.float32(k), np.float32(gs)
    x = np.asarray(x, dtype=np.float32).reshape(-1, c, h, w)
    eps = np.asarray(eps, dtype=np.float32).reshape(-1, c, h, w)
    rows = np.arange(x.shape[0]) // ydiv
    yb = np.asarray(y, dtype=np.float32).reshape(-1, c, h, w)[rows]
    x0 = (x - k * eps) * (np.float32(1) / a)
    hh = _corr_reflect32(x0, t, reverse)
    z = _corr_reflect32(hh.swapaxes(-1, -2), t, reverse).swapaxes(-1, -2)
    s = (yb - z) * gs
    adj = FORMS[form]
    tv = t[::-1].copy() if wrong == "vertical_taps_reversed" else t
    vv = adj(np.ascontiguousarray(s.swapaxes(-1, -2)), tv, reverse, wrong == "bottom_fold_dropped")
    v = adj(np.ascontiguousarray(vv.swapaxes(-1, -2)), t, reverse, False)
    assert v.dtype == np.float32
    return v.reshape(x.shape[0], -1)
