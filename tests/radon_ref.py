"""fp64 semantics of the parallel-beam projector (operators/radon.py, csrc/sp_radon.hip) and numpy
fp32 emulations of the two gathers, independent of the operator's own host form.

For one plane, a table of rows (alpha, beta, length, axis) TAKEN AS EXACT fp32 CONSTANTS, and
s0 = (D-1)/2, i0 = (H-1)/2, j0 = (W-1)/2:

  axis 0:  c(i, s) = alpha (s - s0) + (beta (i - i0) + j0)
           y[a, s] = length * sum_i [(1 - f) x[i, floor c] + f x[i, floor c + 1]],  f = c - floor c
  axis 1:  r(j, s) = alpha (s - s0) + (beta (j - j0) + i0), rows and columns swapped

with 0 for an index off the image.  `dense64` is that matrix in fp64.  `dense32` has every weight
as the fp32 operation sequence produces it (the position rounded after each of its four
operations in the bracketed order, f = c - floor c, 1 - f, all fp32) held as fp64 entries times
the fp64 value of length: what both kernels must reproduce up to the rounding of their sums.
`project32` / `backproject32` emulate the kernels' gathers operation by operation in fp32.
"""

from __future__ import annotations

import functools
import math

import numpy as np

f32 = np.float32


# --- the crossing position: the contract, and two deliberately different forms ---------------
def pos_contract(alpha, beta, ds, dd, off):
    """fl(fl(alpha ds) + fl(fl(beta dd) + off)), every operand fp32."""
    alpha, beta, off = f32(alpha), f32(beta), f32(off)
    return (alpha * np.asarray(ds, f32)).astype(f32) + ((beta * np.asarray(dd, f32)).astype(f32) + off).astype(f32)


def pos_fused(alpha, beta, ds, dd, off):
    """The same expression rounded once (what contraction into fused multiply-adds tends to)."""
    v = np.float64(alpha) * np.asarray(ds, np.float64) + (np.float64(beta) * np.asarray(dd, np.float64)
                                                           + np.float64(off))
    return v.astype(f32)


def pos_reordered(alpha, beta, ds, dd, off):
    """The offset applied last: fl(fl(fl(alpha ds) + fl(beta dd)) + off)."""
    alpha, beta, off = f32(alpha), f32(beta), f32(off)
    return (((alpha * np.asarray(ds, f32)).astype(f32) + (beta * np.asarray(dd, f32)).astype(f32)).astype(f32)
            + off).astype(f32)


def _geometry(row, H, W):
    axis = bool(row[3] != 0)
    nd, nx = (W, H) if axis else (H, W)
    return axis, nd, nx


def _pixel(axis, W, d, xc):
    return xc * W + d if axis else d * W + xc


def table_of(angles) -> np.ndarray:
    """The fp32 table of `angles`, independently of operators.radon.radon_table: math.cos /
    math.sin in fp64, snapped below 1e-12, a tie |cos| == |sin| to axis 0."""
    rows = []
    for th in angles:
        c, s = math.cos(th), math.sin(th)
        c = 0.0 if abs(c) < 1e-12 else c
        s = 0.0 if abs(s) < 1e-12 else s
        if abs(c) >= abs(s):
            rows.append((1.0 / c, -s / c, 1.0 / abs(c), 0.0))
        else:
            rows.append((1.0 / s, -c / s, 1.0 / abs(s), 1.0))
    return np.asarray(rows, dtype=np.float64).astype(f32)


# --- dense matrices ---------------------------------------------------------------------------
def dense64(table, H, W, D) -> np.ndarray:
    """(n_angles * D, H * W) fp64 matrix of one plane, by index arithmetic."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    A = np.zeros((t.shape[0] * D, H * W))
    s0 = (D - 1) / 2.0
    for a, row in enumerate(t):
        axis, nd, nx = _geometry(row, H, W)
        for s in range(D):
            for d in range(nd):
                c = row[0] * (s - s0) + (row[1] * (d - (nd - 1) / 2.0) + (nx - 1) / 2.0)
                fl = math.floor(c)
                f = c - fl
                for xc, w in ((fl, 1.0 - f), (fl + 1, f)):
                    if 0 <= xc < nx:
                        A[a * D + s, _pixel(axis, W, d, xc)] += row[2] * w
    return A


def weights32(table, H, W, D, pos=pos_contract) -> np.ndarray:
    """The weights (without length) the forward gather generates, as an fp32 matrix."""
    t = np.asarray(table, dtype=f32).reshape(-1, 4)
    Wt = np.zeros((t.shape[0] * D, H * W), dtype=f32)
    ds = np.arange(D, dtype=f32) - f32((D - 1) / 2.0)
    for a, row in enumerate(t):
        axis, nd, nx = _geometry(row, H, W)
        for d in range(nd):
            c = pos(row[0], row[1], ds, f32(d) - f32((nd - 1) / 2.0), f32((nx - 1) / 2.0))
            fl = np.floor(c)
            f = (c - fl).astype(f32)
            w0 = (f32(1) - f).astype(f32)
            ic = fl.astype(np.int64)
            for idx, w in ((ic, w0), (ic + 1, f)):
                ok = (idx >= 0) & (idx < nx)
                Wt[a * D + np.nonzero(ok)[0], _pixel(axis, W, d, idx[ok])] = w[ok]
    return Wt


def dense32(table, H, W, D, pos=pos_contract) -> np.ndarray:
    """fp64 entries length * w with w the fp32 weight of the prescribed operation sequence."""
    t = np.asarray(table, dtype=f32).reshape(-1, 4)
    return weights32(t, H, W, D, pos).astype(np.float64) * np.repeat(t[:, 2].astype(np.float64), D)[:, None]


def adjoint_weights32(table, H, W, D, pos=pos_contract, narrow=False):
    """The weights the per-pixel gather finds (fp32 matrix, same layout as weights32) from the
    candidates floor(s*) - 1 .. floor(s*) + 2, and the largest number of rays with a non-zero
    weight that any pixel got from one angle.  `narrow`: the kernel's candidate rule, floor(s*)
    and floor(s*) + 1, the outer two only where s* - floor(s*) is below 1/64 or above 63/64."""
    t = np.asarray(table, dtype=f32).reshape(-1, 4)
    Wt = np.zeros((t.shape[0] * D, H * W), dtype=f32)
    s0 = f32((D - 1) / 2.0)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    di = ii.astype(f32) - f32((H - 1) / 2.0)
    dj = jj.astype(f32) - f32((W - 1) / 2.0)
    most = 0
    for a, row in enumerate(t):
        axis, nd, nx = _geometry(row, H, W)
        dd, dx, target = (dj, di, ii) if axis else (di, dj, jj)
        sstar = s0 + ((dx - row[1] * dd).astype(f32) / row[0]).astype(f32)
        base = np.floor(sstar).astype(np.int64) - 1
        fs = (sstar - np.floor(sstar)).astype(f32)
        count = np.zeros((H, W), dtype=np.int64)
        for u in range(4):
            s = base + u
            ok = (s >= 0) & (s < D)
            if narrow and u == 0:
                ok &= fs < f32(1 / 64)
            if narrow and u == 3:
                ok &= fs > f32(63 / 64)
            c = pos(row[0], row[1], s.astype(f32) - s0, dd, f32((nx - 1) / 2.0))
            fl = np.floor(c)
            f = (c - fl).astype(f32)
            w0 = (f32(1) - f).astype(f32)
            ic = fl.astype(np.int64)
            w = np.where(ic == target, w0, np.where(ic + 1 == target, f, f32(0))).astype(f32)
            hit = ok & ((ic == target) | (ic + 1 == target))
            Wt[a * D + s[hit], (ii * W + jj)[hit]] = w[hit]
            count += hit & (w != 0)
        most = max(most, int(count.max()))
    return Wt, most


# --- fp32 emulations of the kernels' gathers --------------------------------------------------
def project32(table, x, D, pos=pos_contract) -> np.ndarray:
    """A x for one plane x (H, W): every ray summed over the dominant index in order, each term
    fl(fl(w0 v0) + fl(f v1)) added in fp32, then fl(length * sum)."""
    t = np.asarray(table, dtype=f32).reshape(-1, 4)
    x = np.asarray(x, dtype=f32)
    H, W = x.shape
    y = np.zeros((t.shape[0], D), dtype=f32)
    ds = np.arange(D, dtype=f32) - f32((D - 1) / 2.0)
    for a, row in enumerate(t):
        axis, nd, nx = _geometry(row, H, W)
        img = x.T if axis else x  # img[d, cross]
        acc = np.zeros(D, dtype=f32)
        for d in range(nd):
            c = pos(row[0], row[1], ds, f32(d) - f32((nd - 1) / 2.0), f32((nx - 1) / 2.0))
            fl = np.floor(c)
            f = (c - fl).astype(f32)
            w0 = (f32(1) - f).astype(f32)
            ic = fl.astype(np.int64)
            v0 = np.where((ic >= 0) & (ic < nx), img[d, np.clip(ic, 0, nx - 1)], f32(0)).astype(f32)
            v1 = np.where((ic + 1 >= 0) & (ic + 1 < nx), img[d, np.clip(ic + 1, 0, nx - 1)], f32(0)).astype(f32)
            acc = (acc + ((w0 * v0).astype(f32) + (f * v1).astype(f32)).astype(f32)).astype(f32)
        y[a] = (row[2] * acc).astype(f32)
    return y


def backproject32(table, g, H, W, pos=pos_contract) -> np.ndarray:
    """A^T g for one sinogram plane g (n_angles, D): per pixel, angles in order, per angle the
    matching candidates in ascending s, then fl(length * t) added in fp32."""
    t = np.asarray(table, dtype=f32).reshape(-1, 4)
    g = np.asarray(g, dtype=f32)
    D = g.shape[1]
    s0 = f32((D - 1) / 2.0)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    di = ii.astype(f32) - f32((H - 1) / 2.0)
    dj = jj.astype(f32) - f32((W - 1) / 2.0)
    acc = np.zeros((H, W), dtype=f32)
    for a, row in enumerate(t):
        axis, nd, nx = _geometry(row, H, W)
        dd, dx, target = (dj, di, ii) if axis else (di, dj, jj)
        sstar = s0 + ((dx - row[1] * dd).astype(f32) / row[0]).astype(f32)
        base = np.floor(sstar).astype(np.int64) - 1
        tsum = np.zeros((H, W), dtype=f32)
        for u in range(4):
            s = base + u
            ok = (s >= 0) & (s < D)
            c = pos(row[0], row[1], s.astype(f32) - s0, dd, f32((nx - 1) / 2.0))
            fl = np.floor(c)
            f = (c - fl).astype(f32)
            w0 = (f32(1) - f).astype(f32)
            ic = fl.astype(np.int64)
            gv = g[a, np.clip(s, 0, D - 1)]
            term = np.where(ok & (ic == target), (w0 * gv).astype(f32),
                            np.where(ok & (ic + 1 == target), (f * gv).astype(f32), f32(0))).astype(f32)
            tsum = (tsum + term).astype(f32)
        acc = (acc + (row[2] * tsum).astype(f32)).astype(f32)
    return acc


def pass1_32(table, x, eps, y, a, k, gs):
    """DPS pass 1 for one plane in the kernels' fp32 operations: (work, v, sum r^2 in fp64)."""
    x, eps, y = (np.asarray(v, dtype=f32) for v in (x, eps, y))
    a, k, gs = f32(a), f32(k), f32(gs)
    x0 = ((x - (k * eps).astype(f32)).astype(f32) / a).astype(f32)
    r = (y - project32(table, x0, y.shape[1])).astype(f32)
    work = (gs * r).astype(f32)
    return work, backproject32(table, work, *x.shape), float((r.astype(np.float64) ** 2).sum())


# --- the shared cases -------------------------------------------------------------------------
def case_angles(n: int):
    """n angles over a half turn from 1.1 rad: both axes from n = 2 on, no axis angle."""
    return [1.1 + math.pi * a / n for a in range(n)]


AXIS_TABLE = table_of([0.0, math.pi / 2, math.pi, 3 * math.pi / 2])
DYADIC_TABLE = np.asarray([(1, -0.5, 1.25, 0), (-1, 0.25, 1, 1), (1.5, 1, 0.5, 0), (-1.25, -0.75, 2, 1)],
                          dtype=f32)
# slabs wider than the kernel stages (|alpha| 2.5 over 200 rays), beside one that is staged
WIDE_TABLE = np.asarray([(2.5, 0.5, 1.0, 0), (-2.5, -0.25, 1.5, 1), (1.25, 0.5, 1.0, 0)], dtype=f32)
# bands of 32 rows / columns whose slab lies wholly off the image, on either side
SKIP_TABLE = np.asarray([(1, 1, 1, 0), (-1, 1, 0.5, 0)], dtype=f32)
SKIP_TABLE_T = np.asarray([(1, 1, 1, 1), (-1, -1, 2, 1)], dtype=f32)

# name -> (C, H, W, D, table, batch, y_div)
CASES = {
    "9x13": (1, 9, 13, 17, table_of(case_angles(5)), 2, 1),
    "24x20": (2, 24, 20, 33, table_of(case_angles(7)), 2, 1),
    "16x16-short": (1, 16, 16, 12, table_of(case_angles(4)), 2, 2),
    "40x36": (3, 40, 36, 59, table_of(case_angles(23)), 3, 3),
    "64x96": (1, 64, 96, 117, table_of(case_angles(1)), 1, 1),
    "136x72": (1, 136, 72, 155, table_of(case_angles(3)), 1, 1),
    "72x136": (1, 72, 136, 155, table_of(case_angles(3)), 1, 1),
    "200x40": (1, 200, 40, 300, table_of(case_angles(2)), 1, 1),
    "wide-slab": (1, 16, 24, 200, WIDE_TABLE, 2, 1),
    "skip-rows": (1, 96, 8, 16, SKIP_TABLE, 1, 1),
    "skip-cols": (1, 8, 96, 16, SKIP_TABLE_T, 1, 1),
}
# (H, W, D) of the exact cases: D and the cross extent of equal and of different parity (weights
# 1, 0 or 1/2, 1/2 at the axis angles)
EXACT_SHAPES = [(9, 13, 13), (9, 13, 14), (12, 10, 15), (10, 12, 16)]
COEFS = (0.3, math.sqrt(1 - 0.09), 400.0)  # a, k, grad_scale of the randn cases


def case_inputs(name):
    """Seeded randn inputs of a case: x, eps (batch, C, H, W), g (batch, C, nA, D), y (rows, C, nA, D)."""
    C, H, W, D, table, batch, y_div = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    nA = table.shape[0]
    x, eps = (rng.standard_normal((batch, C, H, W)).astype(f32) for _ in range(2))
    g = rng.standard_normal((batch, C, nA, D)).astype(f32)
    y = rng.standard_normal((batch // y_div, C, nA, D)).astype(f32)
    return x, eps, g, y


@functools.lru_cache(maxsize=None)
def matrices(name):
    """(dense64, dense32) of a case, computed once and shared (treat as read-only)."""
    C, H, W, D, table, _, _ = CASES[name]
    return dense64(table, H, W, D), dense32(table, H, W, D)


@functools.lru_cache(maxsize=None)
def reference64(name):
    """fp64 results of a case on case_inputs: dict of 'apply', 'adjoint', 'v', 'work', 'rsq'
    (per sample), each against both matrices: key -> (with dense64, with dense32); plus the
    absolute-value products 'E_apply', 'E_adjoint', 'E_v' with |dense32|."""
    C, H, W, D, table, batch, y_div = CASES[name]
    A64, A32 = matrices(name)
    x, eps, g, y = (v.astype(np.float64) for v in case_inputs(name))
    a, k, gs = (float(f32(v)) for v in COEFS)
    nA = table.shape[0]
    out = {}
    xf, ef, gf = x.reshape(batch * C, H * W), eps.reshape(batch * C, H * W), g.reshape(batch * C, nA * D)
    yf = np.repeat(y, y_div, axis=0).reshape(batch * C, nA * D)
    for tag, A in (("64", A64), ("32", A32)):
        x0 = (xf - k * ef) / a
        r = yf - x0 @ A.T
        out["apply" + tag] = (xf @ A.T).reshape(batch, C, nA, D)
        out["adjoint" + tag] = (gf @ A).reshape(batch, C, H, W)
        out["work" + tag] = (gs * r).reshape(batch, C, nA, D)
        out["v" + tag] = (gs * r @ A).reshape(batch, C, H, W)
        out["rsq" + tag] = (r ** 2).reshape(batch, -1).sum(1)
    absA = np.abs(A32)
    out["E_apply"] = (np.abs(xf) @ absA.T).reshape(batch, C, nA, D)
    out["E_adjoint"] = (np.abs(gf) @ absA).reshape(batch, C, H, W)
    ax0 = (np.abs(xf) + abs(k) * np.abs(ef)) / abs(a)
    out["E_v"] = (abs(gs) * (np.abs(yf) + ax0 @ absA.T) @ absA).reshape(batch, C, H, W)
    return out


@functools.lru_cache(maxsize=None)
def emulation(name):
    """The fp32 emulations of a case on case_inputs: dict 'apply', 'adjoint', 'v', 'work'."""
    C, H, W, D, table, batch, y_div = CASES[name]
    x, eps, g, y = case_inputs(name)
    a, k, gs = COEFS
    nA = table.shape[0]
    out = {key: np.zeros(shape, dtype=f32) for key, shape in
           (("apply", (batch, C, nA, D)), ("adjoint", (batch, C, H, W)), ("v", (batch, C, H, W)),
            ("work", (batch, C, nA, D)))}
    for b in range(batch):
        for c in range(C):
            out["apply"][b, c] = project32(table, x[b, c], D)
            out["adjoint"][b, c] = backproject32(table, g[b, c], H, W)
            out["work"][b, c], out["v"][b, c], _ = pass1_32(table, x[b, c], eps[b, c], y[b // y_div, c],
                                                             a, k, gs)
    return out


def max_over_max(got, ref) -> float:
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def emulation_distance(name):
    """max|emulation - dense64 result| / max|dense64 result| per map: what the rounding of the
    crossing position and of the sums costs at this shape.  The GPU test allows twice this."""
    emu, ref = emulation(name), reference64(name)
    return {key: max_over_max(emu[key], ref[key + "64"]) for key in ("apply", "adjoint", "v")}


def rounding_steps(name):
    """The rounding steps on the longest path of each map's sum (n of the per-element bound):
    A: two products, their sum, max(H, W) - 1 additions, the length -> max(H, W) + 4 covers it;
    A^T: a product, one addition per angle pair, the length, one addition per angle ->
    2 * angles + 4; pass-1 v: their sum plus x0's three operations, the residual and grad_scale,
    and one to spare."""
    C, H, W, D, table, _, _ = CASES[name]
    n_a, n_t = max(H, W) + 4, 2 * table.shape[0] + 4
    return {"apply": n_a, "adjoint": n_t, "v": n_a + n_t + 6}


def rho(got, ref, E, n) -> float:
    """max over elements of |got - ref| / (n 2^-24 E); elements with E == 0 must be exactly 0."""
    got, ref, E = (np.asarray(v, dtype=np.float64) for v in (got, ref, E))
    zero = E == 0
    assert not got[zero].any(), "an element no ray reaches must be exactly 0"
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / (n * 2.0 ** -24 * E[~zero])).max())
