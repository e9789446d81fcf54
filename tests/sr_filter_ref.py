"""A second, independent statement of the filtered super-resolution map
(operators/sr_filter.py), in fp64, and fp32 emulations of the two algorithm shapes a kernel for it
can take.

The map on one plane is A X = A_H X A_W^T with A_L the (L/s, L) matrix
    A_L[o, sym(s o + u - P)] += k[u],   u = 0 .. K-1,   P = (K - s) / 2,
sym the symmetric fold (-1-g -> g, L+g -> L-1-g), built here by index arithmetic; the transpose is
A^T S = A_H^T S A_W.  The matrices take three faults for the tests that show the exact cases can
see them: `shift` moves the window (P + shift), `drop` leaves a fold's terms out ("lo" / "hi"),
and the adjoint emulation can reverse its taps.

Emulations (numpy fp32, every step one rounding: fma(t, p, acc) is evaluated in fp64 and rounded):
  emu_apply   "hv": the horizontal pass over every row, taps ascending, then the vertical pass;
              "vh": columns first
  emu_adjoint a gather per pixel: per axis the terms (output o, tap a - s o), a = e + P, over the
              members e of M(i) = {i, -1-i if i < P, 2L-1-i if i >= L-P} in that order, o
              ascending; "cols_inner" sums the column terms first, "rows_inner" the row terms
"""

from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def sym(g: int, L: int) -> int:
    if g < 0:
        g = -1 - g
    if g >= L:
        g = 2 * L - 1 - g
    assert 0 <= g < L, "more than one fold"
    return g


def matrix_1d(taps, L: int, s: int, shift: int = 0, drop: str | None = None) -> np.ndarray:
    k = np.asarray(taps, dtype=F64)
    K = k.size
    P = (K - s) // 2 + shift
    A = np.zeros((L // s, L), dtype=F64)
    for o in range(L // s):
        for u in range(K):
            g = s * o + u - P
            if (drop == "lo" and g < 0) or (drop == "hi" and g >= L):
                continue
            A[o, sym(g, L)] += k[u]
    return A


def apply64(x, taps, s, **fault):
    x = np.asarray(x, dtype=F64)
    AH, AW = matrix_1d(taps, x.shape[-2], s, **fault), matrix_1d(taps, x.shape[-1], s, **fault)
    return AH @ x @ AW.T


def adjoint64(g, taps, s, **fault):
    g = np.asarray(g, dtype=F64)
    AH, AW = matrix_1d(taps, g.shape[-2] * s, s, **fault), matrix_1d(taps, g.shape[-1] * s, s, **fault)
    return AH.T @ g @ AW


def _fma(t, p, acc):
    return (F64(t) * p.astype(F64) + acc.astype(F64)).astype(F32)


def _strided_pass(x, k, s, P, axis, **fault):
    """fp32 chain over the taps along `axis` of the symmetric extension of x (..., H, W)."""
    x = np.moveaxis(x, axis, -1)
    L, K = x.shape[-1], k.size
    P = P + fault.get("shift", 0)
    drop = fault.get("drop")
    acc = np.zeros(x.shape[:-1] + (L // s,), dtype=F32)
    for u in range(K):
        pos = s * np.arange(L // s) + u - P
        src = np.array([sym(int(g), L) for g in pos])
        vals = x[..., src].copy()
        if drop == "lo":
            vals[..., pos < 0] = 0
        if drop == "hi":
            vals[..., pos >= L] = 0
        acc = _fma(k[u], vals, acc)
    return np.moveaxis(acc, -1, axis)


def emu_apply(x, taps, s, order="hv", **fault):
    k = np.asarray(taps, dtype=F32)
    P = (k.size - s) // 2
    x = np.asarray(x, dtype=F32)
    for axis in ((-1, -2) if order == "hv" else (-2, -1)):
        x = _strided_pass(x, k, s, P, axis, **fault)
    return x


def axis_terms(K: int, s: int, L: int, shift: int = 0, drop: str | None = None):
    """Per pixel i of an axis of length L the list of (o, u) in the gather's order."""
    P = (K - s) // 2 + shift
    No = L // s
    terms = []
    for i in range(L):
        members = [i]
        if i < P and drop != "lo":
            members.append(-1 - i)
        if i >= L - P and drop != "hi":
            members.append(2 * L - 1 - i)
        row = []
        for e in members:
            a = e + P
            for o in range(No):
                if 0 <= a - s * o < K:
                    row.append((o, a - s * o))
        terms.append(row)
    return terms


def _gather_pass(g, k, terms, axis):
    """out[.., i, ..] = fp32 chain over terms[i] of k[u] g[.., o, ..] along `axis`."""
    g = np.moveaxis(g, axis, -1)
    L = len(terms)
    slots = max(len(t) for t in terms)
    acc = np.zeros(g.shape[:-1] + (L,), dtype=F32)
    for n in range(slots):
        o = np.array([t[n][0] if n < len(t) else 0 for t in terms])
        w = np.array([k[t[n][1]] if n < len(t) else 0.0 for t in terms], dtype=F32)
        live = np.array([n < len(t) for t in terms])
        nxt = (w.astype(F64) * g[..., o].astype(F64) + acc.astype(F64)).astype(F32)
        acc = np.where(live, nxt, acc)
    return np.moveaxis(acc, -1, axis)


def emu_adjoint(g, taps, s, order="cols_inner", reverse=False, **fault):
    k = np.asarray(taps, dtype=F32)
    kk = k[::-1] if reverse else k
    g = np.asarray(g, dtype=F32)
    H, W = g.shape[-2] * s, g.shape[-1] * s
    th, tw = axis_terms(k.size, s, H, **fault), axis_terms(k.size, s, W, **fault)
    if order == "cols_inner":
        return _gather_pass(_gather_pass(g, kk, tw, -1), kk, th, -2)
    return _gather_pass(_gather_pass(g, kk, th, -2), kk, tw, -1)


# --- taps ---------------------------------------------------------------------------------------
def keys_cubic(t, a=-0.5):
    t = abs(float(t))
    if t <= 1:
        return (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1
    if t < 2:
        return a * t ** 3 - 5 * a * t ** 2 + 8 * a * t - 4 * a
    return 0.0


def bicubic_taps64(s: int) -> np.ndarray:
    k = np.array([keys_cubic((2 * t + 1 - 4 * s) / (2 * s)) / s for t in range(4 * s)], dtype=F64)
    return k / k.sum()


def exact_taps(K: int) -> np.ndarray:
    """Asymmetric, sparse, multiples of 1/8, non-zero at both ends of the support."""
    k = np.zeros(K, dtype=F32)
    k[0], k[K - 1] = 3 / 8, -1 / 8
    if K >= 4:
        k[K // 2] = 4 / 8
    if K >= 6:
        k[1] = -2 / 8
    if K >= 12:
        k[K - 4] = 1 / 8
    return k


# the exact cases (s, K, H, W): the taps of exact_taps on integers in [-3, 3]
EXACT_SHAPES = [(2, 2, 4, 8), (2, 8, 4, 12), (2, 32, 16, 32), (4, 6, 8, 12), (4, 16, 8, 24), (4, 32, 16, 16),
                (8, 8, 16, 8), (8, 10, 8, 16), (8, 32, 16, 32), (2, 8, 18, 68), (4, 16, 36, 132), (8, 32, 72, 136)]


def exact_data(s, K, H, W, lead=(2,)):
    """(taps, x, eps, g, y) for an exact case: integer fields in [-3, 3] as fp64."""
    rng = np.random.default_rng(100 * s + K)
    x, eps = (rng.integers(-3, 4, size=(*lead, H, W)).astype(F64) for _ in range(2))
    g, y = (rng.integers(-3, 4, size=(*lead, H // s, W // s)).astype(F64) for _ in range(2))
    return exact_taps(K), x, eps, g, y


def random_taps(K: int, seed: int = 0) -> np.ndarray:
    """Asymmetric fp32 taps of either sign, sum about 1."""
    rng = np.random.default_rng(1000 + 37 * K + seed)
    k = rng.standard_normal(K) * 0.3 + 1.0 / K
    return k.astype(F32)
