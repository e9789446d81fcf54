"""Reference for the channel-mixing kind (SP_OP_CHANNEL_MIX): y = M x across the channel axis at
every pixel.  No dependence on the operator's code.  Every pass is stated in fp64 twice: ``Mix`` per
pixel with ``einsum`` and ``Dense`` on the m × n matrix M ⊗ I_{HW} (and the lifts of N, U, V) built
by index arithmetic, on flat rows.  Both evaluate the fp32 tables taken as exact, as the library
defines the map.  ``Emu`` restates every kernel pass in numpy float32 in the operation order that
csrc/sp_chanmix.hip documents (every product and sum rounds on its own; a sum over a channel or
component index runs in ascending order, left to right).  The test cases and the exact cases live
here too.

Roundings on the longest path of a pass (``roundings``), with dot(K) = 2K − 1 (K products, K − 1
sums):
  apply, pinv_t   dot(C)                                                              2C − 1
  adjoint, pinv   dot(Cy)                                                             2Cy − 1
  dps, pgdm       x0 (the fused x − k·eps, the quotient: 2), dot(C), r, the scale by gs, dot(Cy)
                                                                                      2C + 2Cy + 2
  rsq             relative to its own envelope: r twice (2C + 2 each), the square, the thread's
                  4·Cy sequential sums, 6 + 2 levels of the block tree               4C + 4Cy + 13
  prox            dot(C), r, dot(Cy), the weight S/(S·S + ρ) (3), its product, dot(Cy), the sum
                  with x0                                                             2C + 4Cy + 3
  diffpir         x0 by reciprocals (4), the prox, a·z, the difference, 1/k, the product, c_eps·,
                  the sum with c_xi·ξ, the sum with a'·z                              2C + 4Cy + 14
  ddrm            x0 (4), dot(C), f_θ (S·S, c1·σ', the root, the product, the quotient, 1 − r: 6),
                  its product, three sums, dot(C), a'·                                4C + 14
"""

from __future__ import annotations

import numpy as np
import torch

import ddrm_ref as dr

U24 = 2.0 ** -24
F32 = np.float32


# --- tables ---------------------------------------------------------------------------------------
def svd_tables(matrix, rtol: float = 1e-6) -> dict:
    """fp64 tables of a Cy × C matrix: M, N = V diag(P) Uᵀ, U, V (full), S, P and the kept mask."""
    m = np.asarray(matrix, dtype=np.float64)
    cy = m.shape[0]
    u, s, vh = np.linalg.svd(m, full_matrices=True)
    v = vh.T
    keep = s > rtol * s.max()
    p = np.zeros_like(s)
    p[keep] = 1.0 / s[keep]
    return dict(M=m, N=(v[:, :cy] * p) @ u.T, U=u, V=v, S=s, P=p, keep=keep)


def round32(tab: dict) -> dict:
    """The tables as the library is given them: rounded to fp32."""
    return {k: (np.asarray(v, dtype=np.float32) if k != "keep" else np.asarray(v)) for k, v in tab.items()}


def flat_tables(tab32: dict) -> np.ndarray:
    """The descriptor's taps: M, N, U, V, S, P, row-major, back to back."""
    return np.concatenate([np.asarray(tab32[k], dtype=np.float32).reshape(-1) for k in "MNUVSP"])


def _orth(n: int, seed: int) -> np.ndarray:
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def from_spectrum(c: int, s, seed: int) -> np.ndarray:
    """A seeded generic Cy × C matrix with the singular values ``s``."""
    s = np.asarray(s, dtype=np.float64)
    return _orth(len(s), seed) @ np.diag(s) @ _orth(c, seed + 1)[:, :len(s)].T


H4 = 0.5 * np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=np.float64)
PERM = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1], [-1, 0, 0, 0]], dtype=np.float64)  # U V^T not symmetric


def exact_tables(drop: bool = False) -> dict:
    """V the 4 × 4 Hadamard matrix over 2, U a signed permutation, S = 2, P = 1/2 (0 on the last
    component with ``drop``): M = 2 U Vᵀ has entries ±1, N entries ±1/4 or 0 sums of them."""
    s = np.full(4, 2.0)
    p = np.array([0.5, 0.5, 0.5, 0.0 if drop else 0.5])
    return dict(M=PERM @ np.diag(s) @ H4.T, N=(H4 * p) @ PERM.T, U=PERM.copy(), V=H4.copy(), S=s, P=p,
                keep=p != 0)


RANK_DEF = np.array([[0.25, 0.1, 0.05], [0.05, 0.2, 0.15], [0.3, 0.3, 0.2]])  # row 3 = row 1 + row 2
LUMA = np.array([[0.299, 0.587, 0.114]])

# (name, (C, Cy, H, W), the matrix or "exact", rtol)
CASES = [
    ("c3-1x1-mean", (3, 1, 1, 1), np.full((1, 3), 1 / 3), 1e-6),
    ("c3-2x2-luma", (3, 1, 2, 2), LUMA, 1e-6),
    ("c3y2-3x5", (3, 2, 3, 5), from_spectrum(3, (0.9, 0.4), 11), 1e-6),
    ("c3y3-33x35-full", (3, 3, 33, 35), from_spectrum(3, (0.9, 0.6, 0.3), 13), 1e-6),
    ("c3y3-16x12-rankdef", (3, 3, 16, 12), RANK_DEF, 1e-6),
    ("c4y4-8x8-exact", (4, 4, 8, 8), "exact", 0.0),
    ("c3-64x36-mean", (3, 1, 64, 36), np.full((1, 3), 1 / 3), 1e-6),
    ("c8y5-16x24", (8, 5, 16, 24), from_spectrum(8, np.linspace(0.9, 0.3, 5), 17), 1e-6),
    ("c1-4x4", (1, 1, 4, 4), np.array([[0.7]]), 1e-6),
    ("c3y2-32x32-rtol", (3, 2, 32, 32), from_spectrum(3, (0.8, 4e-4), 19), 1e-2),
]
FORMS = ((3, 3), (4, 2))  # (batch, y_div)
TILE = 256  # pixel groups per workgroup


def case(i: int):
    """(name, (C, Cy, H, W), fp64 tables, rtol)."""
    name, shape, m, rtol = CASES[i]
    return name, shape, (exact_tables() if isinstance(m, str) else svd_tables(m, rtol)), rtol


def partials(shape) -> int:
    """sp_rsq_partials: the tiles of 256 groups (four pixels where H·W % 4 == 0, else one)."""
    hw = shape[2] * shape[3]
    return -(-(hw // 4 if hw % 4 == 0 else hw) // TILE)


def expand(y: torch.Tensor, batch: int, ydiv: int) -> torch.Tensor:
    return y.repeat_interleave(ydiv, dim=0)[:batch]


def roundings(what: str, c: int, cy: int) -> int:
    return {"apply": 2 * c - 1, "pinv_t": 2 * c - 1, "adjoint": 2 * cy - 1, "pinv": 2 * cy - 1,
            "dps": 2 * c + 2 * cy + 2, "pgdm": 2 * c + 2 * cy + 2, "rsq": 4 * c + 4 * cy + 13,
            "prox": 2 * c + 4 * cy + 3, "diffpir": 2 * c + 4 * cy + 14, "ddrm": 4 * c + 14}[what]


# --- the passes, once over the four products ------------------------------------------------------------
class _Passes:
    """Every pass in terms of ``mul(name, v, transpose)``: T v (or Tᵀ v) for the table ``name``;
    Vt / Ut are the thin factors (the first Cy columns of V), Vf the full V."""

    def apply(self, x): return self.mul("M", x)
    def adjoint(self, y): return self.mul("M", y, True)
    def pinv(self, y): return self.mul("N", y)
    def pinv_t(self, x): return self.mul("N", x, True)

    def dps(self, x, eps, y, a, k, gs):
        r = y - self.apply((x - k * eps) / a)
        return self.adjoint(gs * r), r.reshape(r.shape[0], -1).square().sum(1)

    def pgdm(self, x, eps, y, a, k, gs):
        return gs * self.pinv(y - self.apply((x - k * eps) / a))

    def prox(self, x0, y, rho):
        s = self.spec(self.S)
        return x0 + self.mul("Vt", (s / (s * s + rho)) * self.mul("U", y - self.apply(x0), True))

    def diffpir(self, x, eps, y, xi, c):
        z = self.prox((x - c["k"] * eps) / c["a"], y, c["rho"])
        return c["a_prev"] * z + (c["c_eps"] * ((x - c["a"] * z) / c["k"]) + c["c_xi"] * xi)

    def class_coefs(self, c, big=None):
        """(f_θ, f_ε, f_y, f_ξ) of the C components: observed iff P ≠ 0, the null space unobserved;
        ``big``: the class mask of the first Cy components (fp64's own when None)."""
        cfull = self.V.shape[0]
        s2 = torch.zeros(cfull, dtype=torch.float64)
        s2[: len(self.S)] = self.S * self.S
        obs = torch.zeros(cfull, dtype=torch.bool)
        obs[: len(self.S)] = self.P != 0
        bigf = dr.big_mask64(s2, c)
        if big is not None:
            bigf[: len(self.S)] = torch.as_tensor(big)
        return dr.coefficients(s2, obs, bigf, c)

    def ddrm(self, x, eps, y, xi, c, big=None):
        f_th, f_ep, f_y, f_xi = (self.spec(f.to(x.dtype)) for f in self.class_coefs(c, big))
        x0 = (x - c["k"] * eps) / c["a"]
        ybar = self.pad(self.spec(self.P) * self.mul("U", y, True))
        w = (f_th * self.mul("Vf", x0, True) + f_ep * self.mul("Vf", eps, True) + f_y * ybar
             + f_xi * self.mul("Vf", xi, True))
        return c["a_prev"] * self.mul("Vf", w)

    def pgdm_gradient(self, x0, y):
        """∂/∂x0 ‖A⁺y − A⁺A x0‖² by the chain rule: −2 (A⁺A)ᵀ (A⁺y − A⁺A x0)."""
        d = self.pinv(y) - self.pinv(self.apply(x0))
        return -2.0 * self.adjoint(self.pinv_t(d))


class Mix(_Passes):
    """Per pixel with einsum, on (B, K, H, W) tensors in ``dtype``."""

    def __init__(self, shape, tab, dtype=torch.float64, absolute=False):
        self.C, self.Cy, self.H, self.W = shape
        t = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dtype) for k, v in tab.items() if k != "keep"}
        if absolute:
            t = {k: v.abs() for k, v in t.items()}
        self.M, self.N, self.U, self.V, self.S, self.P = (t[k] for k in "MNUVSP")
        self.tabs = dict(M=self.M, N=self.N, U=self.U, Vf=self.V, Vt=self.V[:, : self.Cy])

    def mul(self, name, v, transpose=False):
        t = self.tabs[name]
        return torch.einsum("rk,bkhw->brhw", t.t() if transpose else t, v)

    def spec(self, f): return f.view(-1, 1, 1)

    def pad(self, v):
        return torch.cat([v, v.new_zeros(v.shape[0], self.C - self.Cy, self.H, self.W)], dim=1)


def lift(t: torch.Tensor, hw: int) -> torch.Tensor:
    """T ⊗ I_{HW} by index arithmetic: entry (r·HW + p, k·HW + p) is T[r][k]."""
    rows, cols = t.shape
    out = torch.zeros(rows * hw, cols * hw, dtype=t.dtype)
    p = torch.arange(hw)
    for r in range(rows):
        for k in range(cols):
            out[r * hw + p, k * hw + p] = t[r, k]
    return out


class Dense(_Passes):
    """On the dense lifted matrices, flat rows (B, K·HW)."""

    def __init__(self, shape, tab):
        self.C, self.Cy, self.H, self.W = shape
        self.hw = self.H * self.W
        t = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)) for k, v in tab.items() if k != "keep"}
        self.S, self.P, self.V = t["S"], t["P"], t["V"]
        self.tabs = {k: lift(v, self.hw) for k, v in
                     dict(M=t["M"], N=t["N"], U=t["U"], Vf=t["V"], Vt=t["V"][:, : self.Cy]).items()}
        self.A = self.tabs["M"]

    def mul(self, name, v, transpose=False):
        t = self.tabs[name]
        return v @ (t if transpose else t.t())

    def spec(self, f): return f.repeat_interleave(self.hw)

    def pad(self, v):
        return torch.cat([v, v.new_zeros(v.shape[0], (self.C - self.Cy) * self.hw)], dim=1)


def envelope(shape, tab, what, x=None, eps=None, y=None, xi=None, c=None, big=None):
    """The same pass on absolute values with absolute tables (every difference a sum); ``big`` is
    the DDRM class mask the coefficients are taken with."""
    a = Mix(shape, tab, absolute=True)
    ab = lambda v: None if v is None else v.double().abs()  # noqa: E731
    x, eps, y, xi = ab(x), ab(eps), ab(y), ab(xi)
    c = {k: abs(v) for k, v in (c or {}).items()}
    if what in ("apply", "pinv_t"):
        return a.apply(x) if what == "apply" else a.pinv_t(x)
    if what in ("adjoint", "pinv"):
        return a.adjoint(y) if what == "adjoint" else a.pinv(y)
    if what in ("dps", "pgdm", "rsq"):
        r = y + a.apply((x + c["k"] * eps) / c["a"])
        if what == "rsq":
            return r.reshape(r.shape[0], -1).square().sum(1)
        return c["gs"] * (a.adjoint(r) if what == "dps" else a.pinv(r))
    s = a.spec(a.S)
    if what in ("prox", "diffpir"):
        x0 = x if what == "prox" else (x + c["k"] * eps) / c["a"]
        z = x0 + a.mul("Vt", (s / (s * s + c["rho"])) * a.mul("U", y + a.apply(x0), True))
        if what == "prox":
            return z
        return c["a_prev"] * z + (c["c_eps"] * ((x + c["a"] * z) / c["k"]) + c["c_xi"] * xi)
    assert what == "ddrm", what
    f_th, f_ep, f_y, f_xi = (a.spec(f.abs()) for f in Mix(shape, tab).class_coefs(c, big))
    x0 = (x + c["k"] * eps) / c["a"]
    w = (f_th * a.mul("Vf", x0, True) + f_ep * a.mul("Vf", eps, True)
         + f_y * a.pad(a.spec(a.P) * a.mul("U", y, True)) + f_xi * a.mul("Vf", xi, True))
    return c["a_prev"] * a.mul("Vf", w)


def big_mask32(tab32, c) -> torch.Tensor:
    """The class mask of the Cy components as the kernel decides it: (σ'·σ')·(S·S) ≥ σ_y·σ_y in fp32."""
    s = np.asarray(tab32["S"], dtype=np.float32)
    return dr.big_mask32(np.float32(s * s), c)


# --- the kernels in numpy float32 ---------------------------------------------------------------------------
def _dot(t, vs):
    """t[0] v[0], then acc = acc + t[k] v[k], ascending; every operation rounds to fp32."""
    acc = F32(t[0]) * vs[0]
    for k in range(1, len(vs)):
        acc = acc + F32(t[k]) * vs[k]
    return acc


def class_coefs32(c, s2, observed):
    """ddrm_class_coefs of csrc/sp_ops.h in numpy float32."""
    sp, sy, eta, eb, c1 = (F32(c[k]) for k in ("sig_prev", "sig_y", "eta", "eta_b", "c1"))
    one = F32(1)
    sp2, es = sp * sp, eta * sp
    if not observed or s2 == 0:
        return one, c1 * sp, F32(0), es
    if sp2 * s2 >= sy * sy:
        e = eb * sy
        v = sp2 - (e * e) / s2
        return one - eb, F32(0), eb, np.sqrt(max(v, F32(0)), dtype=np.float32)
    r = ((c1 * sp) * np.sqrt(s2, dtype=np.float32)) / sy
    return one - r, F32(0), r, es


class Emu:
    """The kernels' arithmetic on flat fp32 rows; ``stride`` is the distance between the planes of a
    row (H·W in the kernels)."""

    def __init__(self, shape, tab32, stride=None):
        self.C, self.Cy, self.H, self.W = shape
        self.hw = self.H * self.W
        self.stride = self.hw if stride is None else stride
        self.t = {k: np.asarray(tab32[k], dtype=np.float32) for k in "MNUVSP"}

    def planes(self, rows, k):
        rows = np.asarray(rows, dtype=np.float32).reshape(len(rows), -1)
        return [rows[:, j * self.stride: j * self.stride + self.hw] for j in range(k)]

    @staticmethod
    def join(planes):
        return np.concatenate(planes, axis=1)

    def _map(self, t, v, transpose):
        t = t.T if transpose else t
        return [_dot(t[r], v) for r in range(t.shape[0])]

    def apply(self, x): return self.join(self._map(self.t["M"], self.planes(x, self.C), False))
    def adjoint(self, y): return self.join(self._map(self.t["M"], self.planes(y, self.Cy), True))
    def pinv(self, y): return self.join(self._map(self.t["N"], self.planes(y, self.Cy), False))
    def pinv_t(self, x): return self.join(self._map(self.t["N"], self.planes(x, self.C), True))

    def _residual(self, x0, y):
        ax = self._map(self.t["M"], x0, False)
        return [yy - a for yy, a in zip(self.planes(y, self.Cy), ax)]

    def _x0_div(self, x, eps, a, k):
        """fma(-k, eps, x) / a: the product of two fp32 numbers is exact in fp64, where the sum rounds
        to 53 bits before its rounding to fp32 (a double rounding that can differ from the fused
        operation only at an exact tie of the fp64 result; never on the exact cases)."""
        k64 = np.float64(F32(k))
        return [(xx.astype(np.float64) - k64 * ee.astype(np.float64)).astype(np.float32) / F32(a)
                for xx, ee in zip(self.planes(x, self.C), self.planes(eps, self.C))]

    def _x0_rcp(self, x, eps, a, k):
        inv_a = F32(1) / F32(a)
        return [(xx - F32(k) * ee) * inv_a for xx, ee in zip(self.planes(x, self.C), self.planes(eps, self.C))]

    def dps(self, x, eps, y, a, k, gs):
        r = self._residual(self._x0_div(x, eps, a, k), y)
        return self.join(self._map(self.t["M"], [F32(gs) * rr for rr in r], True))

    def pgdm(self, x, eps, y, a, k, gs):
        r = self._residual(self._x0_div(x, eps, a, k), y)
        return self.join([F32(gs) * v for v in self._map(self.t["N"], r, False)])

    def _prox(self, x0, y, rho):
        r = self._residual(x0, y)
        s = self.t["S"]
        d = [(s[j] / (s[j] * s[j] + F32(rho))) * _dot(self.t["U"][:, j], r) for j in range(self.Cy)]
        return [x0[ch] + _dot(self.t["V"][ch, : self.Cy], d) for ch in range(self.C)]

    def prox(self, x0, y, rho):
        return self.join(self._prox(self.planes(x0, self.C), y, rho))

    def diffpir(self, x, eps, y, xi, c):
        z = self._prox(self._x0_rcp(x, eps, c["a"], c["k"]), y, c["rho"])
        inv_k = F32(1) / F32(c["k"])
        a, ap, ce, cx = (F32(c[k]) for k in ("a", "a_prev", "c_eps", "c_xi"))
        out = []
        for xx, zz, nn in zip(self.planes(x, self.C), z, self.planes(xi, self.C)):
            eh = (xx - a * zz) * inv_k
            out.append(ap * zz + (ce * eh + cx * nn))
        return self.join(out)

    def ddrm(self, x, eps, y, xi, c):
        t = self.t
        x0 = self._x0_rcp(x, eps, c["a"], c["k"])
        ev, nz, yv = self.planes(eps, self.C), self.planes(xi, self.C), self.planes(y, self.Cy)
        w = []
        for j in range(self.C):
            obs = j < self.Cy and t["P"][j] != 0
            s = t["S"][j] if j < self.Cy else F32(0)
            th, ep, fy, fx = class_coefs32(c, s * s, obs)
            a0, ae, ax = _dot(t["V"][:, j], x0), _dot(t["V"][:, j], ev), _dot(t["V"][:, j], nz)
            if j < self.Cy:
                ybar = t["P"][j] * _dot(t["U"][:, j], yv)
                w.append(((th * a0 + ep * ae) + fy * ybar) + fx * ax)
            else:
                w.append((th * a0 + ep * ae) + fx * ax)
        return self.join([F32(c["a_prev"]) * _dot(t["V"][ch], w) for ch in range(self.C)])


# --- exact cases --------------------------------------------------------------------------------------
# Integer data in [-3, 3], a = k = 1/2 (x0 = 2x − eps, an integer), gs = 4, ρ = 4 (S·S + ρ = 8, the
# weight 1/4), the DiffPIR scalars of prox_ref.EXACT, the DDRM scalars of ddrm_ref.exact_coefs for the
# singular value 2 (σ_y = 1 big, σ_y = 2 small).  Every table entry is a multiple of 1/4 below 2 and
# every intermediate a dyadic rational of a few bits: no fp32 evaluation rounds.
EXACT_DPS = dict(a=0.5, k=0.5, gs=4.0)
EXACT_PROX = dict(a=0.5, k=0.5, rho=4.0, a_prev=0.5, c_eps=0.25, c_xi=0.125)
EXACT_DDRM = {"big": dr.exact_coefs("big", 0.5), "small": dr.exact_coefs("small", 0.5)}
DYADIC = np.array([[0.25, 0.5, 0.25]])  # colorization weights; exact for the passes that read M alone

# (name, (C, Cy, H, W), tables, the passes that are exact)
ALL_PASSES = ("apply", "adjoint", "pinv", "pinv_t", "dps", "pgdm", "prox", "diffpir", "ddrm")
EXACT_CASES = [
    ("hadamard", (4, 4, 8, 8), exact_tables(), ALL_PASSES),
    ("hadamard-drop", (4, 4, 3, 5), exact_tables(drop=True), ALL_PASSES),
    ("dyadic-colorization", (3, 1, 2, 2), svd_tables(DYADIC), ("apply", "adjoint", "dps")),
]


def exact_data(shape, batch: int, ydiv: int, seed: int = 5):
    """Integer-valued fp32 x, eps, xi (batch, C, H, W) and y (rows, Cy, H, W) in [-3, 3]."""
    c, cy, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randint(-3, 4, (batch, c, h, w), generator=g).float() for _ in range(3))
    y = torch.randint(-3, 4, (-(-batch // ydiv), cy, h, w), generator=g).float()
    return x, eps, xi, y


def run_passes(obj, x, eps, y, xi, regime="big"):
    """Every pass of ``obj`` (Mix, Dense or Emu) at the exact scalars, by name."""
    e, p, c = EXACT_DPS, EXACT_PROX, EXACT_DDRM[regime]
    v = obj.dps(x, eps, y, e["a"], e["k"], e["gs"])
    return {"apply": obj.apply(x), "adjoint": obj.adjoint(y), "pinv": obj.pinv(y), "pinv_t": obj.pinv_t(x),
            "dps": v[0] if isinstance(v, tuple) else v, "pgdm": obj.pgdm(x, eps, y, e["a"], e["k"], -2.0),
            "prox": obj.prox(x, y, p["rho"]), "diffpir": obj.diffpir(x, eps, y, xi, p),
            "ddrm": obj.ddrm(x, eps, y, xi, c)}
