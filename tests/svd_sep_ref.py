"""fp64 semantics of the separable-SVD kind (SP_OP_SVD_SEPARABLE) — TEST INFRASTRUCTURE ONLY.

``A X = A_H X A_Wᵀ`` on every plane.  Two statements of every pass, neither using the operator's
code:

* ``Dense`` — dense Kronecker matrices on flat planes, built by index arithmetic (``kron_dense``):
  ``A = U diag(S) V_obsᵀ``, ``A⁺ = V_obs diag(P) Uᵀ``, ``Π = V_obs diag(K) V_obsᵀ`` and the passes
  as matrix products and, for the prox, a dense solve;
* ``Sep`` — the separable evaluation the kernels use (one product per side), in any dtype, in
  either side order and either summation order, with the wrong variants the exact cases must tell
  apart.

``Tables`` holds the six tables of the descriptor: ``from_factors`` takes the SVDs itself in fp64
(``numpy.linalg.svd``), ``from_flat`` unpacks an operator's fp32 buffer, ``exact`` builds
block-diagonal signed permutations of Sylvester–Hadamard blocks (orders 1, 4, 16, 64 scaled by 1,
1/2, 1/4, 1/8: dyadic and exactly orthogonal) with S and P powers of two, on which no fp32
evaluation of integer data rounds.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

import ddrm_ref as dr


# --- dense Kronecker matrices by index arithmetic -------------------------------------------------
def kron_dense(ah, aw) -> np.ndarray:
    """``K[i·cw + j, k·Cw + l] = ah[i, k]·aw[j, l]``: (ah ⊗ aw) on row-major flat planes, so
    ``K vec(X) = vec(ah X awᵀ)``."""
    ah, aw = np.asarray(ah, dtype=np.float64), np.asarray(aw, dtype=np.float64)
    (rh, ch), (rw, cw) = ah.shape, aw.shape
    out = np.empty((rh * rw, ch * cw), dtype=np.float64)
    for i in range(rh):
        for k in range(ch):
            out[i * rw:(i + 1) * rw, k * cw:(k + 1) * cw] = ah[i, k] * aw
    return out


def reflect_matrix(taps, size: int) -> np.ndarray:
    """One axis of the reflect-padded correlation (``F.pad(mode="reflect")``), dense fp64."""
    t = np.asarray(taps, dtype=np.float64)
    r = t.size // 2
    a = np.zeros((size, size))
    for i in range(size):
        for u in range(t.size):
            g = abs(i + u - r)
            g = 2 * (size - 1) - g if g >= size else g
            a[i, g] += t[u]
    return a


def fold_matrix(taps, size: int, factor: int) -> np.ndarray:
    """One axis of the symmetric-fold filter-and-decimate map (``sr_filter.py``), dense fp64."""
    t = np.asarray(taps, dtype=np.float64)
    p = (t.size - factor) // 2
    a = np.zeros((size // factor, size))
    for i in range(size // factor):
        for u in range(t.size):
            g = factor * i + u - p
            g = -1 - g if g < 0 else g
            g = 2 * size - 1 - g if g >= size else g
            a[i, g] += t[u]
    return a


# --- the tables -----------------------------------------------------------------------------------
@dataclass
class Tables:
    VH: np.ndarray  # (H, H)
    VW: np.ndarray  # (W, W)
    UH: np.ndarray  # (Hy, Hy)
    UW: np.ndarray  # (Wy, Wy)
    S: np.ndarray   # (Hy, Wy)
    P: np.ndarray   # (Hy, Wy)

    @property
    def dims(self):
        return self.VH.shape[0], self.VW.shape[0], self.UH.shape[0], self.UW.shape[0]

    def parts(self):
        return [self.VH, self.VW, self.UH, self.UW, self.S, self.P]

    def flat32(self) -> torch.Tensor:
        """The descriptor's ``taps``: the six tables row-major, back to back, fp32."""
        return torch.from_numpy(np.concatenate([p.reshape(-1) for p in self.parts()]).astype(np.float32))

    def rounded(self) -> "Tables":
        """The fp32 tables promoted back to fp64: what the library's map is defined by."""
        return Tables(*[p.astype(np.float32).astype(np.float64) for p in self.parts()])

    def kept_share(self) -> float:
        return float((self.P != 0).mean())

    @staticmethod
    def from_factors(ah, aw, rtol: float) -> "Tables":
        ah, aw = np.asarray(ah, dtype=np.float64), np.asarray(aw, dtype=np.float64)
        uh, sh, vht = np.linalg.svd(ah, full_matrices=True)
        uw, sw, vwt = np.linalg.svd(aw, full_matrices=True)
        s = np.outer(sh, sw)
        keep = s > rtol * s.max()
        p = np.zeros_like(s)
        p[keep] = 1.0 / s[keep]
        return Tables(vht.T.copy(), vwt.T.copy(), uh, uw, s, p)

    @staticmethod
    def from_flat(flat: torch.Tensor, H: int, W: int, Hy: int, Wy: int) -> "Tables":
        f = flat.detach().cpu().double().numpy()
        out, off = [], 0
        for shape in ((H, H), (W, W), (Hy, Hy), (Wy, Wy), (Hy, Wy), (Hy, Wy)):
            size = shape[0] * shape[1]
            out.append(f[off:off + size].reshape(shape).copy())
            off += size
        assert off == f.size
        return Tables(*out)

    @staticmethod
    def exact(H: int, W: int, blocks_h, blocks_w, seed: int, svals=(1.0, 0.5), cut: float = 0.3) -> "Tables":
        """Square (Hy = H, Wy = W) exact tables: every orthogonal table a block-diagonal signed
        permutation of scaled Hadamard blocks, ``S = s_H ⊗ s_W`` with ``s`` drawn from ``svals``
        (both values present on each axis), ``P = 1/S`` where ``S > cut`` and 0 elsewhere."""
        rng = np.random.default_rng(seed)
        assert sum(blocks_h) == H and sum(blocks_w) == W
        sh, sw = (_two_valued(n, svals, rng) for n in (H, W))
        s = np.outer(sh, sw)
        p = np.zeros_like(s)
        p[s > cut] = 1.0 / s[s > cut]
        return Tables(hadamard_orthogonal(blocks_h, rng), hadamard_orthogonal(blocks_w, rng),
                      hadamard_orthogonal(blocks_h, rng), hadamard_orthogonal(blocks_w, rng), s, p)


def _two_valued(n, svals, rng):
    s = np.asarray(svals, dtype=np.float64)[rng.integers(0, len(svals), n)]
    s[0], s[-1] = svals[0], svals[-1]
    return s


def hadamard(order: int) -> np.ndarray:
    h = np.ones((1, 1))
    while h.shape[0] < order:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == order
    return h


def hadamard_orthogonal(blocks, rng) -> np.ndarray:
    """Block-diagonal of ``hadamard(o) / sqrt(o)`` (o a power of 4, so the scale is dyadic), rows and
    columns permuted, columns signed."""
    n = sum(blocks)
    m, off = np.zeros((n, n)), 0
    for o in blocks:
        root = int(round(o ** 0.5))
        assert root * root == o and o in (1, 4, 16, 64)
        m[off:off + o, off:off + o] = hadamard(o) / root
        off += o
    m = m[rng.permutation(n)][:, rng.permutation(n)] * rng.choice([-1.0, 1.0], n)
    assert np.array_equal(m.T @ m, np.eye(n))
    return m


# --- dense statement ------------------------------------------------------------------------------
class Dense:
    """The passes on flat fp64 planes (rows of H·W, observations rows of Hy·Wy)."""

    def __init__(self, t: Tables):
        H, W, Hy, Wy = t.dims
        V = kron_dense(t.VH, t.VW)
        sel = (np.arange(Hy)[:, None] * W + np.arange(Wy)[None, :]).reshape(-1)  # the observed grid
        self.V, self.Vo, self.U = V, V[:, sel], kron_dense(t.UH, t.UW)
        self.s, self.p = t.S.reshape(-1), t.P.reshape(-1)
        self.k = (self.p != 0).astype(np.float64)
        self.A = self.U @ np.diag(self.s) @ self.Vo.T
        self.Apinv = self.Vo @ np.diag(self.p) @ self.U.T
        self.Pi = self.Vo @ np.diag(self.k) @ self.Vo.T
        self.A_kept = self.U @ np.diag(self.s * self.k) @ self.Vo.T  # what A⁺ and DDRM see

    def prox(self, x0, y, rho):
        n = self.A.shape[1]
        return np.linalg.solve(self.A.T @ self.A + rho * np.eye(n), (y @ self.A + rho * x0).T).T


# --- the separable evaluation ------------------------------------------------------------------------
class Sep:
    """The kernels' evaluation on (..., H, W) planes in ``dtype``.  ``right_first``: the table on
    the right is applied before the one on the left; ``reverse``: every product sums its k index
    backwards.  ``wrong``: "transposed" (V_H used transposed), "swap_u" (U_H and U_W exchanged; needs
    Hy = Wy), "p_for_s" (P where S belongs), "shifted_keep" (P rolled by one column)."""

    def __init__(self, t: Tables, dtype=torch.float64, right_first=False, reverse=False, wrong=None):
        cv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        self.VH, self.VW, self.UH, self.UW, self.S, self.P = (cv(p) for p in t.parts())
        self.H, self.W, self.Hy, self.Wy = t.dims
        self.dtype, self.right_first, self.reverse = dtype, right_first, reverse
        if wrong == "transposed":
            self.VH = self.VH.t().contiguous()
        elif wrong == "swap_u":
            assert self.Hy == self.Wy
            self.UH, self.UW = self.UW, self.UH
        elif wrong == "p_for_s":
            self.S = self.P
        elif wrong == "shifted_keep":
            self.P = torch.roll(self.P, 1, dims=1)
        else:
            assert wrong is None, wrong

    def mm(self, a, b):
        return a.flip(-1) @ b.flip(-2) if self.reverse else a @ b

    def two(self, left, x, right):
        if self.right_first:
            return self.mm(left, self.mm(x, right))
        return self.mm(self.mm(left, x), right)

    # the transforms: T (rows, cols of the spectrum kept), its inverse from that block, T_y
    def T(self, x, full=False):
        r, c = (self.H, self.W) if full else (self.Hy, self.Wy)
        return self.two(self.VH[:, :r].t(), x, self.VW[:, :c])

    def Tinv(self, z, full=False):
        r, c = (self.H, self.W) if full else (self.Hy, self.Wy)
        return self.two(self.VH[:, :r], z, self.VW[:, :c].t())

    def Ty(self, y):
        return self.two(self.UH.t(), y, self.UW)

    def Tyinv(self, z):
        return self.two(self.UH, z, self.UW.t())

    # the maps
    def apply(self, x):
        return self.Tyinv(self.S * self.T(x))

    def adjoint(self, g):
        return self.Tinv(self.S * self.Ty(g))

    def pinv(self, y):
        return self.Tinv(self.P * self.Ty(y))

    def pinv_t(self, x):
        return self.Tyinv(self.P * self.T(x))

    def x0(self, x, eps, a, k):
        sc = lambda v: torch.tensor(v, dtype=self.dtype)  # noqa: E731
        return (x - sc(k) * eps) / sc(a)

    def q_pgdm(self, y):
        return self.P * self.Ty(y)

    def q_prox(self, y):
        return self.S * self.Ty(y)

    def dps(self, x, eps, y, a, k, gs):
        """(v, ‖r‖² per sample); ``y`` one row per sample."""
        r = self.Ty(y) - self.S * self.T(self.x0(x, eps, a, k))
        v = self.Tinv(torch.tensor(gs, dtype=self.dtype) * (self.S * r))
        return v, (r * r).reshape(r.shape[0], -1).sum(1)

    def pgdm(self, x, eps, y, a, k, gs):
        d = self.T(self.x0(x, eps, a, k))
        d = torch.where(self.P != 0, d, torch.zeros_like(d))
        return self.Tinv(torch.tensor(gs, dtype=self.dtype) * (self.q_pgdm(y) - d))

    def prox(self, x0, y, rho):
        rho = torch.tensor(rho, dtype=self.dtype)
        t = self.T(x0, full=True).clone()
        obs = (self.q_prox(y) + rho * t[..., :self.Hy, :self.Wy]) / (self.S * self.S + rho)
        t[..., :self.Hy, :self.Wy] = obs
        return self.Tinv(t, full=True)

    def diffpir(self, x, eps, y, xi, c):
        """``c``: dict a, k, rho, a_prev, c_eps, c_xi."""
        sc = {key: torch.tensor(v, dtype=self.dtype) for key, v in c.items()}
        z = self.prox(self.x0(x, eps, c["a"], c["k"]), y, c["rho"])
        eh = (x - sc["a"] * z) * (1 / sc["k"])
        return sc["a_prev"] * z + (sc["c_eps"] * eh + sc["c_xi"] * xi)

    def ddrm(self, x, eps, y, xi, c):
        """``c``: the dict of ``ddrm_ref.make_coefs``.  The class mask is ddrm_ref's: the pinned fp32
        expression on fp32 data, the fp64 decision otherwise."""
        s2 = torch.zeros(self.H, self.W, dtype=self.dtype)
        s2[:self.Hy, :self.Wy] = self.S * self.S
        observed = torch.zeros(self.H, self.W, dtype=torch.bool)
        observed[:self.Hy, :self.Wy] = self.P != 0
        big = dr.big_mask32(s2, c) if self.dtype == torch.float32 else dr.big_mask64(s2, c)
        f_th, f_ep, f_y, f_xi = dr.coefficients(s2, observed, big, c, self.dtype)
        q = torch.zeros(*x.shape[:-2], self.H, self.W, dtype=self.dtype)
        q[..., :self.Hy, :self.Wy] = self.q_pgdm(y)
        x0 = self.x0(x, eps, c["a"], c["k"])
        T = lambda v: self.T(v, full=True)  # noqa: E731
        spec = ((f_y * q + f_th * T(x0)) + f_ep * T(eps)) + f_xi * T(xi)
        return torch.tensor(c["a_prev"], dtype=self.dtype) * self.Tinv(spec, full=True)


# --- exact scalars and data ------------------------------------------------------------------------------
# DDRM: ddrm_ref.exact_coefs(regime, 1) on S in {1, 1/2, 1/4}: "big" has S = 1 big (f_xi = 1/2,
# f_th = 1/4, f_y = 3/4) and the others small (r = 15/32 S / (1/2)); "small" has every S small
# (r = 3 S / 8).  DPS / PGDM: a = k = 1/2, grad_scale = 2 and -2.  Prox / DiffPIR: S in {1, 0} and
# rho = 1, so S² + rho is 2 or 1; a = k = a_prev = 1/2, c_eps = 1/4, c_xi = 1/2 (with c_eps = 1/2 the
# step would return x whatever z is).
EXACT_DPS = dict(a=0.5, k=0.5, gs=2.0)
EXACT_PROX = dict(a=0.5, k=0.5, rho=1.0, a_prev=0.5, c_eps=0.25, c_xi=0.5)


def exact_data(i: int):
    """Integer-valued fp32 x, eps, xi, cot (4, C, H, W) and y (2, C, Hy, Wy) of exact case i, in
    [-amp, amp]; a batch form (batch, y_div) uses the first `batch` samples and ceil(batch / y_div)
    rows (``exact_form``)."""
    _, C, H, W, _, _, amp = EXACT_CASES[i]
    g = torch.Generator().manual_seed(7 + i)
    x, eps, xi, cot = (torch.randint(-amp, amp + 1, (4, C, H, W), generator=g).float() for _ in range(4))
    y = torch.randint(-amp, amp + 1, (2, C, H, W), generator=g).float()
    return x, eps, xi, cot, y


def exact_form(i: int, batch: int, y_div: int):
    """(x, eps, xi, y rows, y of every sample) of exact case i in one batch form."""
    x, eps, xi, _, y = exact_data(i)
    rows = -(-batch // y_div)
    return x[:batch], eps[:batch], xi[:batch], y[:rows], y[torch.arange(batch) // y_div]


# --- the cases shared by the CPU and GPU tests ----------------------------------------------------------
def _gauss(k, sigma):
    i = np.arange(k, dtype=np.float64) - k // 2
    t = np.exp(-(i ** 2) / (2.0 * sigma ** 2))
    return (t / t.sum()).astype(np.float32).astype(np.float64)  # the fp32 taps of gaussian_taps


def _bicubic(s):
    t = np.abs((2 * np.arange(4 * s, dtype=np.float64) + 1 - 4 * s) / (2 * s))
    a = -0.5
    k = np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1,
                 np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0)) / s
    return (k / k.sum()).astype(np.float32).astype(np.float64)


def _blur(taps, H, W):
    return lambda: (reflect_matrix(taps, H), reflect_matrix(taps, W))


def _zero_sv():
    a = reflect_matrix(_gauss(3, 0.8), 12)
    a[5] = a[4]  # a duplicated row: one singular value is exactly (to rounding) zero
    return a, reflect_matrix(_gauss(3, 0.8), 10)


# name, channels, (A_h, A_w) factory, rtol, the kept share's range
FACTOR_CASES = [
    ("1x3x5", 1, _blur(_gauss(3, 0.8), 3, 5), 3e-2, (0.1, 0.9)),              # below one MFMA tile
    ("3x33x35-g9", 3, _blur(_gauss(9, 3.0), 33, 35), 3e-2, (0.1, 0.9)),
    ("1x64x48-g9", 1, _blur(_gauss(9, 3.0), 64, 48), 3e-2, (0.1, 0.9)),
    ("1x40x36-g3", 1, _blur(_gauss(3, 0.8), 40, 36), 3e-2, (0.1, 0.9)),
    ("1x129x130-g9", 1, _blur(_gauss(9, 3.0), 129, 130), 3e-2, (0.1, 0.9)),    # k-loop, every seam ragged
    ("2x32x32-sr4", 2, lambda: (fold_matrix(_bicubic(4), 32, 4),) * 2, 0.7, (0.1, 0.9)),
    ("1x24x16-sr2x4", 1, lambda: (fold_matrix(_bicubic(2), 24, 2), fold_matrix(_bicubic(4), 16, 4)), 0.7,
     (0.1, 0.9)),
    ("2x32x32-sr4-all", 2, lambda: (fold_matrix(_bicubic(4), 32, 4),) * 2, 3e-2, (1.0, 1.0)),  # all kept
    ("1x12x10-zero", 1, _zero_sv, 3e-2, (0.1, 0.95)),                          # an exactly zero s
    ("3x256x256-g9", 3, _blur(_gauss(9, 3.0), 256, 256), 3e-2, (0.1, 0.9)),    # the workload's size
]

# name, channels, H, W, blocks_h, blocks_w, integer amplitude
EXACT_CASES = [
    ("2x16x16", 2, 16, 16, [16], [16], 4),
    ("1x64x64", 1, 64, 64, [64], [64], 2),
    ("1x20x33", 1, 20, 33, [16, 4], [16, 16, 1], 4),  # ragged: blocks 16+4 and 16+16+1
]
BATCH_FORMS = [(3, 3), (4, 2)]  # (batch, y_div)


def exact_tables(i: int, prox: bool = False) -> Tables:
    _, _, H, W, bh, bw, _ = EXACT_CASES[i]
    return Tables.exact(H, W, bh, bw, seed=100 + i, svals=(1.0, 0.0) if prox else (1.0, 0.5), cut=0.3)
