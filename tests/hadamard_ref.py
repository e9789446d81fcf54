"""fp64 semantics of the Walsh–Hadamard compressed-sensing kind (SP_OP_HADAMARD) — TEST
INFRASTRUCTURE ONLY.  Uses no operator code.

Per channel plane, with ``n_p = H·W = 2^k``:  ``(A x)[r] = n_p^(−1/2) Σ_i (−1)^popcount(j_r & i) d[i] x[i]``,
``j_r`` the r-th kept coefficient in ascending natural (Sylvester) order, ``d`` a ±1 vector.  Every
pass is stated twice:

* ``Had(..., dense=True)`` — on the dense Sylvester matrix built by index arithmetic
  (``sylvester``, planes of at most 4096), the prox as a dense solve, the DDRM step through
  ``ddrm_ref.dense_step`` (``eigh`` of AᵀA);
* ``Had(...)`` — as a butterfly recursion (``fwht``), in any dtype, the DDRM step in the projector
  form ``a'·[base + Aᵀ(f_y y + A w)]``.

``emulate`` is the kernels' own algorithm in numpy float32 (every operation rounds on its own):
source formed at load, d, the levels in either order (low-then-high, high-then-low),
``n_p^(−1/2)`` once per transform, the mask / gather / mid step, the levels again, d, the scale and
the pass's base.  ``wrong`` makes one of five mistakes on purpose, which the exact cases must tell
apart.

The bound of the ``randn`` cases is per element ``|err| ≤ n_r · 2⁻²⁴ · E``: ``E`` the same pass on
absolute values with absolute coefficients (``Had.envelope``; |H| is the all-ones matrix, so an
absolute transform is one sum), ``n_r`` the roundings on the longest path of the algorithm as
``emulate`` writes it (``roundings``): ``k + 2`` per transform (k levels, d, the scale) plus the
elementwise steps counted there.
"""

from __future__ import annotations

import math

import numpy as np
import torch

import ddrm_ref as dr

U24 = 2.0 ** -24


# --- the two statements of the transform ---------------------------------------------------------------
def sylvester(n: int) -> np.ndarray:
    """``H[i, j] = (−1)^popcount(i & j)`` by index arithmetic, fp64, unnormalised."""
    i = np.arange(n)
    a = i[:, None] & i[None, :]
    pop = np.zeros_like(a)
    while a.any():
        pop += a & 1
        a >>= 1
    return np.where(pop & 1, -1.0, 1.0)


def fwht(v, descending: bool = False):
    """Unnormalised transform of the last axis by butterflies, in v's dtype (numpy or torch); the
    levels ascending (h = 1, 2, ...: low then high) or descending."""
    n = v.shape[-1]
    lead = tuple(v.shape[:-1])
    hs = [1 << b for b in range(n.bit_length() - 1)]
    for h in (reversed(hs) if descending else hs):
        w = v.reshape(*lead, n // (2 * h), 2, h)
        a, b = w[..., 0, :], w[..., 1, :]
        if isinstance(v, np.ndarray):
            v = np.stack((a + b, a - b), axis=-2).reshape(*lead, n)
        else:
            v = torch.stack((a + b, a - b), dim=-2).reshape(*lead, n)
    return v


def scale_of(k: int, dtype=torch.float64) -> float:
    """``2^(−k/2)``: a power of two for even k, rounded to fp32 for the fp32 evaluations of odd k."""
    s = 2.0 ** (-k / 2.0)
    return float(np.float32(s)) if dtype in (torch.float32, np.float32) else s


def sequency_permutation(n: int) -> np.ndarray:
    """perm[s] = the natural-order index of the sequency-ordered row s (Gray code, bits reversed)."""
    k = n.bit_length() - 1
    s = np.arange(n)
    g = s ^ (s >> 1)
    out = np.zeros(n, dtype=np.int64)
    for b in range(k):
        out |= ((g >> b) & 1) << (k - 1 - b)
    return out


# --- the operator and its passes -----------------------------------------------------------------------
class Had:
    """(..., C, H, W) <-> (..., C, m_p) in ``dtype``; ``keep`` a bool vector over n_p, ``d`` ±1 or None."""

    def __init__(self, shape, keep, d=None, dtype=torch.float64, dense: bool = False):
        self.C, self.H, self.W = shape
        self.np_ = self.H * self.W
        self.k = self.np_.bit_length() - 1
        assert 1 << self.k == self.np_
        self.keep = torch.as_tensor(np.asarray(keep, dtype=bool))
        self.idx = torch.nonzero(self.keep).squeeze(1)
        self.mp = int(self.idx.numel())
        self.dtype = dtype
        self.d = None if d is None else torch.as_tensor(np.asarray(d, dtype=np.float64)).to(dtype)
        self.scale = torch.tensor(scale_of(self.k, dtype), dtype=dtype)
        self.dense = dense
        if dense:
            assert self.np_ <= 4096
            h = torch.from_numpy(sylvester(self.np_)) * (2.0 ** (-self.k / 2.0))
            a = h[self.idx]
            if self.d is not None:
                a = a * self.d.double()[None, :]
            self.A = a.to(dtype)  # (m_p, n_p)

    def t(self, v):
        return torch.tensor(v, dtype=self.dtype)

    def apply(self, x):
        v = x.to(self.dtype).reshape(*x.shape[:-2], self.np_)
        if self.dense:
            return v @ self.A.T
        if self.d is not None:
            v = v * self.d
        return (self.scale * fwht(v))[..., self.idx]

    def adjoint(self, y):
        y = y.to(self.dtype)
        if self.dense:
            return (y @ self.A).reshape(*y.shape[:-1], self.H, self.W)
        full = torch.zeros(*y.shape[:-1], self.np_, dtype=self.dtype)
        full[..., self.idx] = y
        v = self.scale * fwht(full)
        if self.d is not None:
            v = v * self.d
        return v.reshape(*y.shape[:-1], self.H, self.W)

    pinv = adjoint      # A⁺ = Aᵀ
    pinv_t = apply      # A⁺ᵀ = A

    def x0(self, x, eps, a, k):
        return (x.to(self.dtype) - self.t(k) * eps.to(self.dtype)) / self.t(a)

    def dps(self, x, eps, y, a, k, gs):
        """v = gs·Aᵀ(y − A x0) and ‖y − A x0‖² per sample."""
        r = y.to(self.dtype) - self.apply(self.x0(x, eps, a, k))
        return self.adjoint(self.t(gs) * r), (r * r).reshape(r.shape[0], -1).sum(1)

    def pgdm(self, x, eps, y, a, k, gs):
        """v = gs·(A⁺y − A⁺A x0) = gs·Aᵀ(y − A x0); the sampler passes gs = −2·(its weight)."""
        return self.dps(x, eps, y, a, k, gs)[0]

    def prox(self, x0, y, rho):
        x0 = x0.to(self.dtype)
        if self.dense:  # the normal equations, solved: (AᵀA + ρI) z = Aᵀy + ρ x0
            m = self.A.T @ self.A + rho * torch.eye(self.np_, dtype=self.dtype)
            rhs = self.adjoint(y) + rho * x0
            z = torch.linalg.solve(m, rhs.reshape(-1, self.np_).T).T
            return z.reshape(x0.shape)
        g = self.t(1.0) / (self.t(1.0) + self.t(rho))
        return x0 + self.adjoint(g * (y.to(self.dtype) - self.apply(x0)))

    def diffpir(self, x, eps, y, xi, c):
        x = x.to(self.dtype)
        z = self.prox(self.x0(x, eps, c["a"], c["k"]), y, c["rho"])
        eh = (x - self.t(c["a"]) * z) * (self.t(1.0) / self.t(c["k"]))
        return self.t(c["a_prev"]) * z + (self.t(c["c_eps"]) * eh + self.t(c["c_xi"]) * xi.to(self.dtype))

    def ddrm(self, x, eps, y, xi, c):
        """Dense: the definition (``eigh``); else the projector form with the class coefficients of
        s² = 1 (the fp32 class decision in fp32)."""
        if self.dense:
            assert self.C == 1
            flat = lambda v: v.double().reshape(v.shape[0], -1)  # noqa: E731
            return dr.dense_step(self.A.double(), flat(x), flat(eps), flat(y), flat(xi), c).reshape(x.shape)
        dt = self.dtype
        one = torch.ones((), dtype=dt)
        big = dr.big_mask32(torch.ones((), dtype=torch.float32), c) if dt == torch.float32 else dr.big_mask64(one, c)
        fo = dr.coefficients(one, torch.tensor(True), big, c, dt)
        fu = dr.coefficients(one, torch.tensor(False), torch.tensor(False), c, dt)
        x, eps, xi = x.to(dt), eps.to(dt), xi.to(dt)
        x0 = self.x0(x, eps, c["a"], c["k"])
        w = ((fo[0] - fu[0]) * x0 + (fo[1] - fu[1]) * eps) + (fo[3] - fu[3]) * xi
        base = x0 + (fu[1] * eps + fu[3] * xi)
        return self.t(c["a_prev"]) * (base + self.adjoint(fo[2] * y.to(dt) + self.apply(w)))

    # ---- the same passes on absolute values with absolute coefficients ----
    def _abs_apply(self, x):
        s = x.abs().reshape(*x.shape[:-2], self.np_).sum(-1, keepdim=True) * abs(float(self.scale))
        return s.expand(*s.shape[:-1], self.mp)

    def _abs_adjoint(self, y):
        s = y.abs().sum(-1, keepdim=True) * abs(float(self.scale))
        return s.expand(*s.shape[:-1], self.np_).reshape(*y.shape[:-1], self.H, self.W)

    def envelope(self, what, x=None, eps=None, y=None, xi=None, c=None):
        """E of pass ``what`` (fp64)."""
        ab = lambda v: None if v is None else v.double().abs()  # noqa: E731
        x, eps, y, xi = ab(x), ab(eps), ab(y), ab(xi)
        if what == "apply":
            return self._abs_apply(x)
        if what == "adjoint":
            return self._abs_adjoint(y)
        x0 = x if eps is None else (x + abs(c["k"]) * eps) / abs(c["a"])
        if what in ("dps", "pgdm"):
            return self._abs_adjoint(abs(c["gs"]) * (y + self._abs_apply(x0)))
        if what == "rsq":
            r = y + self._abs_apply(x0)
            return (r * r).reshape(r.shape[0], -1).sum(1)
        if what in ("prox", "diffpir"):
            g = 1.0 / (1.0 + c["rho"])
            z = x0 + self._abs_adjoint(g * (y + self._abs_apply(x0)))
            if what == "prox":
                return z
            eh = (x + abs(c["a"]) * z) / abs(c["k"])
            return abs(c["a_prev"]) * z + (abs(c["c_eps"]) * eh + abs(c["c_xi"]) * xi)
        assert what == "ddrm", what
        one = torch.ones((), dtype=torch.float64)
        fo = dr.coefficients(one, torch.tensor(True), dr.big_mask64(one, c), c)
        fu = dr.coefficients(one, torch.tensor(False), torch.tensor(False), c)
        w = (abs(fo[0] - fu[0]) * x0 + abs(fo[1] - fu[1]) * eps) + abs(fo[3] - fu[3]) * xi
        base = x0 + (abs(fu[1]) * eps + abs(fu[3]) * xi)
        return abs(c["a_prev"]) * (base + self._abs_adjoint(abs(fo[2]) * y + self._abs_apply(w)))


def roundings(what: str, k: int, m: int = 1) -> int:
    """n_r: the roundings on the longest path of ``emulate``'s algorithm, counted as written there.
    A transform t = k + 2: k levels, the product by d, the scale.  x0 = (x − k·eps)/a: 3.
      dps, pgdm  x0 (3); A (t); y − c, gs·r (2); Aᵀ (t)
      prox       A (t); y − c (1); 1 + ρ, 1/·, g·r (3); Aᵀ (t); x0 + v (1)
      diffpir    x0 (3); prox (2t + 5); a·z, x − ·, 1/k, ·inv_k, c_eps·, + c_xi ξ, a_prev z + · (7)
      ddrm       x0 (3); a class coefficient (r = ((c₁σ')·√s²)/σ_y, 1 − r: 5) and its difference to
                 the unobserved one (1), its product and the two sums of w (3); A (t); + f_y·y (1);
                 Aᵀ (t); base + v, a'· (2)
      rsq        relative: k + log₂ m + 4"""
    t = k + 2
    return {"apply": t, "adjoint": t, "dps": 2 * t + 5, "pgdm": 2 * t + 5, "prox": 2 * t + 5,
            "diffpir": 2 * t + 15, "ddrm": 2 * t + 15,
            "rsq": k + int(math.ceil(math.log2(max(m, 2)))) + 4}[what]


# --- the kernels' algorithm in numpy float32 ---------------------------------------------------------
F = np.float32


def _bits_and_ranks(keep: np.ndarray, wrong=None):
    """(kept mask, rank of every coefficient) as the kernel reads them from keep_bits / word_rank."""
    keep = np.asarray(keep, dtype=bool)
    n = keep.size
    words = keep.reshape(n // 64, 64)
    word_rank = np.concatenate([[0], np.cumsum(words.sum(1))[:-1]])
    seen = keep.copy()
    if wrong == "word_boundary":  # the upper half of every 64-bit word read from the lower half
        w = words.copy()
        w[:, 32:] = w[:, :32]
        seen = w.reshape(-1)
        words = w
    within = np.cumsum(words, axis=1) - words  # kept bits below, inside the word
    rank = (word_rank[:, None] + within).reshape(-1)
    if wrong == "rank_shift":
        rank = rank + 1
    return seen, rank


def emulate(what, shape, keep, d, *, x=None, eps=None, y=None, xi=None, c=None, descending=False, wrong=None):
    """Pass ``what`` ("apply", "adjoint", "dps", "pgdm", "prox", "diffpir", "ddrm") in numpy float32 as
    the kernels run it; y has one row per sample.  Returns float32 arrays (dps: (v, rsq))."""
    C, H, W = shape
    n_p = H * W
    k = n_p.bit_length() - 1
    scale = F(scale_of(k, np.float32))
    mp = int(np.asarray(keep).sum())
    seen, rank = _bits_and_ranks(keep, wrong)
    rank = np.minimum(rank, mp - 1)
    dd = np.ones(n_p, dtype=F) if (d is None or wrong == "no_signs") else np.asarray(d, dtype=F)
    perm = sequency_permutation(n_p) if wrong == "sequency" else None
    f32 = lambda v: None if v is None else np.asarray(v, dtype=F)  # noqa: E731
    x, eps, y, xi = f32(x), f32(eps), f32(y), f32(xi)

    def forward(w):  # (B, C, H, W) -> coefficients (B, C, n_p), scaled
        t = fwht(dd * w.reshape(*w.shape[:-2], n_p), descending)
        t = scale * t
        return t[..., perm] if perm is not None else t

    def backward(u, scaled=True):  # (B, C, n_p) -> (B, C, H, W)
        if perm is not None:
            full = np.zeros_like(u)
            full[..., perm] = u
            u = full
        t = fwht(u, descending)
        t = dd * (scale * t) if (scaled and wrong != "one_scale") else dd * t
        return t.reshape(*u.shape[:-1], H, W)

    def gather(yrows):  # y at every coefficient's rank, 0 off the kept set
        return np.where(seen, yrows[..., rank], F(0))

    if what == "apply":
        cf = forward(x)
        out = np.zeros((*cf.shape[:-1], mp), dtype=F)
        out[..., rank[seen]] = cf[..., seen]
        return out
    if what == "adjoint":
        return backward(gather(y))
    a, kk = (F(c["a"]), F(c["k"])) if eps is not None else (None, None)
    x0 = x if eps is None else (x - kk * eps) / a
    if what in ("dps", "pgdm", "prox", "diffpir"):
        g = F(c["gs"]) if what in ("dps", "pgdm") else F(1) / (F(1) + F(c["rho"]))
        r = np.where(seen, gather(y) - forward(x0), F(0))
        v = backward(g * r)
        if what == "dps":
            return v, (r.astype(np.float64) ** 2).reshape(r.shape[0], -1).sum(1)
        if what == "pgdm":
            return v
        z = x0 + v
        if what == "prox":
            return z
        eh = (x - F(c["a"]) * z) * (F(1) / kk)
        return F(c["a_prev"]) * z + (F(c["c_eps"]) * eh + F(c["c_xi"]) * xi)
    assert what == "ddrm", what
    one = torch.ones((), dtype=torch.float32)
    fo = [F(v) for v in dr.coefficients(one, torch.tensor(True), dr.big_mask32(one, c), c, torch.float32)]
    fu = [F(v) for v in dr.coefficients(one, torch.tensor(False), torch.tensor(False), c, torch.float32)]
    w = ((fo[0] - fu[0]) * x0 + (fo[1] - fu[1]) * eps) + (fo[3] - fu[3]) * xi
    u = np.where(seen, fo[2] * gather(y) + forward(w), F(0))
    base = x0 + (fu[1] * eps + fu[3] * xi)
    return F(c["a_prev"]) * (base + backward(u))


WRONG = ("no_signs", "rank_shift", "word_boundary", "sequency", "one_scale")


# --- the cases -----------------------------------------------------------------------------------------------
def random_keep(n_p: int, ratio: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    keep = np.zeros(n_p, dtype=bool)
    keep[rng.permutation(n_p)[: max(1, int(round(ratio * n_p)))]] = True
    return keep


def word_keep(n_p: int) -> np.ndarray:
    """Whole 64-bit words filled next to empty ones: words 0, 2, 3 of every four."""
    w = np.arange(n_p // 64) % 4
    return np.repeat((w == 0) | (w >= 2), 64)


def signs_of(n_p: int, seed: int) -> np.ndarray:
    return np.where(np.random.default_rng(1000 + seed).integers(0, 2, n_p) == 1, 1.0, -1.0).astype(np.float32)


# (name, (C, H, W), kept set, signs): L = 2^12 floats is the low stage's chunk
CASES = [
    ("1x8x8-r50", (1, 8, 8), lambda n: random_keep(n, 0.5, 1), True),          # k = 6: one keep_bits word
    ("3x8x16-r25", (3, 8, 16), lambda n: random_keep(n, 0.25, 2), True),       # k = 7: irrational scale
    ("1x16x64-words", (1, 16, 64), word_keep, True),                            # H != W; whole words
    ("1x64x64-r10", (1, 64, 64), lambda n: random_keep(n, 0.1, 4), True),      # = L
    ("2x64x128-r25", (2, 64, 128), lambda n: random_keep(n, 0.25, 5), True),   # 2 L, odd k
    ("3x128x128-all", (3, 128, 128), lambda n: np.ones(n, dtype=bool), True),   # every coefficient kept
    ("3x256x256-r25", (3, 256, 256), lambda n: random_keep(n, 0.25, 7), True),  # the workload's plane
    ("1x1024x1024-r10", (1, 1024, 1024), lambda n: random_keep(n, 0.1, 8), True),  # the largest: batch 1
    ("1x512x512-one", (1, 512, 512), lambda n: np.arange(n) == 77777, False),   # one coefficient; taps NULL
]
BATCH_FORMS = [(3, 3), (4, 2)]  # (batch, y_div); the 2^20 plane runs (1, 1)
_CASE = {}


def case(i: int):
    """(name, shape, keep, d or None), computed once."""
    if i not in _CASE:
        name, shape, make, signs = CASES[i]
        n_p = shape[1] * shape[2]
        _CASE[i] = (name, shape, make(n_p), signs_of(n_p, i) if signs else None)
    return _CASE[i]


def forms_of(i: int):
    return [(1, 1)] if CASES[i][1][1] * CASES[i][1][2] == 1 << 20 else BATCH_FORMS


def kept_share(i: int) -> float:
    _, shape, keep, _ = case(i)
    return float(keep.mean())


EXACT = [i for i, c in enumerate(CASES) if (c[1][1] * c[1][2]).bit_length() % 2 == 1]  # even k
# dyadic scalars: a = k = 1 (x0 = x − eps), gs = 2, ρ = 1 (1 + ρ = 2); DiffPIR a_prev = c_xi = 1/2,
# c_eps = 1; DDRM σ' = 1, σ_y = 0, η = 0 (c₁ = 1), η_b = 1: f_θ = 0, f_y = 1, f_ξ = σ' = 1 on the kept
# set, so w = −x0 − eps + xi and base = x0 + eps have unit coefficients, a' = 1/2.
EXACT_DPS = dict(a=1.0, k=1.0, gs=2.0)
EXACT_PROX = dict(a=1.0, k=1.0, rho=1.0, a_prev=0.5, c_eps=1.0, c_xi=0.5)
EXACT_DDRM = dr.make_coefs(1.0, 0.0, 0.0, 1.0, a=1.0, k=1.0, a_prev=0.5, c1=1.0)
# The round trip Aᵀ(g y + A w) on integers needs about k + 4 significand bits plus those of g and of
# the elementwise tail: the second transform sums up to 2^k multiples of 2^(−k/2) of size about
# 2^(k/2 + 2).  With unit and power-of-two coefficients that stays inside fp32's 24 up to k = 20:
# tests/test_hadamard_ref.py proves it for every pass on every even-k case (fp32 == fp64, both orders).
EXACT_PASSES = ("apply", "adjoint", "dps", "pgdm", "prox", "diffpir", "ddrm")


def exact_data(i: int, batch: int, y_div: int):
    """Integer-valued fp32 (x, eps, xi) of (batch, C, H, W) in [−3, 3] and y rows (C, m_p) likewise."""
    _, (C, H, W), keep, _ = case(i)
    g = torch.Generator().manual_seed(500 + i)
    x, eps, xi = (torch.randint(-3, 4, (batch, C, H, W), generator=g).float() for _ in range(3))
    y = torch.randint(-3, 4, (-(-batch // y_div), C, int(keep.sum())), generator=g).float()
    return x, eps, xi, y


def expand(y, batch: int, y_div: int):
    return y[torch.arange(batch) // y_div]
