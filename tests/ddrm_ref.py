"""fp64 semantics of the DDRM step and loop — TEST INFRASTRUCTURE ONLY.

The reference has no such sampler.  What ``sp_ddrm_step_ws``, ``ddrm_step_svd`` and ``DDRMSampler``
implement (Kawar et al. 2022, eq. 7-8 in the VP variables) is pinned here:

* ``coefficients`` — (f_θ, f_ε, f_y, f_ξ) of a spectral component from s², the observed mask and
  the class mask, in the dtype asked for; ``big_mask64`` is the fp64 decision σ'²s² ≥ σ_y²,
  ``big_mask32`` the pinned fp32 expression ``(sig_prev*sig_prev) * s2 >= sig_y*sig_y`` in numpy
  float32 (every operation rounds on its own; no division, no square root);
* ``dense_step`` — the definition: AᵀA = VΛVᵀ by ``eigh``, s = √Λ, the y term V·(f_y/Λ)·Vᵀ·Aᵀy;
* ``projector_step`` — A Aᵀ = g·I (identity, inpainting, mask: g = 1; ×s average pooling:
  g = 1/s²), Π = AᵀA/g; ``mask_ops`` / ``sr_ops`` give (Π, Aᵀy/g);
* ``dft_step`` — the periodic blur: s = |M| on the kept frequencies, unobserved elsewhere;
* ``emu_elementwise`` / ``emu_sr`` — the kernels' own order of operations in fp32 (torch on the
  CPU rounds every operation on its own); ``dft_step`` on fp32 inputs is the periodic emulation
  (``torch.fft`` in complex64).  ``variant`` makes a wrong answer on purpose: "swap" exchanges the
  two observed classes, "keep_eps" drops the −c₁σ'ε on the observed set, "xi_plain" does not
  project ξ;
* ``ddrm_coefs`` / ``ddrm_reference`` — the scalars of a step and the loop, in the schedule's dtype;
* ``exact_coefs`` / ``exact_inputs`` — dyadic scalars and integer data on which no fp32 evaluation
  of a one-launch step can round.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("a", "k", "a_prev", "sig_prev", "sig_y", "eta", "eta_b", "c1")
SIG_PREVS = (3.0, 0.23, 0.041, 0.5, 0.0)
SIG_YS = (0.05, 0.0)
ETAS = ((0.85, 1.0), (0.0, 1.0), (1.0, 0.5), (0.5, 0.0))


def make_coefs(sig_prev, sig_y, eta, eta_b, a=0.8, k=0.6, a_prev=0.9, c1=None):
    """The eight scalars as a dict of Python floats; c1 = sqrt(1 - eta^2) in fp64 unless given."""
    c1 = float((1.0 - float(eta) ** 2) ** 0.5) if c1 is None else c1
    return dict(a=a, k=k, a_prev=a_prev, sig_prev=sig_prev, sig_y=sig_y, eta=eta, eta_b=eta_b, c1=c1)


def round32(c):
    """The scalars rounded to fp32 (what the kernels are given), as Python floats."""
    return {key: float(np.float32(c[key])) for key in KEYS}


# --- the class decision and the coefficients ----------------------------------------------------
def big_mask64(s2: torch.Tensor, c) -> torch.Tensor:
    return (c["sig_prev"] ** 2) * s2.double() >= c["sig_y"] ** 2


def big_mask32(s2, c) -> torch.Tensor:
    """The pinned expression on fp32 numbers, in numpy float32."""
    s2 = np.asarray(s2.detach().cpu().numpy() if isinstance(s2, torch.Tensor) else s2)
    assert s2.dtype == np.float32, s2.dtype
    sp, sy = np.float32(c["sig_prev"]), np.float32(c["sig_y"])
    return torch.from_numpy(np.asarray(np.float32(sp * sp) * s2 >= np.float32(sy * sy)))


def s2_of_spectrum32(m: torch.Tensor) -> torch.Tensor:
    """re*re + im*im of a complex64 spectrum in numpy float32, each operation rounded."""
    m = m.detach().cpu().numpy().astype(np.complex64)
    re, im = m.real.astype(np.float32), m.imag.astype(np.float32)
    return torch.from_numpy(np.float32(re * re) + np.float32(im * im))


def coefficients(s2: torch.Tensor, observed: torch.Tensor, big: torch.Tensor, c, dtype=torch.float64,
                 variant: str | None = None):
    """(f_th, f_ep, f_y, f_xi), each of s2's shape in ``dtype``; every operation in that dtype."""
    t = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    sp, sy, eta, eb, c1 = (t(c[key]) for key in ("sig_prev", "sig_y", "eta", "eta_b", "c1"))
    s2 = s2.to(dtype)
    observed = observed & (s2 > 0)
    big = observed & big
    small = observed & ~big
    if variant == "swap":  # sig_y > 0 where the wrong answers are asked for
        big, small = small, big
    one, zero = torch.ones_like(s2), torch.zeros_like(s2)
    es = eta * sp
    r = torch.where(small, ((c1 * sp) * torch.sqrt(s2)) / torch.where(small, sy * one, one), zero)
    e = eb * sy
    v = sp * sp - (e * e) / torch.where(observed, s2, one)
    f_th = torch.where(big, (1 - eb) * one, 1 - r)
    f_y = torch.where(big, eb * one, r)
    f_ep = torch.where(observed, zero, (c1 * sp) * one)
    f_xi = torch.where(big, torch.sqrt(torch.clamp(v, min=0)), es * one)
    return f_th, f_ep, f_y, f_xi


def predict_x0(x, eps, c):
    return (x - c["k"] * eps) / c["a"]


# --- the definition -------------------------------------------------------------------------------
def dense_matrix(apply, x_shape: tuple) -> torch.Tensor:
    """A as an (m, n) float64 matrix: column j is ``apply`` of the j-th unit vector."""
    n = int(np.prod(x_shape))
    eye = torch.eye(n, dtype=torch.float64).reshape(n, *x_shape)
    return apply(eye).reshape(n, -1).T.contiguous()


def dense_step(A: torch.Tensor, x, eps, y, xi, c, rtol: float = 1e-12) -> torch.Tensor:
    """Flat fp64 rows x, eps, xi (B, n), y (B, m).  Eigenvalues below rtol·max are zero."""
    lam, V = torch.linalg.eigh(A.T @ A)
    lam = torch.clamp(lam, min=0)
    observed = lam > rtol * lam.max()
    f_th, f_ep, f_y, f_xi = coefficients(lam, observed, big_mask64(lam, c), c)
    x0 = predict_x0(x.double(), eps.double(), c)
    yt = (y.double() @ A) @ V  # V^T A^T y
    ybar = torch.where(observed, yt / torch.where(observed, lam, torch.ones_like(lam)), torch.zeros_like(lam))
    spec = f_th * (x0 @ V) + f_ep * (eps.double() @ V) + f_y * ybar + f_xi * (xi.double() @ V)
    return c["a_prev"] * (spec @ V.T)


# --- A A^T = g I ------------------------------------------------------------------------------------
def mask_ops(keep: torch.Tensor, packed: bool = True):
    """(Π, y ↦ Aᵀy/g) for the keep mask (n,), True where observed, on flat rows; g = 1."""
    keep = keep.reshape(-1).bool()

    def up(y):
        if not packed:
            return torch.where(keep, y, torch.zeros_like(y))
        out = torch.zeros(y.shape[0], keep.numel(), dtype=y.dtype)
        out[:, keep] = y
        return out
    return (lambda v: torch.where(keep, v, torch.zeros_like(v))), up


def sr_ops(shape: tuple, s: int):
    """(Π, y ↦ Aᵀy/g) for ×s average pooling of (C, H, W) planes on flat rows; g = 1/s²."""
    ys = (shape[0], shape[1] // s, shape[2] // s)
    rep = lambda t: t.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)  # noqa: E731
    proj = lambda v: rep(F.avg_pool2d(v.reshape(-1, *shape), s)).reshape(v.shape)  # noqa: E731
    return proj, (lambda y: rep(y.reshape(-1, *ys)).reshape(y.shape[0], -1))


def projector_step(x, eps, y_up, xi, c, g: float, proj, big=None, variant: str | None = None,
                   x0=None):
    """The projector form in x's dtype.  ``y_up`` is Aᵀy/g, one row per sample; ``x0`` given: used
    instead of ``predict_x0(x, eps)``."""
    dt = x.dtype
    s2 = torch.tensor(g, dtype=dt)
    big = big_mask64(s2, c) if big is None else big
    f_th, _, f_y, f_xi = coefficients(s2, torch.tensor(True), big, c, dt, variant)
    ce = torch.tensor(c["c1"], dtype=dt) * torch.tensor(c["sig_prev"], dtype=dt)
    es = torch.tensor(c["eta"], dtype=dt) * torch.tensor(c["sig_prev"], dtype=dt)
    x0 = predict_x0(x, eps, c) if x0 is None else x0
    inner = (f_th - 1) * x0 + (f_xi - es) * xi
    if variant != "keep_eps":
        inner = inner - ce * eps
    tail = proj(inner) if variant != "xi_plain" else proj(inner - (f_xi - es) * xi) + (f_xi - es) * xi
    return c["a_prev"] * ((x0 + ce * eps + es * xi) + tail + f_y * y_up)


# --- the periodic blur ------------------------------------------------------------------------------
def dft_step(x, eps, y, xi, c, M: torch.Tensor, keep: torch.Tensor, big=None, x0=None) -> torch.Tensor:
    """(B, C, H, W) tensors in x's dtype (fp32: ``torch.fft`` in complex64).  ``M`` (H, W) complex,
    ``keep`` (H, W) bool; ``big`` the class mask (default: the fp64 decision on |M|²); ``x0`` given:
    used instead of ``predict_x0(x, eps)``."""
    dt = x.dtype
    cd = torch.complex128 if dt == torch.float64 else torch.complex64
    M = M.to(cd)
    s2 = (M.real * M.real + M.imag * M.imag).to(dt)
    big = big_mask64(s2, c) if big is None else big
    f_th, f_ep, f_y, f_xi = coefficients(s2, keep, big, c, dt)
    P = torch.where(keep, 1.0 / torch.where(keep, M, torch.ones_like(M)), torch.zeros_like(M))
    x0 = predict_x0(x, eps, c) if x0 is None else x0
    fft = torch.fft.fft2
    spec = f_th * fft(x0) + f_ep * fft(eps) + f_xi * fft(xi) + f_y * (P * fft(y.to(dt)))
    return (c["a_prev"] * torch.fft.ifft2(spec).real).to(dt)


def truncated_blur(M: torch.Tensor, keep: torch.Tensor):
    """x ↦ Re IFFT2(keep·M·FFT2 x) in fp64: the operator DDRM sees (dropped frequencies unobserved)."""
    spec = torch.where(keep, M.to(torch.complex128), torch.zeros_like(M, dtype=torch.complex128))
    return lambda x: torch.fft.ifft2(torch.fft.fft2(x.double()) * spec).real


# --- the kernels' order of operations, in fp32 --------------------------------------------------------
def _f32(c):
    return {key: torch.tensor(c[key], dtype=torch.float32) for key in KEYS}


def emu_elementwise(x, eps, y_full, keep, xi, c, variant: str | None = None) -> torch.Tensor:
    """k_ddrm (csrc/sp_dps.hip): fp32 rows (B, n), ``y_full`` the observation scattered to (B, n)."""
    q = _f32(c)
    s2 = torch.ones((), dtype=torch.float32)
    fo = coefficients(s2, torch.tensor(True), big_mask32(s2, c), c, torch.float32, variant)
    fu = coefficients(s2, torch.tensor(False), torch.tensor(False), c, torch.float32)
    x0 = (x - q["k"] * eps) * (1 / q["a"])
    obs = q["a_prev"] * ((fo[0] * x0 + fo[2] * y_full) + fo[3] * xi)
    if variant == "keep_eps":
        obs = q["a_prev"] * (((fo[0] * x0 + fu[1] * eps) + fo[2] * y_full) + fo[3] * xi)
    # "xi_plain": the observed set's noise weight on every element
    uno = q["a_prev"] * ((x0 + fu[1] * eps) + (fo[3] if variant == "xi_plain" else fu[3]) * xi)
    return torch.where(keep.reshape(-1).bool(), obs, uno)


def emu_sr(x, eps, y, xi, c, shape: tuple, s: int, variant: str | None = None) -> torch.Tensor:
    """k_sr_ddrm (csrc/sp_sr.hip): fp32 rows (B, n), y (B, m).  The block sums are exact on the
    exact cases, so ``avg_pool2d`` stands for the kernel's summation tree there."""
    q = _f32(c)
    s2 = torch.tensor(1.0 / (s * s), dtype=torch.float32)
    fo = coefficients(s2, torch.tensor(True), big_mask32(s2, c), c, torch.float32, variant)
    fu = coefficients(s2, torch.tensor(False), torch.tensor(False), c, torch.float32)
    proj, up = sr_ops(shape, s)
    x0 = (x - q["k"] * eps) * (1 / q["a"])
    g_th, g_xi = fo[0] - 1, fo[3] - fu[3]
    d = (g_th * proj(x0) + g_xi * proj(xi)) + fo[2] * up(y)
    if variant != "keep_eps":
        d = ((g_th * proj(x0) - fu[1] * proj(eps)) + g_xi * proj(xi)) + fo[2] * up(y)
    if variant == "xi_plain":
        d = ((g_th * proj(x0) - fu[1] * proj(eps)) + g_xi * xi) + fo[2] * up(y)
    return q["a_prev"] * (((x0 + fu[1] * eps) + fu[3] * xi) + d)


# --- the scalars of a step and the loop ---------------------------------------------------------------
def ddrm_coefs(acp: torch.Tensor, t: int, t_prev: int, sigma_y: float, eta: float, eta_b: float):
    at, ap = acp[t], acp[t_prev]
    return dict(a=float(at ** 0.5), k=float((1 - at) ** 0.5), a_prev=float(ap ** 0.5),
                sig_prev=float((1 - ap) ** 0.5 / ap ** 0.5), sig_y=float(sigma_y), eta=float(eta),
                eta_b=float(eta_b), c1=float((1 - float(eta) ** 2) ** 0.5))


def ddrm_reference(eps_fn, acp: torch.Tensor, timesteps: list, step_fn, y: torch.Tensor,
                   init: torch.Tensor, noise_of_step, *, sigma_y: float, eta: float = 0.85,
                   eta_b: float = 1.0) -> torch.Tensor:
    """The DDRM loop in the dtype of ``init``: ``step_fn(x, eps, y, xi, c)`` is one step for the
    operator, ``noise_of_step(i)`` is ξ of loop index i (the Philox step index)."""
    x = init
    with torch.no_grad():
        for i in range(len(timesteps) - 1, 1, -1):
            t, t_prev = int(timesteps[i]), int(timesteps[i - 1])
            c = ddrm_coefs(acp, t, t_prev, sigma_y, eta, eta_b)
            x = step_fn(x, eps_fn(x, t), y, noise_of_step(i).to(x.dtype), c)
        t1 = int(timesteps[1])
        return (x - (1 - acp[t1]) ** 0.5 * eps_fn(x, t1)) / acp[t1] ** 0.5


# --- exact cases ----------------------------------------------------------------------------------
# a = k = a_prev = 1/2, eta = 1/2, c1 = 3/4 (taken as given), eta_b = 3/4; with s = sqrt(g):
#   big    sig_prev = 5/8, sig_y = s/2:  e = eta_b sig_y = 3s/8, e^2 / s^2 = 9/64,
#          f_xi = sqrt(25/64 - 9/64) = 1/2, f_th = 1/4, f_y = 3/4, c1 sig_prev = 15/32
#   small  sig_prev = 1/2, sig_y = s:    r = (3/8) s / s = 3/8, f_th = 5/8, f_xi = eta sig_prev = 1/4
# With integer x, eps, xi, y in [-8, 8]: x0 = 2x - eps is an integer, a block mean a multiple of
# 1/64, every coefficient a multiple of 1/32, x' a multiple of 2^-12 below 2^7: every intermediate
# of every evaluation order is an fp32 number, so no fp32 evaluation can round.
def exact_coefs(regime: str, s: int = 1):
    base = dict(a=0.5, k=0.5, a_prev=0.5, eta=0.5, eta_b=0.75, c1=0.75)
    if regime == "big":
        return dict(base, sig_prev=0.625, sig_y=0.5 / s)
    assert regime == "small", regime
    return dict(base, sig_prev=0.5, sig_y=1.0 / s)


def exact_inputs(batch: int, n: int, m_rows: int, m: int, seed: int):
    """Integer-valued fp32 (x, eps, xi) of shape (batch, n) and y of shape (m_rows, m)."""
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randint(-8, 9, (batch, n), generator=g).float() for _ in range(3))
    y = torch.randint(-8, 9, (m_rows, m), generator=g).float()
    return x, eps, xi, y
