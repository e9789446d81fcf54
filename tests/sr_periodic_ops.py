"""fp64 semantics of the periodic blur-and-decimate super-resolution operator — TEST
INFRASTRUCTURE ONLY.

The reference has no such operator.  What ``PeriodicSuperResolutionOperator`` and the
``SP_OP_SR_PERIODIC`` kernels implement is pinned here twice, in float64:

* as dense matrices built by index arithmetic, no FFT anywhere (``dense``: row ``(i, j)`` has
  ``h[u][v]`` at column ``((s·i + u − pad) mod H, (s·j + v − pad) mod W)``), with the truncated
  SVD (``dense_pinv``) and the dense solve of ``(AᵀA + ρI) z = Aᵀy + ρ x0`` (``dense_prox``).
  These are the authority;
* as the spectral identities (``transfer``, ``lam``, ``spectral_*``), which the CPU tests pin to the
  dense matrices and the GPU tests use at sizes where a dense matrix does not fit.

``keep`` is always **given** (the operator's own), so a singular value at the threshold can never
be decided differently by the test and by the code; ``dense_pinv`` keeps the ``keep.sum()`` largest
singular values and the tests assert that the threshold falls in a gap.
"""

from __future__ import annotations

import numpy as np
import torch

from samplers_amd.operators.sr_filter import bicubic_taps, gaussian_filter_taps

ASYM = torch.tensor([1.0, 2.0, 0.0, -1.0, 3.0, 0.5]) / 8

# the issue's six cases: name -> (H, W, s, taps, frequencies kept at rtol 3e-2 / all)
CASES = {
    "bicubic2": (16, 24, 2, bicubic_taps(2), (96, 96)),
    "bicubic4": (32, 16, 4, bicubic_taps(4), (32, 32)),
    "gauss16": (32, 32, 4, gaussian_filter_taps(16, 3.0), (59, 64)),
    "gauss32": (32, 64, 8, gaussian_filter_taps(32, 6.0), (29, 32)),
    "bicubic8cut": (16, 16, 8, bicubic_taps(8)[8:24], (4, 4)),
    "asym": (8, 8, 2, ASYM, (16, 16)),
}


def taps2d(taps) -> np.ndarray:
    t = taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else np.asarray(taps)
    t = t.astype(np.float32).astype(np.float64)
    return np.outer(t, t) if t.ndim == 1 else t


def dense(taps, H: int, W: int, s: int) -> np.ndarray:
    """A of one plane as an (H/s · W/s, H · W) float64 matrix."""
    h = taps2d(taps)
    k = h.shape[0]
    pad = (k - s) // 2
    assert (k - s) % 2 == 0 and s <= k <= min(H, W) and H % s == 0 and W % s == 0
    hl, wl = H // s, W // s
    a = np.zeros((hl * wl, H * W))
    for i in range(hl):
        for j in range(wl):
            for u in range(k):
                r = (s * i + u - pad) % H
                for v in range(k):
                    a[i * wl + j, r * W + (s * j + v - pad) % W] += h[u, v]
    return a


def dense_apply(a: np.ndarray, x: torch.Tensor, out_hw: tuple) -> torch.Tensor:
    """``a`` on every plane of ``x`` (..., h, w) -> (..., *out_hw), float64."""
    flat = x.detach().cpu().double().reshape(-1, a.shape[1]).numpy()
    return torch.from_numpy(flat @ a.T).reshape(*x.shape[:-2], *out_hw)


def dense_pinv(a: np.ndarray, count: int) -> np.ndarray:
    """The Moore–Penrose inverse truncated to the ``count`` largest singular values."""
    u, sv, vt = np.linalg.svd(a, full_matrices=False)
    return (vt[:count].T / sv[:count]) @ u[:, :count].T


def dense_prox(a: np.ndarray, x0: torch.Tensor, y: torch.Tensor, rho: float) -> torch.Tensor:
    """``argmin ½‖y − A z‖² + ρ/2 ‖z − x0‖²`` by the dense solve, per plane."""
    n = a.shape[1]
    xf = x0.detach().cpu().double().reshape(-1, n).numpy()
    yf = y.detach().cpu().double().reshape(-1, a.shape[0]).numpy()
    z = np.linalg.solve(a.T @ a + rho * np.eye(n), (yf @ a + rho * xf).T).T
    return torch.from_numpy(z).reshape(x0.shape)


# --- the spectral route ---------------------------------------------------------------------------
def transfer(taps, H: int, W: int, s: int) -> torch.Tensor:
    """M (complex128, (H, W)): tap (u, v) at ((u − pad) mod H, (v − pad) mod W), transformed,
    conjugated."""
    h = taps2d(taps)
    k = h.shape[0]
    pad = (k - s) // 2
    hc = np.zeros((H, W))
    for u in range(k):
        for v in range(k):
            hc[(u - pad) % H, (v - pad) % W] += h[u, v]
    return torch.from_numpy(np.conj(np.fft.fft2(hc)))


def lam(M: torch.Tensor, s: int) -> torch.Tensor:
    """Λ on the (H/s, W/s) grid by explicit sums over the s² aliases."""
    H, W = M.shape
    hl, wl = H // s, W // s
    mag = M.abs() ** 2
    out = torch.zeros(hl, wl, dtype=torch.float64)
    for a in range(s):
        for b in range(s):
            out += mag[a * hl:(a + 1) * hl, b * wl:(b + 1) * wl]
    return out / (s * s)


def pinv_spectrum(M: torch.Tensor, s: int, keep: torch.Tensor) -> torch.Tensor:
    """P = keept ? conj(M)/Λt : 0 for the given (H/s, W/s) bool mask."""
    lt = lam(M, s).repeat(s, s)
    kt = keep.detach().cpu().bool().repeat(s, s)
    p = torch.zeros_like(M)
    p[kt] = M.conj()[kt] / lt[kt]
    return p


def up(y: torch.Tensor, s: int) -> torch.Tensor:
    out = torch.zeros(*y.shape[:-2], y.shape[-2] * s, y.shape[-1] * s, dtype=y.dtype)
    out[..., ::s, ::s] = y
    return out


def _mul(x: torch.Tensor, spec: torch.Tensor) -> torch.Tensor:
    cd = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    return torch.fft.ifft2(torch.fft.fft2(x) * spec.to(cd)).real.to(x.dtype)


def spectral_down(x: torch.Tensor, spec: torch.Tensor, s: int) -> torch.Tensor:
    """Re ifft2(fft2(x) · spec)[::s, ::s]: A with M, A⁺ᵀ with conj(P)."""
    return _mul(x, spec)[..., ::s, ::s]


def spectral_up(y: torch.Tensor, spec: torch.Tensor, s: int) -> torch.Tensor:
    """Re ifft2(fft2(↑y) · spec): Aᵀ with conj(M), A⁺ with P."""
    return _mul(up(y, s), spec)


def spectral_prox(x0, y, M: torch.Tensor, s: int, rho: float) -> torch.Tensor:
    """x0 + Re ifft2(fft2(↑(y − A x0)) · conj(M)/(Λt + ρ)) in x0's precision."""
    lt = lam(M, s).repeat(s, s)
    return x0 + spectral_up(y.to(x0.dtype) - spectral_down(x0, M, s), M.conj() / (lt + rho), s)


class Ref:
    """The fp64 maps of one operator through the spectral route (``keep`` given)."""

    def __init__(self, taps, H: int, W: int, s: int, keep: torch.Tensor):
        self.s, self.M = s, transfer(taps, H, W, s)
        self.P = pinv_spectrum(self.M, s, keep)

    def A(self, x):
        return spectral_down(x.detach().cpu().double(), self.M, self.s)

    def At(self, y):
        return spectral_up(y.detach().cpu().double(), self.M.conj(), self.s)

    def pinv(self, y):
        return spectral_up(y.detach().cpu().double(), self.P, self.s)

    def pinv_t(self, x):
        return spectral_down(x.detach().cpu().double(), self.P.conj(), self.s)

    def prox(self, x0, y, rho):
        return spectral_prox(x0.detach().cpu().double(), y.detach().cpu().double(), self.M, self.s, rho)
