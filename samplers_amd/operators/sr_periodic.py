"""Periodic blur-and-decimate ×s super-resolution: an anti-alias filter wider than the stride with
wrap-around boundaries, then every s-th sample (the bicubic / Gaussian ×4 task of DPS, DDRM, ΠGDM
and DiffPIR in the form DiffPIR, USRNet and DPIR use).  Away from the border it is
``FilteredSuperResolutionOperator``; unlike it, it has a spectral pseudo-inverse and a closed-form
proximal map, and it runs in HIP (``SP_OP_SR_PERIODIC``).

The reference ships no such operator, so the semantics are defined here and pinned in fp64 by the
dense matrices of ``tests/sr_periodic_ops.py``.  ``x_shape = (C, H, W)``, ``s ∈ {2, 4, 8}`` divides
``H`` and ``W``, each ``2^k`` or ``3·2^k`` in ``[8, 1024]``.  The taps are 1-D ``k[0..K−1]``
(``h[u][v] = k[u]·k[v]``) or a square 2-D ``h``, ``s ≤ K ≤ min(H, W)``, ``K − s`` even,
``pad = (K − s)/2``, used as given (finite fp32, no normalisation):

    ``y[c,i,j] = Σ_{u,v} h[u][v] · x[c, (s·i + u − pad) mod H, (s·j + v − pad) mod W]``

``y_shape = (C, H/s, W/s)``.  With ``↑`` the zero insertion onto the lattice ``[::s, ::s]``:

* ``M = conj(fft2(h_c))``, tap ``(u, v)`` of ``h_c`` at ``((u − pad) mod H, (v − pad) mod W)``
  (``sr_transfer_function``): ``A x = Re ifft2(fft2(x)·M)[::s, ::s]``,
  ``Aᵀ y = Re ifft2(fft2(↑y)·conj(M))``;
* ``Λ[k] = (1/s²) Σ_{a,b<s} |M[kh + a·H/s, kw + b·W/s]|²`` on the ``(H/s, W/s)`` grid
  (``sr_lambda``): ``A Aᵀ`` is diagonal in the low-resolution transform with these eigenvalues,
  and the singular values of A are ``√Λ``;
* ``keep = √Λ > rtol · max √Λ`` (default ``rtol = 3e-2`` as ``PeriodicBlurOperator``); ``Λt`` and
  ``keept`` are Λ and keep tiled s×s to ``H × W``; ``P = keept ? conj(M)/Λt : 0``:
  ``A⁺ y = Re ifft2(fft2(↑y)·P)``, the Moore–Penrose inverse truncated to the kept singular
  values.  ``A⁺A`` is an orthogonal projection and ``A⁺AA⁺ = A⁺``, so
  ``∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2·A⁺(y − A x̂₀)`` and ``pinv_grad_scale = 2``;
* ``apply_prox(x0, y, ρ) = x0 + Re ifft2(fft2(↑(y − A x0)) · conj(M)/(Λt + ρ))`` (every frequency
  divided, not only the kept ones).

M, P and Λt are computed once, in fp64 on the host, and rounded to fp32 (``sr_stored_arrays``).  On
device tensors the four maps and the proximal map run the ``SP_OP_SR_PERIODIC`` kernels
(``csrc/sp_psf_fft.hip``), each map an autograd function whose backward is its transpose; on host
tensors A is a circular ``F.pad`` and a strided ``F.conv2d``, Aᵀ its gradient, A⁺ and the proximal
map ``torch.fft`` with the stored spectra.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import MAX_SIZE, MIN_SIZE, HipWorkspaceMap, _hip_prox, check_rho, transform_size_ok
from .linear import LinearOperator
from .periodic import half_spectrum
from .sr_filter import FACTORS, bicubic_taps, gaussian_filter_taps


def _taps_2d(taps) -> np.ndarray:
    """The ``(K, K)`` fp64 taps of 1-D (outer product, exact in fp64) or square 2-D fp32 taps."""
    t = taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else np.asarray(taps)
    if t.ndim not in (1, 2) or t.size == 0 or (t.ndim == 2 and t.shape[0] != t.shape[1]):
        raise ValueError(f"taps must be 1-D or a square 2-D array, got shape {t.shape}")
    t = t.astype(np.float32).astype(np.float64)
    if not np.isfinite(t).all():
        raise ValueError("taps must be finite")
    return np.outer(t, t) if t.ndim == 1 else t


def sr_transfer_function(taps, H: int, W: int, factor: int) -> Tensor:
    """``M = conj(fft2(h_c))`` as a complex128 ``(H, W)`` tensor, tap ``(u, v)`` of the ``K × K``
    taps at ``((u − pad) mod H, (v − pad) mod W)`` of a zero array, ``pad = (K − factor)/2``."""
    h = _taps_2d(taps)
    k, s = h.shape[0], int(factor)
    if (k - s) % 2 or k < s:
        raise ValueError(f"the number of taps K must be >= the factor with K − s even, got K={k}, s={s}")
    if k > min(H, W):
        raise ValueError(f"K = {k} taps do not fit {H} x {W}")
    pad = (k - s) // 2
    hc = np.zeros((H, W), dtype=np.float64)
    hc[np.ix_((np.arange(k) - pad) % H, (np.arange(k) - pad) % W)] = h
    return torch.from_numpy(np.conj(np.fft.fft2(hc)))


def sr_lambda(M, factor: int) -> Tensor:
    """``Λ`` on the ``(H/s, W/s)`` grid (fp64): the mean of ``|M|²`` over the s² frequencies that
    alias onto each low-resolution one; the eigenvalues of ``A Aᵀ``."""
    m = np.asarray(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M)
    s, (H, W) = int(factor), m.shape
    return torch.from_numpy((np.abs(m) ** 2).reshape(s, H // s, s, W // s).mean(axis=(0, 2)))


def sr_stored_arrays(taps, H: int, W: int, factor: int, rtol: float = 3e-2):
    """``(M, P, Λt, keep)``: the transfer function, the pseudo-inverse multiplier and Λ tiled to
    ``H × W`` (complex128, complex128, float64), and the kept set on the ``(H/s, W/s)`` grid."""
    if not 0.0 < float(rtol) < 1.0:
        raise ValueError(f"rtol must be in (0, 1), got {rtol}")
    s = int(factor)
    m = sr_transfer_function(taps, H, W, s).numpy()
    lam = sr_lambda(m, s).numpy()
    sv = np.sqrt(lam)
    keep = sv > float(rtol) * sv.max()
    lam_t, keep_t = np.tile(lam, (s, s)), np.tile(keep, (s, s))
    p = np.zeros_like(m)
    p[keep_t] = np.conj(m[keep_t]) / lam_t[keep_t]
    return (torch.from_numpy(m), torch.from_numpy(p), torch.from_numpy(lam_t),
            torch.from_numpy(keep))


class PeriodicSuperResolutionOperator(LinearOperator):
    """Depthwise filter ``taps`` with periodic boundaries at stride ``factor`` on an image whose
    sizes are transform lengths; ``y`` has shape ``(C, H/s, W/s)``.  Exact transpose, truncated
    Moore–Penrose inverse and closed-form proximal map (module docstring)."""

    # the maps need a workspace, so PSLD and ReSample take their generic routes over apply /
    # apply_transpose, both HIP here
    hip_linear = False
    # ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2·A⁺(y − A x̂₀)
    pinv_grad_scale = 2.0

    def __init__(self, x_shape: Shape, taps, factor: int = 4, rtol: float = 3e-2,
                 device: Device = None) -> None:
        if factor not in FACTORS:
            raise ValueError(f"factor must be one of {FACTORS}, got {factor!r}")
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        s = int(factor)
        if c <= 0 or not (transform_size_ok(h) and transform_size_ok(w)):
            raise ValueError(f"H and W must each be 2^k or 3*2^k in [{MIN_SIZE}, {MAX_SIZE}], got "
                             f"{(h, w)}")
        if h % s or w % s:
            raise ValueError(f"height and width must be multiples of the factor {s}, got {(h, w)}")
        t = _taps_2d(taps)
        k = int(t.shape[0])
        if not s <= k <= min(h, w):
            raise ValueError(f"the number of taps must be in [factor, min(H, W)] = [{s}, {min(h, w)}], "
                             f"got {k}")
        if (k - s) % 2:
            raise ValueError(f"the number of taps must have the parity of the factor (K − s even), "
                             f"got K={k}, s={s}")
        m, p, lam_t, keep = sr_stored_arrays(taps, h, w, s, rtol)  # from the taps as given: 1-D
        # products stay exact in fp64
        torch.nn.Module.__init__(self)
        self.factor, self.kernel_size, self.pad, self.rtol = s, k, (k - s) // 2, float(rtol)
        hw = w // 2 + 1
        lam_half = lam_t.numpy()[:, :hw].T.astype(np.float32)
        # the descriptor's taps: M and P as (W // 2 + 1, H, 2), then Λt as (W // 2 + 1, H)
        flat = torch.cat([half_spectrum(m).reshape(-1), half_spectrum(p).reshape(-1),
                          torch.from_numpy(np.ascontiguousarray(lam_half)).reshape(-1)])
        self.register_buffer("kernel", torch.from_numpy(t).contiguous().to(device))  # fp64, (K, K)
        self.register_buffer("keep", keep.contiguous().to(device))
        self.register_buffer("spectra", flat.contiguous().to(device))
        self.x_shape = (c, h, w)
        self.y_shape = (c, h // s, w // s)

    @classmethod
    def bicubic(cls, x_shape: Shape, factor: int = 4, rtol: float = 3e-2,
                device: Device = None) -> "PeriodicSuperResolutionOperator":
        """Antialiased bicubic ×1/s: ``bicubic_taps(factor)``, ``K = 4s``."""
        return cls(x_shape, bicubic_taps(factor), factor=factor, rtol=rtol, device=device)

    @classmethod
    def gaussian(cls, x_shape: Shape, factor: int = 4, kernel_size: int = 16, sigma: float = 2.0,
                 rtol: float = 3e-2, device: Device = None) -> "PeriodicSuperResolutionOperator":
        """Gaussian blur + decimation: ``gaussian_filter_taps(kernel_size, sigma)``."""
        return cls(x_shape, gaussian_filter_taps(kernel_size, sigma), factor=factor, rtol=rtol,
                   device=device)

    # --- the stored arrays, as the kernels read them ----------------------------------------
    def _half(self, which: int) -> Tensor:
        """M (0) or P (1) as a complex64 ``(H, W // 2 + 1)`` view's transpose."""
        _, h, w = self.x_shape
        n = (w // 2 + 1) * h * 2
        return torch.view_as_complex(self.spectra[which * n:(which + 1) * n].view(w // 2 + 1, h, 2)
                                     ).transpose(0, 1)

    @property
    def lambda_half(self) -> Tensor:
        """Λt as fp32 ``(H, W // 2 + 1)`` (the transpose of the stored ``(W // 2 + 1, H)``)."""
        _, h, w = self.x_shape
        n = (w // 2 + 1) * h
        return self.spectra[4 * n:].view(w // 2 + 1, h).transpose(0, 1)

    # --- host forms ---------------------------------------------------------------------------
    def _apply_host(self, x: Tensor) -> Tensor:
        _, h, w = self.x_shape
        planes = x.reshape(-1, 1, h, w)
        if self.pad:
            planes = F.pad(planes, (self.pad,) * 4, mode="circular")
        k = self.kernel.to(device=x.device, dtype=x.dtype)
        out = F.conv2d(planes, k.view(1, 1, *k.shape), stride=self.factor)
        return out.reshape(*x.shape[:-3], *self.y_shape)

    def _upsample(self, y: Tensor) -> Tensor:
        up = torch.zeros(*y.shape[:-3], *self.x_shape, dtype=y.dtype, device=y.device)
        up[..., ::self.factor, ::self.factor] = y
        return up

    def _spectral_up(self, y: Tensor, mult: Tensor) -> Tensor:
        """``Re ifft2(fft2(↑y) · mult)`` with a half-spectrum multiplier ``(H, W // 2 + 1)``."""
        _, h, w = self.x_shape
        cdtype = torch.complex128 if y.dtype == torch.float64 else torch.complex64
        return torch.fft.irfft2(torch.fft.rfft2(self._upsample(y)) * mult.to(cdtype), s=(h, w)).to(y.dtype)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, False, False)
        return self._apply_host(x)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, False, True)
        x = torch.zeros(*y.shape[:-3], *self.x_shape, dtype=y.dtype, device=y.device,
                        requires_grad=True)
        with torch.enable_grad():
            # differentiable in y (its backward is A again): PSLD's host form differentiates AᵀA
            (g,) = torch.autograd.grad(self._apply_host(x), x, grad_outputs=y,
                                       create_graph=y.requires_grad)
        return g

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, True, False)
        return self._spectral_up(y, self._half(1))

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """``x0 + Re ifft2(fft2(↑(y − A x0)) · conj(M)/(Λt + ρ))``: ``sp_op_prox_ws`` on device
        tensors, ``torch.fft`` with the stored M and Λt on host tensors."""
        if x0.is_cuda:
            return _hip_prox(self, x0, y, rho)
        rho = check_rho(rho)
        rdtype = torch.float64 if x0.dtype == torch.float64 else torch.float32
        mult = self._half(0).conj() / (self.lambda_half.to(rdtype) + rho)
        return x0 + self._spectral_up(y.to(x0.dtype) - self._apply_host(x0), mult)

    def hip_descriptor(self) -> _hip.SpOp:
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_SR_PERIODIC
        d.channels, d.height, d.width = self.x_shape
        d.n = int(np.prod(self.x_shape))
        d.m = int(np.prod(self.y_shape))
        d.taps = self.spectra.data_ptr()
        d.radius = self.kernel_size
        d.factor = self.factor
        return d
