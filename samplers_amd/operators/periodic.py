"""Periodic (wrap-around) PSF blur with a spectral pseudo-inverse: the blur ``PGDMSampler`` can
invert.

The reference ships no blur operator, so the semantics are defined here and pinned in fp64 by
``tests/periodic_ops.py``.  With the PSF ``h`` of shape ``(K, K)``, ``K = 2R + 1``, on an image
whose own sizes ``H`` and ``W`` are transform lengths (each ``2^k`` or ``3·2^k`` in ``[8, 1024]``)
and ``1 ≤ R``, ``2R + 1 ≤ min(H, W)`` (no tap aliases onto another):

* ``apply`` is ``y[c,i,j] = Σ_{u,v} h[u,v] · x[c, (i+u−R) mod H, (j+v−R) mod W]`` — ``F.pad`` with
  mode ``circular`` followed by ``F.conv2d`` (correlation, no flip), the same map as
  ``FFTPSFBlurOperator(padding="circular").apply`` but on ``H × W`` transforms instead of
  ``padded_size(H + 2R)`` ones; ``y_shape == x_shape``;
* the map is exactly diagonal in the 2-D DFT: ``A x = Re ifft2(fft2(x) · M)`` with the transfer
  function ``M = conj(fft2(h_c))``, ``h_c`` the PSF with its centre tap at ``[0, 0]`` of an
  ``H × W`` zero array (``transfer_function``); ``apply_transpose`` has the multiplier ``conj(M)``;
* ``keep[k] = min(|M[k]|, |M[−k]|) > rtol · max|M|`` (symmetric under ``k → −k``, a bool buffer of
  shape ``(H, W)``); the default ``rtol = 3e-2`` is DDRM's singular-value threshold for deblurring;
* ``apply_pseudo_inverse`` has the multiplier ``P = keep ? 1/M : 0`` (``pseudo_inverse_spectrum``):
  the Moore–Penrose inverse of the blur truncated to the kept frequencies.  ``A⁺A = Π`` is the
  orthogonal projection onto them and ``A⁺ A A⁺ = A⁺`` holds; ``A A⁺ A = A`` does **not** hold
  (``A A⁺ A = A Π`` drops what the blur passes below the threshold);
* ``∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2 (A⁺y − Π x̂₀)`` since Π is symmetric and idempotent:
  ``pinv_grad_scale = 2``, and the fused PGDM pass computes ``A⁺y − Π x̂₀`` directly.

M, keep and P are computed once at construction, in fp64 on the host, and rounded to fp32.  On
device tensors all four maps (A, Aᵀ, A⁺, A⁺ᵀ) run the ``SP_OP_PSF_PERIODIC`` kernels
(``csrc/sp_psf_fft.hip``), each as an autograd function whose backward is its transpose; on host
tensors A is ``F.pad`` / ``F.conv2d`` and A⁺ is ``torch.fft`` with the stored spectrum.
"""

from __future__ import annotations

import numpy as np
import torch

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import (MAX_SIZE, MIN_SIZE, HipWorkspaceMap, _hip_prox, _plane_descriptor,
                   _transpose_by_grad, check_rho, transform_size_ok)
from .linear import LinearOperator
from .psf import _gaussian_psf, _square_kernel
from .psf_fft import psf_pad_torch


size_ok = transform_size_ok


def transfer_function(kernel, H: int, W: int) -> Tensor:
    """``M = conj(fft2(h_c))`` as a complex128 ``(H, W)`` tensor, ``h_c`` the odd-sized kernel
    with its centre tap at ``[0, 0]`` of an ``H × W`` zero array: ``A x = Re ifft2(fft2(x) · M)``."""
    k = np.asarray(kernel.detach().cpu().numpy() if isinstance(kernel, torch.Tensor) else kernel,
                   dtype=np.float64)
    if k.ndim != 2 or k.shape[0] % 2 != 1 or k.shape[1] % 2 != 1:
        raise ValueError(f"kernel sizes must be odd, got {k.shape}")
    if k.shape[0] > H or k.shape[1] > W:
        raise ValueError(f"a kernel of shape {k.shape} does not fit {H} x {W}")
    ru, rv = k.shape[0] // 2, k.shape[1] // 2
    hc = np.zeros((H, W), dtype=np.float64)
    rows = (np.arange(k.shape[0]) - ru) % H
    cols = (np.arange(k.shape[1]) - rv) % W
    hc[np.ix_(rows, cols)] = k
    return torch.from_numpy(np.conj(np.fft.fft2(hc)))


def pseudo_inverse_spectrum(M, rtol: float = 3e-2) -> tuple[Tensor, Tensor]:
    """``(P, keep)`` of a transfer function ``M``: ``keep[k] = min(|M[k]|, |M[−k]|) > rtol·max|M|``
    and ``P = keep ? 1/M : 0`` (complex128), both of M's shape."""
    if not 0.0 < float(rtol) < 1.0:
        raise ValueError(f"rtol must be in (0, 1), got {rtol}")
    m = np.asarray(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M,
                   dtype=np.complex128)
    mag = np.abs(m)
    neg = np.roll(np.flip(mag, axis=(0, 1)), 1, axis=(0, 1))  # |M[-k]|
    keep = np.minimum(mag, neg) > float(rtol) * mag.max()
    p = np.zeros_like(m)
    p[keep] = 1.0 / m[keep]
    return torch.from_numpy(p), torch.from_numpy(keep)


def half_spectrum(S) -> Tensor:
    """The layout the kernels read: columns ``kw ≤ W / 2`` of the ``(H, W)`` spectrum, transposed
    to ``(W // 2 + 1, H)``, as fp32 ``(re, im)`` pairs."""
    s = np.asarray(S.detach().cpu().numpy() if isinstance(S, torch.Tensor) else S)
    s = np.ascontiguousarray(s[:, : s.shape[1] // 2 + 1].T)
    return torch.from_numpy(np.stack([s.real, s.imag], axis=-1).astype(np.float32))


class PeriodicBlurOperator(LinearOperator):
    """Depthwise blur by a dense 2-D PSF with periodic boundaries on an image whose sizes are
    transform lengths, with the pseudo-inverse truncated at ``rtol · max|M|``; ``y`` has
    ``x_shape``.  ``A⁺A`` is an orthogonal projection and ``A⁺AA⁺ = A⁺``; ``AA⁺A = A`` does not
    hold (module docstring)."""

    # as FFTPSFBlurOperator: the maps need a workspace, so PSLD and ReSample take their generic
    # routes over apply / apply_transpose, both HIP here
    hip_linear = False
    # ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2 (A⁺y − Π x̂₀)
    pinv_grad_scale = 2.0

    def __init__(self, x_shape: Shape, kernel, rtol: float = 3e-2, device: Device = None) -> None:
        k = _square_kernel(kernel)
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if not (size_ok(h) and size_ok(w)):
            raise ValueError(f"H and W must each be 2^k or 3*2^k in [{MIN_SIZE}, {MAX_SIZE}], got "
                             f"{(h, w)}")
        r = int(k.shape[0]) // 2
        if not (1 <= r and 2 * r + 1 <= min(h, w)):
            raise ValueError(f"the PSF size 2R + 1 must be in [3, min(H, W)] = [3, {min(h, w)}], "
                             f"got {2 * r + 1}")
        if not 0.0 < float(rtol) < 1.0:
            raise ValueError(f"rtol must be in (0, 1), got {rtol}")
        torch.nn.Module.__init__(self)
        self.kernel_size, self.radius, self.rtol = int(k.shape[0]), r, float(rtol)
        m = transfer_function(k, h, w)
        p, keep = pseudo_inverse_spectrum(m, rtol)
        self.register_buffer("kernel", k.contiguous().to(device))
        self.register_buffer("keep", keep.contiguous().to(device))
        # the descriptor's taps: M then P, each (W // 2 + 1, H, 2)
        self.register_buffer("spectra",
                             torch.stack([half_spectrum(m), half_spectrum(p)]).contiguous().to(device))
        self.x_shape = (c, h, w)
        self.y_shape = self.x_shape

    @classmethod
    def gaussian(cls, x_shape: Shape, kernel_size: int = 61, sigma: float = 3.0,
                 rtol: float = 3e-2, device: Device = None) -> "PeriodicBlurOperator":
        """The isotropic Gaussian PSF as the outer product of ``gaussian_taps``, as
        ``FFTPSFBlurOperator.gaussian``."""
        return cls(x_shape, _gaussian_psf(kernel_size, sigma), rtol=rtol, device=device)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, False, False)
        return psf_pad_torch(x, self.kernel, "circular")

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, False, True)
        return _transpose_by_grad(lambda x: psf_pad_torch(x, self.kernel, "circular"), y)

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, True, False)
        _, h, w = self.x_shape
        p = torch.view_as_complex(self.spectra[1]).transpose(0, 1)  # (H, W // 2 + 1)
        cdtype = torch.complex128 if y.dtype == torch.float64 else torch.complex64
        return torch.fft.irfft2(torch.fft.rfft2(y) * p.to(cdtype), s=(h, w)).to(y.dtype)

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """``Z = (conj(M)·Y + ρ·X0) / (|M|² + ρ)``, ``z = Re ifft2(Z)``: the blur is diagonal in the
        transform, so its proximal map is a per-frequency division (every frequency, not only the
        kept ones: ρ regularises the small |M|).  ``sp_op_prox_ws`` on device tensors,
        ``torch.fft`` with the stored M on host tensors."""
        if x0.is_cuda:
            return _hip_prox(self, x0, y, rho)
        rho = check_rho(rho)
        _, h, w = self.x_shape
        cdtype = torch.complex128 if x0.dtype == torch.float64 else torch.complex64
        m = torch.view_as_complex(self.spectra[0]).transpose(0, 1).to(cdtype)  # (H, W // 2 + 1)
        zs = (m.conj() * torch.fft.rfft2(y.to(x0.dtype)) + rho * torch.fft.rfft2(x0)) / (m.abs() ** 2 + rho)
        return torch.fft.irfft2(zs, s=(h, w)).to(x0.dtype)

    def hip_descriptor(self) -> _hip.SpOp:
        d = _plane_descriptor(_hip.SP_OP_PSF_PERIODIC, self.x_shape)
        d.taps = self.spectra.data_ptr()
        d.radius = self.radius
        d.factor = 0
        return d
