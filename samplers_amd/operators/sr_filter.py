"""Filtered ×s super-resolution: an anti-alias filter wider than the stride, then every s-th
sample (bicubic ×4, Gaussian blur + decimation: the super-resolution task DPS, DDRM, DiffPIR and
ΠGDM are evaluated on).  ``SuperResolutionOperator`` is the special case of a box filter.

The reference ships no such operator, so the semantics are defined here and pinned in fp64 by
``tests/sr_filter_ref.py``.  For 1-D taps ``k[0..K-1]``, the same on both axes, and stride ``s``,
on every channel plane:

    ``y[c,i,j] = Σ_{u,v} k[u]·k[v] · x̃[c, s·i + u − P, s·j + v − P]``,  ``P = (K − s)/2``

with ``x̃`` the image extended **symmetrically**, edge sample repeated: ``x̃[−1−g] = x̃[g]`` and
``x̃[H+g] = x̃[H−1−g]`` (the half-sample convention of MATLAB ``imresize`` and of the DPS code's
resizer), so the window of output ``i`` is centred on the centre of its s-pixel block.

* ``s ∈ {2, 4, 8}`` divides ``H`` and ``W``; ``s ≤ K ≤ 32``; ``K − s`` even;
  ``H, W ≥ max(1, P)`` (one fold per side suffices); ``y_shape = (C, H/s, W/s)``;
* the taps are used as given (any finite fp32 values, no normalisation);
* ``apply_transpose`` is the exact transpose;
* no pseudo-inverse: ``PGDMSampler`` raises ``NotImplementedError`` as for the blurs.

This is the operator's host form only: plain torch on host tensors (an index gather for the
extension and two strided ``F.conv2d``, the transpose through autograd).  The library has no
kind for it yet, so ``hip_descriptor()`` is ``None`` (the fused samplers refuse the operator by
name) and the maps raise ``NotImplementedError`` on device tensors rather than run eager torch
there: a missing kernel is an error ("Filtered super-resolution").
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from samplers_amd.dtypes import Device, Shape, Tensor

from .linear import LinearOperator

FACTORS = (2, 4, 8)
MAX_TAPS = 32


def _keys_cubic(t: np.ndarray, a: float = -0.5) -> np.ndarray:
    t = np.abs(t)
    return np.where(t <= 1, ((a + 2) * t - (a + 3)) * t * t + 1,
                    np.where(t < 2, ((a * t - 5 * a) * t + 8 * a) * t - 4 * a, 0.0))


def bicubic_taps(factor: int) -> Tensor:
    """The ``K = 4s`` taps of antialiased bicubic ×1/s: ``k[t] = cubic((2t + 1 − 4s)/(2s))/s``
    with the Keys cubic (a = −0.5), computed in fp64, divided by their sum, rounded to fp32.
    For s = 2, 4, 8 the sum is exactly s·(1/s) and the taps are dyadic: exact in fp32."""
    if factor not in FACTORS:
        raise ValueError(f"factor must be one of {FACTORS}, got {factor!r}")
    s = int(factor)
    t = np.arange(4 * s, dtype=np.float64)
    k = _keys_cubic((2 * t + 1 - 4 * s) / (2 * s)) / s
    return torch.from_numpy(k / k.sum()).to(torch.float32)


def gaussian_filter_taps(kernel_size: int, sigma: float) -> Tensor:
    """Normalised 1-D Gaussian taps centred on ``(kernel_size − 1)/2`` (a half-sample centre for
    the even sizes the even factors need; for odd sizes these are ``blur.gaussian_taps``),
    computed in fp64, stored fp32."""
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    i = torch.arange(int(kernel_size), dtype=torch.float64) - (int(kernel_size) - 1) / 2.0
    k = torch.exp(-(i ** 2) / (2.0 * float(sigma) ** 2))
    return (k / k.sum()).to(torch.float32)


def symmetric_index(length: int, pad: int, device=None) -> Tensor:
    """Source indices of the extended axis ``[−pad, length + pad)``: ``−1−g → g``,
    ``length+g → length−1−g`` (``pad ≤ length``)."""
    g = torch.arange(-pad, length + pad, device=device)
    g = torch.where(g < 0, -1 - g, g)
    return torch.where(g >= length, 2 * length - 1 - g, g)


def sr_filter_torch(x: Tensor, taps: Tensor, factor: int) -> Tensor:
    """Host (torch) form of the forward map on ``(..., C, H, W)``."""
    k, s = int(taps.numel()), int(factor)
    p = (k - s) // 2
    h, w = x.shape[-2], x.shape[-1]
    planes = x.reshape(-1, 1, h, w)
    ext = planes.index_select(2, symmetric_index(h, p, x.device)).index_select(
        3, symmetric_index(w, p, x.device))
    t = taps.to(device=x.device, dtype=x.dtype)
    out = F.conv2d(ext, t.view(1, 1, 1, k), stride=(1, s))
    out = F.conv2d(out, t.view(1, 1, k, 1), stride=(s, 1))
    return out.reshape(*x.shape[:-2], h // s, w // s)


class FilteredSuperResolutionOperator(LinearOperator):
    """Separable filter ``taps`` at stride ``factor`` on the symmetric extension of every channel
    plane; ``y`` has shape ``(C, H/s, W/s)``."""

    def __init__(self, x_shape: Shape, taps, factor: int = 4, device: Device = None) -> None:
        if factor not in FACTORS:
            raise ValueError(f"factor must be one of {FACTORS}, got {factor!r}")
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        t = torch.as_tensor(np.asarray(taps) if not isinstance(taps, torch.Tensor) else taps)
        t = t.detach().to(device="cpu", dtype=torch.float32)
        if t.ndim != 1:
            raise ValueError("taps must be 1-D (the same filter on both axes)")
        k, s = int(t.numel()), int(factor)
        if not (s <= k <= MAX_TAPS):
            raise ValueError(f"the number of taps must be in [factor, {MAX_TAPS}] = [{s}, {MAX_TAPS}], got {k}")
        if (k - s) % 2:
            raise ValueError(f"the number of taps must have the parity of the factor (K − s even), "
                             f"got K={k}, s={s}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("taps must be finite")
        c, h, w = (int(d) for d in x_shape)
        if min(c, h, w) <= 0 or h % s or w % s:
            raise ValueError(f"height and width must be positive multiples of the factor {s}, "
                             f"got x_shape={tuple(x_shape)}")
        p = (k - s) // 2
        if min(h, w) < max(1, p):
            raise ValueError(f"height and width must be at least the pad P = (K − s)/2 = {p} "
                             f"(one fold per side), got x_shape={tuple(x_shape)}")
        torch.nn.Module.__init__(self)
        self.register_buffer("taps", t.contiguous().to(device))
        self.factor, self.kernel_size, self.pad = s, k, p
        self.x_shape = (c, h, w)
        self.y_shape = (c, h // s, w // s)

    @classmethod
    def gaussian(cls, x_shape: Shape, factor: int = 4, kernel_size: int = 16, sigma: float = 2.0,
                 device: Device = None) -> "FilteredSuperResolutionOperator":
        """Gaussian blur + decimation: ``gaussian_filter_taps(kernel_size, sigma)`` at stride
        ``factor``; ``kernel_size`` must have the parity of ``factor``."""
        if (int(kernel_size) - int(factor)) % 2:
            raise ValueError("kernel_size must have the parity of the factor")
        return FilteredSuperResolutionOperator(x_shape, gaussian_filter_taps(kernel_size, sigma),
                                               factor=factor, device=device)

    def _host_only(self, t: Tensor) -> None:
        if t.is_cuda:
            raise NotImplementedError(f"{type(self).__name__} has no native (HIP) kernels yet: its maps "
                                      "run on host tensors only")

    def apply(self, x: Tensor) -> Tensor:
        self._host_only(x)
        return sr_filter_torch(x, self.taps, self.factor)

    def apply_transpose(self, y: Tensor) -> Tensor:
        self._host_only(y)
        x = torch.zeros(*y.shape[:-3], *self.x_shape, dtype=y.dtype, device=y.device,
                        requires_grad=True)
        with torch.enable_grad():
            (g,) = torch.autograd.grad(sr_filter_torch(x, self.taps, self.factor), x, grad_outputs=y)
        return g

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        raise NotImplementedError(f"{type(self).__name__} has no pseudo-inverse")


class BicubicSuperResolutionOperator(FilteredSuperResolutionOperator):
    """Antialiased bicubic ×1/s (``bicubic_taps(factor)``, ``K = 4s``): on every output whose
    window lies inside the image it equals
    ``F.interpolate(mode="bicubic", antialias=True, scale_factor=1/s)``; at the border torch clips
    and renormalises the window where this operator extends the image symmetrically."""

    def __init__(self, x_shape: Shape, factor: int = 4, device: Device = None) -> None:
        super().__init__(x_shape, bicubic_taps(factor), factor=factor, device=device)
