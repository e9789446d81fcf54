"""Point-spread-function blur: a dense depthwise 2-D PSF (motion blur, the DPS paper's 61×61
Gaussian, anisotropic Gaussians, defocus discs, measured PSFs).

The reference ships no blur operator, so the semantics are defined here and pinned in fp64 by
``tests/psf_ops.py``.  With the PSF ``h`` of shape ``(K, K)``, ``K = 2R + 1``, ``1 ≤ R ≤ 30``:

* ``apply`` is a **correlation** on every channel plane, as ``F.conv2d`` (no kernel flip):
  ``y[c,i,j] = Σ_{u,v} h[u,v] · x̃[c, i+u−R, j+v−R]`` with ``x̃`` the image reflect-padded by
  ``R`` on both spatial axes (``F.pad(mode="reflect")``, edge sample not repeated);
  ``H, W > 2R``; ``y_shape == x_shape``;
* ``apply_transpose`` is the exact adjoint: the zero-extended correlation with the flipped PSF,
  then the padded halo folded back onto the pixels it was reflected from;
* the taps are used as given (any finite fp32 values, negative ones allowed, no normalisation);
* no pseudo-inverse: ``PGDMSampler`` raises ``NotImplementedError`` as for
  ``GaussianBlurOperator``.

On device tensors the maps run the ``SP_OP_PSF`` kernels (``csrc/sp_psf.hip``), whose work
follows the PSF's non-zero support: a thin motion trajectory in a 61×61 box costs its support,
not the box.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import HipLinearMap, _plane_descriptor, _transpose_by_grad
from .blur import gaussian_taps
from .linear import LinearOperator

MAX_KERNEL_SIZE = 61


def psf_reflect_torch(x: Tensor, kernel: Tensor) -> Tensor:
    """Host (torch) form of the forward map on ``(..., C, H, W)`` for a square odd ``kernel``."""
    r = (kernel.shape[-1] - 1) // 2
    shape = x.shape
    planes = x.reshape(-1, 1, shape[-2], shape[-1])
    p = F.pad(planes, (r, r, r, r), mode="reflect")
    out = F.conv2d(p, kernel.to(x.dtype).view(1, 1, *kernel.shape))
    return out.reshape(shape)


def _square_kernel(kernel, max_size: int | None = None) -> Tensor:
    """``kernel`` as a finite fp32 ``(K, K)`` tensor, a rectangular one zero-padded and centred.
    With ``max_size`` both sizes are in ``[3, max_size]``; without, the larger is at least 3."""
    k = torch.as_tensor(np.asarray(kernel) if not isinstance(kernel, torch.Tensor) else kernel)
    k = k.detach().to(device="cpu", dtype=torch.float32)
    if k.ndim != 2:
        raise ValueError("kernel must be 2-D (Kh, Kw)")
    kh, kw = int(k.shape[0]), int(k.shape[1])
    if max_size is None:
        if kh % 2 != 1 or kw % 2 != 1 or max(kh, kw) < 3:
            raise ValueError(f"kernel sizes must be odd and the larger at least 3, got {(kh, kw)}")
    elif any(size % 2 != 1 or not (3 <= size <= max_size) for size in (kh, kw)):
        raise ValueError(f"kernel sizes must be odd and in [3, {max_size}], got {(kh, kw)}")
    if not bool(torch.isfinite(k).all()):
        raise ValueError("kernel values must be finite")
    size = max(kh, kw)
    out = torch.zeros(size, size, dtype=torch.float32)
    oy, ox = (size - kh) // 2, (size - kw) // 2
    out[oy:oy + kh, ox:ox + kw] = k
    return out


def _gaussian_psf(kernel_size: int, sigma: float, max_size: int | None = None) -> Tensor:
    """The isotropic Gaussian PSF as the outer product of ``gaussian_taps``, ``(K, K)`` fp32."""
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    if kernel_size % 2 != 1 or kernel_size < 3 or (max_size is not None and kernel_size > max_size):
        raise ValueError("kernel_size must be odd and " +
                         ("at least 3" if max_size is None else f"in [3, {max_size}]"))
    t = gaussian_taps(kernel_size, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


class PSFBlurOperator(LinearOperator):
    """Depthwise blur by a dense 2-D PSF with reflect padding; ``y`` has ``x_shape``."""

    def __init__(self, x_shape: Shape, kernel, device: Device = None) -> None:
        k = _square_kernel(kernel, MAX_KERNEL_SIZE)
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        r = k.shape[0] // 2
        if x_shape[-1] <= 2 * r or x_shape[-2] <= 2 * r:
            raise ValueError("image must be larger than the blur kernel for reflect padding")
        torch.nn.Module.__init__(self)
        self.kernel_size, self.radius = int(k.shape[0]), int(r)
        self.register_buffer("kernel", k.contiguous().to(device))
        self.x_shape = tuple(int(d) for d in x_shape)
        self.y_shape = self.x_shape

    @classmethod
    def gaussian(cls, x_shape: Shape, kernel_size: int = 61, sigma: float = 3.0,
                 device: Device = None) -> "PSFBlurOperator":
        """The isotropic Gaussian PSF as the outer product of ``gaussian_taps`` (the DPS
        paper's deblurring kernel is ``kernel_size=61, sigma=3``)."""
        return cls(x_shape, _gaussian_psf(kernel_size, sigma, MAX_KERNEL_SIZE), device=device)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipLinearMap.apply(self, x, False)
        return psf_reflect_torch(x, self.kernel)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipLinearMap.apply(self, y, True)
        return _transpose_by_grad(lambda x: psf_reflect_torch(x, self.kernel), y)

    def hip_descriptor(self) -> _hip.SpOp:
        d = _plane_descriptor(_hip.SP_OP_PSF, self.x_shape)
        d.taps = self.kernel.data_ptr()
        d.radius = self.radius
        return d


def motion_blur_kernel(kernel_size: int = 61, intensity: float = 0.5, seed: int = 0) -> Tensor:
    """A random motion-blur PSF: a random-walk camera trajectory through the centre of a
    ``kernel_size`` box, rasterised with bilinear weights; ``(K, K)`` fp32, non-negative, sum 1.

    Host only, computed in fp64 from ``numpy.random.default_rng(seed)``, so it is deterministic
    per seed.  ``intensity`` in [0, 1] sets how far the heading wanders per step; 0 gives a
    straight segment through the centre.
    """
    if kernel_size % 2 != 1 or not (3 <= kernel_size <= MAX_KERNEL_SIZE):
        raise ValueError(f"kernel_size must be odd and in [3, {MAX_KERNEL_SIZE}]")
    if not (0.0 <= intensity <= 1.0):
        raise ValueError("intensity must be in [0, 1]")
    rng = np.random.default_rng(seed)
    r = kernel_size // 2
    steps = 4 * kernel_size          # sub-pixel steps: the path is densely sampled
    step_len = 0.9 * r / (steps / 2)  # each half reaches at most 0.9 R from the centre
    theta0 = rng.uniform(0.0, 2.0 * np.pi)
    turns = rng.normal(0.0, 1.0, size=(2, steps // 2))

    def half(direction: float, turn: np.ndarray) -> np.ndarray:
        heading = theta0 + (np.pi if direction < 0 else 0.0) + \
            np.cumsum(turn) * intensity * (np.pi / 16.0)
        pts = np.cumsum(np.stack([np.sin(heading), np.cos(heading)], axis=1) * step_len, axis=0)
        return pts

    path = np.concatenate([half(-1.0, turns[0])[::-1], np.zeros((1, 2)), half(1.0, turns[1])])
    path = np.clip(path, -(r - 1e-9), r - 1e-9) + r  # (row, col) in [0, K-1)
    k = np.zeros((kernel_size, kernel_size), dtype=np.float64)
    i0 = np.floor(path).astype(np.int64)
    f = path - i0
    for dy in (0, 1):
        for dx in (0, 1):
            wgt = (f[:, 0] if dy else 1.0 - f[:, 0]) * (f[:, 1] if dx else 1.0 - f[:, 1])
            np.add.at(k, (np.minimum(i0[:, 0] + dy, kernel_size - 1),
                          np.minimum(i0[:, 1] + dx, kernel_size - 1)), wgt)
    k /= k.sum()
    return torch.from_numpy(k).to(torch.float32)


class MotionBlurOperator(PSFBlurOperator):
    """``PSFBlurOperator`` over ``motion_blur_kernel(kernel_size, intensity, seed)``."""

    def __init__(self, x_shape: Shape, kernel_size: int = 61, intensity: float = 0.5, seed: int = 0,
                 device: Device = None) -> None:
        super().__init__(x_shape, motion_blur_kernel(kernel_size, intensity, seed), device=device)
        self.intensity, self.seed = float(intensity), int(seed)
