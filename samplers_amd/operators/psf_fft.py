"""Point-spread-function blur through FFTs: the map of ``PSFBlurOperator`` without its radius
cap and with three boundary modes, for large dense PSFs (measured PSFs of 101² taps and more).

The reference ships no blur operator, so the semantics are defined here and pinned in fp64 by
``tests/psf_fft_ops.py``.  With the PSF ``h`` of shape ``(K, K)``, ``K = 2R + 1``:

* ``apply`` is the **correlation** of ``PSFBlurOperator`` on every channel plane (no kernel flip):
  ``y[c,i,j] = Σ_{u,v} h[u,v] · x̃[c, i+u−R, j+v−R]`` with ``x̃`` the image extended by ``R`` on both
  spatial axes according to ``padding``: ``"reflect"`` (edge sample not repeated), ``"circular"``
  (wrap-around) or ``"zeros"`` — ``F.pad`` with mode ``reflect``, ``circular`` or ``constant``;
  ``y_shape == x_shape``;
* ``apply_transpose`` is the exact adjoint: the zero-extended convolution with ``h``, then the
  padded margin folded back by the transpose of the extension (reflect: by mirror, circular: by
  wrap-around, zeros: cropped);
* ``1 ≤ R ≤ min(H, W) − 1`` and ``H + 2R, W + 2R ≤ 1024`` (``padded_size``): every pixel then
  has at most three fold pre-images per axis;
* the taps are used as given (any finite fp32 values, negative ones allowed, no normalisation);
* no pseudo-inverse: ``PGDMSampler`` rejects the operator as it rejects ``PSFBlurOperator``
  (``PeriodicBlurOperator`` in ``periodic.py`` is the circular map on an image whose own sizes are
  transform lengths, where the blur is diagonal and has a spectral pseudo-inverse).

On device tensors the maps run the ``SP_OP_PSF_FFT`` kernels (``csrc/sp_psf_fft.hip``: in-LDS row
and column FFTs of ``Nh × Nw`` points, a multiply with the PSF's spectrum, the boundary handled by
index functions while staging and folding); on host tensors plain ``F.conv2d``.  The spectrum is
computed once at construction, in fp64 on the host (``psf_spectrum``).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import MAX_SIZE, MIN_SIZE, HipWorkspaceMap, _plane_descriptor, _transpose_by_grad
from .linear import LinearOperator
from .psf import _gaussian_psf, _square_kernel

PADDINGS = ("reflect", "circular", "zeros")  # the descriptor's `factor`: 0, 1, 2
_PAD_MODE = {"reflect": "reflect", "circular": "circular", "zeros": "constant"}


def padded_size(n: int) -> int:
    """The transform length of an extended axis of ``n`` samples: the smallest ``2^k`` or
    ``3·2^k`` in ``[MIN_SIZE, MAX_SIZE]`` that is ``≥ n``; ``ValueError`` beyond ``MAX_SIZE``."""
    n = int(n)
    if n > MAX_SIZE:
        raise ValueError(f"extended size {n} exceeds the limit of {MAX_SIZE} (size + 2 * radius)")
    size = MIN_SIZE
    while True:
        for cand in (size, size + size // 2):
            if cand >= n:
                return cand
        size *= 2


def psf_spectrum(kernel, Nh: int, Nw: int) -> Tensor:
    """The half spectrum the ``SP_OP_PSF_FFT`` kernels read: the unnormalised ``fft2`` of the
    ``(K, K)`` PSF placed at ``[0, K) × [0, K)`` of an ``Nh × Nw`` zero array, computed in fp64 and
    rounded to fp32, as ``(re, im)`` pairs of shape ``(Nw // 2 + 1, Nh, 2)`` — the row transform's
    index ``kw ≤ Nw / 2`` slow, the column transform's ``kh`` fast."""
    k = np.asarray(kernel.detach().cpu().numpy() if isinstance(kernel, torch.Tensor) else kernel,
                   dtype=np.float64)
    if k.ndim != 2 or k.shape[0] > Nh or k.shape[1] > Nw:
        raise ValueError(f"a kernel of shape {k.shape} does not fit {Nh} x {Nw}")
    spec = np.fft.rfft2(k, s=(Nh, Nw))            # (Nh, Nw // 2 + 1)
    spec = np.ascontiguousarray(spec.T)           # (Nw // 2 + 1, Nh)
    out = np.stack([spec.real, spec.imag], axis=-1).astype(np.float32)
    return torch.from_numpy(out)


def psf_pad_torch(x: Tensor, kernel: Tensor, padding: str) -> Tensor:
    """Host (torch) form of the forward map on ``(..., C, H, W)`` for a square odd ``kernel``;
    differentiable."""
    r = (kernel.shape[-1] - 1) // 2
    shape = x.shape
    planes = x.reshape(-1, 1, shape[-2], shape[-1])
    p = F.pad(planes, (r, r, r, r), mode=_PAD_MODE[padding])
    out = F.conv2d(p, kernel.to(x.dtype).view(1, 1, *kernel.shape))
    return out.reshape(shape)


class FFTPSFBlurOperator(LinearOperator):
    """Depthwise blur by a dense 2-D PSF of any radius below the image size, with reflect,
    circular or zero padding, through FFTs; ``y`` has ``x_shape``."""

    # the descriptor has no sp_op_apply / sp_op_adjoint (its maps need a workspace): PSLD and
    # ReSample take their generic routes over apply / apply_transpose, both HIP here
    hip_linear = False

    def __init__(self, x_shape: Shape, kernel, padding: str = "reflect", device: Device = None) -> None:
        k = _square_kernel(kernel)
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        if padding not in PADDINGS:
            raise ValueError(f"padding must be one of {PADDINGS}, got {padding!r}")
        c, h, w = (int(d) for d in x_shape)
        r = int(k.shape[0]) // 2
        if not (1 <= r <= min(h, w) - 1):
            raise ValueError(f"the PSF radius must be in [1, min(H, W) - 1] = [1, {min(h, w) - 1}], "
                             f"got {r}")
        nh, nw = padded_size(h + 2 * r), padded_size(w + 2 * r)  # ValueError beyond MAX_SIZE
        torch.nn.Module.__init__(self)
        self.kernel_size, self.radius, self.padding = int(k.shape[0]), r, padding
        self.padded_shape = (nh, nw)
        self.register_buffer("kernel", k.contiguous().to(device))
        self.register_buffer("spectrum", psf_spectrum(k, nh, nw).contiguous().to(device))
        self.x_shape = (c, h, w)
        self.y_shape = self.x_shape

    @classmethod
    def gaussian(cls, x_shape: Shape, kernel_size: int = 61, sigma: float = 3.0,
                 padding: str = "reflect", device: Device = None) -> "FFTPSFBlurOperator":
        """The isotropic Gaussian PSF as the outer product of ``gaussian_taps``, as
        ``PSFBlurOperator.gaussian`` without its size cap."""
        return cls(x_shape, _gaussian_psf(kernel_size, sigma), padding=padding, device=device)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, False, False)
        return psf_pad_torch(x, self.kernel, self.padding)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, False, True)
        return _transpose_by_grad(lambda x: psf_pad_torch(x, self.kernel, self.padding), y)

    def hip_descriptor(self) -> _hip.SpOp:
        d = _plane_descriptor(_hip.SP_OP_PSF_FFT, self.x_shape)
        d.taps = self.spectrum.data_ptr()
        d.radius = self.radius
        d.factor = PADDINGS.index(self.padding)
        return d
