"""fp64 semantics of the FFT-domain point-spread-function blur — TEST INFRASTRUCTURE ONLY.

The reference has no blur operator.  What ``FFTPSFBlurOperator`` and the ``SP_OP_PSF_FFT`` kernels
implement is pinned here by plain torch in float64: ``F.pad`` by R on both spatial axes with mode
``reflect``, ``circular`` or ``constant`` (``padding`` = "reflect", "circular", "zeros"), then a
depthwise 2-D **correlation** with the (K, K) PSF (``F.conv2d``, no kernel flip); the adjoint is
autograd of that map (the exact transpose by construction: the zero-extended convolution, then the
margin folded back by the transpose of the extension).

``route="fft"`` evaluates the same correlation of the padded image through ``torch.fft`` (fp64,
differentiable), for the large cases where the direct route takes seconds to minutes on the CPU;
``tests/test_psf_fft_api.py`` pins it to the direct route.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

PADDINGS = ("reflect", "circular", "zeros")
_MODE = {"reflect": "reflect", "circular": "circular", "zeros": "constant"}


def _h64(h) -> torch.Tensor:
    h = torch.as_tensor(np.asarray(h) if not isinstance(h, torch.Tensor) else h)
    assert h.ndim == 2 and h.shape[0] == h.shape[1] and h.shape[0] % 2 == 1, tuple(h.shape)
    return h.detach().cpu().to(torch.float64)


def blur(x: torch.Tensor, h, padding: str = "reflect", route: str = "direct") -> torch.Tensor:
    """A x on (..., C, H, W) in x's dtype (differentiable: the oracle loops run it in fp32 / fp64)."""
    hk = _h64(h).to(x.dtype)
    k = hk.shape[0]
    r = k // 2
    shp = x.shape
    planes = x.reshape(-1, 1, shp[-2], shp[-1])
    p = F.pad(planes, (r, r, r, r), mode=_MODE[padding])
    if route == "direct":
        return F.conv2d(p, hk.view(1, 1, k, k)).reshape(shp)
    assert route == "fft", route
    size = p.shape[-2:]
    spec = torch.fft.rfft2(p, s=size) * torch.fft.rfft2(hk, s=size).conj()
    return torch.fft.irfft2(spec, s=size)[..., : shp[-2], : shp[-1]].reshape(shp)


def adjoint(y: torch.Tensor, h, padding: str = "reflect", route: str = "direct") -> torch.Tensor:
    """Aᵀ y by autograd of the forward map; differentiable in y (create_graph), so loops that
    backpropagate through Aᵀ (PSLD's x_eff) see the exact transpose."""
    x = torch.zeros_like(y, requires_grad=True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(blur(x, h, padding, route), x, grad_outputs=y,
                                   create_graph=y.requires_grad)
    return g


def apply64(x: torch.Tensor, h, padding: str = "reflect", route: str = "direct") -> torch.Tensor:
    """Forward map on (..., C, H, W) in float64."""
    return blur(x.to(torch.float64), h, padding, route)


def adjoint64(y: torch.Tensor, h, padding: str = "reflect", route: str = "direct") -> torch.Tensor:
    """Aᵀ y in float64 by autograd of ``apply64``."""
    return adjoint(y.detach().to(torch.float64), h, padding, route)


def psf_ops(shape: tuple, h, padding: str = "reflect", route: str = "direct"):
    """(apply, adjoint) on flat (B, n) float64 numpy arrays for oracle.closed_form."""

    def apply(x: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], *shape))
        return apply64(t, h, padding, route).reshape(x.shape[0], -1).numpy()

    def adj(y: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64).reshape(y.shape[0], *shape))
        return adjoint64(t, h, padding, route).reshape(y.shape[0], -1).numpy()

    return apply, adj


def source_index(n: int, d: int, padding: str):
    """(index, valid) of x̃[i + d] for i < n along an axis of n pixels extended by ``padding``:
    reflect mirrors about the edge sample, circular wraps, zeros has no source outside."""
    i = torch.arange(n) + d
    inside = (i >= 0) & (i < n)
    if padding == "reflect":
        j = torch.where(i < 0, -i, i)
        j = torch.where(j >= n, 2 * (n - 1) - j, j)
        return j, torch.ones(n, dtype=torch.bool)
    if padding == "circular":
        return i % n, torch.ones(n, dtype=torch.bool)
    assert padding == "zeros", padding
    return i.clamp(0, n - 1), inside


def shifted(x: torch.Tensor, dy: int, dx: int, padding: str = "reflect") -> torch.Tensor:
    """out[..., i, j] = x̃[..., i + dy, j + dx] (what a delta PSF at (R + dy, R + dx) computes)."""
    h, w = x.shape[-2:]
    iy, vy = source_index(h, dy, padding)
    ix, vx = source_index(w, dx, padding)
    out = x[..., iy, :][..., ix]
    return out * (vy[:, None] & vx[None, :]).to(x.dtype)
