"""fp64 semantics of the periodic blur and its spectral pseudo-inverse — TEST INFRASTRUCTURE ONLY.

The reference has no blur operator.  What ``PeriodicBlurOperator`` and the ``SP_OP_PSF_PERIODIC``
kernels implement is pinned here by plain torch in float64:

* ``blur`` — the direct wrap-around correlation, ``F.pad(mode="circular")`` by R then ``F.conv2d``
  with the (K, K) PSF (no flip); ``route="fft"`` evaluates the same map as
  ``Re ifft2(fft2(x) · M)`` with the transfer function ``M`` (``transfer``);
* ``adjoint`` — autograd of ``blur`` (the exact transpose by construction);
* ``transfer`` — ``M = conj(fft2(h_c))``, ``h_c`` the PSF with its centre tap at ``[0, 0]``;
* ``pinv`` — ``A⁺ y = Re ifft2(fft2(y) · P)`` with ``P = keep ? 1/M : 0`` for a **given** keep
  mask.  The tests pass the operator's own ``keep``, so a frequency at the threshold can never be
  decided differently by the test and by the code;
* ``pgdm_grad`` — ``∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖²`` in closed form, ``−2 (A⁺y − Π x̂₀)``, and
  ``pgdm_grad_autograd`` — the same by autograd of the reference's loss (``pgdm.py:110-115``).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _h64(h) -> torch.Tensor:
    h = torch.as_tensor(np.asarray(h) if not isinstance(h, torch.Tensor) else h)
    assert h.ndim == 2 and h.shape[0] == h.shape[1] and h.shape[0] % 2 == 1, tuple(h.shape)
    return h.detach().cpu().to(torch.float64)


def transfer(h, H: int, W: int) -> torch.Tensor:
    """M (complex128, (H, W)): tap (u, v) placed at ((u − R) mod H, (v − R) mod W), transformed,
    conjugated."""
    hk = _h64(h)
    k = hk.shape[0]
    r = k // 2
    assert k <= H and k <= W, (k, H, W)
    hc = torch.zeros(H, W, dtype=torch.float64)
    for u in range(k):
        for v in range(k):
            hc[(u - r) % H, (v - r) % W] += hk[u, v]
    return torch.fft.fft2(hc).conj()


def _mul(x: torch.Tensor, spec: torch.Tensor) -> torch.Tensor:
    """Re ifft2(fft2(x) · spec) on (..., H, W) in x's precision (differentiable)."""
    cd = torch.complex128 if x.dtype == torch.float64 else torch.complex64
    return torch.fft.ifft2(torch.fft.fft2(x) * spec.to(cd)).real.to(x.dtype)


def blur(x: torch.Tensor, h, route: str = "direct") -> torch.Tensor:
    """A x on (..., C, H, W) in x's dtype (differentiable)."""
    hk = _h64(h).to(x.dtype)
    k = hk.shape[0]
    r = k // 2
    shp = x.shape
    if route == "fft":
        return _mul(x, transfer(h, shp[-2], shp[-1]))
    assert route == "direct", route
    planes = x.reshape(-1, 1, shp[-2], shp[-1])
    p = F.pad(planes, (r, r, r, r), mode="circular")
    return F.conv2d(p, hk.view(1, 1, k, k)).reshape(shp)


def adjoint(y: torch.Tensor, h, route: str = "direct") -> torch.Tensor:
    """Aᵀ y by autograd of the forward map."""
    x = torch.zeros_like(y, requires_grad=True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(blur(x, h, route), x, grad_outputs=y,
                                   create_graph=y.requires_grad)
    return g


def apply64(x, h, route="direct"):
    return blur(x.to(torch.float64), h, route)


def adjoint64(y, h, route="direct"):
    return adjoint(y.detach().to(torch.float64), h, route)


def pinv_spectrum(h, keep: torch.Tensor) -> torch.Tensor:
    """P = keep ? 1/M : 0 (complex128) for the given (H, W) bool mask."""
    keep = keep.detach().cpu().bool()
    m = transfer(h, *keep.shape)
    p = torch.zeros_like(m)
    p[keep] = 1.0 / m[keep]
    return p


def pinv(y: torch.Tensor, h, keep: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """A⁺ y (or A⁺ᵀ y: the multiplier conj(P)) on (..., C, H, W) in y's dtype (differentiable)."""
    p = pinv_spectrum(h, keep)
    return _mul(y, p.conj() if transpose else p)


def projection(x: torch.Tensor, keep: torch.Tensor) -> torch.Tensor:
    """Π x = A⁺ A x: the kept frequencies of x."""
    return _mul(x, keep.detach().cpu().to(torch.complex128))


def pgdm_grad(x0: torch.Tensor, y: torch.Tensor, h, keep: torch.Tensor) -> torch.Tensor:
    """−2 (A⁺y − Π x̂₀)."""
    return -2.0 * (pinv(y, h, keep) - projection(x0, keep))


def pgdm_grad_autograd(x0: torch.Tensor, y: torch.Tensor, h, keep: torch.Tensor,
                       route: str = "direct") -> torch.Tensor:
    """autograd of ‖A⁺y − A⁺(A x̂₀)‖² in x̂₀ (the reference's consistency loss)."""
    x = x0.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        loss = (pinv(y, h, keep) - pinv(blur(x, h, route), h, keep)).pow(2).sum()
        (g,) = torch.autograd.grad(loss, x)
    return g


def periodic_ops(shape: tuple, h, route: str = "direct"):
    """(apply, adjoint) on flat (B, n) float64 numpy arrays for oracle.closed_form."""

    def apply(x: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], *shape))
        return apply64(t, h, route).reshape(x.shape[0], -1).numpy()

    def adj(y: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64).reshape(y.shape[0], *shape))
        return adjoint64(t, h, route).reshape(y.shape[0], -1).numpy()

    return apply, adj
