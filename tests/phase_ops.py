"""fp64 semantics of Fourier phase retrieval — TEST INFRASTRUCTURE ONLY.

The reference has no such operator.  What ``PhaseRetrievalOperator`` and the ``SP_OP_PHASE``
kernels implement is pinned here in float64 (torch on the CPU): per channel plane

    y = |fft2(zero_pad(x), norm="ortho")|       unshifted, DC at [0, 0]

with ``pad_h`` zero rows above and below and ``pad_w`` zero columns left and right, and the
Jacobian-transpose product of a y-space cotangent ``g`` in closed form,

    J(x)^T g = crop(Re(ifft2(g * z / |z|, norm="ortho"))),   z = fft2(pad(x)),  z/|z| := 0 at 0

(``tests/test_phase_api.py`` pins the closed form to torch's fp64 autograd of the forward map).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _pads(pad) -> tuple[int, int]:
    if isinstance(pad, (tuple, list)):
        return int(pad[0]), int(pad[1])
    return int(pad), int(pad)


def spectrum(x: torch.Tensor, pad) -> torch.Tensor:
    """z = fft2(zero_pad(x), ortho) on (..., C, H, W) in x's precision (differentiable)."""
    ph, pw = _pads(pad)
    return torch.fft.fft2(F.pad(x, (pw, pw, ph, ph)), norm="ortho")


def amplitude(x: torch.Tensor, pad) -> torch.Tensor:
    """The forward map in x's dtype (differentiable: the oracle loops run it in fp32 / fp64)."""
    return spectrum(x, pad).abs()


def apply64(x: torch.Tensor, pad) -> torch.Tensor:
    return amplitude(x.detach().to(torch.float64), pad)


def vjp64(x: torch.Tensor, g: torch.Tensor, pad) -> torch.Tensor:
    """J(x)^T g in float64 by the closed form."""
    ph, pw = _pads(pad)
    z = spectrum(x.detach().to(torch.float64), pad)
    u = g.detach().to(torch.float64) * torch.sgn(z)
    full = torch.fft.ifft2(u, norm="ortho").real
    h, w = x.shape[-2:]
    return full[..., ph:ph + h, pw:pw + w]


def phase_ops(shape: tuple, pad):
    """(apply, vjp) on flat float64 numpy arrays: ``apply(x)`` is (B, n) -> (B, m) as
    ``oracle.closed_form`` expects; ``vjp(x, g)`` takes the place of the linear kinds' adjoint
    and is evaluated at the point ``x``."""
    c, h, w = shape

    def apply(x: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], c, h, w))
        return apply64(t, pad).reshape(x.shape[0], -1).numpy()

    def vjp(x: np.ndarray, g: np.ndarray) -> np.ndarray:
        ph, pw = _pads(pad)
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], c, h, w))
        gt = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float64).reshape(
            g.shape[0], c, h + 2 * ph, w + 2 * pw))
        return vjp64(t, gt, pad).reshape(x.shape[0], -1).numpy()

    return apply, vjp


def residual_pass64(x, eps, y_rows, y_div: int, a: float, k: float, gs: float, apply, vjp):
    """``oracle.closed_form.residual_pass`` for a nonlinear operator: (v, ||r_b||^2) with
    x0 = (x - k eps) / a, r = y - A(x0), v = J(x0)^T (gs r)."""
    x = np.asarray(x, dtype=np.float64)
    eps = np.asarray(eps, dtype=np.float64)
    x0 = (x - k * eps) / a
    rows = np.arange(x.shape[0]) // y_div
    r = np.asarray(y_rows, dtype=np.float64)[rows] - apply(x0)
    return vjp(x0, gs * r), (r.reshape(r.shape[0], -1) ** 2).sum(axis=1)
