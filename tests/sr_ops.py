"""fp64 semantics of the ×s super-resolution operator — TEST INFRASTRUCTURE ONLY.

The reference has no super-resolution operator.  What ``SuperResolutionOperator`` and the
``SP_OP_SR`` kernels implement is pinned here by plain torch: ``F.avg_pool2d(x, s)`` per channel
plane in float64, the adjoint by autograd of that map (the exact transpose by construction),
and the pseudo-inverse A⁺ = s²·Aᵀ (nearest-neighbour replication).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def pool(x: torch.Tensor, s: int) -> torch.Tensor:
    """A x on (B, C, H, W) in x's dtype (differentiable: the oracle loops run it in fp32 / fp64)."""
    return F.avg_pool2d(x, s)


def replicate(y: torch.Tensor, s: int) -> torch.Tensor:
    """A⁺ y = s²·Aᵀ y: every y value over its s×s block."""
    return y.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)


def adjoint_closed(y: torch.Tensor, s: int) -> torch.Tensor:
    """Aᵀ y in closed form (differentiable in y, for loops that backpropagate through Aᵀ)."""
    return replicate(y, s) / (s * s)


def apply64(x: torch.Tensor, s: int) -> torch.Tensor:
    """Forward map on (B, C, H, W) in float64."""
    return pool(x.to(torch.float64), s)


def adjoint64(y: torch.Tensor, s: int) -> torch.Tensor:
    """Aᵀ y in float64 by autograd of the forward map; y is (B, C, H/s, W/s)."""
    shape = (*y.shape[:-2], y.shape[-2] * s, y.shape[-1] * s)
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(apply64(x, s), x, grad_outputs=y.to(torch.float64))
    return g


def sr_ops(shape: tuple, s: int):
    """(apply, adjoint) on flat (B, n) / (B, m) float64 numpy arrays for oracle.closed_form."""
    c, h, w = shape

    def apply(x: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(x.shape[0], c, h, w))
        return apply64(t, s).reshape(x.shape[0], -1).numpy()

    def adjoint(y: np.ndarray) -> np.ndarray:
        t = torch.from_numpy(
            np.ascontiguousarray(y, dtype=np.float64).reshape(y.shape[0], c, h // s, w // s))
        return adjoint64(t, s).reshape(y.shape[0], -1).numpy()

    return apply, adjoint
