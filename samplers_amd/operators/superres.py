"""×s super-resolution operator (average-pool downsampling, s ∈ {2, 4, 8}).

The reference ships no super-resolution operator, so its semantics are defined here and
pinned in fp64 by ``tests/sr_ops.py``:

* ``apply`` is ``F.avg_pool2d(x, s)`` on every channel plane: ``y_shape = (C, H/s, W/s)``,
  ``H`` and ``W`` divisible by ``s``;
* ``apply_transpose`` is the exact adjoint: each ``y`` value divided by s² and replicated over
  its s×s block;
* ``apply_pseudo_inverse`` is A⁺ = s²·Aᵀ, the nearest-neighbour replication of ``y``
  (A A⁺ = I and A⁺A is the projection onto block-constant images), so ``PGDMSampler`` accepts
  the operator.  ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2·s²·Aᵀ(y − A x̂₀): ``pinv_grad_scale = 2 s²``.

1/s² is a power of two, so the scaling in A, Aᵀ and A⁺ is exact in fp32; only the s²-term
block sum rounds.  On device tensors the maps run the ``SP_OP_SR`` kernels
(``csrc/sp_sr.hip``), which sum every block in one fixed order, whatever the batch or shard.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import HipLinearMap, _hip_prox, _isometry_prox
from .linear import LinearOperator

FACTORS = (2, 4, 8)


class SuperResolutionOperator(LinearOperator):
    """s×s average pooling of every channel plane; ``y`` has shape ``(C, H/s, W/s)``."""

    def __init__(self, x_shape: Shape, factor: int = 4, device: Device = None) -> None:
        if factor not in FACTORS:
            raise ValueError(f"factor must be one of {FACTORS}, got {factor!r}")
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if min(c, h, w) <= 0 or h % factor or w % factor:
            raise ValueError(f"height and width must be positive multiples of the factor {factor}, "
                             f"got x_shape={tuple(x_shape)}")
        torch.nn.Module.__init__(self)  # no buffers: the operator is its shape and factor
        self.factor = int(factor)
        self.x_shape = (c, h, w)
        self.y_shape = (c, h // factor, w // factor)

    @property
    def pinv_grad_scale(self) -> float:
        """c in ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −c·Aᵀ(y − A x̂₀): 2·s² since A⁺ = s²·Aᵀ."""
        return 2.0 * self.factor * self.factor

    def _replicate(self, y: Tensor) -> Tensor:
        s = self.factor
        return y.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipLinearMap.apply(self, x, False)
        batch = x.shape[: x.ndim - 3]
        y = F.avg_pool2d(x.reshape(-1, *self.x_shape), self.factor)
        return y.reshape(*batch, *self.y_shape)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipLinearMap.apply(self, y, True)
        return self._replicate(y) / float(self.factor * self.factor)

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        if y.is_cuda:  # s² · Aᵀ y (exact scaling), differentiable like the adjoint
            return HipLinearMap.apply(self, y, True) * float(self.factor * self.factor)
        return self._replicate(y)

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """``z = x0 + (y − A x0 replicated over its block) / (1 + ρ s²)`` (A Aᵀ = I / s²);
        ``sp_op_prox_ws`` on device tensors."""
        if x0.is_cuda:
            return _hip_prox(self, x0, y, rho)
        return _isometry_prox(self, x0, y, rho, gram=1.0 / float(self.factor * self.factor))

    def hip_descriptor(self) -> _hip.SpOp:
        c, h, w = self.x_shape
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_SR
        d.channels, d.height, d.width = c, h, w
        d.n = int(math.prod(self.x_shape))
        d.m = int(math.prod(self.y_shape))
        d.factor = self.factor
        return d
