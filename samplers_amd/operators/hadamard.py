"""Compressed sensing on a scrambled Walsh–Hadamard transform: ``y = S·H·D·x`` on every channel
plane — the compressed-sensing task of the DDRM, ΠGDM and DDNM papers.

Per plane, with the flattened index ``i = h·W + w`` and ``n_p = H·W = 2^k`` (``6 ≤ k ≤ 20``),

    ``(A x)[c][r] = n_p^(−1/2) · Σ_i (−1)^popcount(j_r & i) · d[i] · x[c][i]``,

``j_r`` the r-th kept coefficient in ascending order (the natural, Sylvester, order of ``H``) and
``d ∈ {±1}^{n_p}`` a fixed sign vector; the kept set and ``d`` are shared by the channels and
``y`` has shape ``(C, m_p)``.  ``H`` is symmetric and orthogonal, so ``Aᵀ = D·H·Sᵀ``,
``A Aᵀ = I_m`` and ``A⁺ = Aᵀ``: a partial isometry whose SVD is ``U = I``, ``s = 1`` and ``Vᵀ`` the
transform itself.  Every sampler has an exact form for it: DPS and PGDM pass 1
(``pinv_grad_scale = 2``), the closed-form proximal map ``z = x0 + Aᵀ(y − A x0)/(1 + ρ)`` and the
DDRM step with one class for the whole kept set.

On device tensors the maps run the ``SP_OP_HADAMARD`` kernels (``csrc/sp_hadamard.hip``: add /
subtract levels in LDS), each an autograd function whose backward is its transpose; on host tensors
a reshape-butterfly transform in the tensor's dtype.  ``n_p^(−1/2)`` is applied once per transform:
a power of two for even ``k``, ``2^(−k/2)`` rounded to the tensor's dtype for odd ``k``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import HipWorkspaceMap, _hip_prox, _isometry_prox
from .inpainting import keep_bitmask
from .linear import SVDOperator

MIN_LOG2, MAX_LOG2 = 6, 20


def fwht(t: Tensor) -> Tensor:
    """The unnormalised Walsh–Hadamard transform (natural order) of the last axis, a power of two
    long, by reshape butterflies in the tensor's dtype."""
    n = t.shape[-1]
    lead = t.shape[:-1]
    h = 1
    while h < n:
        v = t.reshape(*lead, n // (2 * h), 2, h)
        a, b = v[..., 0, :], v[..., 1, :]
        t = torch.stack((a + b, a - b), dim=-2).reshape(*lead, n)
        h *= 2
    return t


class HadamardOperator(SVDOperator):
    """``y = S·H·D·x`` per channel plane (module docstring): ``kept`` a bool mask over ``n_p`` or an
    index tensor (default: ``round(ratio·n_p)`` indices drawn from a CPU ``torch.Generator(seed)``),
    ``signs`` ``True`` (drawn from the same generator, after the kept set), ``False`` / ``None``
    (all +1) or a ±1 tensor of ``n_p`` values."""

    # the maps need a workspace, so PSLD and ReSample take their generic routes
    hip_linear = False
    # ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2 Aᵀ(y − A x̂₀)
    pinv_grad_scale = 2.0

    def __init__(self, x_shape: Shape, ratio: float = 0.25, seed: int = 0, kept=None, signs=True,
                 device: Device = None) -> None:
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if c < 1 or h < 1 or w < 1:
            raise ValueError(f"x_shape must be positive, got {tuple(x_shape)}")
        n_p = h * w
        if n_p & (n_p - 1):
            raise ValueError(f"the plane size H·W must be a power of two, got {h}·{w} = {n_p}")
        k = n_p.bit_length() - 1
        if not MIN_LOG2 <= k <= MAX_LOG2:
            raise ValueError(f"k = log2(H·W) out of range: must be in [{MIN_LOG2}, {MAX_LOG2}], got {k}")
        gen = torch.Generator().manual_seed(int(seed))
        if kept is None:
            if not 0.0 < float(ratio) <= 1.0:
                raise ValueError(f"ratio must be in (0, 1], got {ratio}")
            m_p = int(round(float(ratio) * n_p))
            keep = torch.zeros(n_p, dtype=torch.bool)
            keep[torch.randperm(n_p, generator=gen)[:m_p]] = True
        else:
            kt = torch.as_tensor(kept).detach().cpu()
            if kt.dtype == torch.bool:
                if kt.numel() != n_p:
                    raise ValueError(f"kept has the wrong length: a mask must have {n_p} entries, "
                                     f"got {kt.numel()}")
                keep = kt.reshape(-1).clone()
            else:
                idx = kt.reshape(-1).to(torch.int64)
                if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n_p):
                    raise ValueError(f"kept indices must be in [0, {n_p}), the wrong length of plane")
                keep = torch.zeros(n_p, dtype=torch.bool)
                keep[idx] = True
        if not bool(keep.any()):
            raise ValueError("the kept set is empty: at least one coefficient must be observed")
        if signs is True:
            d = torch.randint(0, 2, (n_p,), generator=gen).to(torch.float32) * 2.0 - 1.0
        elif signs is False or signs is None:
            d = None
        else:
            d = torch.as_tensor(signs).detach().cpu().reshape(-1).to(torch.float32)
            if d.numel() != n_p:
                raise ValueError(f"signs has the wrong length: {n_p} values expected, got {d.numel()}")
            if not bool((d.abs() == 1.0).all()):
                raise ValueError("signs must be ±1")
        torch.nn.Module.__init__(self)
        self.log2_plane = k
        self.x_shape = (c, h, w)
        m_p = int(keep.sum())
        self.y_shape = (c, m_p)
        bits, rank = keep_bitmask(keep.numpy())
        self.register_buffer("keep", keep.to(device))
        self.register_buffer("kept_indices", torch.nonzero(keep, as_tuple=False).squeeze(1).to(device))
        self.register_buffer("signs", None if d is None else d.contiguous().to(device))
        self.register_buffer("_keep_bits", torch.from_numpy(bits.view(np.int64)).to(device))
        self.register_buffer("_word_rank", torch.from_numpy(rank).to(device))
        self.register_buffer("_singular_values", torch.ones(self.y_shape, dtype=torch.float32, device=device))

    @property
    def shape(self) -> tuple[int, int]:
        return int(math.prod(self.y_shape)), int(math.prod(self.x_shape))

    def get_singular_values(self) -> Tensor:
        return self._singular_values

    # ---- host maps: reshape butterflies in the tensor's dtype ----
    def _scale(self, t: Tensor) -> Tensor:
        return torch.tensor(2.0 ** (-self.log2_plane / 2.0), dtype=t.dtype)

    def _host_apply(self, x: Tensor) -> Tensor:
        c, h, w = self.x_shape
        v = x.reshape(*x.shape[:-2], h * w)
        if self.signs is not None:
            v = v * self.signs.to(v)
        return (self._scale(v) * fwht(v))[..., self.kept_indices.to(v.device)]

    def _host_transpose(self, y: Tensor) -> Tensor:
        c, h, w = self.x_shape
        full = torch.zeros(*y.shape[:-1], h * w, dtype=y.dtype, device=y.device)
        full[..., self.kept_indices.to(y.device)] = y
        v = self._scale(full) * fwht(full)
        if self.signs is not None:
            v = v * self.signs.to(v)
        return v.reshape(*y.shape[:-1], h, w)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, False, False)
        return self._host_apply(x)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, False, True)
        return self._host_transpose(y)

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, True, False)
        return self._host_transpose(y)

    def apply_pseudo_inverse_transpose(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, True, True)
        return self._host_apply(x)

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """``z = x0 + Aᵀ(y − A x0) / (1 + ρ)`` (A Aᵀ = I): ``sp_op_prox_ws`` on device tensors."""
        if x0.is_cuda:
            return _hip_prox(self, x0, y, rho)
        return _isometry_prox(self, x0, y.to(x0.dtype), rho)

    # ---- the SVD: U = I, s = 1, Vᵀ = A ----
    def apply_U(self, z: Tensor) -> Tensor:
        return z

    def apply_U_transpose(self, y: Tensor) -> Tensor:
        return y

    def apply_V_transpose(self, x: Tensor) -> Tensor:
        return self.apply(x)

    def apply_V(self, z: Tensor) -> Tensor:
        return self.apply_transpose(z)

    def hip_descriptor(self) -> _hip.SpOp:
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_HADAMARD
        d.channels, d.height, d.width = self.x_shape
        d.n, d.m = int(math.prod(self.x_shape)), int(math.prod(self.y_shape))
        d.keep_bits = self._keep_bits.data_ptr()
        d.word_rank = self._word_rank.data_ptr()
        d.taps = None if self.signs is None else self.signs.data_ptr()
        d.radius = d.factor = 0
        return d
