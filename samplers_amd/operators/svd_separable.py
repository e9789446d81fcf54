"""Separable-SVD operator: ``A X = A_H X A_Wᵀ`` on every channel plane, with two small dense
matrices ``A_H`` (Hy × H) and ``A_W`` (Wy × W) — the construction of the DDRM paper's deblurring
operators.  Any blur under any boundary rule and any filter-and-decimate super-resolution is of
this form; the SVDs of the two 1-D factors give the whole operator's SVD,

    ``A = (U_H ⊗ U_W) · diag(s_H[i]·s_W[j]) · (V_H ⊗ V_W)ᵀ``,

for any sizes (no transform lengths, no periodic boundaries).  With ``T(X) = V_Hᵀ X V_W`` (the top
left ``Hy × Wy`` block of which is the observed grid), ``T_y(Y) = U_Hᵀ Y U_W`` and
``S[i,j] = s_H[i]·s_W[j]``:

* ``apply``: ``U_H (S ⊙ T(x)[:Hy,:Wy]) U_Wᵀ``, ``apply_transpose`` its exact transpose (the full S);
* the kept set is ``S > rtol·max S`` (``rtol = 3e-2`` is DDRM's threshold for deblurring);
  ``apply_pseudo_inverse`` has the multiplier ``P = 1/S`` there and 0 elsewhere: ``A⁺A`` is an
  orthogonal projection, ``A⁺AA⁺ = A⁺``, ``pinv_grad_scale = 2`` (as ``PeriodicBlurOperator``);
* ``apply_prox``: ``z = T⁻¹[(S ⊙ T_y(y) + ρ T(x0)) / (S² + ρ)]`` on the observed grid and ``T(x0)``
  itself outside it: exact for the full A, every component divided;
* the thin ``SVDOperator`` interface: ``apply_V_transpose`` is the observed block of ``T``,
  ``get_singular_values()`` is S with the dropped components set to 0 (the spectrum the
  pseudo-inverse and DDRM see), ``singular_values_full`` is S.

The SVDs are taken once at construction in fp64 on the host with a deterministic sign (the
largest-magnitude entry of every column of V is positive, U follows) and rounded to fp32; the map
is defined by the fp32 tables taken as exact.  On device tensors A, Aᵀ, A⁺ and A⁺ᵀ run the
``SP_OP_SVD_SEPARABLE`` kernels (``csrc/sp_svd_sep.hip``), each an autograd function whose backward
is its transpose; on host tensors every map is a pair of ``torch.matmul`` in the tensor's dtype.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import HipWorkspaceMap, _hip_prox, check_rho
from .blur import gaussian_taps
from .linear import SVDOperator
from .sr_filter import FACTORS, bicubic_taps

MIN_SIZE, MAX_SIZE = 2, 512


def reflect_blur_matrix(taps, size: int) -> np.ndarray:
    """The dense (size × size) fp64 matrix of the 1-D correlation with ``taps`` (odd count,
    ``2R + 1``, ``size > 2R``) on the reflect-padded axis (``F.pad(mode="reflect")``: the edge
    sample is not repeated): one axis of ``GaussianBlurOperator``'s map."""
    t = np.asarray(taps, dtype=np.float64).reshape(-1)
    if t.size % 2 != 1:
        raise ValueError(f"the number of taps must be odd, got {t.size}")
    r = t.size // 2
    if size <= 2 * r:
        raise ValueError(f"the axis must be longer than 2R = {2 * r} for reflect padding, got {size}")
    a = np.zeros((size, size), dtype=np.float64)
    for i in range(size):
        for u in range(t.size):
            g = i + u - r
            g = -g if g < 0 else (2 * (size - 1) - g if g >= size else g)
            a[i, g] += t[u]
    return a


def symmetric_decimate_matrix(taps, size: int, factor: int) -> np.ndarray:
    """The dense (size/factor × size) fp64 matrix of one axis of ``sr_filter.py``'s map: ``taps``
    (``K``, ``K − factor`` even) at stride ``factor`` on the symmetric extension (edge sample
    repeated), window offset ``P = (K − factor)/2``."""
    t = np.asarray(taps, dtype=np.float64).reshape(-1)
    k, s = t.size, int(factor)
    if s < 1 or size % s:
        raise ValueError(f"the factor must divide the axis, got {size} and {factor}")
    if k < s or (k - s) % 2:
        raise ValueError(f"the number of taps K must be >= the factor with K − s even, got K={k}, s={s}")
    p = (k - s) // 2
    if size < max(1, p):
        raise ValueError(f"the axis must be at least the pad P = {p}, got {size}")
    a = np.zeros((size // s, size), dtype=np.float64)
    for i in range(size // s):
        for u in range(k):
            g = s * i + u - p
            g = -1 - g if g < 0 else (2 * size - 1 - g if g >= size else g)
            a[i, g] += t[u]
    return a


def factor_svd(a: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(U, s, V)`` of a (rows × cols, rows ≤ cols) fp64 matrix: ``U`` (rows × rows) and ``V``
    (cols × cols, full: the right singular vectors by descending singular value, then the
    null-space completion) orthogonal, ``a = U[:, :rows] diag(s) V[:, :rows]ᵀ``; the
    largest-magnitude entry of every column of V is positive (the first of equals) and U follows."""
    u, s, vh = np.linalg.svd(np.asarray(a, dtype=np.float64), full_matrices=True)
    v = vh.T.copy()
    idx = np.argmax(np.abs(v), axis=0)
    sign = np.where(v[idx, np.arange(v.shape[1])] < 0, -1.0, 1.0)
    v *= sign
    u = u * sign[: u.shape[1]]
    return u, s, v


def _factor(name: str, a, size: int) -> np.ndarray:
    m = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != size:
        raise ValueError(f"{name} must be a 2-D matrix with {size} columns, got shape {m.shape}")
    if not 1 <= m.shape[0] <= size:
        raise ValueError(f"{name} must have between 1 and {size} rows, got {m.shape[0]}")
    if not np.isfinite(m).all():
        raise ValueError(f"{name} must be finite")
    return m


class SeparableSVDOperator(SVDOperator):
    """``A X = A_h X A_wᵀ`` on every channel plane through the SVDs of ``A_h`` (Hy × H) and
    ``A_w`` (Wy × W); ``y`` has shape ``(C, Hy, Wy)`` (module docstring)."""

    # the maps need a workspace, so PSLD and ReSample take their generic routes
    hip_linear = False
    # ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −2 (A⁺y − Π x̂₀)
    pinv_grad_scale = 2.0

    def __init__(self, x_shape: Shape, A_h, A_w, rtol: float = 3e-2, device: Device = None) -> None:
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if c < 1 or not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
            raise ValueError(f"H and W must be in [{MIN_SIZE}, {MAX_SIZE}] and C positive, got "
                             f"x_shape={tuple(x_shape)}")
        if not 0.0 < float(rtol) < 1.0:
            raise ValueError(f"rtol must be in (0, 1), got {rtol}")
        ah, aw = _factor("A_h", A_h, h), _factor("A_w", A_w, w)
        uh, sh, vh = factor_svd(ah)
        uw, sw, vw = factor_svd(aw)
        s = np.outer(sh, sw)
        if not s.max() > 0.0:
            raise ValueError("A_h and A_w must be non-zero")
        keep = s > float(rtol) * s.max()
        p = np.zeros_like(s)
        p[keep] = 1.0 / s[keep]
        torch.nn.Module.__init__(self)
        self.rtol = float(rtol)
        self.x_shape, self.y_shape = (c, h, w), (c, ah.shape[0], aw.shape[0])
        tables = [vh, vw, uh, uw, s, p]
        self._sizes = [t.shape for t in tables]
        # the descriptor's taps: V_H, V_W, U_H, U_W, S, P, row-major, back to back
        flat = np.concatenate([t.reshape(-1) for t in tables]).astype(np.float32)
        self.register_buffer("tables", torch.from_numpy(flat).contiguous().to(device))
        self.register_buffer("keep", torch.from_numpy(keep).contiguous().to(device))

    # ---- convenience constructors ----
    @classmethod
    def from_taps(cls, x_shape: Shape, taps_h, taps_w, rtol: float = 3e-2,
                  device: Device = None) -> "SeparableSVDOperator":
        """An anisotropic reflect-padded blur: ``taps_h`` along the rows, ``taps_w`` along the
        columns (odd counts, used as given)."""
        _, h, w = (int(d) for d in x_shape)
        return cls(x_shape, reflect_blur_matrix(_taps(taps_h), h), reflect_blur_matrix(_taps(taps_w), w),
                   rtol=rtol, device=device)

    @classmethod
    def gaussian_blur(cls, x_shape: Shape, kernel_size: int = 9, sigma: float = 3.0,
                      rtol: float = 3e-2, device: Device = None) -> "SeparableSVDOperator":
        """The map of ``GaussianBlurOperator(x_shape, kernel_size, sigma)``: its fp32 taps, reflect
        padding."""
        if kernel_size % 2 != 1 or kernel_size < 3:
            raise ValueError("kernel_size must be odd and at least 3")
        if sigma <= 0:
            raise ValueError("sigma must be positive")
        t = gaussian_taps(kernel_size, sigma)
        return cls.from_taps(x_shape, t, t, rtol=rtol, device=device)

    @classmethod
    def uniform_blur(cls, x_shape: Shape, kernel_size: int = 9, rtol: float = 3e-2,
                     device: Device = None) -> "SeparableSVDOperator":
        """The box blur of ``kernel_size`` (odd) taps ``1 / kernel_size``, reflect padding."""
        if kernel_size % 2 != 1 or kernel_size < 3:
            raise ValueError("kernel_size must be odd and at least 3")
        t = torch.full((kernel_size,), 1.0 / kernel_size, dtype=torch.float64).to(torch.float32)
        return cls.from_taps(x_shape, t, t, rtol=rtol, device=device)

    @classmethod
    def filtered_sr(cls, x_shape: Shape, taps, factor: int = 4, rtol: float = 3e-2,
                    device: Device = None) -> "SeparableSVDOperator":
        """The map of ``FilteredSuperResolutionOperator(x_shape, taps, factor)``: ``taps`` at stride
        ``factor`` on the symmetric extension of both axes."""
        if factor not in FACTORS:
            raise ValueError(f"factor must be one of {FACTORS}, got {factor!r}")
        _, h, w = (int(d) for d in x_shape)
        t = _taps(taps)
        return cls(x_shape, symmetric_decimate_matrix(t, h, factor), symmetric_decimate_matrix(t, w, factor),
                   rtol=rtol, device=device)

    @classmethod
    def bicubic_sr(cls, x_shape: Shape, factor: int = 4, rtol: float = 3e-2,
                   device: Device = None) -> "SeparableSVDOperator":
        """Antialiased bicubic ×1/factor: ``filtered_sr`` with ``bicubic_taps(factor)``."""
        return cls.filtered_sr(x_shape, bicubic_taps(factor), factor, rtol=rtol, device=device)

    # ---- the tables ----
    def _table(self, i: int) -> Tensor:
        off = sum(int(np.prod(s)) for s in self._sizes[:i])
        return self.tables[off: off + int(np.prod(self._sizes[i]))].view(*self._sizes[i])

    V_h = property(lambda self: self._table(0))
    V_w = property(lambda self: self._table(1))
    U_h = property(lambda self: self._table(2))
    U_w = property(lambda self: self._table(3))
    singular_values_full = property(lambda self: self._table(4))
    pinv_multiplier = property(lambda self: self._table(5))

    @property
    def shape(self) -> tuple[int, int]:
        return int(math.prod(self.y_shape)), int(math.prod(self.x_shape))

    def get_singular_values(self) -> Tensor:
        s = self.singular_values_full
        return torch.where(self.keep, s, torch.zeros_like(s))

    # ---- host maps: pairs of matmuls in the tensor's dtype ----
    def _hy_wy(self) -> tuple[int, int]:
        return self.y_shape[1], self.y_shape[2]

    def _host_only(self, t: Tensor) -> None:
        if t.is_cuda:
            raise NotImplementedError(f"{type(self).__name__}: apply_V / apply_U and their transposes are "
                                      "the host form of the factors; on the device use apply, "
                                      "apply_transpose, apply_pseudo_inverse or the fused samplers")

    def apply_V_transpose(self, x: Tensor) -> Tensor:
        self._host_only(x)
        hy, wy = self._hy_wy()
        vh, vw = self.V_h.to(x), self.V_w.to(x)
        return vh[:, :hy].t() @ x @ vw[:, :wy]

    def apply_V(self, z: Tensor) -> Tensor:
        self._host_only(z)
        hy, wy = self._hy_wy()
        vh, vw = self.V_h.to(z), self.V_w.to(z)
        return vh[:, :hy] @ z @ vw[:, :wy].t()

    def apply_U_transpose(self, y: Tensor) -> Tensor:
        self._host_only(y)
        return self.U_h.to(y).t() @ y @ self.U_w.to(y)

    def apply_U(self, z: Tensor) -> Tensor:
        self._host_only(z)
        return self.U_h.to(z) @ z @ self.U_w.to(z).t()

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, False, False)
        return self.apply_U(self.apply_V_transpose(x) * self.singular_values_full.to(x))

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, False, True)
        return self.apply_V(self.apply_U_transpose(y) * self.singular_values_full.to(y))

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipWorkspaceMap.apply(self, y, True, False)
        return self.apply_V(self.apply_U_transpose(y) * self.pinv_multiplier.to(y))

    def apply_pseudo_inverse_transpose(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipWorkspaceMap.apply(self, x, True, True)
        return self.apply_U(self.apply_V_transpose(x) * self.pinv_multiplier.to(x))

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """``z = T⁻¹[(S ⊙ T_y(y) + ρ T(x0)) / (S² + ρ)]`` on the observed grid, ``T(x0)`` itself
        outside it.  ``sp_op_prox_ws`` on device tensors, matmuls on host tensors."""
        if x0.is_cuda:
            return _hip_prox(self, x0, y, rho)
        rho = check_rho(rho)
        hy, wy = self._hy_wy()
        vh, vw, s = self.V_h.to(x0), self.V_w.to(x0), self.singular_values_full.to(x0)
        t = vh.t() @ x0 @ vw
        obs = (s * self.apply_U_transpose(y.to(x0.dtype)) + rho * t[..., :hy, :wy]) / (s * s + rho)
        t = torch.cat([torch.cat([obs, t[..., :hy, wy:]], dim=-1), t[..., hy:, :]], dim=-2)
        return vh @ t @ vw.t()

    def hip_descriptor(self) -> _hip.SpOp:
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_SVD_SEPARABLE
        d.channels, d.height, d.width = self.x_shape
        d.n, d.m = int(math.prod(self.x_shape)), int(math.prod(self.y_shape))
        d.taps = self.tables.data_ptr()
        d.radius, d.factor = self.y_shape[1], self.y_shape[2]
        return d


def _taps(t) -> np.ndarray:
    a = np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
    if a.ndim != 1 or a.size < 1:
        raise ValueError("taps must be 1-D")
    if not np.isfinite(a).all():
        raise ValueError("taps must be finite")
    return a
