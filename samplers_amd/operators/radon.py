"""Parallel-beam computed tomography: the Radon transform of every channel plane by Joseph's
method (sparse-view and limited-angle CT, the inverse problem the ReSample paper leads with).

The reference ships no tomography operator, so the semantics are defined here and pinned in
fp64 by ``tests/radon_ref.py``.  ``x_shape = (C, H, W)``, ``y_shape = (C, n_angles, D)``: a
sinogram plane has the angles on the slow axis and ``D`` detector bins on the fast one.  Pixel
and detector spacing are 1.  With ``s0 = (D−1)/2``, ``i0 = (H−1)/2``, ``j0 = (W−1)/2`` every
angle ``θ`` has one row ``(alpha, beta, length, axis)`` of :func:`radon_table`:

* ``axis == 0`` (``|cos θ| ≥ |sin θ|``): ``(1/cos θ, −sin θ/cos θ, 1/|cos θ|, 0)``.  Ray ``s``
  crosses image row ``i`` at column ``c = alpha·(s − s0) + (beta·(i − i0) + j0)`` and
  ``y[a, s] = length · Σ_i [(1 − f)·x[i, ⌊c⌋] + f·x[i, ⌊c⌋ + 1]]``, ``f = c − ⌊c⌋``, a column
  outside ``[0, W)`` contributing 0;
* ``axis == 1``: ``(1/sin θ, −cos θ/sin θ, 1/|sin θ|, 1)`` with rows and columns swapped: ray
  ``s`` crosses column ``j`` at row ``alpha·(s − s0) + (beta·(j − j0) + i0)``.

The table is computed in fp64 and rounded to fp32, and the map is defined by those fp32 values
taken as exact constants.  Any ``D ≥ 1`` is legal: rays that miss the image give 0, pixels that
project beyond the detector are seen by fewer rays.  ``apply_transpose`` is the exact
transpose.  There is no pseudo-inverse (filtered back-projection is not ``A⁺``), so
``PGDMSampler`` raises ``NotImplementedError`` as for ``PSFBlurOperator``.

On device tensors the maps run the ``SP_OP_RADON`` kernels (``csrc/sp_radon.hip``); on host
tensors a sparse matrix built once from the table, in the tensor's dtype (fp64 tensors get the
fp64 weights), differentiable through its transpose.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import HipLinearMap
from .linear import LinearOperator

MIN_SIZE, MAX_SIZE = 8, 512
MAX_ANGLES, MAX_DETECTOR = 512, 1024


def radon_table(angles) -> Tensor:
    """The ``(n_angles, 4)`` fp32 table ``(alpha, beta, length, axis)`` of ``angles`` (radians).

    Computed in fp64; a ``cos`` or ``sin`` below 1e-12 in magnitude is snapped to 0 first, so
    the axis angles 0, π/2, π, 3π/2 get exact rows; a tie ``|cos| == |sin|`` is ``axis == 0``.
    """
    th = np.asarray(torch.as_tensor(angles).detach().cpu().numpy()
                    if isinstance(angles, torch.Tensor) else angles, dtype=np.float64).reshape(-1)
    if th.size == 0 or not np.isfinite(th).all():
        raise ValueError("angles must be a non-empty sequence of finite values")
    c, s = np.cos(th), np.sin(th)
    c[np.abs(c) < 1e-12] = 0.0
    s[np.abs(s) < 1e-12] = 0.0
    axis = np.abs(c) < np.abs(s)
    num = np.where(axis, s, c)  # the dominant component: |num| >= 1/sqrt(2)
    den = np.where(axis, c, s)
    table = np.stack([1.0 / num, -den / num, 1.0 / np.abs(num), axis.astype(np.float64)], axis=1)
    return torch.from_numpy(table.astype(np.float32))


def default_detector_size(height: int, width: int) -> int:
    """An odd number of bins that covers the image diagonal: ``2·⌈√(H² + W²)/2⌉ + 1``."""
    return 2 * math.ceil(math.sqrt(height * height + width * width) / 2.0) + 1


def radon_matrix(table, height: int, width: int, detector_size: int):
    """COO triplets ``(rows, cols, values)`` of the ``(n_angles·D, H·W)`` matrix of one plane,
    in fp64 from the fp32 ``table`` values taken as exact (entries off the image left out)."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    H, W, D = int(height), int(width), int(detector_size)
    ds = np.arange(D, dtype=np.float64) - (D - 1) / 2.0
    rows, cols, vals = [], [], []
    for a, (alpha, beta, length, axis) in enumerate(t):
        nd, nx = (W, H) if axis else (H, W)
        d = np.arange(nd, dtype=np.float64)
        c = alpha * ds[:, None] + (beta * (d[None, :] - (nd - 1) / 2.0) + (nx - 1) / 2.0)  # (D, nd)
        fl = np.floor(c)
        f = c - fl
        ic = fl.astype(np.int64)
        r = np.broadcast_to(a * D + np.arange(D, dtype=np.int64)[:, None], ic.shape)
        di = np.broadcast_to(np.arange(nd, dtype=np.int64)[None, :], ic.shape)
        for idx, w in ((ic, 1.0 - f), (ic + 1, f)):
            ok = (idx >= 0) & (idx < nx)
            pix = idx * W + di if axis else di * W + idx
            rows.append(r[ok])
            cols.append(pix[ok])
            vals.append(length * w[ok])
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


class _SparseMap(torch.autograd.Function):
    """``S @ x`` for a constant sparse ``S`` with its transpose ``St`` at hand."""

    @staticmethod
    def forward(ctx, S: Tensor, St: Tensor, x: Tensor) -> Tensor:
        ctx.S, ctx.St = S, St
        return torch.sparse.mm(S, x)

    @staticmethod
    def backward(ctx, g: Tensor):
        return None, None, _SparseMap.apply(ctx.St, ctx.S, g.contiguous())


class RadonOperator(LinearOperator):
    """Parallel-beam projector of every channel plane; ``y`` has shape ``(C, n_angles, D)``.

    ``angles`` in radians (default ``π·a/num_angles``, ``a = 0 … num_angles − 1``);
    ``detector_size`` defaults to :func:`default_detector_size`.  PSLD and ReSample compose their
    pixel passes from ``sp_op_apply`` / ``sp_op_adjoint`` (``hip_linear``), which size every
    observation-space buffer by ``m``.
    """

    hip_linear = True

    def __init__(self, x_shape: Shape, angles=None, num_angles: int = 23,
                 detector_size: int | None = None, device: Device = None) -> None:
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if c < 1 or not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
            raise ValueError(f"channels must be positive and height, width in [{MIN_SIZE}, {MAX_SIZE}], "
                             f"got {tuple(x_shape)}")
        if angles is None:
            if not (1 <= int(num_angles) <= MAX_ANGLES):
                raise ValueError(f"num_angles must be in [1, {MAX_ANGLES}]")
            angles = [math.pi * a / int(num_angles) for a in range(int(num_angles))]
        table = radon_table(angles)  # raises on empty or non-finite angles
        if table.shape[0] > MAX_ANGLES:
            raise ValueError(f"at most {MAX_ANGLES} angles, got {table.shape[0]}")
        d = default_detector_size(h, w) if detector_size is None else int(detector_size)
        if not (1 <= d <= MAX_DETECTOR):
            raise ValueError(f"detector_size must be in [1, {MAX_DETECTOR}], got {d}")
        torch.nn.Module.__init__(self)
        self.register_buffer("table", table.contiguous().to(device))
        self.angles = tuple(float(a) for a in np.asarray(angles, dtype=np.float64).reshape(-1))
        self.num_angles, self.detector_size = int(table.shape[0]), d
        self.x_shape = (c, h, w)
        self.y_shape = (c, self.num_angles, d)
        self._mats: dict = {}

    @classmethod
    def limited_angle(cls, x_shape: Shape, num_angles: int, span: float,
                      detector_size: int | None = None, device: Device = None) -> "RadonOperator":
        """``num_angles`` equally spaced angles covering ``[0, span)`` radians."""
        if not (1 <= int(num_angles) <= MAX_ANGLES):
            raise ValueError(f"num_angles must be in [1, {MAX_ANGLES}]")
        if not (math.isfinite(span) and span > 0):
            raise ValueError("span must be positive and finite")
        return cls(x_shape, angles=[span * a / int(num_angles) for a in range(int(num_angles))],
                   detector_size=detector_size, device=device)

    # --- host form ---------------------------------------------------------
    def _matrices(self, dtype: torch.dtype, device: torch.device) -> tuple[Tensor, Tensor]:
        """(A, Aᵀ) of one plane as coalesced sparse tensors, built once per dtype and device."""
        key = (dtype, str(device))
        if key not in self._mats:
            _, h, w = self.x_shape
            r, c, v = radon_matrix(self.table.detach().cpu().numpy(), h, w, self.detector_size)
            idx = torch.from_numpy(np.stack([r, c]))
            val = torch.from_numpy(v)
            size = (self.num_angles * self.detector_size, h * w)
            A = torch.sparse_coo_tensor(idx, val, size).coalesce()
            At = torch.sparse_coo_tensor(idx.flip(0), val, size[::-1]).coalesce()
            self._mats[key] = (A.to(device=device, dtype=dtype), At.to(device=device, dtype=dtype))
        return self._mats[key]

    def _host_map(self, t: Tensor, transpose: bool) -> Tensor:
        _, h, w = self.x_shape
        in_plane = (self.num_angles, self.detector_size) if transpose else (h, w)
        out_plane = (h, w) if transpose else (self.num_angles, self.detector_size)
        dtype = t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float32
        A, At = self._matrices(dtype, t.device)
        lead = t.shape[:-2]
        flat = t.to(dtype).reshape(-1, in_plane[0] * in_plane[1]).t()
        out = _SparseMap.apply(At, A, flat) if transpose else _SparseMap.apply(A, At, flat)
        return out.t().reshape(*lead, *out_plane)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipLinearMap.apply(self, x, False)
        return self._host_map(x, False)

    def apply_transpose(self, y: Tensor) -> Tensor:
        if y.is_cuda:
            return HipLinearMap.apply(self, y, True)
        return self._host_map(y, True)

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        raise NotImplementedError("RadonOperator has no pseudo-inverse (filtered back-projection "
                                  "is not A⁺)")

    def hip_descriptor(self) -> _hip.SpOp:
        c, h, w = self.x_shape
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_RADON
        d.channels, d.height, d.width = c, h, w
        d.n = c * h * w
        d.m = c * self.num_angles * self.detector_size
        d.taps = self.table.data_ptr()
        d.radius = self.num_angles
        d.factor = self.detector_size
        return d
