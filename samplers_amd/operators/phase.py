"""Fourier phase retrieval with oversampling, the nonlinear task of the DPS paper (Chung et al.,
2022): only the amplitude of the zero-padded image's 2-D Fourier transform is observed.

The reference ships no such operator, so the semantics are defined here and pinned in fp64 by
``tests/phase_ops.py``.  For ``x`` of shape ``(C, H, W)`` and pads ``(pad_h, pad_w)``:

* ``apply``: ``y = |fft2(zero_pad(x), norm="ortho")|`` per channel plane, with ``pad_h`` zero rows
  above and below and ``pad_w`` zero columns left and right; ``y_shape = (C, Nh, Nw)``,
  ``Nh = H + 2 pad_h``, ``Nw = W + 2 pad_w``.  The layout is unshifted (DC at ``[0, 0]``); the DPS
  authors' code differs only by an ``fftshift`` permutation of ``y``.  The *full* spectrum is the
  observation: with independent noise on both Hermitian halves ``y`` is not symmetric, and the
  residual norm and the gradient run over all ``C·Nh·Nw`` elements;
* ``pad=None`` applies the DPS paper's rule ``pad = int(oversample / 8 * size)`` per axis
  (256 → 64, a 384 × 384 plane); ``pad`` is an int or ``(pad_h, pad_w)``;
* each padded size must be ``2^k`` or ``3·2^k`` in ``[8, 1024]`` (the transforms the HIP kernels
  implement): 256 → 384, 512 → 768, any doubling, ``pad = 0``;
* the Jacobian-transpose product of a cotangent ``g`` in y-space is
  ``crop(Re(ifft2(g · z/|z|, norm="ortho")))`` with ``z = fft2(pad(x))`` and ``z/|z| := 0`` where
  ``|z| = 0`` (torch's ``sgn``): never NaN or inf;
* no ``apply_transpose`` and no pseudo-inverse (the operator is not linear): ``PGDMSampler``
  rejects it and ``PSLDSampler`` fails at ``apply_transpose``.

On device tensors ``apply`` and its backward run the ``SP_OP_PHASE`` kernels
(``csrc/sp_phase.hip``: in-LDS FFTs; the padded complex spectrum never reaches memory); on host
tensors plain ``torch.fft``, which torch differentiates itself.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor

from .base import (MAX_SIZE, MIN_SIZE, NonlinearOperator, _flatten_batch, _work,
                   transform_size_ok)

valid_padded_size = transform_size_ok


def nearest_valid_pads(size: int, pad: int) -> list[int]:
    """The valid pads of an axis of ``size`` pixels closest to ``pad`` (below and above)."""
    ok = [p for p in range(0, (MAX_SIZE - size) // 2 + 1) if valid_padded_size(size + 2 * p)]
    below = [p for p in ok if p <= pad]
    above = [p for p in ok if p > pad]
    return below[-1:] + above[:1]


def phase_torch(x: Tensor, pad_h: int, pad_w: int) -> Tensor:
    """Host (torch) form of the forward map on ``(..., C, H, W)``; differentiable."""
    return torch.fft.fft2(F.pad(x, (pad_w, pad_w, pad_h, pad_h)), norm="ortho").abs()


class HipPhaseMap(torch.autograd.Function):
    """``sp_op_apply_ws`` with ``sp_op_vjp_ws`` as its backward.  The backward saves ``x`` and
    recomputes the spectrum; it is not differentiable itself (no double backward)."""

    @staticmethod
    def forward(ctx, op: "PhaseRetrievalOperator", x: Tensor) -> Tensor:
        _hip.require_cuda(x, type(op).__name__)
        if x.dtype != torch.float32:
            raise _hip.HipLibraryError(f"{type(op).__name__}: HIP operators compute in fp32")
        lib, desc = _hip.load_library(), op.hip_descriptor()
        flat, batch = _flatten_batch(x.detach(), op.x_shape)
        ctx.op, ctx.batch = op, batch
        ctx.save_for_backward(flat)
        out = torch.empty((flat.shape[0], *op.y_shape), device=x.device, dtype=torch.float32)
        if flat.shape[0] > 0:
            work = _work(lib, desc, flat.shape[0], flat)
            _hip.check(lib.sp_op_apply_ws(desc, _hip.ptr(flat), _hip.ptr(out), flat.shape[0],
                                          _hip.ptr(work), _hip.stream_of(x)), "sp_op_apply_ws")
        return out.reshape(*batch, *op.y_shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g: Tensor):
        op = ctx.op
        (flat,) = ctx.saved_tensors
        lib, desc = _hip.load_library(), op.hip_descriptor()
        gf, _ = _flatten_batch(g.to(torch.float32), op.y_shape)
        dx = torch.empty_like(flat)
        if flat.shape[0] > 0:
            work = _work(lib, desc, flat.shape[0], flat)
            _hip.check(lib.sp_op_vjp_ws(desc, _hip.ptr(flat), _hip.ptr(gf), _hip.ptr(dx),
                                        flat.shape[0], _hip.ptr(work), _hip.stream_of(g)),
                       "sp_op_vjp_ws")
        return None, dx.reshape(*ctx.batch, *op.x_shape)


class PhaseRetrievalOperator(NonlinearOperator):
    """``y = |fft2(zero_pad(x), norm="ortho")|`` per channel plane; ``y_shape = (C, Nh, Nw)``."""

    # nonlinear: the descriptor's sp_op_adjoint-based routes (ReSample's composed consistency,
    # PSLD's pixel pass) do not apply
    hip_linear = False

    def __init__(self, x_shape: Shape, oversample: float = 2.0, pad=None, device: Device = None) -> None:
        if len(x_shape) != 3:
            raise ValueError("x_shape must be (C, H, W)")
        c, h, w = (int(d) for d in x_shape)
        if pad is None:
            pad_h, pad_w = int(oversample / 8.0 * h), int(oversample / 8.0 * w)
        elif isinstance(pad, (tuple, list)):
            pad_h, pad_w = (int(p) for p in pad)
        else:
            pad_h = pad_w = int(pad)
        for name, size, p in (("height", h, pad_h), ("width", w, pad_w)):
            if p < 0 or not valid_padded_size(size + 2 * p):
                raise ValueError(
                    f"{name} {size} with pad {p} gives a padded size of {size + 2 * p}; it must be "
                    f"2^k or 3*2^k in [{MIN_SIZE}, {MAX_SIZE}] with pad >= 0 — nearest valid pads: "
                    f"{nearest_valid_pads(size, p)}")
        torch.nn.Module.__init__(self)
        self.pad_h, self.pad_w = pad_h, pad_w
        self.x_shape = (c, h, w)
        self.y_shape = (c, h + 2 * pad_h, w + 2 * pad_w)
        # device marker, as the other operators' buffers: .to(device) moves it
        self.register_buffer("_marker", torch.zeros(1, device=device), persistent=False)

    def apply(self, x: Tensor) -> Tensor:
        if x.is_cuda:
            return HipPhaseMap.apply(self, x)
        return phase_torch(x, self.pad_h, self.pad_w)

    def hip_descriptor(self) -> _hip.SpOp:
        c, h, w = self.x_shape
        d = _hip.SpOp()
        d.kind = _hip.SP_OP_PHASE
        d.channels, d.height, d.width = c, h, w
        d.n = int(math.prod(self.x_shape))
        d.m = int(math.prod(self.y_shape))
        d.radius, d.factor = self.pad_h, self.pad_w
        return d
