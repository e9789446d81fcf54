"""Forward-operator plugin API (mirrors ``/root/reference/samplers/operators/base.py:8-113``).

An ``Operator`` is an ``nn.Module`` holding its long-lived tensors as buffers.
Operators that the HIP library implements natively also expose
``hip_descriptor()`` -> :class:`samplers_amd._hip.SpOp`, which the fused DPS
kernels consume; on device tensors their ``apply`` / ``apply_transpose`` run
HIP kernels (differentiable through :class:`HipLinearMap`, or through
:class:`HipWorkspaceMap` for the linear kinds whose maps need a workspace: the
FFT blurs).  On host tensors they run plain torch ops — only setup code (shape
inference, synthetic observations) touches that path.

The helpers the operator modules share live here too: the workspace of a map
(``_work``), the lengths the in-LDS FFT kernels transform (``transform_size_ok``,
``MIN_SIZE``, ``MAX_SIZE``), the transpose of a host map through autograd
(``_transpose_by_grad``) and the descriptor of a plane-to-plane kind
(``_plane_descriptor``).
"""

from __future__ import annotations

import math
from abc import ABC, abstractmethod

import torch

from samplers_amd import _hip
from samplers_amd.dtypes import Device, Shape, Tensor


class Operator(torch.nn.Module, ABC):
    """Generic forward model ``A`` (``apply`` mandatory; ``apply_transpose`` and
    ``apply_pseudo_inverse`` optional, raising ``NotImplementedError``)."""

    # c in ∂/∂x̂₀ ‖A⁺y − A⁺A x̂₀‖² = −c·Aᵀ(y − A x̂₀) for natively implemented operators with a
    # pseudo-inverse (the fused PGDM step): 2 for partial isometries (A⁺ = Aᵀ).
    pinv_grad_scale: float = 2.0
    # True when a HIP descriptor's sp_op_apply / sp_op_adjoint routes apply (every natively
    # implemented linear operator); a nonlinear native operator sets it False
    hip_linear: bool = True

    def __init__(self, x_shape: Shape, device: Device = None) -> None:
        super().__init__()
        self.x_shape = tuple(x_shape)
        self.y_shape = self._infer_y_shape(self.x_shape, device=device)

    def _infer_y_shape(self, x_shape: Shape, device: Device = None) -> Shape:
        """Run a zero batch of one through ``apply`` (reference ``base.py:36-49``)."""
        device = device or next(self.buffers(), torch.tensor(0)).device
        dummy = torch.zeros((1, *x_shape), dtype=torch.float32, device=device)
        with torch.no_grad():
            y = self.apply(dummy)
        return tuple(y.shape[1:])

    @abstractmethod
    def apply(self, x: Tensor) -> Tensor:
        """Forward map ``y = A(x)`` for ``x`` of shape ``(*batch, *x_shape)``."""

    def apply_transpose(self, y: Tensor) -> Tensor:
        raise NotImplementedError("Transpose not defined for this operator")

    def apply_pseudo_inverse(self, y: Tensor) -> Tensor:
        raise NotImplementedError("Pseudo-inverse not defined for this operator")

    def apply_prox(self, x0: Tensor, y: Tensor, rho: float) -> Tensor:
        """The proximal map of the data term, ``argmin_u ‖y − A u‖² + ρ ‖u − x0‖²`` =
        ``(AᵀA + ρI)⁻¹(Aᵀy + ρ x0)`` for ``ρ > 0`` (DiffPIR's data step, HQS / plug-and-play).
        Only the operators with a closed form implement it."""
        raise NotImplementedError(f"{type(self).__name__} has no closed-form proximal map "
                                  "(apply_prox)")

    def apply_prox_cg(self, x0: Tensor, y: Tensor, rho: float, iterations: int = 32,
                      tol: float = 1e-6, return_iterations: bool = False):
        """The same proximal map for every linear operator, by at most ``iterations`` steps of
        regularised CGLS on ``(AᵀA + ρI) z = Aᵀy + ρ x0`` with a per-sample stop at
        ``‖g‖² ≤ tol²·‖g₀‖²`` ("Proximal map by conjugate gradients"; the stop is
        part of the map).  On host tensors the recurrence runs in plain torch in the tensor's
        dtype through ``apply`` / ``apply_transpose``; on device tensors it is one call of
        ``sp_op_prox_cg_ws`` (the operator needs a HIP descriptor).  With ``return_iterations``
        the result is ``(z, iters)``, ``iters`` an int32 tensor of the batch shape: the live
        iterations of each sample."""
        rho, iterations, tol = check_cg(rho, iterations, tol)
        run = _hip_prox_cg if x0.is_cuda else _host_prox_cg
        z, iters = run(self, x0, y, rho, iterations, tol)
        return (z, iters) if return_iterations else z

    def forward(self, x: Tensor) -> Tensor:
        return self.apply(x)

    # --- HIP integration -------------------------------------------------
    def hip_descriptor(self) -> "_hip.SpOp | None":
        """Descriptor for the fused kernels, or ``None`` if the operator has no
        native implementation (the samplers then refuse the fused path)."""
        return None


class NonlinearOperator(Operator):
    """Non-linear degradation operator (``apply`` required; adjoint optional)."""

    @abstractmethod
    def apply(self, x: Tensor) -> Tensor: ...

    def apply_prox_cg(self, x0: Tensor, y: Tensor, rho: float, iterations: int = 32,
                      tol: float = 1e-6, return_iterations: bool = False):
        raise NotImplementedError(f"{type(self).__name__} is nonlinear: the conjugate-gradient "
                                  "proximal map (apply_prox_cg) needs a linear operator")


def _flatten_batch(t: Tensor, sample_shape: Shape) -> tuple[Tensor, tuple[int, ...]]:
    nd = len(sample_shape)
    batch = tuple(t.shape[: t.ndim - nd])
    b = 1
    for s in batch:
        b *= s
    return t.reshape(b, *sample_shape).contiguous(), batch


class HipLinearMap(torch.autograd.Function):
    """Differentiable wrapper around ``sp_op_apply`` / ``sp_op_adjoint``.

    ``forward(op, x, transpose)`` applies A (or A^T); the backward of a linear
    map is its adjoint, so third-party samplers can differentiate through any
    natively implemented operator without leaving HIP.
    """

    @staticmethod
    def forward(ctx, op: Operator, x: Tensor, transpose: bool) -> Tensor:
        ctx.op, ctx.transpose = op, transpose
        return _hip_linear(op, x, transpose)

    @staticmethod
    def backward(ctx, g: Tensor):
        return None, _hip_linear(ctx.op, g.contiguous(), not ctx.transpose), None


def _hip_linear(op: Operator, t: Tensor, transpose: bool) -> Tensor:
    _hip.require_cuda(t, type(op).__name__)
    lib = _hip.load_library()
    desc = op.hip_descriptor()
    in_shape, out_shape = (op.y_shape, op.x_shape) if transpose else (op.x_shape, op.y_shape)
    if t.dtype != torch.float32:
        raise _hip.HipLibraryError(f"{type(op).__name__}: HIP operators compute in fp32")
    flat, batch = _flatten_batch(t, in_shape)
    out = torch.empty((flat.shape[0], *out_shape), device=t.device, dtype=torch.float32)
    if flat.shape[0] > 0:
        fn = lib.sp_op_adjoint if transpose else lib.sp_op_apply
        _hip.check(fn(desc, _hip.ptr(flat), _hip.ptr(out), flat.shape[0], _hip.stream_of(t)),
                   "sp_op_adjoint" if transpose else "sp_op_apply")
    return out.reshape(*batch, *out_shape)


def _work(lib, desc, batch: int, like: Tensor) -> Tensor:
    """The workspace of ``sp_op_apply_ws`` / ``sp_op_vjp_ws`` / ``sp_op_pinv_ws`` for ``batch``."""
    floats = int(lib.sp_op_workspace(desc, batch))
    if floats < 0:
        raise _hip.HipLibraryError(f"sp_op_workspace rejected the descriptor ({floats})")
    return torch.empty(max(floats, 2), device=like.device, dtype=torch.float32)


class HipWorkspaceMap(torch.autograd.Function):
    """A linear map that runs through a workspace:
    ``forward(op, t, pinv, transpose)`` is ``sp_op_apply_ws`` (A), ``sp_op_vjp_ws`` (Aᵀ) or
    ``sp_op_pinv_ws`` (A⁺, A⁺ᵀ); the backward of a linear map is its transpose, so it
    differentiates to any order."""

    @staticmethod
    def forward(ctx, op: Operator, t: Tensor, pinv: bool, transpose: bool) -> Tensor:
        ctx.op, ctx.pinv, ctx.transpose = op, pinv, transpose
        return _hip_workspace_map(op, t, pinv, transpose)

    @staticmethod
    def backward(ctx, g: Tensor):
        return None, HipWorkspaceMap.apply(ctx.op, g.to(torch.float32).contiguous(), ctx.pinv,
                                           not ctx.transpose), None, None


def _hip_workspace_map(op: Operator, t: Tensor, pinv: bool, transpose: bool) -> Tensor:
    _hip.require_cuda(t, type(op).__name__)
    if t.dtype != torch.float32:
        raise _hip.HipLibraryError(f"{type(op).__name__}: HIP operators compute in fp32")
    lib, desc = _hip.load_library(), op.hip_descriptor()
    # A and A^+T take x_shape to y_shape, A^T and A^+ the other way (the same shape but for the
    # periodic super-resolution operator)
    in_shape, out_shape = ((op.x_shape, op.y_shape) if pinv == transpose
                           else (op.y_shape, op.x_shape))
    flat, batch = _flatten_batch(t.detach(), in_shape)
    n = flat.shape[0]
    out = torch.empty((n, *out_shape), device=flat.device, dtype=torch.float32)
    if n > 0:
        work, stream = _work(lib, desc, n, flat), _hip.stream_of(t)
        if pinv:
            _hip.check(lib.sp_op_pinv_ws(desc, _hip.ptr(flat), _hip.ptr(out), n, int(transpose),
                                         _hip.ptr(work), stream), "sp_op_pinv_ws")
        elif transpose:  # A^T: the x argument of sp_op_vjp_ws is not read
            _hip.check(lib.sp_op_vjp_ws(desc, _hip.ptr(flat), _hip.ptr(flat), _hip.ptr(out), n,
                                        _hip.ptr(work), stream), "sp_op_vjp_ws")
        else:
            _hip.check(lib.sp_op_apply_ws(desc, _hip.ptr(flat), _hip.ptr(out), n, _hip.ptr(work),
                                          stream), "sp_op_apply_ws")
    return out.reshape(*batch, *out_shape)


def check_rho(rho: float) -> float:
    rho = float(rho)
    if not (rho > 0.0 and math.isfinite(rho)):
        raise ValueError(f"rho must be positive and finite, got {rho}")
    return rho


def _isometry_prox(op: Operator, x0: Tensor, y: Tensor, rho: float, gram: float = 1.0) -> Tensor:
    """Host closed form for ``A Aᵀ = gram · I``: ``z = x0 + Aᵀ(y − A x0) / (gram + ρ)``."""
    return x0 + op.apply_transpose(y - op.apply(x0)) / (gram + check_rho(rho))


def _hip_prox(op: Operator, x0: Tensor, y: Tensor, rho: float) -> Tensor:
    """``sp_op_prox_ws`` on device tensors: ``x0`` of shape ``(*batch, *x_shape)``, one row of
    ``y`` per sample.  The kinds that prepare (the periodic blur) transform ``y`` first."""
    rho = check_rho(rho)
    _hip.require_cuda(x0, type(op).__name__)
    _hip.require_cuda(y, type(op).__name__)
    if x0.dtype != torch.float32 or y.dtype != torch.float32:
        raise _hip.HipLibraryError(f"{type(op).__name__}: HIP operators compute in fp32")
    lib, desc = _hip.load_library(), op.hip_descriptor()
    flat, batch = _flatten_batch(x0.detach(), op.x_shape)
    rows, y_batch = _flatten_batch(y.detach(), op.y_shape)
    if y_batch != batch:
        raise ValueError(f"x0 and y must share their batch dimensions, got {batch} and {y_batch}")
    out = torch.empty_like(flat)
    n = flat.shape[0]
    if n > 0:
        stream = _hip.stream_of(x0)
        floats, qsize = int(lib.sp_prox_workspace(desc, n)), int(lib.sp_prox_prepare_size(desc, n))
        if floats < 0 or qsize < 0:
            raise _hip.HipLibraryError(f"sp_prox_workspace rejected the descriptor ({floats})")
        work = torch.empty(floats, device=flat.device, dtype=torch.float32) if floats else None
        q = torch.empty(qsize, device=flat.device, dtype=torch.float32) if qsize else None
        _hip.check(lib.sp_prox_prepare(desc, _hip.ptr(rows), n, _hip.ptr(q), stream),
                   "sp_prox_prepare")
        _hip.check(lib.sp_op_prox_ws(desc, _hip.ptr(flat), _hip.ptr(rows), _hip.ptr(q), n, 1, rho,
                                     _hip.ptr(out), _hip.ptr(work), stream), "sp_op_prox_ws")
    return out.reshape(*batch, *op.x_shape)


def check_cg(rho: float, iterations: int, tol: float) -> tuple[float, int, float]:
    rho, tol = check_rho(rho), float(tol)
    if int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"iterations must be a positive integer, got {iterations!r}")
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"tol must be non-negative and finite, got {tol}")
    return rho, int(iterations), tol


def _host_prox_cg(op: Operator, x0: Tensor, y: Tensor, rho: float, iterations: int,
                  tol: float) -> tuple[Tensor, Tensor]:
    """The recurrence of ``apply_prox_cg`` on host tensors, every sample with scalars of its own
    (tensors of the flat batch): a sample that is not live keeps every vector through
    ``torch.where``, never through a product by 0."""
    flat, batch = _flatten_batch(x0.detach(), op.x_shape)
    rows, y_batch = _flatten_batch(y.detach(), op.y_shape)
    if y_batch != batch:
        raise ValueError(f"x0 and y must share their batch dimensions, got {batch} and {y_batch}")
    nb = flat.shape[0]
    sq = lambda t: (t.reshape(nb, -1) ** 2).sum(1)  # noqa: E731
    per = lambda v, t: v.reshape(nb, *([1] * (t.ndim - 1)))  # noqa: E731
    s = rows - op.apply(flat)
    d = torch.zeros_like(flat)
    g = op.apply_transpose(s)
    p = g.clone()
    gamma = sq(g)
    gamma0 = gamma.clone()
    iters = torch.zeros(nb, dtype=torch.int32, device=flat.device)
    for _ in range(iterations):
        q = op.apply(p)
        delta = sq(q) + rho * sq(p)
        live = ((gamma > (tol * tol) * gamma0) & (delta > 0) & torch.isfinite(gamma)
                & torch.isfinite(delta))
        if not bool(live.any()):
            break  # every sample has stopped, and stopping is sticky
        alpha = gamma / delta
        d = torch.where(per(live, d), d + per(alpha, d) * p, d)
        s = torch.where(per(live, s), s - per(alpha, s) * q, s)
        g = torch.where(per(live, g), op.apply_transpose(s) - rho * d, g)
        gamma_new = sq(g)
        p = torch.where(per(live, p), g + per(gamma_new / gamma, p) * p, p)
        gamma = torch.where(live, gamma_new, gamma)
        iters = iters + live.to(torch.int32)
    z = torch.where(per(iters > 0, flat), flat + d, flat)
    return z.reshape(*batch, *op.x_shape), iters.reshape(batch)


def _hip_prox_cg(op: Operator, x0: Tensor, y: Tensor, rho: float, iterations: int,
                 tol: float) -> tuple[Tensor, Tensor]:
    """``sp_op_prox_cg_ws`` on device tensors: ``x0`` of shape ``(*batch, *x_shape)``, one row of
    ``y`` per sample."""
    name = type(op).__name__
    _hip.require_cuda(y, name)
    desc = op.hip_descriptor()
    if desc is None:
        raise NotImplementedError(f"{name} has no native (HIP) kernels: apply_prox_cg runs on "
                                  "host tensors only")
    if x0.dtype != torch.float32 or y.dtype != torch.float32:
        raise _hip.HipLibraryError(f"{name}: HIP operators compute in fp32")
    lib = _hip.load_library()
    flat, batch = _flatten_batch(x0.detach(), op.x_shape)
    rows, y_batch = _flatten_batch(y.detach(), op.y_shape)
    if y_batch != batch:
        raise ValueError(f"x0 and y must share their batch dimensions, got {batch} and {y_batch}")
    out = torch.empty_like(flat)
    n = flat.shape[0]
    iters = torch.zeros(n, device=flat.device, dtype=torch.int32)
    if n > 0:
        floats = int(lib.sp_prox_cg_workspace(desc, n, 0))
        if floats == -3:  # SP_EUNSUPPORTED: a nonlinear kind
            raise NotImplementedError(f"{name}: the library has no linear maps for its kind "
                                      "(apply_prox_cg)")
        if floats < 0:
            raise _hip.HipLibraryError(f"sp_prox_cg_workspace rejected the descriptor ({floats})")
        work = torch.empty(floats, device=flat.device, dtype=torch.float32)
        _hip.check(lib.sp_op_prox_cg_ws(desc, _hip.ptr(flat), _hip.ptr(rows), n, 1, rho, iterations,
                                        tol, _hip.ptr(out), _hip.ptr(iters), _hip.ptr(work),
                                        _hip.stream_of(x0)), "sp_op_prox_cg_ws")
    return out.reshape(*batch, *op.x_shape), iters.reshape(batch)


MIN_SIZE, MAX_SIZE = 8, 1024


def transform_size_ok(n: int) -> bool:
    """``n`` is ``2^k`` or ``3·2^k`` in ``[MIN_SIZE, MAX_SIZE]``: a length the kernels transform."""
    n = int(n)
    if n < MIN_SIZE or n > MAX_SIZE:
        return False
    while n % 2 == 0:
        n //= 2
    return n in (1, 3)


def _transpose_by_grad(fn, y: Tensor) -> Tensor:
    """``Aᵀ y`` of a differentiable linear host map ``fn`` whose output has its input's shape."""
    x = torch.zeros_like(y, requires_grad=True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(x), x, grad_outputs=y)
    return g


def _plane_descriptor(kind: int, x_shape: Shape) -> "_hip.SpOp":
    """The descriptor of a kind on ``(C, H, W)`` planes with ``n = m = C·H·W``."""
    d = _hip.SpOp()
    d.kind = kind
    d.channels, d.height, d.width = x_shape
    d.n = d.m = int(math.prod(x_shape))
    return d
