"""Diffusion Posterior Sampling on the MI355X hot path.

Same call contract as ``DPSSampler.__call__`` of the reference
(``/root/reference/samplers/samplers/dps.py:25-134``); the loop body
(``dps.py:91-122``) is rebuilt around two fused HIP passes with the prior's
input-VJP between them::

    eps = unet(x, t)                               the prior (its layers on this project's kernels)
    v, |r|^2 partials = sp_dps_residual(x, eps, y) HIP pass 1: x0, A x0, residual, A^T grad
    w = J_eps^T v                                  the prior's input VJP (PyTorch-ROCm autograd)
    x <- sp_dps_update(x, eps, y|v, w, noise)      HIP pass 2: bridge mean + std*xi + guidance

which is algebraically the reference's ``autograd.grad(log_likelihood(predict_x0(x)).sum(), x)``
followed by ``ddim_step`` and ``x += gamma / (||r_b|| + 1e-9) * grad``
(closed form: SURVEY.md §8a A9).  Timesteps and schedule scalars stay on the
host, so a step issues no device->host synchronisation.

Noise (``rng=``):
  * ``"philox"`` (default): standard normals drawn inside pass 2 by Philox4x32-10
    keyed by (seed, step, global sample index, element) — identical whatever the
    batch sharding or micro-batching;
  * ``"torch"``: the reference's draw order — ``torch.randn`` for x_T and one
    ``torch.randn_like`` per step on the sample's device;
  * ``noise_fn(kind, step, shape)``: injected tensors (parity tests replay the
    reference's captured noise).
"""

from __future__ import annotations

import contextlib
from typing import Callable, Generic, TypeVar

import numpy as np
import torch
from torch import Tensor

from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.networks.base import EpsilonNetwork, host_alphas_cumprod
from samplers_amd.samplers.base import PosteriorSampler
from samplers_amd.samplers.loop import (NoiseFn, draw_seed, initial_sample,  # noqa: F401
                                        run_sampler)
from samplers_amd.samplers.utils.bridge_kernels import bridge_coefficients, x0_coefficients

Condition_co = TypeVar("Condition_co", covariant=True)


class KernelTimer:
    """Per-launch durations of the library's timed kernels.

    Uses the library's dispatch-packet events (``sp_timing_enable``: a start/stop
    hipEvent pair attached to each kernel's AQL packet via hipExtLaunchKernel),
    i.e. the kernel's own execution interval on its launch stream — the same
    interval rocprofv3's kernel trace reports — not a host-side bracket.  Each
    record carries the launch's algorithmic work (``sp_timing_collect_work``):
    samples for the two DPS passes, FLOPs for the fp32-MFMA convolution tile.
    """

    _KIND = {1: "dps_residual", 2: "dps_update", 3: "conv3x3_fwd", 4: "conv3x3_bwd_input",
             5: "wino3x3_fwd", 6: "wino3x3_bwd_input", 7: "conv3x3_bf16"}
    _CAP = 1 << 16

    def __init__(self) -> None:
        self.batches: list[tuple[str, int]] = []
        self._lib = _hip.load_library()
        self._lib.sp_timing_enable(1)

    def span(self, name: str, batch: int):
        timer = self

        class _Span:
            def __enter__(self):
                return self

            def __exit__(self, *exc):
                timer.batches.append((name, batch))
                return False

        return _Span()

    def summary(self) -> dict[str, dict[str, float]]:
        """{kind: {count, ms, work}} over the launches since the last call; ``samples`` is
        the DPS passes' work, ``flops`` the convolutions'."""
        import ctypes

        kinds = (ctypes.c_int32 * self._CAP)()
        ms = (ctypes.c_float * self._CAP)()
        work = (ctypes.c_double * self._CAP)()
        n = self._lib.sp_timing_collect_work(kinds, ms, work, self._CAP)
        out: dict[str, dict[str, float]] = {}
        for kind, t, w in zip(kinds[:n], ms[:n], work[:n]):
            name = self._KIND.get(kind, f"kind{kind}")
            d = out.setdefault(name, {"count": 0, "ms": 0.0, "work": 0.0})
            d["count"] += 1
            d["ms"] += float(t)
            d["work"] += float(w)
        for name, d in out.items():
            d["samples" if name.startswith("dps") else "flops"] = d["work"]
        self.batches.clear()
        return out

    def clear(self) -> None:
        self.summary()

    def close(self) -> None:
        self.clear()
        self._lib.sp_timing_enable(0)


class FusedStep:
    """What the fused steps of the samplers share: the observation rows on the device, ``q`` (the
    rows as a kind's launches read them, prepared once per call: y is fixed across the steps),
    the micro-batch chunks, a work buffer kept between steps, the bracket of a launch for
    ``KernelTimer`` and the final ``predict_x0``.

    ``observation_rows``: ``(num_rows, *y_shape)`` fp32 device tensor; sample b
    uses row ``b // y_div`` (``y_div`` = reconstructions per observation).
    """

    def __init__(self, network: EpsilonNetwork, operator, y_div: int, micro_batch: int | None,
                 timer: KernelTimer | None) -> None:
        self.network, self.operator = network, operator
        self.y_div = int(y_div)
        self.micro_batch, self.timer = micro_batch, timer
        self.q: Tensor | None = None
        self._work: Tensor | None = None

    def _bind_rows(self, observation_rows: Tensor, sampler: str) -> None:
        _hip.require_cuda(observation_rows, sampler)
        if observation_rows.dtype != torch.float32:
            raise TypeError("the HIP path computes in fp32; cast the observation to float32")
        self.lib = _hip.load_library()
        self.y = observation_rows.contiguous()

    def _prepare_q(self, size: str, prepare: str, *, optional: bool = False) -> None:
        """``q`` of ``size(desc, rows)`` floats, filled by ``prepare`` (both entry points by name);
        an ``optional`` one stays None where the kind has nothing to prepare."""
        rows = self.y.shape[0]
        floats = int(getattr(self.lib, size)(self.desc, rows))
        if floats < 0 or not (floats or optional):
            raise _hip.HipLibraryError(f"{size} rejected the descriptor ({floats})")
        if floats:
            self.q = torch.empty((rows, floats // rows), device=self.y.device, dtype=torch.float32)
            _hip.check(getattr(self.lib, prepare)(self.desc, _hip.ptr(self.y), rows, _hip.ptr(self.q),
                                                  _hip.stream_of(self.y)), prepare)

    def _chunks(self, batch: int):
        mb = self.micro_batch or batch
        mb = max(self.y_div, (mb // self.y_div) * self.y_div)  # chunks never split an observation
        for b0 in range(0, batch, mb):
            yield b0, min(batch, b0 + mb)

    def _kept_work(self, floats: int, like: Tensor) -> Tensor:
        """At least ``floats`` floats on ``like``'s device, kept between steps (grow-only)."""
        if self._work is None or self._work.numel() < floats or self._work.device != like.device:
            self._work = torch.empty(floats, device=like.device, dtype=torch.float32)
        return self._work

    def _timed(self, name: str, batch: int):
        """Brackets one launch for the kernel timer, if there is one."""
        return self.timer.span(name, batch) if self.timer else contextlib.nullcontext()

    def predict_x0(self, x: Tensor, t: int) -> Tensor:
        """Final ``predict_x0`` (``dps.py:125-126``): prior forward + HIP epilogue."""
        a, k = x0_coefficients(host_alphas_cumprod(self.network), t)
        out = torch.empty_like(x)
        for b0, b1 in self._chunks(x.shape[0]):
            with torch.no_grad():
                eps = self.network.forward(x[b0:b1], t).contiguous()
            _hip.check(self.lib.sp_predict_x0(_hip.ptr(x[b0:b1]), _hip.ptr(eps), eps.numel(), a, k,
                                              _hip.ptr(out[b0:b1]), _hip.stream_of(x)),
                       "sp_predict_x0")
        return out


class FusedDPSStep(FusedStep):
    """One guided DPS iteration (``dps.py:91-122``) over a flat batch, on HIP.
    ``observation_rows`` as ``FusedStep``."""

    def __init__(self, network: EpsilonNetwork, inverse_problem: InverseProblem,
                 observation_rows: Tensor, y_div: int, *, gamma: float = 1.0, eta: float = 1.0,
                 micro_batch: int | None = None, timer: KernelTimer | None = None,
                 reuse_v: bool = False, mode: str = "dps", guidance_weight: float = 1.0) -> None:
        op = inverse_problem.operator
        desc = _hip.descriptor_of(op)
        if desc is None:
            raise NotImplementedError(
                f"{type(op).__name__} has no native (HIP) implementation; the fused DPS path "
                "supports IdentityOperator, InpaintingOperator (and subclasses), "
                "GaussianBlurOperator, SuperResolutionOperator, PSFBlurOperator (and subclasses), "
                "FFTPSFBlurOperator, PeriodicBlurOperator, PeriodicSuperResolutionOperator, "
                "SeparableSVDOperator, HadamardOperator, ChannelMixOperator, RadonOperator and "
                "PhaseRetrievalOperator"
            )
        super().__init__(network, op, y_div, micro_batch, timer)
        self._bind_rows(observation_rows, "DPSSampler")
        self.desc = desc
        self.m = int(desc.m)
        self.n = int(desc.n)
        self.partials = int(self.lib.sp_rsq_partials(desc))
        if self.partials <= 0:
            raise _hip.HipLibraryError(f"operator descriptor rejected ({self.partials})")
        if mode not in ("dps", "pgdm"):
            raise ValueError(mode)
        self.traits = int(self.lib.sp_op_traits(desc))
        self.pinv = bool(self.traits & _hip.SP_TRAIT_PINV)
        if mode == "pgdm" and not self.traits & (_hip.SP_TRAIT_LINEAR | _hip.SP_TRAIT_PINV):
            raise NotImplementedError(f"{type(op).__name__} has no apply_pseudo_inverse (nonlinear, "
                                      "or a blur through a workspace): PGDM does not apply")
        self.mode = mode
        # DPS: d log p/d(Ax) = c r.  PGDM: d/dx0 of ||A^+ y - A^+ A x0||^2 = -c A^T r with the
        # operator's pinv_grad_scale c: 2 for the partial isometries (A^+ = A^T: identity,
        # inpainting, mask), 2 s^2 for x s super-resolution (A^+ = s^2 A^T).  A kind with a
        # pseudo-inverse of its own (SP_TRAIT_PINV): v = -2 (A^+ y - A^+ A x0) from sp_pgdm_residual_ws.
        self.grad_scale = -float(getattr(op, "pinv_grad_scale", 2.0))
        if mode == "dps":
            gs = getattr(inverse_problem.noise, "grad_scale", None)
            if gs is None:
                from samplers_amd.noise import probe_grad_scale

                gs = lambda: probe_grad_scale(inverse_problem.noise)  # noqa: E731
            c = gs()
            if c is None:
                raise NotImplementedError(f"{type(inverse_problem.noise).__name__} has no constant "
                                          "likelihood-gradient factor; use GenericDPSStep")
            self.grad_scale = float(c)
        self.guidance_weight = float(guidance_weight)
        self.gamma, self.eta = float(gamma), float(eta)
        # pass 2 re-derives v from (x, eps, y) (default: SURVEY §8d's minimal bytes, 4n + m per
        # sample; with non-temporal loads and 2 float4 groups per thread it is 7 % faster than
        # re-reading pass 1's v, 42.3 vs 45.2 us at B = 64, 256^2) or re-reads v (reuse_v, and
        # always for the kinds whose pass 2 is the identity-kind kernel over v: the library's trait).
        self.needs_v = bool(self.traits & _hip.SP_TRAIT_UPDATE_READS_V) or bool(reuse_v)
        # PGDM through the kind's own pseudo-inverse: Q = P FFT2(y), once (y is fixed across steps)
        if mode == "pgdm" and self.pinv:
            if int(self.lib.sp_op_workspace(desc, 1)) == 0:
                self.q = self.y  # nothing to prepare: the launch reads the rows themselves
            else:
                self._prepare_q("sp_op_workspace", "sp_pgdm_prepare")

    def coefficients(self, t: int, t_prev: int, s: int) -> _hip.SpDpsCoefs:
        acp = host_alphas_cumprod(self.network)
        a, k = x0_coefficients(acp, t)
        br = bridge_coefficients(acp, ell=t, t=t_prev, s=s, eta=self.eta)
        # PGDM: sample = ddim - guidance_weight * sqrt(1 - acp_t) * grad   (pgdm.py:131-135)
        gamma = self.gamma if self.mode == "dps" else float(np.float32(-self.guidance_weight) *
                                                                  np.float32(k))
        return _hip.SpDpsCoefs(a, k, self.grad_scale, br.c_ell, br.c_s, br.std, gamma, 1e-9)

    def workspace(self, batch: int, like: Tensor) -> Tensor | None:
        """Pass 1's work buffer for ``batch`` samples (``sp_dps_workspace`` floats; None where
        the operator's pass needs none).  Allocated by torch on the launch stream, so a graph
        capture records it like every other buffer of the step."""
        if not self.traits & _hip.SP_TRAIT_DPS_WORKSPACE:  # one-pass kinds: no host call in the step loop
            return None
        floats = int(self.lib.sp_dps_workspace(self.desc, batch))
        if floats < 0:
            raise _hip.HipLibraryError(f"sp_dps_workspace rejected the descriptor ({floats})")
        return torch.empty(floats, device=like.device, dtype=torch.float32) if floats else None

    def __call__(self, x: Tensor, step: int, t: int, t_prev: int, s: int, *,
                 xi: Tensor | None = None, seed: int = 0, sample_offset: int = 0) -> Tensor:
        """Advance ``x`` (flat ``(B, *x_shape)``, contiguous fp32) one step, in place."""
        lib, desc = self.lib, self.desc
        coefs = self.coefficients(t, t_prev, s)
        stream = _hip.stream_of(x)
        batch = x.shape[0]
        for b0, b1 in self._chunks(batch):
            xc = x[b0:b1]
            bc = b1 - b0
            yc = self.y[b0 // self.y_div:]
            with torch.enable_grad():
                xr = xc.detach().requires_grad_(True)
                eps = self.network.forward(xr, t)
            eps_c = eps.detach()
            if not eps_c.is_contiguous():
                eps_c = eps_c.contiguous()
            v = torch.empty_like(xc)
            part = torch.empty((bc, self.partials), device=x.device, dtype=torch.float32)
            with self._timed("dps_residual", bc):
                work = self.workspace(bc, xc)
                if self.q is not None:
                    _hip.check(lib.sp_pgdm_residual_ws(desc, _hip.ptr(xc), _hip.ptr(eps_c),
                                                       _hip.ptr(self.q[b0 // self.y_div:]), bc,
                                                       self.y_div, coefs, _hip.ptr(v), _hip.ptr(work),
                                                       stream), "sp_pgdm_residual_ws")
                else:
                    _hip.check(lib.sp_dps_residual_ws(desc, _hip.ptr(xc), _hip.ptr(eps_c),
                                                      _hip.ptr(yc), bc, self.y_div, coefs, _hip.ptr(v),
                                                      _hip.ptr(part), _hip.ptr(work), stream),
                               "sp_dps_residual_ws")
            (w,) = torch.autograd.grad(eps, xr, grad_outputs=v.view_as(eps))
            del eps, xr
            w = w.contiguous()
            xic = None if xi is None else xi[b0:b1].contiguous()
            with self._timed("dps_update", bc):
                _hip.check(lib.sp_dps_update(desc, _hip.ptr(xc), _hip.ptr(eps_c), _hip.ptr(yc),
                                             _hip.ptr(v) if self.needs_v else None, _hip.ptr(w),
                                             _hip.ptr(part) if self.mode == "dps" else None,
                                             _hip.ptr(xic), seed, step,
                                             sample_offset + b0, bc, self.y_div, coefs, _hip.ptr(xc),
                                             stream),
                           "sp_dps_update")
        return x


class GenericDPSStep(FusedDPSStep):
    """One DPS / PGDM iteration for plugins the HIP library does not know.

    The reference differentiates through *any* ``Operator`` and ``NoiseModel``
    (``dps.py:99-103``, ``pgdm.py:104-119``).  Here the residual cotangent
    ``v = ∂(objective)/∂x̂₀`` comes from torch autograd through the plugin's own
    ``apply`` (and ``log_prob`` / ``apply_pseudo_inverse``) on the device, and everything
    else stays on the HIP path: x̂₀ by ``sp_predict_x0``, the prior's input-VJP with
    ``grad_outputs = v``, and pass 2 (``sp_dps_update`` over an identity descriptor of
    the sample, v given) for the bridge mean, noise and guidance.  The per-sample
    ``‖r_b‖²`` enters pass 2 through its partial-sum slot (column 0, the rest zero, so
    the fixed-order sum is exact).
    """

    def __init__(self, network: EpsilonNetwork, inverse_problem: InverseProblem,
                 observation_rows: Tensor, y_div: int, *, gamma: float = 1.0, eta: float = 1.0,
                 micro_batch: int | None = None, timer: KernelTimer | None = None,
                 mode: str = "dps", guidance_weight: float = 1.0, **_unused) -> None:
        from samplers_amd.operators import IdentityOperator

        if mode not in ("dps", "pgdm"):
            raise ValueError(mode)
        _hip.require_cuda(observation_rows, "DPSSampler")
        self.lib = _hip.load_library()
        self.network = network
        self.problem = inverse_problem
        self.operator = inverse_problem.operator
        self.x_shape = tuple(self.operator.x_shape)
        self.desc = IdentityOperator(self.x_shape).hip_descriptor()
        self.n = self.m = int(self.desc.n)
        self.partials = int(self.lib.sp_rsq_partials(self.desc))
        self.y = observation_rows
        self.y_div = int(y_div)
        self.mode = mode
        self.grad_scale = 0.0  # unused: v comes from autograd
        self.guidance_weight = float(guidance_weight)
        self.gamma, self.eta = float(gamma), float(eta)
        self.needs_v = True
        self.micro_batch = micro_batch
        self.timer = timer
        self._pinv_y = None

    def _rows(self, b0: int, b1: int) -> Tensor:
        idx = torch.arange(b0, b1, device=self.y.device) // self.y_div
        return self.y.index_select(0, idx)

    def _cotangent(self, x0: Tensor, b0: int, b1: int) -> tuple[Tensor, Tensor | None]:
        """(v = ∂ objective / ∂x̂₀, ‖r_b‖² per sample or None) by autograd through the plugin."""
        op = self.operator
        y = self._rows(b0, b1)
        with torch.enable_grad():
            x0r = x0.detach().requires_grad_(True)
            if self.mode == "dps":  # inverse_problem.log_likelihood (inverse_problem.py:17-21)
                r = y - op.apply(x0r)
                obj = self.problem.noise.log_prob(r).sum()
            else:  # PGDM consistency loss (pgdm.py:110-115)
                y_inv = op.apply_pseudo_inverse(y)
                obj = (y_inv - op.apply_pseudo_inverse(op.forward(x0r))).pow(2).sum()
                r = None
            (v,) = torch.autograd.grad(obj, x0r)
        rsq = None
        if r is not None:
            rsq = r.detach().reshape(r.shape[0], -1).float().square().sum(dim=1)
        return v.to(torch.float32).contiguous(), rsq

    def __call__(self, x: Tensor, step: int, t: int, t_prev: int, s: int, *,
                 xi: Tensor | None = None, seed: int = 0, sample_offset: int = 0) -> Tensor:
        lib, desc = self.lib, self.desc
        coefs = self.coefficients(t, t_prev, s)
        stream = _hip.stream_of(x)
        for b0, b1 in self._chunks(x.shape[0]):
            xc = x[b0:b1]
            bc = b1 - b0
            with torch.enable_grad():
                xr = xc.detach().requires_grad_(True)
                eps = self.network.forward(xr, t)
            eps_c = eps.detach().contiguous()
            x0 = torch.empty_like(xc)
            _hip.check(lib.sp_predict_x0(_hip.ptr(xc), _hip.ptr(eps_c), xc.numel(), coefs.a,
                                         coefs.k, _hip.ptr(x0), stream), "sp_predict_x0")
            v, rsq = self._cotangent(x0, b0, b1)
            part = None
            if rsq is not None:
                part = torch.zeros((bc, self.partials), device=x.device, dtype=torch.float32)
                part[:, 0] = rsq
            (w,) = torch.autograd.grad(eps, xr, grad_outputs=v.view_as(eps))
            del eps, xr
            xic = None if xi is None else xi[b0:b1].contiguous()
            _hip.check(lib.sp_dps_update(desc, _hip.ptr(xc), _hip.ptr(eps_c), None, _hip.ptr(v),
                                         _hip.ptr(w.contiguous()), _hip.ptr(part), _hip.ptr(xic),
                                         seed, step, sample_offset + b0, bc, 1, coefs,
                                         _hip.ptr(xc), stream), "sp_dps_update")
        return x


def native_plugins(inverse_problem) -> bool:
    """True when the operator has a HIP descriptor and the noise a constant ∂log p/∂(Ax)
    factor, i.e. the fused passes can replace autograd entirely."""
    if _hip.descriptor_of(inverse_problem.operator) is None:
        return False
    gs = getattr(inverse_problem.noise, "grad_scale", None)
    if gs is None:
        from samplers_amd.noise import probe_grad_scale

        return probe_grad_scale(inverse_problem.noise) is not None
    return gs() is not None


def host_svd_operator(operator, observation: Tensor) -> bool:
    """An ``SVDOperator`` with HIP kernels whose observation lives on the host: its maps are plain
    torch there, so PGDM, DiffPIR and DDRM run it in torch (set-up and reference runs)."""
    from samplers_amd.operators.linear import SVDOperator

    return (isinstance(operator, SVDOperator) and _hip.descriptor_of(operator) is not None
            and not observation.is_cuda)


def host_predict_x0(step: FusedStep, x: Tensor, t: int) -> Tensor:
    """``predict_x0`` in plain torch: the prior's forward and ``(x − k·eps)/a``."""
    a, k = x0_coefficients(host_alphas_cumprod(step.network), t)
    out = torch.empty_like(x)
    for b0, b1 in step._chunks(x.shape[0]):
        with torch.no_grad():
            out[b0:b1] = (x[b0:b1] - k * step.network.forward(x[b0:b1], t)) / a
    return out


def host_noise(xi: Tensor | None) -> Tensor:
    if xi is None:
        raise ValueError("rng='philox' draws on the device; on host tensors pass rng='torch' or a "
                         "noise_fn")
    return xi


class HostPGDMStep(FusedStep):
    """One PGDM iteration on host tensors for ``host_svd_operator``s (``pgdm.py:104-135`` as
    written): x̂₀, the gradient of ‖A⁺y − A⁺A x̂₀‖² in the sample by autograd through the prior and
    the operator's host maps, the bridge update in torch.  The device path is ``FusedDPSStep``."""

    def __init__(self, network: EpsilonNetwork, inverse_problem: InverseProblem,
                 observation_rows: Tensor, y_div: int, *, eta: float = 1.0,
                 micro_batch: int | None = None, timer: KernelTimer | None = None,
                 guidance_weight: float = 1.0, **_unused) -> None:
        super().__init__(network, inverse_problem.operator, y_div, micro_batch, timer)
        self.y = observation_rows
        self.eta, self.guidance_weight = float(eta), float(guidance_weight)

    def __call__(self, x: Tensor, step: int, t: int, t_prev: int, s: int, *,
                 xi: Tensor | None = None, seed: int = 0, sample_offset: int = 0) -> Tensor:
        xi, op = host_noise(xi), self.operator
        acp = host_alphas_cumprod(self.network)
        a, k = x0_coefficients(acp, t)
        br = bridge_coefficients(acp, ell=t, t=t_prev, s=s, eta=self.eta)
        for b0, b1 in self._chunks(x.shape[0]):
            xc = x[b0:b1]
            y = self.y[torch.arange(b0, b1) // self.y_div].to(xc.dtype)
            with torch.enable_grad():
                xr = xc.detach().requires_grad_(True)
                x0 = (xr - k * self.network.forward(xr, t)) / a
                loss = (op.apply_pseudo_inverse(y) - op.apply_pseudo_inverse(op.apply(x0))).pow(2).sum()
                (grad,) = torch.autograd.grad(loss, xr)
            with torch.no_grad():
                xc.copy_(br.c_ell * xc + br.c_s * x0.detach() + br.std * xi[b0:b1]
                         - self.guidance_weight * k * grad)
        return x

    def predict_x0(self, x: Tensor, t: int) -> Tensor:
        return host_predict_x0(self, x, t)


def make_dps_step(network, inverse_problem, observation_rows, y_div, **kw):
    """The fused HIP step for native plugins, the generic-plugin step otherwise."""
    mode = kw.get("mode", "dps")
    if mode == "pgdm" and host_svd_operator(inverse_problem.operator, observation_rows):
        return HostPGDMStep(network, inverse_problem, observation_rows, y_div, **kw)
    native_op = _hip.descriptor_of(inverse_problem.operator) is not None
    if (mode == "dps" and native_plugins(inverse_problem)) or (mode == "pgdm" and native_op):
        return FusedDPSStep(network, inverse_problem, observation_rows, y_div, **kw)
    return GenericDPSStep(network, inverse_problem, observation_rows, y_div, **kw)


# hipGraph replay by default where it pays: below GRAPH_AUTO_MAX_BATCH samples.
# Measured (profiles/round5/final/bench_call_b1.json): a whole 1000-step call at batch 1 runs
# 9.47 ms per step eager and 10.05 ms replayed — the captured step runs GroupNorm's two-pass
# kernels, and the eager step is no longer host-bound once no per-launch timing events are
# attached (bench.py's B = 1 eager figure, 11.4 ms, carries them); from batch 2 on the eager step
# wins by more (tools/graph_sweep.sh).  So the automatic choice is off (0); graph=True replays.
# Capture costs about three steps (two warm-up steps and the capture), so short solves stay eager.
GRAPH_AUTO_MAX_BATCH = 0
GRAPH_AUTO_MIN_STEPS = 8


def graph_auto(step, x: Tensor, guided_steps: int, *, rng: str, noise_fn, callback,
               micro_batch: int | None) -> bool:
    """Whether ``DPSSampler(graph=None)`` replays a captured step: the fused HIP step (native
    operator and noise plugins), in-kernel Philox noise, no callback / kernel timer /
    micro-batching, a flat batch of at most ``GRAPH_AUTO_MAX_BATCH`` and at least
    ``GRAPH_AUTO_MIN_STEPS`` guided iterations, and a prior that declares itself capturable
    (``graph_capturable``: this project's priors, whose layers run on HIP kernels and
    allocate nothing outside torch's caching allocator; a third-party network stays eager
    unless it sets the flag).  ``SAMPLERS_AMD_GRAPH=0`` turns the automatic choice off."""
    import os

    if os.environ.get("SAMPLERS_AMD_GRAPH", "auto").lower() in ("0", "off", "false", "eager"):
        return False
    return (getattr(step.network, "graph_capturable", False)
            and isinstance(step, FusedDPSStep) and not isinstance(step, GenericDPSStep)
            and step.timer is None and rng == "philox" and noise_fn is None and callback is None
            and (not micro_batch or micro_batch >= x.shape[0]) and x.is_cuda
            and 0 < x.shape[0] <= GRAPH_AUTO_MAX_BATCH and guided_steps >= GRAPH_AUTO_MIN_STEPS)


class DPSSampler(PosteriorSampler, Generic[Condition_co]):
    """DPS (Chung et al., 2022) with the guided step fused into two HIP passes."""

    def __call__(
        self,
        inverse_problem: InverseProblem,
        num_sampling_steps: int = 50,
        num_reconstructions: int = 1,
        gamma: float = 1.0,
        eta: float = 1.0,
        condition: Condition_co | None = None,
        keep_reconstruction_dim: bool = False,
        *args,
        rng: str = "philox",
        seed: int | None = None,
        noise_fn: NoiseFn | None = None,
        sample_offset: int = 0,
        micro_batch: int | None = None,
        timer: KernelTimer | None = None,
        graph: bool | None = None,
        callback: Callable[[int, Tensor], None] | None = None,
        **kwargs,
    ) -> Tensor:
        """Run DPS; returns ``(*batch_shape, R, *x_shape)`` (R squeezed when 1).

        Extra keyword-only options (all default to the reference behaviour):
        ``rng`` / ``seed`` / ``noise_fn`` choose the noise source (module
        docstring); ``sample_offset`` is the global index of this shard's first
        flat sample (multi-GPU, keeps Philox streams shard-invariant);
        ``micro_batch`` bounds how many samples share one prior forward+VJP;
        ``graph=True`` replays one hipGraph-captured step for every iteration
        (``samplers.graph``; Philox noise only) — same samples, no per-launch host work;
        ``graph=None`` (default) applies the automatic rule ``graph_auto`` (native plugins,
        Philox noise, no callback / timer / micro-batching, a flat batch of at most
        ``GRAPH_AUTO_MAX_BATCH`` and enough steps) — currently **off**: ``GRAPH_AUTO_MAX_BATCH``
        is 0 because replay measured slower than eager at every batch, so
        ``graph=None`` runs eagerly; ``graph=False`` always runs eagerly;
        ``callback(i, x)`` is called after guided iteration ``i`` with the flat sample (a view of
        the working buffer: copy it to keep it; not with ``graph=True``).
        """
        if args or kwargs:
            print(f"Warning: Unused args={args}, kwargs={kwargs} in DPSSampler")

        def make_step(net, y_rows):
            return make_dps_step(net, inverse_problem, y_rows, num_reconstructions, gamma=gamma,
                                 eta=eta, micro_batch=micro_batch, timer=timer)

        def advance(step, x, ts, seed, loop):
            replay = graph
            if replay is None:
                replay = graph_auto(step, x, len(ts) - 2, rng=rng, noise_fn=noise_fn,
                                    callback=callback, micro_batch=micro_batch)
            self.execution = "graph" if replay else "eager"  # what the last call ran
            if not replay:
                return loop(callback)
            if not isinstance(step, FusedDPSStep) or isinstance(step, GenericDPSStep):
                raise ValueError("graph=True needs natively implemented plugins")
            if noise_fn is not None or rng != "philox":
                raise ValueError("graph=True needs the in-kernel Philox noise (rng='philox')")
            if callback is not None:
                raise ValueError("graph=True replays the steps without returning to the host: "
                                 "no per-iteration callback")
            from .graph import GraphedStepLoop, schedule_for

            GraphedStepLoop(step, x, schedule_for(ts), seed=seed,
                            sample_offset=sample_offset).replay()

        return run_sampler(self, inverse_problem, make_step, num_sampling_steps=num_sampling_steps,
                           num_reconstructions=num_reconstructions, condition=condition, rng=rng,
                           seed=seed, noise_fn=noise_fn, sample_offset=sample_offset,
                           keep_reconstruction_dim=keep_reconstruction_dim, require="DPSSampler",
                           anchored=True, advance=advance)
