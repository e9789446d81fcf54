"""DiffPIR: denoising diffusion models for plug-and-play image restoration (Zhu et al., 2023).

The reference has no such sampler; the semantics are this project's own, stated in DESIGN.md §3
and in fp64 by ``tests/prox_ref.py``.  The loop is ``PGDMSampler``'s (``i = len(ts)−1 … 2``,
``t = ts[i]``, ``t_prev = ts[i−1]``, the Philox step index is ``i``, the result is
``predict_x0(x, ts[1])``); one step is::

    eps = unet(x, t)                                      the prior, under no_grad: no VJP
    x  <- sp_diffpir_step_ws(x, eps, y | q, noise)        HIP: x0, the proximal data step, the update

with ``x0 = (x − k·eps)/a``, ``z = argmin_u ‖y − A u‖² + ρ_t ‖u − x0‖²``,
``eps_hat = (x − a·z)/k`` and ``x' = a_prev·z + k_prev·(sqrt(1−ζ)·eps_hat + sqrt(ζ)·ξ)``, where
``ρ_t = λ · max(σ_n, σ_min)² · ᾱ_t / (1 − ᾱ_t)``.  The network is called once per step and never
differentiated, which is where the step's time goes in DPS and PGDM.

``prox="closed_form"`` (the default) runs only the operators whose proximal map has a closed form
(``Operator.apply_prox``: identity, inpainting / mask, ×s super-resolution, periodic blur, periodic
blur-and-decimate super-resolution); the others raise ``NotImplementedError``.  ``prox="cg"``
computes ``z`` by ``cg_iterations`` steps of conjugate gradients with a per-sample stop at
``cg_tol`` (``sp_diffpir_step_cg_ws``, ``Operator.apply_prox_cg``) for every linear operator with
a HIP descriptor: the Gaussian, PSF and FFT blurs and the Radon transform too.  ``prox="auto"``
takes the closed form where there is one and conjugate gradients elsewhere.
The noise model must be ``GaussianNoise``: σ_n enters ρ_t.  The step runs eagerly (no graph
replay form).  Noise sources (``rng`` / ``seed`` / ``noise_fn``) are ``DPSSampler``'s.
"""

from __future__ import annotations

from typing import Generic, TypeVar

import torch
from torch import Tensor

from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.networks.base import EpsilonNetwork, host_alphas_cumprod
from samplers_amd.noise import GaussianNoise
from samplers_amd.samplers.base import PosteriorSampler
from samplers_amd.samplers.dps import (FusedStep, KernelTimer, NoiseFn, host_noise, host_predict_x0,
                                       host_svd_operator)
from samplers_amd.samplers.loop import run_sampler
from samplers_amd.samplers.utils.bridge_kernels import diffpir_coefficients

Condition_co = TypeVar("Condition_co", covariant=True)


def prox_descriptor(operator) -> "_hip.SpOp":
    """The operator's HIP descriptor if the library has a proximal map for its kind
    (``sp_prox_workspace`` is the probe; it answers on the host), else ``NotImplementedError``
    naming the operator."""
    desc = _hip.descriptor_of(operator)
    if desc is None or int(_hip.load_library().sp_prox_workspace(desc, 1)) < 0:
        raise NotImplementedError(
            f"{type(operator).__name__} has no closed-form proximal map (apply_prox): DiffPIR "
            "supports IdentityOperator, InpaintingOperator (and subclasses), "
            "SuperResolutionOperator, PeriodicBlurOperator, "
            "PeriodicSuperResolutionOperator, SeparableSVDOperator, HadamardOperator and "
            "ChannelMixOperator")
    return desc


PROX_MODES = ("closed_form", "cg", "auto")


def cg_descriptor(operator) -> "_hip.SpOp":
    """The operator's HIP descriptor if ``sp_diffpir_step_cg_ws`` serves its kind (every linear
    kind; ``sp_prox_cg_workspace`` is the probe), else ``NotImplementedError`` naming it."""
    desc = _hip.descriptor_of(operator)
    if desc is None or int(_hip.load_library().sp_prox_cg_workspace(desc, 1, 1)) < 0:
        raise NotImplementedError(
            f"{type(operator).__name__} has no linear HIP maps for the conjugate-gradient "
            "proximal step (prox='cg'): DiffPIR needs a linear operator with a HIP descriptor")
    return desc


class FusedDiffPIRStep(FusedStep):
    """One DiffPIR iteration over a flat batch: the prior's forward under ``no_grad`` and
    ``sp_diffpir_step_ws``.  Owns what is fixed across the steps: ``q`` (the prepared observation
    of the kinds that transform it, once per call), the workspace of a chunk and the micro-batch
    chunks.  ``observation_rows`` as ``FusedDPSStep``.  With ``prox="cg"`` (or ``"auto"`` on a kind
    without a closed form) the data step is ``sp_diffpir_step_cg_ws``; ``iterations`` then holds the
    live iterations of every step so far, an int32 device tensor ``(steps, batch)`` that the loop
    appends to and never reads."""

    def __init__(self, network: EpsilonNetwork, inverse_problem: InverseProblem,
                 observation_rows: Tensor, y_div: int, *, guidance_weight: float = 7.0,
                 zeta: float = 0.3, min_noise_std: float = 1e-3, micro_batch: int | None = None,
                 timer: KernelTimer | None = None, prox: str = "closed_form",
                 cg_iterations: int = 16, cg_tol: float = 1e-4) -> None:
        op, noise = inverse_problem.operator, inverse_problem.noise
        if not isinstance(noise, GaussianNoise):
            raise ValueError(f"DiffPIR needs GaussianNoise (its sigma sets rho), got "
                             f"{type(noise).__name__}")
        self.sigma = float(noise.sigma.detach().cpu().item())
        self.guidance_weight, self.zeta = float(guidance_weight), float(zeta)
        self.min_noise_std = float(min_noise_std)
        if not 0.0 <= self.zeta <= 1.0:
            raise ValueError(f"zeta must be in [0, 1], got {zeta}")
        if not self.guidance_weight > 0.0:
            raise ValueError(f"guidance_weight must be positive, got {guidance_weight}")
        if prox not in PROX_MODES:
            raise ValueError(f"prox must be one of {PROX_MODES}, got {prox!r}")
        if int(cg_iterations) != cg_iterations or int(cg_iterations) < 1:
            raise ValueError(f"cg_iterations must be a positive integer, got {cg_iterations!r}")
        if not (float(cg_tol) >= 0.0 and float(cg_tol) < float("inf")):
            raise ValueError(f"cg_tol must be non-negative and finite, got {cg_tol}")
        self.cg_iterations, self.cg_tol = int(cg_iterations), float(cg_tol)
        self.cg = prox == "cg"
        if prox == "auto":  # the closed form where sp_prox_workspace has one
            desc = _hip.descriptor_of(op)
            self.cg = desc is None or int(_hip.load_library().sp_prox_workspace(desc, 1)) < 0
        self.desc = cg_descriptor(op) if self.cg else prox_descriptor(op)
        self.iterations: Tensor | None = None
        super().__init__(network, op, y_div, micro_batch, timer)
        # an SVDOperator with HIP kernels runs through its host maps on host tensors
        self.host = host_svd_operator(op, observation_rows)
        if self.host:
            self.y = observation_rows
            return
        self._bind_rows(observation_rows, "DiffPIRSampler")
        if not self.cg:  # conjugate gradients prepare nothing: the maps read y itself
            self._prepare_q("sp_prox_prepare_size", "sp_prox_prepare", optional=True)

    def coefficients(self, t: int, t_prev: int) -> _hip.SpProxCoefs:
        c = diffpir_coefficients(host_alphas_cumprod(self.network), t, t_prev, self.sigma,
                                 self.guidance_weight, self.zeta, self.min_noise_std)
        return _hip.SpProxCoefs(c.a, c.k, c.rho, c.a_prev, c.c_eps, c.c_xi)

    def workspace(self, batch: int, like: Tensor) -> Tensor | None:
        """The step's work buffer for ``batch`` samples (``sp_prox_workspace`` floats), kept
        between steps; None where the kind needs none."""
        if self.q is None and not self.cg:
            return None
        floats = int(self.lib.sp_prox_cg_workspace(self.desc, batch, 1) if self.cg
                     else self.lib.sp_prox_workspace(self.desc, batch))
        if floats < 0:
            raise _hip.HipLibraryError(f"sp_prox_workspace rejected the descriptor ({floats})")
        return self._kept_work(floats, like)

    def __call__(self, x: Tensor, step: int, t: int, t_prev: int, *, xi: Tensor | None = None,
                 seed: int = 0, sample_offset: int = 0) -> Tensor:
        """Advance ``x`` (flat ``(B, *x_shape)``, contiguous fp32) one step, in place."""
        coefs = self.coefficients(t, t_prev)
        if self.host:
            return self._host_step(x, coefs, t, host_noise(xi))
        stream = _hip.stream_of(x)
        iters = torch.zeros(x.shape[0], device=x.device, dtype=torch.int32) if self.cg else None
        for b0, b1 in self._chunks(x.shape[0]):
            xc, bc, row = x[b0:b1], b1 - b0, b0 // self.y_div
            with torch.no_grad():
                eps = self.network.forward(xc, t)
            eps = eps.contiguous()
            xic = None if xi is None else xi[b0:b1].contiguous()
            with self._timed("diffpir_step", bc):
                if self.cg:
                    _hip.check(self.lib.sp_diffpir_step_cg_ws(
                        self.desc, _hip.ptr(xc), _hip.ptr(eps), _hip.ptr(self.y[row:]),
                        _hip.ptr(xic), seed, step, sample_offset + b0, bc, self.y_div, coefs,
                        self.cg_iterations, self.cg_tol, _hip.ptr(xc), _hip.ptr(iters[b0:b1]),
                        _hip.ptr(self.workspace(bc, xc)), stream), "sp_diffpir_step_cg_ws")
                else:
                    _hip.check(self.lib.sp_diffpir_step_ws(
                        self.desc, _hip.ptr(xc), _hip.ptr(eps), _hip.ptr(self.y[row:]),
                        _hip.ptr(self.q[row:]) if self.q is not None else None, _hip.ptr(xic), seed,
                        step, sample_offset + b0, bc, self.y_div, coefs, _hip.ptr(xc),
                        _hip.ptr(self.workspace(bc, xc)), stream), "sp_diffpir_step_ws")
        if iters is not None:  # appended on the device; nothing here waits for it
            self.iterations = (iters[None] if self.iterations is None
                               else torch.cat([self.iterations, iters[None]]))
        return x


    def _host_step(self, x: Tensor, c: _hip.SpProxCoefs, t: int, xi: Tensor) -> Tensor:
        """The step in plain torch through ``apply_prox`` / ``apply_prox_cg`` on host tensors."""
        op = self.operator
        iters = torch.zeros(x.shape[0], dtype=torch.int32)
        with torch.no_grad():
            for b0, b1 in self._chunks(x.shape[0]):
                xc = x[b0:b1]
                y = self.y[torch.arange(b0, b1) // self.y_div].to(xc.dtype)
                x0 = (xc - c.k * self.network.forward(xc, t)) / c.a
                if self.cg:
                    z, iters[b0:b1] = op.apply_prox_cg(x0, y, c.rho, self.cg_iterations, self.cg_tol,
                                                       return_iterations=True)
                else:
                    z = op.apply_prox(x0, y, c.rho)
                xc.copy_(c.a_prev * z + (c.c_eps * ((xc - c.a * z) * (1.0 / c.k)) + c.c_xi * xi[b0:b1]))
        if self.cg:
            self.iterations = (iters[None] if self.iterations is None
                               else torch.cat([self.iterations, iters[None]]))
        return x

    def predict_x0(self, x: Tensor, t: int) -> Tensor:
        return host_predict_x0(self, x, t) if self.host else super().predict_x0(x, t)


class DiffPIRSampler(PosteriorSampler, Generic[Condition_co]):
    """DiffPIR (Zhu et al., 2023): one network call per step, the data step a proximal map (in
    closed form, or by conjugate gradients for the linear operators without one) fused with the
    update into HIP launches."""

    def __call__(
        self,
        inverse_problem: InverseProblem,
        num_sampling_steps: int = 100,
        num_reconstructions: int = 1,
        guidance_weight: float = 7.0,
        zeta: float = 0.3,
        min_noise_std: float = 1e-3,
        condition: Condition_co | None = None,
        keep_reconstruction_dim: bool = False,
        *args,
        rng: str = "philox",
        seed: int | None = None,
        noise_fn: NoiseFn | None = None,
        sample_offset: int = 0,
        micro_batch: int | None = None,
        timer: KernelTimer | None = None,
        prox: str = "closed_form",
        cg_iterations: int = 16,
        cg_tol: float = 1e-4,
        **kwargs,
    ) -> Tensor:
        """Run DiffPIR; returns ``(*batch_shape, R, *x_shape)`` (R squeezed when 1).
        ``guidance_weight`` is λ, ``zeta`` the share of fresh noise in a step, ``min_noise_std``
        the floor of σ_n inside ρ_t; the keyword-only options are ``PGDMSampler``'s, and
        ``prox`` (``"closed_form"``, ``"cg"`` or ``"auto"``), ``cg_iterations`` and ``cg_tol``
        choose the data step (module docstring).  The step object of the last call stays on the
        sampler as ``last_step`` (its ``iterations``: the conjugate-gradient counts per step)."""
        if args or kwargs:
            print(f"Warning: Unused args={args}, kwargs={kwargs} in DiffPIRSampler")

        def make_step(net, y_rows):
            self.last_step = FusedDiffPIRStep(
                net, inverse_problem, y_rows, num_reconstructions, guidance_weight=guidance_weight,
                zeta=zeta, min_noise_std=min_noise_std, micro_batch=micro_batch, timer=timer,
                prox=prox, cg_iterations=cg_iterations, cg_tol=cg_tol)
            return self.last_step

        return run_sampler(self, inverse_problem, make_step, num_sampling_steps=num_sampling_steps,
                           num_reconstructions=num_reconstructions, condition=condition, rng=rng,
                           seed=seed, noise_fn=noise_fn, sample_offset=sample_offset,
                           keep_reconstruction_dim=keep_reconstruction_dim)
