"""Pseudoinverse-Guided Diffusion Models (mirrors ``/root/reference/samplers/samplers/pgdm.py:18-147``).

Loop body (``pgdm.py:104-135``) on the same two fused HIP passes as DPS:
pass 1 computes v = ∂/∂x0 ||A⁺y − A⁺A x0||² = −c Aᵀ(y − A x0) with the operator's
``pinv_grad_scale`` c (2 for the identity / inpainting / mask operators, which are
partial isometries with A⁺ = Aᵀ; 2·s² for ×s super-resolution, A⁺ = s²·Aᵀ), the
prior's input-VJP gives w = Jᵀv, and pass 2 writes
``ddim_step(x, x0) − guidance_weight·sqrt(1−ᾱ_t)·(v − k w)/a``.
``PeriodicBlurOperator`` has a pseudo-inverse of its own (a per-frequency division): its pass 1
is ``sp_pgdm_residual_ws``, v = −2 (A⁺y − A⁺A x0), over Q = P ⊙ FFT2(y) prepared once per call.
``PeriodicSuperResolutionOperator`` likewise (v = −2 A⁺(y − A x0), q holding y itself), and
``SeparableSVDOperator`` (v = −2 (A⁺y − Π x0) through the SVDs of its two factors, q = P ⊙ U_Hᵀ y U_W;
on host tensors ``HostPGDMStep``, the reference's loop body in plain torch through its host maps).
``HadamardOperator`` (A⁺ = Aᵀ) likewise: v = −2 Aᵀ(y − A x0), q holding y itself.
``ChannelMixOperator``: v = −2 A⁺(y − A x0) per pixel in one launch that reads the observation rows
themselves (no q, no workspace).
Operators without ``apply_pseudo_inverse`` raise ``NotImplementedError`` as in
the reference (``pgdm.py:56-66``).
"""

from __future__ import annotations

from typing import Generic, TypeVar

import torch
from torch import Tensor

from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.samplers.base import PosteriorSampler
from samplers_amd.samplers.dps import KernelTimer, NoiseFn, host_svd_operator, make_dps_step
from samplers_amd.samplers.loop import run_sampler

Condition_co = TypeVar("Condition_co", covariant=True)


class PGDMSampler(PosteriorSampler, Generic[Condition_co]):
    """PGDM (Song et al., ICLR 2023) with the guided step fused into two HIP passes."""

    def __call__(
        self,
        inverse_problem: InverseProblem,
        num_sampling_steps: int = 50,
        num_reconstructions: int = 1,
        guidance_weight: float = 1.0,
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
        **kwargs,
    ) -> Tensor:
        operator = inverse_problem.operator
        try:
            dummy_y = torch.zeros((1, *operator.y_shape),
                                  device=next(operator.buffers(), torch.tensor(0)).device)
            operator.apply_pseudo_inverse(dummy_y)
        except NotImplementedError as exc:
            raise NotImplementedError(
                "The operator in the inverse_problem must implement 'apply_pseudo_inverse' for PGDM."
            ) from exc
        if args or kwargs:
            print(f"Warning: Unused args={args}, kwargs={kwargs} in PGDMSampler")


        def make_step(net, y_rows):
            return make_dps_step(net, inverse_problem, y_rows, num_reconstructions, eta=eta,
                                 micro_batch=micro_batch, timer=timer, mode="pgdm",
                                 guidance_weight=guidance_weight)

        return run_sampler(self, inverse_problem, make_step, num_sampling_steps=num_sampling_steps,
                           num_reconstructions=num_reconstructions, condition=condition, rng=rng,
                           seed=seed, noise_fn=noise_fn, sample_offset=sample_offset,
                           keep_reconstruction_dim=keep_reconstruction_dim,
                           # an SVDOperator with HIP kernels runs through its host maps on host tensors
                           require=None if host_svd_operator(operator, inverse_problem.observation)
                           else "PGDMSampler", anchored=True)
