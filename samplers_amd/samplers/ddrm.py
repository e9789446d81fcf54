"""DDRM: denoising diffusion restoration models (Kawar et al., 2022).

The reference has no such sampler; the semantics are this project's own, stated in DESIGN.md §3
and in fp64 by ``tests/ddrm_ref.py``.  The loop is ``PGDMSampler``'s (``i = len(ts)−1 … 2``,
``t = ts[i]``, ``t_prev = ts[i−1]``, the Philox step index is ``i``, the start is
``initial_sample``, the result is ``predict_x0(x, ts[1])``); one step is::

    eps = unet(x, t)                                   the prior, under no_grad: no VJP
    x  <- sp_ddrm_step_ws(x, eps, y | q, noise)        HIP: x0 and the spectral update

With ``A = U S Vᵀ``, ``x0 = (x − k·eps)/a``, ``ȳ = S⁺Uᵀy``, ``σ' = sqrt(1−ᾱ')/sqrt(ᾱ')`` and
``c₁ = sqrt(1−η²)`` every spectral component of the next sample belongs to one of three classes
by its singular value ``s``:

===============  =================  ================  ===========  =================================
class            condition          f_θ               f_y          f_ξ
===============  =================  ================  ===========  =================================
unobserved       s = 0 or dropped   1 (f_ε = c₁σ')    0            ησ'
observed, small  σ's < σ_y          1 − c₁σ's/σ_y     c₁σ's/σ_y    ησ'
observed, big    σ's ≥ σ_y          1 − η_b           η_b          sqrt(max(σ'² − η_b²σ_y²/s², 0))
===============  =================  ================  ===========  =================================

and ``x' = a'·V[f_θ⊙Vᵀx0 + f_ε⊙Vᵀeps + f_y⊙ȳ + f_ξ⊙Vᵀξ]`` with ``ξ ~ N(0, I)`` in space (V is
orthogonal, so Vᵀξ is white: the noise is the ordinary Philox plane).  σ_y is handled per singular
value — there is no ρ to tune — and every component has exactly the marginal variance σ'² the
schedule asks for.  The class is decided by the one fp32 expression
``(σ'·σ')·s² ≥ σ_y·σ_y``.

The fused path (``sp_ddrm_workspace`` is the probe) serves the identity, inpainting / mask,
×s average-pooling super-resolution, the periodic blur, the separable-SVD operator (any blur
or filtered super-resolution of the form ``A_H X A_Wᵀ``) and the Walsh–Hadamard compressed-sensing
operator (a partial isometry: one class for its whole kept set) and the channel-mixing operator
(colorization: the SVD of its small matrix at every pixel); any other ``SVDOperator`` without a
HIP descriptor takes ``ddrm_step_svd``, the same step in plain torch through its factors (so does
the separable-SVD, Hadamard and channel-mixing operators on host tensors); the rest
raise ``NotImplementedError``.  The noise model must be ``GaussianNoise`` unless ``noise_std`` is
given.  The run starts from ``initial_sample`` rather than DDRM's spectral initialisation: at
``ᾱ_T ≈ 4e-5`` the two coincide.  Noise sources (``rng`` / ``seed`` / ``noise_fn``) are
``DPSSampler``'s.
"""

from __future__ import annotations

from typing import Generic, TypeVar

import torch
from torch import Tensor

from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.networks.base import EpsilonNetwork, host_alphas_cumprod
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators.linear import SVDOperator
from samplers_amd.samplers.base import PosteriorSampler
from samplers_amd.samplers.dps import FusedStep, KernelTimer, NoiseFn
from samplers_amd.samplers.loop import run_sampler
from samplers_amd.samplers.utils.bridge_kernels import (DDRMCoefficients, ddrm_coefficients,
                                                        x0_coefficients)

Condition_co = TypeVar("Condition_co", covariant=True)

SUPPORTED = ("IdentityOperator, InpaintingOperator (and subclasses), SuperResolutionOperator, "
             "PeriodicBlurOperator, SeparableSVDOperator, HadamardOperator, ChannelMixOperator, or an "
             "SVDOperator without "
             "a HIP descriptor (GeneralSVDOperator)")


def ddrm_descriptor(operator) -> "_hip.SpOp | None":
    """The operator's HIP descriptor if the library has a DDRM step for its kind
    (``sp_ddrm_workspace`` is the probe; it answers on the host), else None."""
    desc = _hip.descriptor_of(operator)
    if desc is None or int(_hip.load_library().sp_ddrm_workspace(desc, 1)) < 0:
        return None
    return desc


def ddrm_step_svd(operator: SVDOperator, x: Tensor, eps: Tensor, y: Tensor, xi: Tensor,
                  coefs: DDRMCoefficients) -> Tensor:
    """One DDRM step for any ``SVDOperator``, in plain torch through ``apply_U_transpose``,
    ``apply_V`` and ``apply_V_transpose``, in the tensors' dtype on their device.  The projector
    form over span(V), so thin factors work: what lies outside span(V) is unobserved,

        x'/a' = [x0 + c₁σ'·eps + ησ'·ξ]
                + V[(f_θ−1)⊙Vᵀx0 + (f_ε−c₁σ')⊙Vᵀeps + (f_ξ−ησ')⊙Vᵀξ + f_y⊙ȳ].

    ``x``, ``eps``, ``xi``: ``(B, *x_shape)``; ``y``: ``(B, *y_shape)`` or one row per
    ``B / rows`` consecutive samples."""
    c, dt = coefs, x.dtype
    s = operator.get_singular_values().to(dt)
    scal = lambda v: torch.tensor(v, dtype=dt, device=x.device)  # noqa: E731
    sp, sy, eta, eb, c1 = scal(c.sig_prev), scal(c.sig_y), scal(c.eta), scal(c.eta_b), scal(c.c1)
    s2 = s * s
    observed = s2 > 0
    big = observed & ((sp * sp) * s2 >= sy * sy)
    small = observed & ~big
    safe_s2 = torch.where(observed, s2, torch.ones_like(s2))
    r = torch.where(small, (c1 * sp) * s / torch.where(small, sy, torch.ones_like(sy)),
                    torch.zeros_like(s))
    es, ce = eta * sp, c1 * sp
    f_th = torch.where(big, 1 - eb, 1 - r)
    f_y = torch.where(big, eb.expand_as(s), r)
    f_ep = torch.where(observed, torch.zeros_like(s), ce)
    f_xi = torch.where(big, torch.sqrt(torch.clamp(sp * sp - (eb * sy) ** 2 / safe_s2, min=0)), es)
    if y.shape[0] != x.shape[0]:
        y = y.repeat_interleave(x.shape[0] // y.shape[0], dim=0)
    ybar = torch.where(observed, operator.apply_U_transpose(y.to(dt)) /
                       torch.where(observed, s, torch.ones_like(s)), torch.zeros_like(s))
    x0 = (x - c.k * eps) / c.a
    vt = operator.apply_V_transpose
    spec = (f_th - 1) * vt(x0) + (f_ep - ce) * vt(eps) + (f_xi - es) * vt(xi) + f_y * ybar
    return c.a_prev * ((x0 + ce * eps + es * xi) + operator.apply_V(spec))


def _check_unit(name: str, v: float) -> float:
    if not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must be in [0, 1], got {v}")
    return float(v)


class FusedDDRMStep(FusedStep):
    """One DDRM iteration over a flat batch: the prior's forward under ``no_grad`` and
    ``sp_ddrm_step_ws`` (or ``ddrm_step_svd`` for an ``SVDOperator`` without a descriptor: plain
    torch on the tensors' device).  Owns what is fixed across the steps: ``q`` (the periodic
    kind's prepared observation, ``sp_pgdm_prepare``'s, once per call), the workspace of a chunk
    and the micro-batch chunks.  ``observation_rows`` as ``FusedDPSStep``."""

    def __init__(self, network: EpsilonNetwork, inverse_problem: InverseProblem,
                 observation_rows: Tensor, y_div: int, *, eta: float = 0.85, eta_b: float = 1.0,
                 noise_std: float | None = None, micro_batch: int | None = None,
                 timer: KernelTimer | None = None) -> None:
        op, noise = inverse_problem.operator, inverse_problem.noise
        self.eta, self.eta_b = _check_unit("eta", eta), _check_unit("eta_b", eta_b)
        if noise_std is not None:
            if not (float(noise_std) >= 0.0 and float(noise_std) < float("inf")):
                raise ValueError(f"noise_std must be non-negative and finite, got {noise_std}")
            self.sigma = float(noise_std)
        elif isinstance(noise, GaussianNoise):
            self.sigma = float(noise.sigma.detach().cpu().item())
        else:
            raise ValueError(f"DDRM needs GaussianNoise (its sigma is sigma_y) or an explicit "
                             f"noise_std, got {type(noise).__name__}")
        super().__init__(network, op, y_div, micro_batch, timer)
        self.desc = ddrm_descriptor(op)
        # an SVDOperator with a fused step still runs through its factors on host tensors
        host_svd = (self.desc is not None and isinstance(op, SVDOperator)
                    and not observation_rows.is_cuda)
        self.fused = self.desc is not None and not host_svd
        if not self.fused:
            if not isinstance(op, SVDOperator) or not (host_svd or _hip.descriptor_of(op) is None):
                raise NotImplementedError(
                    f"{type(op).__name__} has no DDRM step: DDRMSampler supports {SUPPORTED}")
            self.y = observation_rows
            return
        self._bind_rows(observation_rows, "DDRMSampler")
        if int(self.lib.sp_ddrm_workspace(self.desc, 1)) > 0:  # the spectral kinds: q = P T_y(y), once
            self._prepare_q("sp_op_workspace", "sp_pgdm_prepare")

    def coefficients(self, t: int, t_prev: int) -> DDRMCoefficients:
        return ddrm_coefficients(host_alphas_cumprod(self.network), t, t_prev, self.sigma, self.eta,
                                 self.eta_b)

    def workspace(self, batch: int, like: Tensor) -> Tensor | None:
        """The step's work buffer for ``batch`` samples (``sp_ddrm_workspace`` floats), kept
        between steps; None where the kind needs none."""
        if self.q is None:
            return None
        floats = int(self.lib.sp_ddrm_workspace(self.desc, batch))
        if floats < 0:
            raise _hip.HipLibraryError(f"sp_ddrm_workspace rejected the descriptor ({floats})")
        return self._kept_work(floats, like)

    def _noise(self, xc: Tensor, seed: int, step: int, sample_offset: int) -> Tensor:
        """The Philox plane of the fused path, for the torch path on a device tensor."""
        if not xc.is_cuda:
            raise ValueError("rng='philox' draws on the device; on host tensors pass rng='torch' "
                             "or a noise_fn")
        out = torch.empty_like(xc, dtype=torch.float32)
        _hip.check(_hip.load_library().sp_randn(_hip.ptr(out), out.shape[0], out[0].numel(), seed,
                                                step, sample_offset, _hip.stream_of(out)),
                   "sp_randn")
        return out.to(xc.dtype)

    def __call__(self, x: Tensor, step: int, t: int, t_prev: int, *, xi: Tensor | None = None,
                 seed: int = 0, sample_offset: int = 0) -> Tensor:
        """Advance ``x`` (flat ``(B, *x_shape)``, contiguous) one step, in place."""
        c = self.coefficients(t, t_prev)
        for b0, b1 in self._chunks(x.shape[0]):
            xc, bc, row = x[b0:b1], b1 - b0, b0 // self.y_div
            with torch.no_grad():
                eps = self.network.forward(xc, t)
            eps = eps.contiguous()
            xic = None if xi is None else xi[b0:b1].contiguous()
            with self._timed("ddrm_step", bc):
                if self.fused:
                    coefs = _hip.SpDdrmCoefs(c.a, c.k, c.a_prev, c.sig_prev, c.sig_y, c.eta, c.eta_b,
                                             c.c1)
                    _hip.check(self.lib.sp_ddrm_step_ws(
                        self.desc, _hip.ptr(xc), _hip.ptr(eps), _hip.ptr(self.y[row:]),
                        _hip.ptr(self.q[row:]) if self.q is not None else None, _hip.ptr(xic), seed,
                        step, sample_offset + b0, bc, self.y_div, coefs, _hip.ptr(xc),
                        _hip.ptr(self.workspace(bc, xc)), _hip.stream_of(x)), "sp_ddrm_step_ws")
                else:
                    if xic is None:
                        xic = self._noise(xc, seed, step, sample_offset + b0)
                    with torch.no_grad():
                        yc = self.y[row:row + -(-bc // self.y_div)].to(device=xc.device)
                        xc.copy_(ddrm_step_svd(self.operator, xc, eps, yc, xic.to(xc.dtype), c))
        return x

    def predict_x0(self, x: Tensor, t: int) -> Tensor:
        """Final ``predict_x0``: the prior's forward and ``(x − k·eps)/a`` (``sp_predict_x0`` on
        the fused path)."""
        if self.fused:
            return super().predict_x0(x, t)
        a, k = x0_coefficients(host_alphas_cumprod(self.network), t)
        out = torch.empty_like(x)
        for b0, b1 in self._chunks(x.shape[0]):
            with torch.no_grad():
                out[b0:b1] = (x[b0:b1] - k * self.network.forward(x[b0:b1], t)) / a
        return out


class DDRMSampler(PosteriorSampler, Generic[Condition_co]):
    """DDRM (Kawar et al., 2022): one network call per step, the update taken per singular value
    of the operator and fused into HIP launches."""

    def __call__(
        self,
        inverse_problem: InverseProblem,
        num_sampling_steps: int = 20,
        num_reconstructions: int = 1,
        eta: float = 0.85,
        eta_b: float = 1.0,
        noise_std: float | None = None,
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
        """Run DDRM; returns ``(*batch_shape, R, *x_shape)`` (R squeezed when 1).  ``eta`` and
        ``eta_b`` are the paper's η and η_b; ``noise_std`` overrides the noise model's σ_y
        (``noise_std=0`` is noiseless DDRM); the keyword-only options are ``PGDMSampler``'s.  The
        step object of the last call stays on the sampler as ``last_step``."""
        if args or kwargs:
            print(f"Warning: Unused args={args}, kwargs={kwargs} in DDRMSampler")

        def make_step(net, y_rows):
            self.last_step = FusedDDRMStep(net, inverse_problem, y_rows, num_reconstructions,
                                           eta=eta, eta_b=eta_b, noise_std=noise_std,
                                           micro_batch=micro_batch, timer=timer)
            return self.last_step

        return run_sampler(self, inverse_problem, make_step, num_sampling_steps=num_sampling_steps,
                           num_reconstructions=num_reconstructions, condition=condition, rng=rng,
                           seed=seed, noise_fn=noise_fn, sample_offset=sample_offset,
                           keep_reconstruction_dim=keep_reconstruction_dim)
