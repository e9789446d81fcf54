"""fp64 semantics of the proximal data step and of the DiffPIR loop — TEST INFRASTRUCTURE ONLY.

The reference has no such sampler.  What ``Operator.apply_prox``, ``sp_op_prox_ws``,
``sp_diffpir_step_ws`` and ``DiffPIRSampler`` implement is pinned here in plain torch:

* ``dense_matrix`` / ``dense_prox`` — A as a dense (m, n) matrix (the map applied to the unit
  vectors) and ``z = solve(AᵀA + ρI, Aᵀy + ρ x0)``: the definition, with no closed form in it;
* ``mask_prox``, ``sr_prox``, ``periodic_prox`` — the three closed forms (r = y − A x0):
  ``z = x0 + Aᵀr / (1 + ρ)`` for A Aᵀ = I (identity, inpainting, mask; unobserved pixels keep x0),
  ``z = x0 + (r replicated over its s×s block) / (1 + ρ s²)`` for the block mean, and
  ``Z = (conj(M)·Y + ρ·X0) / (|M|² + ρ)`` for the periodic blur with ``M = periodic_ops.transfer``.
  They compute in the dtype of ``x0``: fp64 is the reference, fp32 (plain torch, ``torch.fft``) the
  error yardstick of the GPU tests.  ``form="blend"`` evaluates the first two as
  ``(y + ρ x0) / (1 + ρ)`` on the observed part instead of ``x0 + r / (1 + ρ)``;
* ``diffpir_update`` — ``x' = a_prev·z + (c_eps·(x − a·z)/k + c_xi·ξ)`` and ``predict_x0``;
* ``diffpir_coefs`` — the six scalars of a step in the dtype of the schedule;
* ``diffpir_reference`` — the loop, in the calling style of ``oracle/dps_loop.dps_reference``;
* ``exact_inputs`` / ``EXACT`` — integer data on which no fp32 evaluation of a step can round.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

import periodic_ops as po

RHOS = (1e-4, 1e-2, 1.0, 50.0)


# --- the definition ---------------------------------------------------------------------------
def dense_matrix(apply, x_shape: tuple) -> torch.Tensor:
    """A as an (m, n) float64 matrix: column j is ``apply`` of the j-th unit vector."""
    n = 1
    for d in x_shape:
        n *= d
    eye = torch.eye(n, dtype=torch.float64).reshape(n, *x_shape)
    return apply(eye).reshape(n, -1).T.contiguous()


def dense_prox(A: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, rho: float) -> torch.Tensor:
    """``solve(AᵀA + ρI, Aᵀy + ρ x0)`` on flat fp64 rows ``x0`` (B, n), ``y`` (B, m)."""
    n = A.shape[1]
    lhs = A.T @ A + rho * torch.eye(n, dtype=torch.float64)
    rhs = y.double() @ A + rho * x0.double()
    return torch.linalg.solve(lhs, rhs.T).T


def residual(A: torch.Tensor, z: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, rho: float):
    """The optimality residual ``Aᵀ(A z − y) + ρ (z − x0)`` (zero at the minimiser)."""
    return (z @ A.T - y) @ A + rho * (z - x0)


# --- the closed forms -------------------------------------------------------------------------
def mask_prox(x0: torch.Tensor, y: torch.Tensor, keep: torch.Tensor, rho: float,
              packed: bool = True, form: str = "residual") -> torch.Tensor:
    """``x0`` (B, n); ``keep`` bool (n,), True where observed; ``y`` the packed kept pixels
    (B, m) in ascending order, or the full (B, n) row (``packed=False``: the mask kind, whose
    masked entries of y are not read)."""
    keep = keep.reshape(-1).bool()
    yk = y if packed else y[:, keep]
    z = x0.clone()
    xk = x0[:, keep]
    if form == "residual":
        z[:, keep] = xk + (yk - xk) / (1 + rho)
    else:
        z[:, keep] = (yk + rho * xk) / (1 + rho)
    return z


def sr_prox(x0: torch.Tensor, y: torch.Tensor, s: int, rho: float, form: str = "residual",
            shift: int = 0) -> torch.Tensor:
    """``x0`` (B, C, H, W), ``y`` (B, C, H/s, W/s).  ``shift`` rolls the block grid by that many
    columns (a wrong answer on purpose: the exact cases must tell it apart)."""
    xs = torch.roll(x0, -shift, dims=-1) if shift else x0
    mean = F.avg_pool2d(xs, s)
    rep = lambda t: t.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)  # noqa: E731
    d = 1 + rho * s * s
    if form == "residual":
        z = xs + rep((y - mean) / d)
    else:
        z = (xs - rep(mean)) + rep((y + (rho * s * s) * mean) / d)
    return torch.roll(z, shift, dims=-1) if shift else z


def periodic_prox(x0: torch.Tensor, y: torch.Tensor, h, rho: float) -> torch.Tensor:
    """``x0``, ``y`` (B, C, H, W); fp64 in, the reference; fp32 in, ``torch.fft`` in complex64."""
    H, W = x0.shape[-2:]
    cd = torch.complex128 if x0.dtype == torch.float64 else torch.complex64
    m = po.transfer(h, H, W).to(cd)
    zs = (m.conj() * torch.fft.fft2(y) + rho * torch.fft.fft2(x0)) / ((m.abs() ** 2).to(x0.dtype) + rho)
    return torch.fft.ifft2(zs).real.to(x0.dtype)


# --- one step and the loop --------------------------------------------------------------------
def predict_x0(x, eps, a, k):
    return (x - k * eps) / a


def diffpir_update(x, z, xi, a, k, a_prev, c_eps, c_xi):
    """``x' = a_prev z + (c_eps eps_hat + c_xi xi)`` with ``eps_hat = (x − a z) / k``."""
    return a_prev * z + (c_eps * ((x - a * z) / k) + c_xi * xi)


def diffpir_coefs(acp: torch.Tensor, t: int, t_prev: int, sigma: float, guidance_weight: float,
                  zeta: float, min_noise_std: float):
    """(a, k, rho, a_prev, c_eps, c_xi) in acp's dtype."""
    at, ap = acp[t], acp[t_prev]
    s = max(float(sigma), float(min_noise_std))
    rho = guidance_weight * s * s * at / (1 - at)
    kp = (1 - ap) ** 0.5
    return at ** 0.5, (1 - at) ** 0.5, rho, ap ** 0.5, kp * (1 - zeta) ** 0.5, kp * zeta ** 0.5


def diffpir_reference(eps_fn, acp: torch.Tensor, timesteps: list, apply, prox, y: torch.Tensor,
                      init: torch.Tensor, noise_of_step, *, sigma: float,
                      guidance_weight: float = 7.0, zeta: float = 0.3,
                      min_noise_std: float = 1e-3) -> torch.Tensor:
    """The DiffPIR loop in the dtype of ``init``.  ``prox(x0, y, rho)`` is the data step;
    ``apply`` is taken for the calling style of the other loops and only shapes y's check;
    ``noise_of_step(i)`` is ξ of loop index i (the Philox step index)."""
    x = init
    assert apply(init).shape[1:] == y.shape[1:], (apply(init).shape, y.shape)
    with torch.no_grad():
        for i in range(len(timesteps) - 1, 1, -1):
            t, t_prev = int(timesteps[i]), int(timesteps[i - 1])
            a, k, rho, a_prev, c_eps, c_xi = diffpir_coefs(acp, t, t_prev, sigma, guidance_weight,
                                                           zeta, min_noise_std)
            x0 = predict_x0(x, eps_fn(x, t), a, k)
            z = prox(x0, y, rho)
            x = diffpir_update(x, z, noise_of_step(i).to(x.dtype), a, k, a_prev, c_eps, c_xi)
        t1 = int(timesteps[1])
        return predict_x0(x, eps_fn(x, t1), acp[t1] ** 0.5, (1 - acp[t1]) ** 0.5)


# --- exact cases --------------------------------------------------------------------------------
# a = k = 1/2, a_prev = 1/2, c_eps = 1/4, c_xi = 1/8; rho = 1 (1 / s^2 for SR): 1 + rho s^2 = 2.
# With integer x, eps, y, xi in [-8, 8]: x0 = 2x - eps is an integer, a block mean a multiple of
# 1/64, z a multiple of 1/128, x' one of 1/1024, all below 2^7 - every intermediate of every
# evaluation order is an fp32 number, so no fp32 evaluation can round.
EXACT = dict(a=0.5, k=0.5, a_prev=0.5, c_eps=0.25, c_xi=0.125)


def exact_rho(s: int = 1) -> float:
    return 1.0 / (s * s)


def exact_inputs(batch: int, n: int, m_rows: int, m: int, seed: int):
    """Integer-valued fp32 (x, eps, xi) of shape (batch, n) and y of shape (m_rows, m)."""
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randint(-8, 9, (batch, n), generator=g).float() for _ in range(3))
    y = torch.randint(-8, 9, (m_rows, m), generator=g).float()
    return x, eps, xi, y


def step_from_prox(x, eps, xi, y_rows, prox, rho, c=EXACT):
    """(z, x') of one step in the dtype of x; ``prox(x0, y, rho)`` with y already one row per
    sample."""
    x0 = predict_x0(x, eps, c["a"], c["k"])
    z = prox(x0, y_rows, rho)
    return z, diffpir_update(x, z, xi, c["a"], c["k"], c["a_prev"], c["c_eps"], c["c_xi"])
