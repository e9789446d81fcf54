"""fp64 semantics of the proximal map by conjugate gradients — TEST INFRASTRUCTURE ONLY.

``Operator.apply_prox_cg``, ``sp_op_prox_cg_ws`` and ``sp_diffpir_step_cg_ws`` compute, per sample,
``z = (AᵀA + ρI)⁻¹(Aᵀy + ρ x0)`` by regularised CGLS in ``d = z − x0`` with a stop of its own
(DESIGN.md §3).  This file restates that recurrence independently of the library's host form, one
sample at a time on a dense matrix:

* ``dense`` — A of a host operator as a float64 (m, n) matrix (``prox_ref.dense_matrix``);
* ``cgls`` — the recurrence in any dtype: fp64 is the reference, fp32 the emulation whose own
  distance to the reference is the yardstick of the GPU tests; ``stop=False`` is the recurrence
  without the ``live`` test, which is what shows why the test is part of the semantics;
* ``solve`` — the definition, ``prox_ref.dense_prox``;
* ``optimality`` — ``‖(AᵀA + ρ)z − Aᵀy − ρ x0‖ / ‖Aᵀ(y − A x0)‖`` in fp64;
* ``step`` — the DiffPIR step around a data step;
* ``NAMES`` / ``case`` — the ten operators the CPU and GPU tests share (the smallest shapes that
  reach every path of csrc/sp_cg.hip), each with its dense matrix and seeded inputs, built once.

    s = y − A x0 ;  d = 0 ;  g = Aᵀ s ;  p = g ;  γ = ‖g‖² ;  γ₀ = γ ;  iters = 0
    repeat K times:
        q = A p ;  δ = ‖q‖² + ρ ‖p‖²
        live = (γ > tol²·γ₀) and (δ > 0) and γ, δ finite
        if live:  α = γ/δ ;  d += α p ;  s −= α q ;  g = Aᵀ s − ρ d ;  γ' = ‖g‖²
                  β = γ'/γ ;  p = g + β p ;  γ = γ' ;  iters += 1
        else:     nothing changes
    z = x0 + d
"""

from __future__ import annotations

import math

import torch

import prox_ref as pr


def _psf3():
    return torch.tensor([[0.05, 0.10, 0.00], [0.20, 0.30, 0.10], [0.00, 0.15, 0.10]])


def _half_mask(n):
    keep = torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5
    keep[0] = True
    return ~keep


def _operators():
    from samplers_amd import operators as ops
    from samplers_amd.operators.sr_filter import gaussian_filter_taps

    return {
        # below one vector
        "identity": lambda: ops.IdentityOperator((3,)),
        # several workgroups and partials per sample, m != n
        "inpaint": lambda: ops.InpaintingOperator((5000,), _half_mask(5000)),
        "sr4": lambda: ops.SuperResolutionOperator((3, 16, 24), 4),
        # n % 4 != 0
        "blur": lambda: ops.GaussianBlurOperator((3, 33, 35), 5, 1.0),
        "psf": lambda: ops.PSFBlurOperator((2, 12, 12), _psf3()),
        "psf_fft": lambda: ops.FFTPSFBlurOperator((3, 16, 16), _psf3(), padding="reflect"),
        "periodic": lambda: ops.PeriodicBlurOperator((1, 8, 12), _psf3()),
        # the workspace kinds with m != n
        "sr_periodic": lambda: ops.PeriodicSuperResolutionOperator((1, 16, 16),
                                                                   gaussian_filter_taps(4, 1.0), 2),
        "radon_small": lambda: ops.RadonOperator((1, 9, 13), num_angles=7),
        # odd sizes, and a detector wide enough for m > n
        "radon_wide": lambda: ops.RadonOperator((1, 40, 36), num_angles=5, detector_size=301),
    }


NAMES = ("identity", "inpaint", "sr4", "blur", "psf", "psf_fft", "periodic", "sr_periodic",
         "radon_small", "radon_wide")
ISOMETRIES = ("identity", "inpaint", "sr4")        # A Aᵀ ∝ I: CG is exact after one iteration
CLOSED_FORM = ISOMETRIES + ("periodic", "sr_periodic")  # the kinds sp_op_prox_ws serves
BATCHES = ((3, 3), (4, 2))  # (batch, y_div)
_CASES: dict = {}


class Case:
    """A host operator of the table above, its dense fp64 matrix and seeded inputs: ``x`` and
    ``eps`` (4, n), ``xi`` (4, n), ``y`` (2, m).  (batch 3, y_div 3) takes the first three samples
    against row 0, (batch 4, y_div 2) all four against rows 0, 0, 1, 1."""

    def __init__(self, name: str) -> None:
        self.name = name
        self.op = _operators()[name]()
        self.A = dense(self.op)
        self.m, self.n = self.A.shape
        g = torch.Generator().manual_seed(1000 + NAMES.index(name))
        self.x, self.eps, self.xi = (torch.randn(4, self.n, generator=g) for _ in range(3))
        self.y = torch.randn(2, self.m, generator=g)
        self._memo: dict = {}

    def inputs(self, batch: int, ydiv: int):
        """(x rows, y rows repeated per sample) of a batch configuration."""
        return self.x[:batch], self.y[:batch // ydiv].repeat_interleave(ydiv, dim=0)

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]


def case(name: str) -> Case:
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def dense(op) -> torch.Tensor:
    """A of a host operator as an (m, n) float64 matrix."""
    return pr.dense_matrix(lambda t: op.apply(t).reshape(t.shape[0], -1), tuple(op.x_shape))


def solve(A: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, rho: float) -> torch.Tensor:
    return pr.dense_prox(A, x0.double(), y.double(), rho)


def _one(A, At, x0, y, rho, K, tol, stop):
    dt = A.dtype
    rho_t, tol_t = torch.tensor(rho, dtype=dt), torch.tensor(tol, dtype=dt)
    s = y - A @ x0
    d = torch.zeros_like(x0)
    g = At @ s
    p = g.clone()
    gamma = (g * g).sum()
    gamma0 = gamma.clone()
    iters = 0
    for _ in range(K):
        q = A @ p
        delta = (q * q).sum() + rho_t * (p * p).sum()
        if stop:
            live = (bool(gamma > (tol_t * tol_t) * gamma0) and bool(delta > 0)
                    and math.isfinite(float(gamma)) and math.isfinite(float(delta)))
            if not live:
                break  # nothing changed, so p and with it the decision are the same next time
        alpha = gamma / delta
        d = d + alpha * p
        s = s - alpha * q
        g = At @ s - rho_t * d
        gamma_new = (g * g).sum()
        p = g + (gamma_new / gamma) * p
        gamma = gamma_new
        iters += 1
    return (x0 + d if iters else x0.clone()), iters


def cgls(A: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, rho: float, K: int, tol: float,
         dtype=torch.float64, stop: bool = True):
    """(z (B, n), iters (B,)) of the recurrence in ``dtype`` on flat rows ``x0`` (B, n), ``y``
    (B, m): A, x0, y and the scalars are rounded to ``dtype`` first, every sample runs alone."""
    Ad = A.to(dtype)
    At = Ad.T
    zs, its = [], []
    for b in range(x0.shape[0]):
        z, it = _one(Ad, At, x0[b].to(dtype), y[b].to(dtype), float(rho), int(K), float(tol), stop)
        zs.append(z)
        its.append(it)
    return torch.stack(zs), torch.tensor(its, dtype=torch.int32)


def optimality(A: torch.Tensor, z: torch.Tensor, x0: torch.Tensor, y: torch.Tensor, rho: float):
    """Per sample ``‖(AᵀA + ρ)z − Aᵀy − ρ x0‖ / ‖Aᵀ(y − A x0)‖`` in fp64 (0 where both vanish)."""
    z, x0, y = z.double(), x0.double(), y.double()
    num = pr.residual(A, z, x0, y, rho).norm(dim=1)
    den = ((y - x0 @ A.T) @ A).norm(dim=1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), num)


def distance(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got − ref| / max|ref| in fp64."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def step(x, eps, xi, z_of_x0, c):
    """(z, x') of one DiffPIR step in the dtype of x around the data step ``z_of_x0(x0)``, with the
    scalars ``c`` = dict(a, k, a_prev, c_eps, c_xi)."""
    z = z_of_x0(pr.predict_x0(x, eps, c["a"], c["k"]))
    return z, pr.diffpir_update(x, z, xi, c["a"], c["k"], c["a_prev"], c["c_eps"], c["c_xi"])
