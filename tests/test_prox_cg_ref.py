"""The reference of the conjugate-gradient proximal map (tests/prox_cg_ref.py) against the
definition, and why its stop rule is part of the semantics.  No GPU.

Measured here (fp32 emulation, the inputs of ``prox_cg_ref.Case``): with the rule at tol = 1e-6 the
emulation ends 3e-8 … 1.2e-5 × max|ref| from the dense solve (the largest on the 40×36 Radon case
at ρ = 1, after 52 iterations) with an optimality residual of at most 2e-5 (box SR at ρ = 50), and
K = 300 returns the bits of K = 64.  Without the rule, on the 5-tap Gaussian blur of a 3×16² image
at ρ = 50, the fp32 recurrence is 5.8 × max|ref| away at K = 32 and 9e15 away at K = 128."""

import pytest
import torch

import prox_cg_ref as cg
import prox_ref as pr
from samplers_amd import operators as ops

SMALL = [n for n in cg.NAMES if n not in ("inpaint", "blur")]  # the two large ones: once, below


def _rhos(name):
    return pr.RHOS if name in cg.ISOMETRIES else (1.0, 50.0)


@pytest.mark.parametrize("name", SMALL)
def test_fp64_recurrence_reaches_the_dense_solve(name):
    c = cg.case(name)
    x, y = c.inputs(4, 2)
    for rho in _rhos(name):
        z, iters = cg.cgls(c.A, x, y, rho, 2000, 1e-13)
        assert int(iters.max()) < 2000, "not converged"
        assert cg.distance(z, cg.solve(c.A, x, y, rho)) <= 1e-10, (name, rho)
        assert float(cg.optimality(c.A, z, x, y, rho).max()) <= 1e-10


@pytest.mark.parametrize("name", ["inpaint", "blur"])
def test_large_cases_reach_the_dense_solve(name):
    c = cg.case(name)
    x, y = c.inputs(3, 3)
    z, _ = cg.cgls(c.A, x, y, 1.0, 500, 1e-13)
    assert cg.distance(z, c.memo(("solve", 3, 1.0), lambda: cg.solve(c.A, x, y, 1.0))) <= 1e-10


def test_blow_up_without_the_stop_rule_and_its_absence_with_it():
    op = ops.GaussianBlurOperator((3, 16, 16), 5, 1.0)
    A = cg.dense(op)
    g = torch.Generator().manual_seed(3)
    x0, y = torch.randn(2, A.shape[1], generator=g), torch.randn(2, A.shape[0], generator=g)
    ref = cg.solve(A, x0, y, 50.0)
    far = {K: cg.distance(cg.cgls(A, x0, y, 50.0, K, 0.0, torch.float32, stop=False)[0], ref)
           for K in (32, 128)}
    print("without the rule:", far)
    # gamma reaches rounding level after 3 iterations and beta = gamma' / gamma becomes noise:
    # far beyond the 2e-5 of every bound at K = 32, beyond any number an image holds at K = 128
    assert not far[32] <= 1e-3 and not far[128] <= 1e6
    for tol in (1e-5, 1e-6):
        z, iters = cg.cgls(A, x0, y, 50.0, 300, tol, torch.float32)
        assert bool(torch.isfinite(z).all()) and int(iters.max()) <= 4
        assert cg.distance(z, ref) <= 2e-5
        assert torch.equal(z, cg.cgls(A, x0, y, 50.0, 64, tol, torch.float32)[0])


@pytest.mark.parametrize("name", cg.NAMES)
def test_the_rule_keeps_every_case_finite_at_300_iterations(name):
    c = cg.case(name)
    x, y = c.inputs(4, 2)
    for rho in _rhos(name):
        for tol in (1e-5, 1e-6):
            z, iters = cg.cgls(c.A, x, y, rho, 300, tol, torch.float32)
            assert bool(torch.isfinite(z).all()), (name, rho, tol)
            assert int(iters.max()) < 64, (name, rho, tol, iters.tolist())
            assert torch.equal(z, cg.cgls(c.A, x, y, rho, 64, tol, torch.float32)[0])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", SMALL)
def test_zero_residual_returns_x0_bitwise(name, dtype):
    c = cg.case(name)
    x = c.x.to(dtype)
    Ad = c.A.to(dtype)
    y = torch.stack([Ad @ x[b] for b in range(4)])  # the recurrence's own A x0: s = 0 exactly
    z, iters = cg.cgls(c.A, x, y, 1.0, 8, 1e-6, dtype)
    assert iters.tolist() == [0, 0, 0, 0]
    assert torch.equal(z, x) and not bool(torch.isnan(z).any())


@pytest.mark.parametrize("name", cg.ISOMETRIES)
def test_isometries_converge_in_two_iterations(name):
    """A Aᵀ ∝ I: AᵀA has one non-zero eigenvalue, so the first iteration is exact; the second is
    the allowance for a residual left above tol by rounding."""
    c = cg.case(name)
    x, y = c.inputs(4, 2)
    for rho in pr.RHOS:
        want = c.memo(("solve", 4, rho), lambda: cg.solve(c.A, x, y, rho))
        for dtype, tol, bound in ((torch.float64, 1e-6, 1e-10), (torch.float32, 1e-6, 2e-5)):
            z, iters = cg.cgls(c.A, x, y, rho, 64, tol, dtype)
            assert int(iters.max()) <= 2 and int(iters.min()) >= 1, (name, rho, iters.tolist())
            assert cg.distance(z, want) <= bound, (name, rho, dtype)
