"""tests/radon_ref.py against the operator's host form and against itself (no GPU): the fp64
matrix, the fp32-weight matrix, the fp32 emulations of the two gathers, the exact cases, and why
the crossing position must be ONE operation sequence in both gathers.

Rounding bound of the emulations (and of the kernels, test_radon_gpu.py): per element
|out - dense32 result| <= n 2^-24 E with E the same product on absolute values and n the
rounding steps on the longest path of the sum (radon_ref.rounding_steps)."""

import math

import numpy as np
import pytest
import torch

import radon_ref as rr
from samplers_amd.operators import RadonOperator

NAMES = list(rr.CASES)


def _operator(name):
    C, H, W, D, table, _, _ = rr.CASES[name]
    op = RadonOperator((C, H, W), num_angles=table.shape[0], detector_size=D)
    op.table = torch.from_numpy(table.copy())  # the case's own table (hand-made ones included)
    return op


@pytest.mark.parametrize("name", NAMES)
def test_dense64_matches_the_host_form(name):
    C, H, W, D, table, batch, _ = rr.CASES[name]
    op = _operator(name)
    x, _, g, _ = (torch.from_numpy(v).double() for v in rr.case_inputs(name))
    A = rr.matrices(name)[0]
    ax = (x.reshape(batch * C, H * W).numpy() @ A.T).reshape(batch, C, -1, D)
    atg = (g.reshape(batch * C, -1).numpy() @ A).reshape(batch, C, H, W)
    got_ax, got_atg = op.apply(x), op.apply_transpose(g)
    assert got_ax.dtype == torch.float64 and tuple(got_ax.shape) == (batch, *op.y_shape)
    assert np.abs(got_ax.numpy() - ax).max() <= 1e-12 * np.abs(ax).max()
    assert np.abs(got_atg.numpy() - atg).max() <= 1e-12 * np.abs(atg).max()
    # the host form is differentiable: the backward of A is A^T and of A^T, A
    xr = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=g)
    assert torch.equal(gx, got_atg)
    gr = g.clone().requires_grad_()
    (gg,) = torch.autograd.grad(op.apply_transpose(gr), gr, grad_outputs=x)
    assert torch.equal(gg, got_ax)


@pytest.mark.parametrize("name", NAMES)
def test_emulations_match_dense32_within_the_rounding_bound(name, parity_record):
    emu, ref, n = rr.emulation(name), rr.reference64(name), rr.rounding_steps(name)
    for key in ("apply", "adjoint", "v"):
        rho = rr.rho(emu[key], ref[key + "32"], ref["E_" + key], n[key])
        parity_record(f"emulation_{key}_rho", rho, 1.0)
        assert rho <= 1.0, (key, rho)
    # the distance to the exact-geometry matrix, which the GPU test doubles for its bound
    for key, dist in rr.emulation_distance(name).items():
        print(f"{name}: emulation {key} vs dense64 {dist:.3g}")
        parity_record(f"emulation_{key}_vs_dense64", dist, None)
        assert dist <= 2e-5


@pytest.mark.parametrize("name", NAMES)
def test_both_gathers_find_the_same_fp32_weights(name):
    C, H, W, D, table, _, _ = rr.CASES[name]
    fwd = rr.weights32(table, H, W, D)
    adj, most = rr.adjoint_weights32(table, H, W, D)
    assert np.array_equal(fwd, adj)
    # the kernel's narrower candidate rule loses no ray
    assert np.array_equal(fwd, rr.adjoint_weights32(table, H, W, D, narrow=True)[0])
    if np.abs(table[:, 0]).min() >= 1:
        assert most <= 2  # |alpha| >= 1: at most two rays per pixel per angle
    # the same from the matrix: non-zeros per (angle, pixel)
    nz = (fwd.reshape(table.shape[0], D, H * W) != 0).sum(1)
    assert nz.max() == most


def test_a_different_position_formula_breaks_the_adjoint_weights():
    """The contract matters: with the position contracted into fused operations, or with the
    offsets applied in another order, in ONE of the two gathers the weights are no longer the
    same fp32 numbers (and some rays land on the other side of a pixel boundary)."""
    C, H, W, D, table, _, _ = rr.CASES["40x36"]
    fwd = rr.weights32(table, H, W, D)
    for other in (rr.pos_fused, rr.pos_reordered):
        adj, _ = rr.adjoint_weights32(table, H, W, D, pos=other)
        assert not np.array_equal(fwd, adj)
        assert np.abs(fwd.astype(np.float64) - adj).max() < 1e-3  # the same map, other roundings
        assert np.array_equal(rr.weights32(table, H, W, D, pos=other), adj)  # consistent again


EXACT_SHAPES = rr.EXACT_SHAPES


def exact_inputs(H, W, D, nA, seed=0):
    rng = np.random.default_rng(seed)
    x, eps = (rng.integers(-3, 4, size=(H, W)).astype(np.float32) for _ in range(2))
    g, y = (rng.integers(-3, 4, size=(nA, D)).astype(np.float32) for _ in range(2))
    return x, eps, g, y


@pytest.mark.parametrize("table_name", ["axis", "dyadic"])
@pytest.mark.parametrize("H,W,D", EXACT_SHAPES)
def test_exact_cases_are_bit_exact_in_the_emulations(table_name, H, W, D):
    """Axis angles and dyadic tables on integer data with a = k = 1/2, grad_scale 4: no fp32
    operation rounds, so the emulations equal the fp64 products bit for bit."""
    table = rr.AXIS_TABLE if table_name == "axis" else rr.DYADIC_TABLE
    if table_name == "axis":
        assert table.tolist() == [[1, 0, 1, 0], [1, 0, 1, 1], [-1, 0, 1, 0], [-1, 0, 1, 1]]
    x, eps, g, y = exact_inputs(H, W, D, table.shape[0])
    A = rr.dense64(table, H, W, D)
    assert np.array_equal(A, rr.dense32(table, H, W, D))  # the positions do not round either
    ax = (A @ x.reshape(-1).astype(np.float64)).reshape(-1, D)
    atg = (A.T @ g.reshape(-1).astype(np.float64)).reshape(H, W)
    assert np.array_equal(rr.project32(table, x, D).astype(np.float64), ax)
    assert np.array_equal(rr.backproject32(table, g, H, W).astype(np.float64), atg)
    work, v, _ = rr.pass1_32(table, x, eps, y, 0.5, 0.5, 4.0)
    x0 = 2.0 * x.astype(np.float64) - eps
    w64 = 4.0 * (y.astype(np.float64) - (A @ x0.reshape(-1)).reshape(-1, D))
    assert np.array_equal(work.astype(np.float64), w64)
    assert np.array_equal(v.astype(np.float64), (A.T @ w64.reshape(-1)).reshape(H, W))
    if table_name == "axis" and (D - W) % 2:
        assert 0.5 in A  # the half weights really occur


def test_rays_that_miss_the_image_are_zero():
    C, H, W, D, table, _, _ = rr.CASES["200x40"]
    A = rr.matrices("200x40")[0]
    empty = ~A.any(axis=1)
    assert empty.any() and not empty.all()
    y = rr.emulation("200x40")["apply"].reshape(-1)
    assert not y[empty].any()
    # a detector shorter than the diagonal: some pixels are seen by fewer rays
    A16 = rr.matrices("16x16-short")[0]
    per_pixel = (A16 != 0).sum(0)
    assert per_pixel.min() < per_pixel.max()


def test_tables_agree_with_the_operator():
    from samplers_amd.operators import radon_table

    for n in (1, 2, 3, 4, 5, 7, 23):
        assert np.array_equal(radon_table(rr.case_angles(n)).numpy(), rr.table_of(rr.case_angles(n)))
    t = rr.table_of([math.pi * a / 23 for a in range(23)])
    assert np.abs(t[:, 0]).min() >= 1 and np.abs(t[:, 1]).max() <= 1
