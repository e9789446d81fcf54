"""PeriodicSuperResolutionOperator on the host against dense fp64 matrices built by index
arithmetic: the host maps, the spectral identities, the truncated SVD, the dense proximal solve,
the algebra of the pseudo-inverse, the PGDM gradient identity, and the operators it must agree
with.  No GPU."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sr_periodic_ops as so
from samplers_amd.operators import (FilteredSuperResolutionOperator,
                                    PeriodicSuperResolutionOperator)
from samplers_amd.operators.sr_periodic import sr_lambda, sr_stored_arrays, sr_transfer_function

RHOS = (1e-4, 1e-2, 1.0, 50.0)
_cache = {}


def case(name):
    """(operator, dense A, H, W, s, taps), built once per case and shared."""
    if name not in _cache:
        H, W, s, taps, _ = so.CASES[name]
        op = PeriodicSuperResolutionOperator((2, H, W), taps, factor=s)
        _cache[name] = (op, so.dense(taps, H, W, s), H, W, s, taps)
    return _cache[name]


def _x(shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _err(got, ref):
    wide = torch.complex128 if got.is_complex() or ref.is_complex() else torch.float64
    return float((got.to(wide) - ref.to(wide)).abs().max() / ref.to(wide).abs().max())


@pytest.mark.parametrize("name", list(so.CASES))
def test_kept_counts(name):
    op = case(name)[0]
    kept, total = so.CASES[name][4]
    assert (int(op.keep.sum()), op.keep.numel()) == (kept, total)


@pytest.mark.parametrize("name", list(so.CASES))
def test_host_maps_match_the_dense_matrix(name):
    op, a, H, W, s, _ = case(name)
    x, y = _x((3, 2, H, W), 1), _x((3, 2, H // s, W // s), 2)
    assert _err(op.apply(x), so.dense_apply(a, x, (H // s, W // s))) <= 1e-12
    assert _err(op.apply_transpose(y), so.dense_apply(a.T, y, (H, W))) <= 1e-12
    assert op.apply(x).dtype == torch.float64 and tuple(op.y_shape) == (2, H // s, W // s)
    # fp32 in, fp32 out
    assert _err(op.apply(x.float()), so.dense_apply(a, x, (H // s, W // s))) <= 2e-6
    assert op.hip_linear is False and op.pinv_grad_scale == 2.0


@pytest.mark.parametrize("name", list(so.CASES))
def test_spectral_identities_match_the_dense_matrix(name):
    op, a, H, W, s, taps = case(name)
    M = so.transfer(taps, H, W, s)
    x, y = _x((2, H, W), 3), _x((2, H // s, W // s), 4)
    assert _err(so.spectral_down(x, M, s), so.dense_apply(a, x, (H // s, W // s))) <= 1e-13
    assert _err(so.spectral_up(y, M.conj(), s), so.dense_apply(a.T, y, (H, W))) <= 1e-13
    # the singular values of A are sqrt(Lambda)
    sv = np.linalg.svd(a, compute_uv=False)
    want = np.sort(np.sqrt(so.lam(M, s).numpy().ravel()))[::-1]
    assert np.abs(sv - want).max() <= 1e-13 * want.max()
    # the module's own helpers are the same arrays
    assert _err(sr_transfer_function(taps, H, W, s), M) <= 1e-14
    assert _err(sr_lambda(M, s), so.lam(M, s)) <= 1e-14


@pytest.mark.parametrize("name", list(so.CASES))
def test_pseudo_inverse_is_the_truncated_svd(name):
    op, a, H, W, s, taps = case(name)
    count = int(op.keep.sum())
    sv = np.linalg.svd(a, compute_uv=False)
    # the threshold falls in a gap: the count decides nothing
    assert sv[count - 1] > op.rtol * sv[0] * (1 + 1e-6)
    assert count == sv.size or sv[count] < op.rtol * sv[0] * (1 - 1e-6)
    ap = so.dense_pinv(a, count)
    ref = so.Ref(taps, H, W, s, op.keep)
    x, y = _x((2, H, W), 5), _x((2, H // s, W // s), 6)
    want = so.dense_apply(ap, y, (H, W))
    assert _err(ref.pinv(y), want) <= 1e-12
    assert _err(ref.pinv_t(x), so.dense_apply(ap.T, x, (H // s, W // s))) <= 1e-12
    # the operator's host map (fp32-rounded P): fp64 in, fp64 out
    got = op.apply_pseudo_inverse(y)
    assert got.dtype == torch.float64 and _err(got, want) <= 2e-6
    assert _err(op.apply_pseudo_inverse(y.float()), want) <= 1e-5
    # differentiable on the host: the backward of A^+ is A^+T
    yr = y.clone().requires_grad_()
    (g,) = torch.autograd.grad(op.apply_pseudo_inverse(yr), yr, grad_outputs=x)
    assert _err(g, ref.pinv_t(x)) <= 2e-6


@pytest.mark.parametrize("name", list(so.CASES))
def test_prox_is_the_dense_solve(name):
    op, a, H, W, s, taps = case(name)
    M = so.transfer(taps, H, W, s)
    x0, y = _x((2, H, W), 7), _x((2, H // s, W // s), 8)
    for rho in RHOS:
        want = so.dense_prox(a, x0, y, rho)
        assert _err(so.spectral_prox(x0, y, M, s, rho), want) <= 1e-11, rho
        assert _err(op.apply_prox(x0, y, rho), want) <= 2e-6, rho
        assert _err(op.apply_prox(x0.float(), y.float(), rho), want) <= 2e-5, rho
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            op.apply_prox(x0, y, bad)


@pytest.mark.parametrize("name", list(so.CASES))
def test_adjoint_identity(name):
    op, a, H, W, s, _ = case(name)
    x, y = _x((2, H, W), 9), _x((2, H // s, W // s), 10)
    lhs, rhs = float((op.apply(x) * y).sum()), float((x * op.apply_transpose(y)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(x.norm() * y.norm())
    # the host transpose is differentiable in y, and its backward is A (PSLD's oracle loop
    # differentiates x - A^T A x through it)
    yr = y.clone().requires_grad_()
    (g,) = torch.autograd.grad(op.apply_transpose(yr), yr, grad_outputs=x)
    assert _err(g, so.dense_apply(a, x, (H // s, W // s))) <= 1e-12


@pytest.mark.parametrize("name", list(so.CASES))
def test_pseudo_inverse_algebra(name):
    op, a, H, W, s, taps = case(name)
    ref = so.Ref(taps, H, W, s, op.keep)
    x, z, y = _x((2, H, W), 11), _x((2, H, W), 12), _x((2, H // s, W // s), 13)
    pi = lambda t: ref.pinv(ref.A(t))  # noqa: E731
    assert _err(ref.pinv(ref.A(ref.pinv(y))), ref.pinv(y)) <= 1e-12      # A^+ A A^+ = A^+
    assert _err(pi(pi(x)), pi(x)) <= 1e-12                               # idempotent
    assert abs(float((pi(x) * z).sum() - (x * pi(z)).sum())) <= 1e-12 * float(x.norm() * z.norm())
    # and in dense form
    ap = so.dense_pinv(a, int(op.keep.sum()))
    proj = ap @ a
    assert np.abs(proj @ proj - proj).max() <= 1e-12 and np.abs(proj - proj.T).max() <= 1e-12


@pytest.mark.parametrize("name", list(so.CASES))
def test_pgdm_gradient_identity(name):
    """d/dx0 ||A^+ y - A^+ A x0||^2 = -2 A^+ (y - A x0), against autograd of the loss."""
    op, a, H, W, s, taps = case(name)
    ref = so.Ref(taps, H, W, s, op.keep)
    x0, y = _x((2, H, W), 14), _x((2, H // s, W // s), 15)
    closed = -2.0 * ref.pinv(y - ref.A(x0))
    xr = x0.clone().requires_grad_()
    loss = (so.spectral_up(y, ref.P, s) - so.spectral_up(so.spectral_down(xr, ref.M, s), ref.P, s)
            ).pow(2).sum()
    (g,) = torch.autograd.grad(loss, xr)
    assert _err(g, closed) <= 1e-12
    # through the operator's own host maps, as GenericDPSStep differentiates
    xf = x0.float().requires_grad_()
    loss = (op.apply_pseudo_inverse(y.float()) - op.apply_pseudo_inverse(op.forward(xf))).pow(2).sum()
    (g,) = torch.autograd.grad(loss, xf)
    assert _err(g, closed) <= 2e-5


@pytest.mark.parametrize("s,taps", [(2, so.CASES["bicubic2"][3]), (4, so.CASES["bicubic4"][3]),
                                    (4, so.CASES["gauss16"][3]), (2, so.ASYM)])
def test_equals_the_filtered_operator_inside_the_image(s, taps):
    H, W = 32, 48
    x = _x((2, 1, H, W), 16)
    got = PeriodicSuperResolutionOperator((1, H, W), taps, factor=s).apply(x)
    want = FilteredSuperResolutionOperator((1, H, W), taps, factor=s).apply(x)
    pad = (taps.numel() - s) // 2
    lo = -(-pad // s)                    # first output whose window starts at or after pixel 0
    hi_h, hi_w = (H - taps.numel() + pad) // s + 1, (W - taps.numel() + pad) // s + 1
    assert lo < hi_h and lo < hi_w
    inner = (slice(None), slice(None), slice(lo, hi_h), slice(lo, hi_w))
    assert _err(got[inner], want[inner]) <= 1e-14
    if pad:  # and the border differs: wrap is not the symmetric fold
        assert float((got - want).abs().max()) > 1e-3


@pytest.mark.parametrize("s", [2, 4, 8])
def test_box_taps_are_average_pooling(s):
    x = _x((2, 3, 16, 24), 17)
    op = PeriodicSuperResolutionOperator((3, 16, 24), torch.full((s,), 1.0 / s), factor=s)
    assert _err(op.apply(x), F.avg_pool2d(x, s)) <= 1e-15
    assert int(op.keep.sum()) == op.keep.numel()  # A A^T = I / s^2: every singular value is 1 / s


def test_two_dimensional_taps():
    h = torch.randn(4, 4, generator=torch.Generator().manual_seed(18)) / 4
    op = PeriodicSuperResolutionOperator((1, 16, 16), h, factor=2)
    a = so.dense(h, 16, 16, 2)
    x = _x((2, 1, 16, 16), 19)
    assert _err(op.apply(x), so.dense_apply(a, x, (8, 8))) <= 1e-12
    assert np.linalg.matrix_rank(so.taps2d(h)) > 1  # not separable


@pytest.mark.parametrize("name", list(so.CASES))
def test_layout_of_the_stored_arrays(name):
    """spectra = M then P as (re, im) pairs [W / 2 + 1][H], then Lambda_t as fp32 [W / 2 + 1][H]."""
    op, a, H, W, s, taps = case(name)
    hw = W // 2 + 1
    assert op.spectra.dtype == torch.float32 and op.spectra.is_contiguous()
    assert op.spectra.numel() == 5 * hw * H
    M = so.transfer(taps, H, W, s)
    P = so.pinv_spectrum(M, s, op.keep)
    lt = so.lam(M, s).repeat(s, s)
    flat = op.spectra
    for i, spec in enumerate((M, P)):
        got = torch.view_as_complex(flat[i * 2 * hw * H:(i + 1) * 2 * hw * H].view(hw, H, 2))
        want = spec[:, :hw].T
        # fp32 rounding of each entry; the floor is the fp64 transforms' own round-off in M
        # (1e-15 max|M|), which P divides by the smallest kept Lambda
        floor = 1e-15 * float(M.abs().max()) * (1.0 if i == 0 else 1.0 / float(lt[op.keep.repeat(s, s)].min()))
        tol = 1e-7 * want.abs() + floor
        assert bool(((got - want).abs() <= tol).all()), i
    got = flat[4 * hw * H:].view(hw, H)
    want = lt[:, :hw].T
    assert bool(((got - want).abs() <= 1e-7 * want.abs()).all())
    # the helper returns the same arrays before rounding, keep on the low-resolution grid
    m2, p2, l2, k2 = sr_stored_arrays(taps, H, W, s, op.rtol)
    assert _err(m2, M) <= 1e-14 and _err(l2, lt) <= 1e-14 and torch.equal(k2, op.keep)
    assert float((p2 - P).abs().max()) <= 1e-15 * float(M.abs().max()) / float(lt[op.keep.repeat(s, s)].min())
    assert tuple(op.keep.shape) == (H // s, W // s) and op.keep.dtype == torch.bool
    # P is zero on the dropped frequencies, tiled (and where M itself vanishes)
    assert bool((p2[~op.keep.repeat(s, s)] == 0).all())
    assert torch.equal(p2 != 0, op.keep.repeat(s, s) & (m2 != 0))
