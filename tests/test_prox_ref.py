"""tests/prox_ref.py, the fp64 statement of the proximal data step, against its own definition.

No GPU.  The closed forms are held to a dense solve of (AᵀA + ρI) z = Aᵀy + ρ x0 at 1e-10, their
limits to the identity (ρ → ∞) and to the pseudo-inverse projection (ρ → 0), and the exact cases to
the claim the GPU tests rest on: on that integer data an fp32 evaluation in either formula shape
returns the fp64 result bit for bit, and a wrong mask bit or block origin does not."""

import pytest
import torch
import torch.nn.functional as F

import periodic_ops as po
import prox_ref as pr

TOL = 1e-10


def _keep(n, seed):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(n, generator=g) < 0.5
    keep[0], keep[1] = True, False
    return keep


def _psf(k, seed):
    return torch.randn(k, k, generator=torch.Generator().manual_seed(seed)).double() / k


def _families():
    """name -> (A dense, closed form on flat fp64 rows, n, m)."""
    out = {}
    n = 23
    keep = _keep(n, 3)
    eye = torch.eye(n, dtype=torch.float64)
    out["identity"] = (eye, lambda x0, y, rho: pr.mask_prox(x0, y, torch.ones(n, dtype=torch.bool), rho))
    out["inpaint"] = (eye[keep], lambda x0, y, rho: pr.mask_prox(x0, y, keep, rho))
    out["mask"] = (torch.diag(keep.double()),
                   lambda x0, y, rho: pr.mask_prox(x0, y, keep, rho, packed=False))
    for s, shape in ((2, (2, 4, 6)), (4, (1, 8, 4)), (8, (1, 8, 8))):
        ys = (shape[0], shape[1] // s, shape[2] // s)
        out[f"sr{s}"] = (pr.dense_matrix(lambda x, s=s: F.avg_pool2d(x, s), shape),
                         lambda x0, y, rho, s=s, shape=shape, ys=ys: pr.sr_prox(
                             x0.reshape(-1, *shape), y.reshape(-1, *ys), s, rho).reshape(x0.shape))
    for name, shape, h in (("periodic8", (1, 8, 8), _psf(3, 5)), ("periodic8x12", (2, 8, 12), _psf(5, 6))):
        out[name] = (pr.dense_matrix(lambda x, h=h: po.blur(x, h), shape),
                     lambda x0, y, rho, shape=shape, h=h: pr.periodic_prox(
                         x0.reshape(-1, *shape), y.reshape(-1, *shape), h, rho).reshape(x0.shape))
    return out


FAMILIES = _families()


@pytest.mark.parametrize("rho", pr.RHOS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_closed_form_is_the_dense_solve(name, rho):
    A, prox = FAMILIES[name]
    m, n = A.shape
    g = torch.Generator().manual_seed(11)
    x0, y = torch.randn(3, n, generator=g).double(), torch.randn(3, m, generator=g).double()
    z = prox(x0, y, rho)
    want = pr.dense_prox(A, x0, y, rho)
    assert float((z - want).abs().max()) <= TOL, name
    assert float(pr.residual(A, z, x0, y, rho).abs().max()) <= TOL, name
    if name.startswith(("identity", "inpaint", "mask", "sr")):  # the other formula shape
        form = FAMILIES_BLEND[name](x0, y, rho)
        assert float((form - want).abs().max()) <= TOL, name


def _blend():
    n = 23
    keep = _keep(n, 3)
    out = {"identity": lambda x0, y, rho: pr.mask_prox(x0, y, torch.ones(n, dtype=torch.bool), rho,
                                                       form="blend"),
           "inpaint": lambda x0, y, rho: pr.mask_prox(x0, y, keep, rho, form="blend"),
           "mask": lambda x0, y, rho: pr.mask_prox(x0, y, keep, rho, packed=False, form="blend")}
    for s, shape in ((2, (2, 4, 6)), (4, (1, 8, 4)), (8, (1, 8, 8))):
        ys = (shape[0], shape[1] // s, shape[2] // s)
        out[f"sr{s}"] = lambda x0, y, rho, s=s, shape=shape, ys=ys: pr.sr_prox(
            x0.reshape(-1, *shape), y.reshape(-1, *ys), s, rho, form="blend").reshape(x0.shape)
    return out


FAMILIES_BLEND = _blend()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_large_rho_returns_x0(name):
    A, prox = FAMILIES[name]
    m, n = A.shape
    g = torch.Generator().manual_seed(12)
    x0, y = torch.randn(2, n, generator=g).double(), torch.randn(2, m, generator=g).double()
    assert float((prox(x0, y, 1e13) - x0).abs().max()) <= TOL


def test_masked_pixels_keep_x0_and_observed_ones_reach_y():
    n = 23
    keep = _keep(n, 3)
    g = torch.Generator().manual_seed(13)
    x0, y = torch.randn(2, n, generator=g).double(), torch.randn(2, int(keep.sum()), generator=g).double()
    z = pr.mask_prox(x0, y, keep, 1e-2)
    assert torch.equal(z[:, ~keep], x0[:, ~keep])
    assert float((pr.mask_prox(x0, y, keep, 1e-13)[:, keep] - y).abs().max()) <= TOL


def test_small_rho_is_the_pseudo_inverse_projection():
    """x0 + A⁺(y − A x0) on the kept set of a PSF that keeps every frequency (then A⁺ = A⁻¹)."""
    from samplers_amd.operators.periodic import pseudo_inverse_spectrum

    shape = (1, 8, 12)
    h = torch.zeros(3, 3, dtype=torch.float64)
    h[1, 1], h[0, 1], h[1, 2] = 1.0, 0.2, -0.1
    _, keep = pseudo_inverse_spectrum(po.transfer(h, 8, 12).resolve_conj())
    assert bool(keep.all())
    g = torch.Generator().manual_seed(14)
    x0, y = (torch.randn(2, *shape, generator=g).double() for _ in range(2))
    want = x0 + po.pinv(y - po.blur(x0, h), h, keep)
    assert float((pr.periodic_prox(x0, y, h, 1e-12) - want).abs().max()) <= 1e-9


def test_periodic_prox_matches_the_operator_on_the_host():
    from samplers_amd.operators import PeriodicBlurOperator

    shape, h = (2, 8, 24), _psf(5, 9)
    g = torch.Generator().manual_seed(15)
    x0, y = (torch.randn(2, *shape, generator=g).double() for _ in range(2))
    op = PeriodicBlurOperator(shape, h.float())
    for rho in pr.RHOS:  # the operator's M is rounded to fp32
        got = op.apply_prox(x0, y, rho)
        ref = pr.periodic_prox(x0, y, h.float(), rho)
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) / min(1.0, rho ** 0.5)


# --- the exact cases ------------------------------------------------------------------------------
def _exact_mask(n, seed, packed):
    keep = _keep(n, seed)
    m = int(keep.sum()) if packed else n
    x, eps, xi, y = pr.exact_inputs(3, n, 3, m, seed)
    return keep, x, eps, xi, y


@pytest.mark.parametrize("packed", [True, False])
def test_exact_mask_cases_do_not_round(packed):
    n = 65
    keep, x, eps, xi, y = _exact_mask(n, 21, packed)
    rho = pr.exact_rho()
    z64, out64 = pr.step_from_prox(x.double(), eps.double(), xi.double(), y.double(),
                                   lambda a, b, r: pr.mask_prox(a, b, keep, r, packed), rho)
    for form in ("residual", "blend"):
        z32, out32 = pr.step_from_prox(x, eps, xi, y,
                                       lambda a, b, r: pr.mask_prox(a, b, keep, r, packed, form), rho)
        assert z32.dtype == torch.float32
        assert torch.equal(z32.double(), z64) and torch.equal(out32.double(), out64), form
    wrong = keep.clone()
    j = int(torch.nonzero(keep)[3])
    wrong[j] = False  # one mask bit reversed
    if packed:
        wrong[int(torch.nonzero(~keep)[0])] = True  # the packed row keeps its length
    zw, ow = pr.step_from_prox(x, eps, xi, y, lambda a, b, r: pr.mask_prox(a, b, wrong, r, packed), rho)
    assert not torch.equal(zw.double(), z64) and not torch.equal(ow.double(), out64)


@pytest.mark.parametrize("s,shape", [(2, (1, 2, 2)), (8, (1, 8, 8)), (2, (3, 16, 24)), (4, (3, 16, 24)),
                                     (8, (2, 32, 40))])
def test_exact_sr_cases_do_not_round(s, shape):
    c, hh, ww = shape
    n, m = c * hh * ww, c * hh * ww // (s * s)
    x, eps, xi, y = pr.exact_inputs(2, n, 2, m, 31 + s)
    rho = pr.exact_rho(s)
    sh = lambda t: t.reshape(-1, *shape)  # noqa: E731
    ysh = lambda t: t.reshape(-1, c, hh // s, ww // s)  # noqa: E731
    z64, out64 = pr.step_from_prox(sh(x).double(), sh(eps).double(), sh(xi).double(), ysh(y).double(),
                                   lambda a, b, r: pr.sr_prox(a, b, s, r), rho)
    for form in ("residual", "blend"):
        z32, out32 = pr.step_from_prox(sh(x), sh(eps), sh(xi), ysh(y),
                                       lambda a, b, r: pr.sr_prox(a, b, s, r, form), rho)
        assert torch.equal(z32.double(), z64) and torch.equal(out32.double(), out64), form
    if ww == s:  # one block per row: the rolled grid holds the same pixels
        return
    zw, ow = pr.step_from_prox(sh(x), sh(eps), sh(xi), ysh(y),
                               lambda a, b, r: pr.sr_prox(a, b, s, r, shift=1), rho)
    assert not torch.equal(zw.double(), z64) and not torch.equal(ow.double(), out64)


def test_reference_loop_runs_and_is_deterministic():
    import stand_ins as si

    shape, b, N = (3, 8, 8), 2, 6
    core = si.EpsCore("conv", 3, 0.1).double()
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).double()
    init, steps = si.replay_noise(3, (b, *shape), N)
    keep = _keep(3 * 64, 4)
    apply = lambda x: x.reshape(x.shape[0], -1)[:, keep]  # noqa: E731
    y = apply(si.fixture_x_true(b, shape).double())
    prox = lambda x0, yy, rho: pr.mask_prox(x0.reshape(b, -1), yy, keep, rho).reshape(x0.shape)  # noqa: E731
    run = lambda: pr.diffpir_reference(lambda x, t: core(x, t), acp,  # noqa: E731
                                       si.leading_timesteps_ascending(N).tolist(), apply, prox, y,
                                       init.double(), lambda i: steps[i], sigma=0.05)
    one, two = run(), run()
    assert torch.equal(one, two) and torch.isfinite(one).all() and one.shape == (b, *shape)
