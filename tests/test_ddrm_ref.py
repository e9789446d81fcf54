"""The DDRM step's three forms against each other on the CPU (tests/ddrm_ref.py): the projector
form (A Aᵀ = g·I) and the DFT form (periodic blur) against the dense eigendecomposition at 1e-10,
the two identities every class satisfies, the fp32 class mask against the fp64 decision, and the
exact cases on which the fp32 emulations of the kernels return the fp64 result bit for bit - and a
swapped class, a kept −c₁σ'ε on the observed set or an unprojected ξ does not."""

import itertools

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import periodic_ops as po
from samplers_amd.operators import PeriodicBlurOperator
from samplers_amd.operators.blur import gaussian_taps

SCALARS = [dr.make_coefs(sp, sy, eta, eb) for sp, sy, (eta, eb)
           in itertools.product(dr.SIG_PREVS, dr.SIG_YS, dr.ETAS)]
TOL = 1e-10


def _data(batch, n, m, seed):
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randn(batch, n, generator=g, dtype=torch.float64) for _ in range(3))
    return x, eps, xi, torch.randn(batch, m, generator=g, dtype=torch.float64)


def _close(got, ref):
    scale = max(float(ref.abs().max()), 1e-300)
    return float((got - ref).abs().max()) / scale


# --- projector form against the dense form -----------------------------------------------------------
def _projector_cases():
    g = torch.Generator().manual_seed(5)
    keep = torch.rand(12, generator=g) < 0.5
    keep[0], keep[1] = True, False
    yield "identity", (12,), 1.0, dr.mask_ops(torch.ones(12, dtype=torch.bool)), lambda x: x
    yield "inpaint", (12,), 1.0, dr.mask_ops(keep), lambda x: x[:, keep]
    for s, shape in ((2, (1, 4, 4)), (4, (1, 8, 8))):
        yield (f"sr{s}", shape, 1.0 / (s * s), dr.sr_ops(shape, s),
               lambda x, s=s: torch.nn.functional.avg_pool2d(x, s).reshape(x.shape[0], -1))


@pytest.mark.parametrize("name,shape,g,ops,apply", list(_projector_cases()),
                         ids=[c[0] for c in _projector_cases()])
def test_projector_form_is_the_dense_form(name, shape, g, ops, apply):
    proj, up = ops
    A = dr.dense_matrix(apply, shape)
    assert torch.allclose(A @ A.T, g * torch.eye(A.shape[0], dtype=torch.float64), atol=1e-14)
    x, eps, xi, y = _data(3, A.shape[1], A.shape[0], 17)
    worst = 0.0
    for c in SCALARS:
        ref = dr.dense_step(A, x, eps, y, xi, c)
        got = dr.projector_step(x, eps, up(y), xi, c, g, proj)
        worst = max(worst, _close(got, ref))
    print(f"{name}: projector against dense {worst:.3g}")
    assert worst <= TOL


# --- DFT form against the dense form -------------------------------------------------------------------
def _gauss(k, sigma):
    t = gaussian_taps(k, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


def _psf(kind):
    if kind == "gauss":
        return _gauss(5, 1.2)
    g = torch.Generator().manual_seed(23)
    h = torch.rand(5, 5, generator=g)
    return h / h.sum()


@pytest.mark.parametrize("kind", ["random5", "gauss"])
def test_dft_form_is_the_dense_form(kind):
    shape = (1, 8, 8)
    op = PeriodicBlurOperator(shape, _psf(kind))
    keep, M = op.keep.clone(), po.transfer(op.kernel, 8, 8)
    if kind == "gauss":
        assert 0.0 < float(keep.float().mean()) < 1.0  # some frequencies dropped
    A = dr.dense_matrix(dr.truncated_blur(M, keep), shape)
    x, eps, xi, _ = _data(3, 64, 64, 29)
    y = po.blur(torch.randn(3, *shape, dtype=torch.float64), op.kernel).reshape(3, -1)
    y = y + 0.05 * torch.randn(3, 64, dtype=torch.float64)
    r = lambda t: t.reshape(3, *shape)  # noqa: E731
    worst = 0.0
    for c in SCALARS:
        ref = dr.dense_step(A, x, eps, y, xi, c)
        got = dr.dft_step(r(x), r(eps), r(y), r(xi), c, M, keep).reshape(3, -1)
        worst = max(worst, _close(got, ref))
    print(f"{kind}: DFT against dense {worst:.3g}, kept {float(keep.float().mean()):.2f}")
    assert worst <= TOL


# --- the identities ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SCALARS, ids=lambda c: f"{c['sig_prev']}-{c['sig_y']}-{c['eta']}-{c['eta_b']}")
def test_the_two_identities_hold_in_every_class(c):
    s = torch.cat([torch.zeros(2, dtype=torch.float64),
                   torch.logspace(-4, 1, 200, dtype=torch.float64)])
    s2 = s * s
    for observed in (torch.ones_like(s2, dtype=torch.bool), torch.arange(s2.numel()) % 3 != 0):
        f_th, f_ep, f_y, f_xi = dr.coefficients(s2, observed, dr.big_mask64(s2, c), c)
        assert float((f_th + f_y - 1).abs().max()) <= 1e-14
        obs = observed & (s2 > 0)
        var_y = torch.where(obs, f_y ** 2 * c["sig_y"] ** 2 / torch.where(obs, s2, torch.ones_like(s2)),
                            torch.zeros_like(s2))
        marginal = var_y + f_ep ** 2 + f_xi ** 2
        assert float((marginal - c["sig_prev"] ** 2).abs().max()) <= 1e-12 * max(c["sig_prev"] ** 2, 1.0)
        assert bool((f_y[~obs] == 0).all()) and bool((f_ep[obs] == 0).all())


# --- the class mask -----------------------------------------------------------------------------------------
def test_fp32_mask_is_the_fp64_decision_away_from_the_threshold():
    g = torch.Generator().manual_seed(31)
    s2 = torch.exp(torch.rand(20000, generator=g) * 22.0 - 16.0).float()
    M = po.transfer(_gauss(5, 1.2), 24, 16).to(torch.complex64)
    s2 = torch.cat([s2, dr.s2_of_spectrum32(M).reshape(-1), torch.zeros(3), torch.ones(3)])
    checked = 0
    for c in SCALARS + [dr.make_coefs(0.25, 0.25, 0.5, 1.0), dr.make_coefs(0.1, 0.3, 0.5, 1.0)]:
        c = dr.round32(c)
        got = dr.big_mask32(s2, c)
        want = dr.big_mask64(s2, c)
        if c["sig_y"] > 0:
            ratio = (c["sig_prev"] ** 2) * s2.double() / c["sig_y"] ** 2
            far = (ratio - 1).abs() > 1e-5
        else:
            far = torch.ones_like(want)
        checked += int(far.sum())
        assert torch.equal(got[far], want[far]), c
    assert checked > 100000
    # on the threshold itself the expression is what it is: s2 = 1, sig_prev = sig_y -> big
    assert bool(dr.big_mask32(np.ones(1, np.float32), dr.make_coefs(0.25, 0.25, 0.5, 1.0)).all())


def test_fp32_dft_emulation_is_near_the_fp64_form_given_the_mask():
    shape = (2, 24, 16)
    op = PeriodicBlurOperator(shape, _gauss(9, 1.5))
    M32 = po.transfer(op.kernel, 24, 16).to(torch.complex64)
    g = torch.Generator().manual_seed(37)
    x, eps, xi, y = (torch.randn(3, *shape, generator=g) for _ in range(4))
    for c in (dr.make_coefs(0.5, 0.05, 0.85, 1.0), dr.make_coefs(0.041, 0.05, 0.85, 1.0)):
        c = dr.round32(c)
        big = dr.big_mask32(dr.s2_of_spectrum32(M32), c)
        ref = dr.dft_step(x.double(), eps.double(), y.double(), xi.double(), c, M32.to(torch.complex128),
                          op.keep, big)
        got = dr.dft_step(x, eps, y, xi, c, M32, op.keep, big)
        assert _close(got.double(), ref) <= 2e-5


# --- exact cases ----------------------------------------------------------------------------------------------
EXACT = [("identity", 1), ("mask", 1), ("sr", 2), ("sr", 4), ("sr", 8)]


def _exact_case(kind, s, regime, variant=None):
    """(fp32 emulation, fp64 projector form) of one exact step."""
    c = dr.exact_coefs(regime, s)
    if kind == "sr":
        shape = (2, 2 * s, 3 * s)
        n, m = 6 * s * s * 2, 12
        x, eps, xi, y = dr.exact_inputs(3, n, 3, m, 40 + s)
        proj, up = dr.sr_ops(shape, s)
        emu = dr.emu_sr(x, eps, y, xi, c, shape, s, variant)
        ref = dr.projector_step(x.double(), eps.double(), up(y.double()), xi.double(), c, 1.0 / (s * s), proj)
    else:
        n = 37
        keep = torch.ones(n, dtype=torch.bool)
        if kind == "mask":
            keep = torch.arange(n) % 3 != 1
        x, eps, xi, y = dr.exact_inputs(3, n, 3, n, 50)
        proj, up = dr.mask_ops(keep, packed=False)
        emu = dr.emu_elementwise(x, eps, up(y), keep, xi, c, variant)
        ref = dr.projector_step(x.double(), eps.double(), up(y.double()), xi.double(), c, 1.0, proj)
    return emu, ref


@pytest.mark.parametrize("regime", ["big", "small"])
@pytest.mark.parametrize("kind,s", EXACT)
def test_exact_cases_emulations_return_the_fp64_result(kind, s, regime):
    emu, ref = _exact_case(kind, s, regime)
    assert emu.dtype == torch.float32 and torch.equal(ref.float().double(), ref)  # an fp32 number
    assert torch.equal(emu.double(), ref)
    c = dr.exact_coefs(regime, s)
    g = torch.tensor(1.0 / (s * s), dtype=torch.float32)
    assert bool(dr.big_mask32(g, c)) == (regime == "big") == bool(dr.big_mask64(g, c))


# in the small class f_xi = eta sig_prev on and off the observed set: projecting xi or not is the
# same map there, so that wrong answer is asked for in the big class alone
WRONG = [(v, r) for v in ("swap", "keep_eps", "xi_plain") for r in ("big", "small")
         if (v, r) != ("xi_plain", "small")]


@pytest.mark.parametrize("variant,regime", WRONG)
@pytest.mark.parametrize("kind,s", EXACT[1:])
def test_exact_cases_tell_wrong_answers_apart(kind, s, regime, variant):
    emu, ref = _exact_case(kind, s, regime, variant)
    assert not torch.equal(emu.double(), ref)
    # and the projector form's own wrong variants differ from the dense form's answer too
    right, _ = _exact_case(kind, s, regime)
    assert float((emu - right).abs().max()) > 1e-3
