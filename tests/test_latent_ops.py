"""tests/latent_ops.py pinned without a GPU: the fp64 restatements against torch autograd,
``torch.optim.AdamW`` and the oracle's ReSample expressions, and negative controls showing that
the comparison helpers reject the failures the GPU tests exist to catch (a stale last tile, a
zeroed tail, a wrong observation row, swapped coefficients, a rank off by one, a wrong residual
norm, a skipped stride trip)."""

import math

import numpy as np
import pytest
import torch

import latent_ops as lo
import stand_ins as si
from oracle import blur as oblur
from oracle import closed_form, resample_loop
from samplers_amd.samplers.resample import adamw_coefficients
from samplers_amd.samplers.utils.bridge_kernels import eps_step_coefficients


def _mask_keep(shape, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(math.prod(shape), generator=g) >= 0.5).numpy()


def _kind_ops(kind, shape):
    """(numpy apply, numpy adjoint, torch apply, torch adjoint) of one operator kind; the torch
    maps are differentiable and act on flat (B, n) / (B, m) float64 tensors."""
    n = math.prod(shape)
    if kind == "identity":
        return (*closed_form.identity_ops(), lambda x: x, lambda y: y)
    keep = _mask_keep(shape)
    if kind == "inpaint":
        kept = np.flatnonzero(keep)
        idx = torch.from_numpy(kept)

        def adj_t(y):
            return torch.zeros(y.shape[0], n, dtype=y.dtype).index_copy(1, idx, y)

        return (*closed_form.inpaint_ops(kept, n), lambda x: x[:, idx], adj_t)
    if kind == "mask":
        kt = torch.from_numpy(keep).to(torch.float64)
        return (*closed_form.mask_ops(keep), lambda x: x * kt, lambda y: y * kt)
    k1d = oblur.taps(5, 1.5)
    b = lambda x: oblur.blur(x.reshape(-1, *shape), k1d).reshape(x.shape[0], -1)  # noqa: E731
    bt = lambda y: oblur.blur_adjoint(y.reshape(-1, *shape), k1d).reshape(y.shape[0], -1)  # noqa: E731
    return (*oblur.blur_ops(shape, k1d), b, bt)


@pytest.mark.parametrize("kind", ["identity", "inpaint", "mask", "blur"])
def test_psld_cotangent_is_the_autograd_gradient(kind):
    """sp_psld_cotangent's documented value is d/dx0 of omega ||y - A x0|| + <u, x_eff(x0)> with
    the batch-global norm, y_div = 2."""
    shape, batch, y_div, omega = (1, 19, 21), 4, 2, 0.3
    apply, adjoint, a_t, at_t = _kind_ops(kind, shape)
    n = math.prod(shape)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(batch, n, generator=g, dtype=torch.float64)
    u = torch.randn(batch, n, generator=g, dtype=torch.float64)
    m = apply(x0.numpy()).shape[1]
    y = torch.randn(batch // y_div, m, generator=g, dtype=torch.float64)
    x_eff, atr, rsq = lo.psld_pixel64(x0, y, y_div, apply, adjoint)
    got = lo.psld_cotangent64(atr, u, rsq.sum(), omega, apply, adjoint)

    xr = x0.clone().requires_grad_()
    yb = y[torch.arange(batch) // y_div]
    ax = a_t(xr)
    x_eff_t = at_t(yb) + xr - at_t(ax)
    loss = omega * torch.linalg.norm(yb - ax) + (u * x_eff_t).sum()
    (ref,) = torch.autograd.grad(loss, xr)
    np.testing.assert_allclose(x_eff, x_eff_t.detach().numpy(), rtol=0, atol=1e-13)
    err = np.abs(got - ref.numpy()).max()
    print("cotangent vs autograd", kind, err)
    assert err < 1e-13
    # a zero norm: only the (I - A^T A) u term, finite
    zero = lo.psld_cotangent64(atr, u, 0.0, omega, apply, adjoint)
    np.testing.assert_array_equal(zero, u.numpy() - adjoint(apply(u.numpy())))


def test_adamw64_and_pixel_opt64_match_torch_adamw():
    """Five torch.optim.AdamW steps on fp64 tensors (lr = 1e-2, MSELoss(y, A x), inpainting).
    The only difference is the fp32 rounding of the host coefficients (~6e-8 each): bound 1e-6
    relative to max|p|."""
    shape, batch, y_div, lr = (1, 19, 21), 4, 2, 1e-2
    apply, adjoint, a_t, _ = _kind_ops("inpaint", shape)
    n = math.prod(shape)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(batch, n, generator=g, dtype=torch.float64)
    y = torch.randn(batch // y_div, apply(x.numpy()).shape[1], generator=g, dtype=torch.float64)
    yb = y[torch.arange(batch) // y_div]
    total = yb.numel()
    gs = float(np.float32(-2.0 / total))

    p = x.clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr)
    xs, ms, vs = x.numpy(), np.zeros((batch, n)), np.zeros((batch, n))
    ps, m2, v2 = x.numpy(), np.zeros((batch, n)), np.zeros((batch, n))
    for step in range(1, 6):
        opt.zero_grad()
        loss = torch.nn.MSELoss()(yb, a_t(p))
        loss.backward()
        grad = p.grad.detach().numpy().copy()
        c = adamw_coefficients(step, lr)
        # the fused pass: its partials are the loss of x before the update
        xs, ms, vs, rsq = lo.pixel_opt64(xs, ms, vs, y, y_div, gs, c, apply, adjoint)
        assert abs(rsq.sum() / total - loss.item()) <= 1e-6 * loss.item()  # x is within 1e-6
        ps, m2, v2 = lo.adamw64(ps, grad, m2, v2, c)
        opt.step()
        ref = p.detach().numpy()
        scale = np.abs(ref).max()
        e1, e2 = np.abs(xs - ref).max() / scale, np.abs(ps - ref).max() / scale
        print("adamw step", step, e1, e2)
        assert e1 < 1e-6 and e2 < 1e-6
        st = opt.state[p]
        # the moments see the fp32 betas directly: 1 - fp32(beta) is off by up to
        # 2^-24 beta / (1 - beta) relative = 5.4e-7 (beta1 = 0.9), 6e-5 (beta2 = 0.999)
        assert np.abs(m2 - st["exp_avg"].numpy()).max() <= 1e-6 * np.abs(m2).max()
        assert np.abs(v2 - st["exp_avg_sq"].numpy()).max() <= 1e-4 * np.abs(v2).max()


def _acp():
    return torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)


@pytest.mark.parametrize("eta", [1.0, 0.0])
def test_ddim_eps64_matches_the_oracle_step(eta):
    """oracle.resample_loop.ddim_step_eps in fp64 with the same draw.  The helper takes the
    fp32 coefficients of eps_step_coefficients (sigma and dir go through 1 - a_t / a_prev in
    fp32, a cancellation of ~1 digit at t = 500 -> 480), so the distance is a few 1e-7; the bound
    is the kernels' own 2e-5 x max|reference|."""
    acp = _acp()
    g = torch.Generator().manual_seed(2)
    x, e, xi = (torch.randn(3, 1003, generator=g, dtype=torch.float64) for _ in range(3))
    ref = resample_loop.ddim_step_eps(x, lambda v, t: e, acp.double(), 500, 480, eta,
                                      lambda shape: xi)
    from samplers_amd import _hip

    c = eps_step_coefficients(acp.numpy(), 500, 480, eta)
    assert (c["sigma"] == 0.0) == (eta == 0.0)
    coefs = _hip.SpEpsCoefs(c["sqrt_oma"], c["oma"], c["sqrt_a"], c["sqrt_a_prev"], c["sigma"],
                            c["dir"])
    for got, want in zip(lo.ddim_eps64(x, e, coefs, xi), ref):
        err = lo.assert_close_scaled(got, want.numpy())
        print("ddim_eps64 vs oracle", eta, err)
        assert err < 2e-6


def test_stochastic_resample64_matches_the_oracle_expression():
    """The expression of oracle/resample_loop.py's resample step, in fp64 torch, with a_prev and
    sigma as resample.py forms them (fp32, sigma_scale = 40)."""
    f = np.float32
    acp = _acp().numpy()
    a_t, a_prev = f(acp[500]), f(acp[480])
    sigma = float(f(40.0) * (f(1) - a_prev) / (f(1) - a_t) * (f(1) - a_t / a_prev))
    g = torch.Generator().manual_seed(4)
    z_opt, snap, noise = (torch.randn(3, 1003, generator=g, dtype=torch.float64) for _ in range(3))
    ap, sg = torch.tensor(float(a_prev), dtype=torch.float64), torch.tensor(sigma, dtype=torch.float64)
    ref = (sg * ap.sqrt() * z_opt + (1 - ap) * snap) / (sg + 1 - ap) \
        + noise * torch.sqrt(1 / (1 / sg + 1 / (1 - ap)))
    got = lo.stochastic_resample64(z_opt, snap, float(a_prev), sigma, noise)
    assert np.abs(got - ref.numpy()).max() < 1e-13


def test_scaled_combine64_and_stop_rules():
    b = np.arange(6.0).reshape(2, 3)
    a = np.ones((2, 3))
    np.testing.assert_allclose(lo.scaled_combine64(a, 2.0, b, 3.0, 4.0), 2.0 + 1.5 * b)
    np.testing.assert_array_equal(lo.scaled_combine64(None, 0.0, b, 3.0, None), 3.0 * b)
    np.testing.assert_array_equal(lo.scaled_combine64(a, 2.0, b, 3.0, 0.0), 2.0 * a)
    # strict compare in double: 3 / 4 is not below 0.75, but is below the next double
    r = lo.StopRule(4.0, 0.75)
    assert r.check(np.full(12, 0.25)) and r.stop == 0 and r.loss == 0.75
    r = lo.StopRule(4.0, float(np.nextafter(0.75, 1.0)))
    assert r.check(np.full(12, 0.25)) and r.stop == 1
    assert not r.check(np.full(12, 1.0)) and r.loss == 0.75  # sticky
    # the plateau rule: quiet below plateau_from, then stops on the first rise
    p = lo.StopRule(300.0, 0.5, plateau_from=3)
    seen = []
    for itr, loss in enumerate([5, 4, 6, 3, 2, 2.5, 1]):
        wrote = p.check(np.full(300, float(loss)), itr)
        seen.append((wrote, p.stop, p.prev))
    assert seen == [(True, 0, None), (True, 0, None), (True, 0, None), (True, 0, 3.0),
                    (True, 0, 2.0), (True, 1, 2.5), (False, 1, 2.5)]
    q = lo.StopRule(300.0, 0.5, plateau_from=3)
    q.check(np.full(300, 0.25), 0)
    assert q.stop == 1 and q.prev is None


# --- negative controls: the helpers must reject these known-wrong outputs ------------------------
def _inpaint_case(shape=(1, 37, 83), batch=3, y_div=1, seed=7):
    n = math.prod(shape)
    keep = _mask_keep(shape, seed)
    kept = np.flatnonzero(keep)
    apply, adjoint = closed_form.inpaint_ops(kept, n)
    g = np.random.default_rng(seed)
    x0 = g.standard_normal((batch, n))
    y = g.standard_normal((batch // y_div, kept.size))
    return n, keep, kept, apply, adjoint, x0, y


def test_control_last_partial_tile_left_at_prefill():
    n, _, _, apply, adjoint, x0, y = _inpaint_case()
    x_eff, atr, _ = lo.psld_pixel64(x0, y, 1, apply, adjoint)
    lo.assert_close_scaled(x_eff.astype(np.float32), x_eff)
    tile = 2 * 256  # V = 1, two groups per thread: the last tile starts at 2560 and is 511 long
    wrong = x_eff.astype(np.float32)
    wrong[:, (n // tile) * tile:] = np.nan
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(wrong, x_eff)
    wrong = x_eff.astype(np.float32)
    wrong[-1, -1] = np.nan  # a single element of the last sample
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(wrong, x_eff)


def test_control_tail_of_a_4320_row_zeroed():
    g = np.random.default_rng(0)
    ref = g.standard_normal((6, 4320))
    wrong = ref.astype(np.float32)
    wrong[:, 4096:] = 0.0  # the 224 elements past the last full tile
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(wrong, ref)
    rsq = (ref ** 2).sum(1)
    part = np.stack([(ref[:, :2048] ** 2).sum(1), (ref[:, 2048:4096] ** 2).sum(1),
                     (ref[:, 4096:] ** 2).sum(1)], axis=1)
    lo.assert_rsq(part.astype(np.float32), rsq)
    part[:, 2] = 0.0
    with pytest.raises(AssertionError):
        lo.assert_rsq(part, rsq)
    part[:, 2] = np.nan
    with pytest.raises(AssertionError):
        lo.assert_rsq(part, rsq)


def test_control_y_div_ignored():
    n, _, _, apply, adjoint, x0, _ = _inpaint_case(shape=(1, 19, 21), batch=6)
    y = np.random.default_rng(1).standard_normal((6, apply(x0).shape[1]))
    x_eff, atr, rsq = lo.psld_pixel64(x0, y[:2], 3, apply, adjoint)       # rows b // 3
    w_eff, w_atr, w_rsq = lo.psld_pixel64(x0, y, 1, apply, adjoint)        # row b
    for wrong, ref in ((w_eff, x_eff), (w_atr, atr)):
        with pytest.raises(AssertionError):
            lo.assert_close_scaled(wrong, ref)
    with pytest.raises(AssertionError):
        lo.assert_rsq(w_rsq.reshape(-1, 1), rsq)


def test_control_oma_and_sqrt_oma_swapped():
    from samplers_amd import _hip

    c = eps_step_coefficients(_acp().numpy(), 500, 480, 1.0)
    good = _hip.SpEpsCoefs(c["sqrt_oma"], c["oma"], c["sqrt_a"], c["sqrt_a_prev"], c["sigma"], c["dir"])
    swap = _hip.SpEpsCoefs(c["oma"], c["sqrt_oma"], c["sqrt_a"], c["sqrt_a_prev"], c["sigma"], c["dir"])
    g = np.random.default_rng(2)
    x, e, xi = (g.standard_normal((3, 1003)) for _ in range(3))
    for wrong, ref in zip(lo.ddim_eps64(x, e, swap, xi), lo.ddim_eps64(x, e, good, xi)):
        with pytest.raises(AssertionError):
            lo.assert_close_scaled(wrong, ref)


def test_control_inpaint_rank_off_by_one_from_the_second_word():
    n, keep, kept, apply, adjoint, x0, y = _inpaint_case()
    x_eff, atr, rsq = lo.psld_pixel64(x0, y, 1, apply, adjoint)
    # the kernel's gather with rank + 1 for every element of word 1 and later
    rank = np.cumsum(keep) - keep
    shifted = np.minimum(rank + (np.arange(n) >= 64), kept.size - 1)
    yv = np.where(keep[None, :], y[:, shifted], 0.0)
    w_eff = np.where(keep[None, :], yv, x0)
    r = np.where(keep[None, :], yv - x0, 0.0)
    np.testing.assert_allclose(w_eff[:, :64], x_eff[:, :64], rtol=0, atol=1e-15)  # word 0 is right
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(w_eff, x_eff)
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(r, atr)
    with pytest.raises(AssertionError):
        lo.assert_rsq((r ** 2).sum(1).reshape(-1, 1), rsq)


def test_control_masked_elements_in_the_wrong_residual_norm():
    n, keep, kept, apply, adjoint, x0, y = _inpaint_case()
    _, _, rsq = lo.psld_pixel64(x0, y, 1, apply, adjoint)
    # INPAINT: the dropped elements counted as r = 0 - x0
    with pytest.raises(AssertionError):
        lo.assert_rsq((rsq + (x0[:, ~keep] ** 2).sum(1)).reshape(-1, 1), rsq)
    # MASK: the dropped elements' y^2 belong to the norm (A x0 = 0 there)
    m_apply, m_adjoint = closed_form.mask_ops(keep)
    yf = np.random.default_rng(3).standard_normal((3, n))
    _, _, m_rsq = lo.psld_pixel64(x0, yf, 1, m_apply, m_adjoint)
    with pytest.raises(AssertionError):
        lo.assert_rsq((m_rsq - (yf[:, ~keep] ** 2).sum(1)).reshape(-1, 1), m_rsq)


@pytest.mark.parametrize("n,vec", [(12288, 4), (3071, 1)])
def test_control_one_stride_trip_skipped(n, vec):
    """batch 400: 12 blocks of work against a cap of 4096 // 400 = 10, so elements
    [10 * 256 * V, n) belong to the second trip; stale there (NaN prefill, or the input)."""
    cap = 4096 // 400
    g = np.random.default_rng(4)
    ref = g.standard_normal((400, n))
    assert cap * 256 * vec < n
    for stale in (np.nan, 0.0):
        wrong = ref.astype(np.float32)
        wrong[:, cap * 256 * vec:] = stale
        with pytest.raises(AssertionError):
            lo.assert_close_scaled(wrong, ref)
    wrong = ref.astype(np.float32)
    wrong[399, cap * 256 * vec:] = ref[399, cap * 256 * vec:] * (1 + 1e-3)  # the last sample only
    with pytest.raises(AssertionError):
        lo.assert_close_scaled(wrong, ref)
