"""tests/kind_harness.py itself, on the host: the guard bands catch a write on either side, the
trajectory bound accepts the fp32 loop and rejects one pushed 10 bounds away, and `reference_loop`
is the four reference functions under one name."""

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import kind_harness as kh
import prox_ref as pr
import stand_ins as si
from oracle import dps_loop
from oracle.latent_loops import pgdm_reference


def test_guard_bands_catch_a_write_on_either_side():
    floats = 24
    whole, view = kh.guarded(floats, "cpu")
    assert whole.numel() == floats + 32 and view.numel() == floats and torch.isnan(whole).all()
    view.fill_(1.0)  # the view lies between the bands
    kh.check_guards(whole, floats)
    for index in (15, 16 + floats):
        whole, _ = kh.guarded(floats, "cpu")
        whole[index] = 0.0
        with pytest.raises(AssertionError):
            kh.check_guards(whole, floats)
    whole, _ = kh.guarded(0, "cpu")  # a kind without a workspace
    kh.check_guards(whole, 0)


def _recurrence(dt):
    """x <- 1.7 x (1 - x) + 0.1 over 40 steps: fp32 drifts from fp64 by a few ulps per step."""
    x = torch.linspace(0.1, 0.9, 64, dtype=torch.float64).to(dt)
    for _ in range(40):
        x = 1.7 * x * (1 - x) + 0.1
    return x


def test_loop_bound_and_bound_check():
    ref32, bound = kh.loop_bound(_recurrence)
    cond = si.relative_error(_recurrence(torch.float64), ref32)
    assert ref32.dtype == torch.float32 and bound == max(1e-4, 20 * cond)
    seen = []
    record = lambda metric, value, bound, **extra: seen.append((metric, value, bound, extra))  # noqa: E731
    kh.bound_check(_recurrence(torch.float32).reshape(8, 8), _recurrence, "toy", record)
    assert seen == [("toy_rel_l2", 0.0, bound, dict(fp32_to_fp64=cond))]
    with pytest.raises(AssertionError):
        kh.bound_check(_recurrence(torch.float32) * (1 + 10 * bound), _recurrence, "toy", record)
    assert len(seen) == 2 and seen[1][0] == "toy_rel_l2" and seen[1][1] > bound  # recorded before it asserts


class _Identity:
    """A = I: every map a copy, the prox and the DDRM step simple closed forms."""

    def __init__(self):
        self.coefs = []

    apply = pinv = staticmethod(lambda x: x)

    def prox(self, x0, y, rho):
        return (y + rho * x0) / (1 + rho)

    def ddrm(self, x, eps, y, xi, c):
        self.coefs.append(c)
        return c["a_prev"] * ((x - c["k"] * eps) / c["a"] + 0.1 * (y - x)) + 0.05 * xi


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("sampler", ["dps", "pgdm", "diffpir", "ddrm"])
def test_reference_loop_is_the_reference_function(sampler, dt):
    n_steps, sigma, shape = 5, 0.05, (2, 1, 4, 4)
    init, steps = si.replay_noise(3, shape, n_steps)
    y = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    ts = si.leading_timesteps_ascending(n_steps).tolist()
    eps_fn = lambda x, t: 0.1 * x  # noqa: E731
    noise = lambda i: steps[i].to(dt)  # noqa: E731
    S, acp = _Identity(), kh.acp(dt)
    got = kh.reference_loop(sampler, S, eps_fn, acp, ts, y, init, noise, dt, sigma)
    a = (eps_fn, acp, ts)
    if sampler == "dps":
        want = dps_loop.dps_reference(*a, S.apply, dps_loop.gaussian_log_prob(sigma), y.to(dt), init.to(dt), noise,
                                      gamma=kh.GAMMA, eta=kh.ETA)
    elif sampler == "pgdm":
        want = pgdm_reference(*a, S.apply, S.pinv, y.to(dt), init.to(dt), noise, guidance_weight=kh.GUIDANCE,
                              eta=kh.ETA)
    elif sampler == "diffpir":
        want = pr.diffpir_reference(*a, S.apply, lambda x0, yy, rho: S.prox(x0, yy, float(rho)), y.to(dt),
                                    init.to(dt), noise, sigma=sigma)
    else:
        seen, S.coefs = S.coefs, []
        assert len(seen) == n_steps - 2
        for c in seen:  # the scalars the kernels are given: rounded to fp32 in the fp32 loop only
            assert (c == dr.round32(c)) == (dt == torch.float32)
        step = lambda x, e, yy, xi, c: S.ddrm(x, e, yy, xi, dr.round32(c) if dt == torch.float32 else c)  # noqa: E731
        want = dr.ddrm_reference(*a, step, y.to(dt), init.to(dt), noise, sigma_y=sigma)
    assert got.dtype == dt and torch.equal(got, want)
    with pytest.raises(AssertionError):
        kh.reference_loop("psld", S, eps_fn, acp, ts, y, init, noise, dt, sigma)


def test_small_helpers():
    assert kh.f32(dict(a=0.1)) == dict(a=float(np.float32(0.1)))
    assert kh.acp(torch.float64).dtype == torch.float64 and float(kh.acp()[0]) == 1.0
    d = kh.make_descriptor(3, 12, 6, c=1, h=3, w=4, radius=2, factor=5)
    assert (d.kind, d.n, d.m, d.channels, d.height, d.width, d.radius, d.factor) == (3, 12, 6, 1, 3, 4, 2, 5)
    assert not d.taps and not d.keep_bits and not d.word_rank
    net, flags = kh.counting_net("conv", 1, 0.1)
    net.set_sampling_parameters(4)
    x, t = torch.zeros(1, 1, 4, 4), torch.tensor(5)
    with torch.no_grad():
        net.forward(x, t)
    net.forward(x, t)
    assert flags == [False, True] and net.graph_flags is flags
    script = kh.DEBUG_SWEEP_CHILD("test_some_gpu")
    assert "import test_some_gpu as T" in script and "debug build: clean" in script
    compile(script, "child", "exec")
