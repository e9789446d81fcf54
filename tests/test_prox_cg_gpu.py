"""The proximal data step by conjugate gradients on the GPU (sp_op_prox_cg_ws,
sp_diffpir_step_cg_ws; csrc/sp_cg.hip) through the raw entry points, into NaN-filled outputs and a
NaN-filled workspace between guard bands, against the fp64 semantics of tests/prox_cg_ref.py; then
Operator.apply_prox_cg on device tensors and DiffPIRSampler(prox="cg") against the reference loop.

Shapes (prox_cg_ref._operators) are the smallest that reach every path: n = 3 below one vector;
inpaint n = 5000 with several workgroups and partials per sample and m != n; SR x4 (3,16,24);
Gaussian blur (3,33,35) with n % 4 != 0; an asymmetric 3x3 PSF on (2,12,12); PSF_FFT reflect
(3,16,16); PSF_PERIODIC (1,8,12); SR_PERIODIC (1,16,16), s = 2, K = 4 (the workspace kinds, m != n);
Radon (1,9,13) with 7 angles and (1,40,36) with 5 angles on a 301-bin detector (odd sizes, m > n).
Every case runs at (batch 3, y_div 3) and (batch 4, y_div 2).

Bounds.  Few iterations (K = 1, 2, 3, tol = 0) against the fp64 recurrence at the same K, and
converged (K = 64, tol = 1e-6) against the dense fp64 solve: max|err| <= max(2e-5, 4 x the CPU
fp32 emulation's own distance to that reference) x max|ref|; the optimality residual under
max(1e-5, 4 x the emulation's).  The few-iteration form is not extended to large K: CG amplifies
rounding (the emulation itself drifts to 1e-3 at K = 8 on the 9x13 Radon case).  Trajectories:
max(1e-4, 20 x the fp32 reference loop's distance to its fp64 run), the project's rule.

Measured on an MI355X: see README.md "Proximal map by conjugate gradients" (parity_record has every
figure)."""


import pytest
import torch

import prox_cg_ref as cg
import prox_ref as pr
import stand_ins as si
from exact_cases import Guarded
from kind_harness import DEBUG_SWEEP_CHILD, run_debug_child, stream as _stream
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import (GaussianBlurOperator, RadonOperator, RandomInpaintingOperator,
                                    SuperResolutionOperator)

pytestmark = pytest.mark.gpu

SEED, STEP, OFFSET = 11, 5, 7
_DEV: dict = {}


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


COEFS = dict(a=_f32(0.8), k=_f32(0.6), a_prev=_f32(0.9), c_eps=_f32(0.35), c_xi=_f32(0.25))


def _coefs(rho):
    return _hip.SpProxCoefs(COEFS["a"], COEFS["k"], rho, COEFS["a_prev"], COEFS["c_eps"], COEFS["c_xi"])


class Dev:
    """The device twin of a prox_cg_ref.Case: an operator of its own (Module.to moves in place)."""

    def __init__(self, name, device):
        self.c = cg.case(name)
        self.op = cg._operators()[name]().to(device)
        self.desc = self.op.hip_descriptor()
        assert (int(self.desc.n), int(self.desc.m)) == (self.c.n, self.c.m)
        self.n, self.m = self.c.n, self.c.m


def _dev(name, device):
    if name not in _DEV:
        _DEV[name] = Dev(name, device)
    return _DEV[name]


def _work(lib, d, batch, step, device):
    floats = int(lib.sp_prox_cg_workspace(d.desc, batch, step))
    assert floats > 0
    return Guarded((floats,), 64, device)


def run_prox(lib, d, x0, y, ydiv, rho, K, tol, alias=False, iters=True):
    """(z, iters) of sp_op_prox_cg_ws; alias: z_out = x0."""
    batch = x0.shape[0]
    work, out = _work(lib, d, batch, 0, x0.device), Guarded((batch, d.n), 64, x0.device)
    it = torch.full((batch,), -1, dtype=torch.int32, device=x0.device)
    if alias:
        out.t.copy_(x0)
    src = out.t if alias else x0
    _hip.check(lib.sp_op_prox_cg_ws(d.desc, src.data_ptr(), y.data_ptr(), batch, ydiv, rho, K, tol,
                                    out.ptr(), it.data_ptr() if iters else None, work.ptr(),
                                    _stream()), "sp_op_prox_cg_ws")
    work.check(nan_ok=True)
    return out.check(), it


def run_step(lib, d, x, eps, y, xi, ydiv, rho, K, tol, alias=False, offset=OFFSET):
    """(x', iters) of sp_diffpir_step_cg_ws; alias: x_out = x."""
    batch = x.shape[0]
    work, out = _work(lib, d, batch, 1, x.device), Guarded((batch, d.n), 64, x.device)
    it = torch.full((batch,), -1, dtype=torch.int32, device=x.device)
    if alias:
        out.t.copy_(x)
    src = out.t if alias else x
    _hip.check(lib.sp_diffpir_step_cg_ws(d.desc, src.data_ptr(), eps.data_ptr(), y.data_ptr(),
                                         xi.data_ptr() if xi is not None else None, SEED, STEP, offset,
                                         batch, ydiv, _coefs(rho), K, tol, out.ptr(), it.data_ptr(),
                                         work.ptr(), _stream()), "sp_diffpir_step_cg_ws")
    work.check(nan_ok=True)
    return out.check(), it


def _to(device, *ts):
    return tuple(t.to(device).contiguous() for t in ts)


def _rhos(name):
    return pr.RHOS if name in cg.ISOMETRIES else (1.0, 50.0)


# --- 1. few iterations, every kernel ----------------------------------------------------------------
@pytest.mark.parametrize("rho", pr.RHOS)
@pytest.mark.parametrize("name", cg.NAMES)
def test_few_iterations_match_the_fp64_recurrence(cuda, parity_record, name, rho):
    lib, d = _hip.load_library(), _dev(name, cuda)
    c, rho = d.c, _f32(rho)
    worst = 0.0
    for batch, ydiv in cg.BATCHES:
        x, yr = c.inputs(batch, ydiv)
        eps, xi = c.eps[:batch], c.xi[:batch]
        xd, ed, xid, yd = _to(cuda, x, eps, xi, c.y[:batch // ydiv])
        for K in (1, 2, 3):
            z64, _ = cg.cgls(c.A, x, yr, rho, K, 0.0)
            z32, _ = cg.cgls(c.A, x, yr, rho, K, 0.0, torch.float32)
            _, s64 = cg.step(x.double(), eps.double(), xi.double(),
                             lambda x0: cg.cgls(c.A, x0, yr, rho, K, 0.0)[0], COEFS)
            _, s32 = cg.step(x, eps, xi, lambda x0: cg.cgls(c.A, x0, yr, rho, K, 0.0, torch.float32)[0],
                             COEFS)
            z, it = run_prox(lib, d, xd, yd, ydiv, rho, K, 0.0)
            out, its = run_step(lib, d, xd, ed, yd, xid, ydiv, rho, K, 0.0)
            for what, got, ref, emu in (("z", z, z64, z32), ("step", out, s64, s32)):
                yard = cg.distance(emu, ref)
                bound = max(2e-5, 4 * yard)
                err = cg.distance(got.cpu(), ref)
                print(f"{name} rho={rho:g} b{batch} K={K} {what}: err {err:.3g} emulation {yard:.3g} "
                      f"bound {bound:.3g} iters {it.tolist()}")
                parity_record(f"cg_few_{what}_max_err_over_max", err, bound, rho=rho, K=K, emulation=yard)
                worst = max(worst, err / bound)
                assert err <= bound, (name, what, K, batch, err, bound)
            assert int(it.max()) <= K and int(its.max()) <= K and int(it.min()) >= 0
    print(f"{name} rho={rho:g}: worst err / bound {worst:.3g}")


# --- 2. converged, 3. the stop rule -----------------------------------------------------------------
def _converged_reference(c, batch, ydiv, rho):
    x, yr = c.inputs(batch, ydiv)

    def make():
        ref = cg.solve(c.A, x, yr, rho)
        emu, emu_it = cg.cgls(c.A, x, yr, rho, 64, 1e-6, torch.float32)
        assert bool(torch.isfinite(emu).all()) and int(emu_it.max()) < 64
        return ref, cg.distance(emu, ref), float(cg.optimality(c.A, emu, x, yr, rho).max())

    return c.memo(("converged", batch, ydiv, rho), make)


@pytest.mark.parametrize("name,rho", [(n, r) for n in cg.NAMES for r in _rhos(n)])
def test_converged_against_the_dense_solve_and_the_stop_rule(cuda, parity_record, name, rho):
    lib, d = _hip.load_library(), _dev(name, cuda)
    c, rho = d.c, _f32(rho)
    for batch, ydiv in cg.BATCHES:
        x, yr = c.inputs(batch, ydiv)
        ref, yard, opt_yard = _converged_reference(c, batch, ydiv, rho)
        xd, yd = _to(cuda, x, c.y[:batch // ydiv])
        z, it = run_prox(lib, d, xd, yd, ydiv, rho, 64, 1e-6)
        assert bool(torch.isfinite(z).all())
        bound, err = max(2e-5, 4 * yard), cg.distance(z.cpu(), ref)
        opt_bound = max(1e-5, 4 * opt_yard)
        opt = float(cg.optimality(c.A, z.cpu(), x, yr, rho).max())
        print(f"{name} rho={rho:g} b{batch}: err {err:.3g} emulation {yard:.3g} bound {bound:.3g}; "
              f"optimality {opt:.3g} emulation {opt_yard:.3g} bound {opt_bound:.3g}; iters {it.tolist()}")
        parity_record("cg_converged_max_err_over_max", err, bound, rho=rho, emulation=yard)
        parity_record("cg_converged_optimality", opt, opt_bound, rho=rho, emulation=opt_yard)
        assert err <= bound and opt <= opt_bound, (name, err, bound, opt, opt_bound)
        assert 1 <= int(it.min()) and int(it.max()) < 64, it.tolist()
        if name in cg.ISOMETRIES:
            assert int(it.max()) <= 2, it.tolist()
        # stopped samples never change: 300 iterations return the bits of 64
        z300, it300 = run_prox(lib, d, xd, yd, ydiv, rho, 300, 1e-6)
        assert torch.equal(z300, z) and torch.equal(it300, it)


@pytest.mark.parametrize("name", ["blur", "radon_small", "radon_wide"])
def test_every_iteration_is_live_at_a_small_rho(cuda, name):
    lib, d = _hip.load_library(), _dev(name, cuda)
    for batch, ydiv in cg.BATCHES:
        xd, yd = _to(cuda, d.c.x[:batch], d.c.y[:batch // ydiv])
        z, it = run_prox(lib, d, xd, yd, ydiv, _f32(1e-4), 8, 1e-6)
        assert it.tolist() == [8] * batch and bool(torch.isfinite(z).all())


def _mixed_batch(d, cuda):
    """Four samples that do not stop together: random data, no residual at all (y = A x0 by the
    library: stopped from the start), a residual 1e-3 times a random one, random data again."""
    xd = d.c.x.to(cuda).contiguous()
    ax = d.op.apply(xd.reshape(4, *d.op.x_shape)).reshape(4, d.m)
    yd = d.c.y.repeat_interleave(2, dim=0).to(cuda).contiguous()
    yd[1] = ax[1]
    yd[2] = ax[2] + 1e-3 * (yd[0] - ax[2])
    return xd, yd.contiguous()


@pytest.mark.parametrize("name", cg.NAMES)
def test_zero_residual_and_independence_of_the_other_samples(cuda, name):
    lib, d = _hip.load_library(), _dev(name, cuda)
    rho = 1.0
    xd, yd = _mixed_batch(d, cuda)
    z, it = run_prox(lib, d, xd, yd, 1, rho, 64, 1e-6)
    print(name, "iters", it.tolist())
    assert bool(torch.isfinite(z).all())
    assert int(it[1]) == 0 and torch.equal(z[1], xd[1])  # bit for bit, no NaN
    assert int(it[0]) >= 1 and int(it[3]) >= 1
    z2, it2 = run_prox(lib, d, xd, yd, 1, rho, 64, 1e-6)  # the same call twice
    assert torch.equal(z2, z) and torch.equal(it2, it)
    for b in range(4):  # a sample alone
        za, ia = run_prox(lib, d, xd[b:b + 1].contiguous(), yd[b:b + 1].contiguous(), 1, rho, 64, 1e-6)
        assert torch.equal(za, z[b:b + 1]) and int(ia[0]) == int(it[b]), b
    # iters_out may be NULL; z_out may alias x0
    assert torch.equal(run_prox(lib, d, xd, yd, 1, rho, 64, 1e-6, iters=False)[0], z)
    assert torch.equal(run_prox(lib, d, xd, yd, 1, rho, 64, 1e-6, alias=True)[0], z)
    # the step form on the same observations: the zero-residual sample differs (its x0 does)
    eps = d.c.eps.to(cuda).contiguous()
    out, its = run_step(lib, d, xd, eps, yd, None, 1, rho, 64, 1e-6)
    for b in (0, 2):
        oa, ia = run_step(lib, d, xd[b:b + 1].contiguous(), eps[b:b + 1].contiguous(),
                          yd[b:b + 1].contiguous(), None, 1, rho, 64, 1e-6, offset=OFFSET + b)
        assert torch.equal(oa, out[b:b + 1]) and int(ia[0]) == int(its[b]), b


@pytest.mark.parametrize("name", cg.NAMES)
def test_y_div_aliasing_and_philox(cuda, name):
    lib, d = _hip.load_library(), _dev(name, cuda)
    rho, K, tol = _f32(0.37), 5, 1e-4
    xd, ed, yd = _to(cuda, d.c.x, d.c.eps, d.c.y)
    rows = yd.repeat_interleave(2, dim=0).contiguous()
    z, it = run_prox(lib, d, xd, yd, 2, rho, K, tol)
    zr, itr = run_prox(lib, d, xd, rows, 1, rho, K, tol)  # y_div = 2 against repeated rows
    assert torch.equal(z, zr) and torch.equal(it, itr)
    xi = torch.empty(4, d.n, device=cuda)
    _hip.check(lib.sp_randn(xi.data_ptr(), 4, d.n, SEED, STEP, OFFSET, _stream()), "sp_randn")
    given, itg = run_step(lib, d, xd, ed, yd, xi, 2, rho, K, tol)
    drawn, itd = run_step(lib, d, xd, ed, yd, None, 2, rho, K, tol)  # xi = NULL: the bits of sp_randn
    assert torch.equal(drawn, given) and torch.equal(itd, itg)
    assert torch.equal(run_step(lib, d, xd, ed, rows, None, 1, rho, K, tol)[0], drawn)
    assert torch.equal(run_step(lib, d, xd, ed, yd, None, 2, rho, K, tol, alias=True)[0], drawn)
    other, _ = run_step(lib, d, xd, ed, yd, None, 2, rho, K, tol, offset=OFFSET + 1)
    assert not torch.equal(other, drawn)


# --- 5. against the closed forms ----------------------------------------------------------------------
def _closed_form(lib, d, x0, y, ydiv, rho):
    rows, batch = y.shape[0], x0.shape[0]
    qsize, floats = int(lib.sp_prox_prepare_size(d.desc, rows)), int(lib.sp_prox_workspace(d.desc, batch))
    assert qsize >= 0 and floats >= 0
    q = torch.empty(max(qsize, 1), device=x0.device) if qsize else None
    work = torch.empty(floats, device=x0.device) if floats else None
    _hip.check(lib.sp_prox_prepare(d.desc, y.data_ptr(), rows, q.data_ptr() if qsize else None,
                                   _stream()), "sp_prox_prepare")
    out = torch.empty_like(x0)
    _hip.check(lib.sp_op_prox_ws(d.desc, x0.data_ptr(), y.data_ptr(), q.data_ptr() if qsize else None,
                                 batch, ydiv, rho, out.data_ptr(), work.data_ptr() if floats else None,
                                 _stream()), "sp_op_prox_ws")
    return out


@pytest.mark.parametrize("name,rho", [(n, r) for n in cg.CLOSED_FORM for r in _rhos(n)])
def test_against_the_closed_forms(cuda, parity_record, name, rho):
    lib, d = _hip.load_library(), _dev(name, cuda)
    c, rho = d.c, _f32(rho)
    for batch, ydiv in cg.BATCHES:
        _, yard, _ = _converged_reference(c, batch, ydiv, rho)
        xd, yd = _to(cuda, c.x[:batch], c.y[:batch // ydiv])
        z, _ = run_prox(lib, d, xd, yd, ydiv, rho, 64, 1e-6)
        closed = _closed_form(lib, d, xd, yd, ydiv, rho)
        bound, err = max(2e-5, 4 * yard), cg.distance(z.cpu(), closed.cpu())
        print(f"{name} rho={rho:g} b{batch}: cg to closed form {err:.3g} bound {bound:.3g}")
        parity_record("cg_to_closed_form_max_err_over_max", err, bound, rho=rho)
        assert err <= bound, (name, rho, err, bound)


# --- 6. Python --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cg.NAMES)
def test_device_apply_prox_cg_matches_the_host(cuda, parity_record, name):
    d = _dev(name, cuda)
    c, host = d.c, cg.case(name).op
    x0 = c.x.reshape(2, 2, *host.x_shape)  # two leading batch dimensions
    y = c.y.repeat_interleave(2, dim=0).reshape(2, 2, *host.y_shape)
    for rho in (1.0, 50.0):
        got, it = d.op.apply_prox_cg(x0.to(cuda), y.to(cuda), rho, iterations=64, return_iterations=True)
        assert got.shape == x0.shape and got.is_cuda and got.dtype == torch.float32
        assert it.shape == (2, 2) and it.dtype == torch.int32 and it.is_cuda
        ref, yard, _ = _converged_reference(c, 4, 2, _f32(rho))
        want, wit = host.apply_prox_cg(x0, y, rho, iterations=64, return_iterations=True)
        bound = max(2e-5, 4 * yard)
        err = cg.distance(got.cpu().reshape(4, -1), ref)
        host_err = cg.distance(want.reshape(4, -1), ref)
        print(f"{name} rho={rho:g}: device {err:.3g} host {host_err:.3g} bound {bound:.3g} "
              f"iters {it.flatten().tolist()} host {wit.flatten().tolist()}")
        parity_record("apply_prox_cg_max_err_over_max", err, bound, rho=rho, host=host_err)
        assert err <= bound and host_err <= bound
        assert int(it.max()) < 64 and int(wit.max()) < 64
    assert torch.equal(d.op.apply_prox_cg(x0[0, 0].to(cuda), y[0, 0].to(cuda), 1.0, iterations=64),
                       d.op.apply_prox_cg(x0.to(cuda), y.to(cuda), 1.0, iterations=64)[0, 0])


B, N, SIGMA, CG_K = 2, 8, 0.05, 6


def _traj_problem(name, cuda):
    """(device problem, host operator, y, shape) of a trajectory case."""
    if name == "blur":
        shape, make = (3, 32, 32), lambda: GaussianBlurOperator((3, 32, 32), 9, 3.0)
    elif name == "radon":
        shape, make = (1, 32, 32), lambda: RadonOperator((1, 32, 32), num_angles=8)
    elif name == "inpaint":
        shape, make = (3, 32, 32), lambda: RandomInpaintingOperator((3, 32, 32), 0.5, seed=3)
    else:
        shape, make = (3, 32, 32), lambda: SuperResolutionOperator((3, 32, 32), 4)
    host = make()
    g = torch.Generator().manual_seed(41)
    y = host.apply(si.fixture_x_true(B, shape, seed=9).double()).float()
    y = y + SIGMA * torch.randn(y.shape, generator=g)
    prob = InverseProblem(make().to(cuda), y.to(cuda), GaussianNoise(SIGMA).to(cuda))
    return prob, host, y, shape


def _reference(dt, host, y, shape, init, steps):
    core = si.EpsCore("conv", shape[0], 0.1).to(dt)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).to(dt)
    prox = lambda x0, yy, rho: host.apply_prox_cg(x0, yy, float(rho), iterations=CG_K, tol=1e-4)  # noqa: E731
    return pr.diffpir_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                                host.apply, prox, y.to(dt), init.to(dt), lambda i: steps[i].to(dt),
                                sigma=SIGMA)


@pytest.mark.parametrize("name", ["blur", "radon", "inpaint"])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, name):
    from samplers_amd.samplers import DiffPIRSampler

    prob, host, y, shape = _traj_problem(name, cuda)
    net = si.make_samplers_amd_net("conv", shape[0], 0.1, device=cuda)
    grads, inner = [], net.forward

    def forward(x, t):
        e = inner(x, t)
        grads.append(bool(e.requires_grad) or torch.is_grad_enabled())
        return e

    net.forward = forward
    init, steps = si.replay_noise(17, (B, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    sampler = DiffPIRSampler(net)
    out = sampler(prob, num_sampling_steps=N, noise_fn=fn, prox="cg", cg_iterations=CG_K)
    assert tuple(out.shape) == (B, *shape) and bool(torch.isfinite(out).all())
    assert len(grads) >= 2 and not any(grads)  # every network call ran under no_grad: no graph
    its = sampler.last_step.iterations  # kept on the device, one row per step
    assert its.is_cuda and its.dtype == torch.int32 and tuple(its.shape) == (len(steps), B)
    assert int(its.min()) >= 1 and int(its.max()) <= CG_K
    ref32 = _reference(torch.float32, host, y, shape, init, steps)
    cond = si.relative_error(_reference(torch.float64, host, y, shape, init, steps), ref32)
    bound = max(1e-4, 20 * cond)
    err = si.relative_error(out.cpu(), ref32)
    print(f"diffpir cg {name}: rel l2 {err:.3g}, fp32 reference to fp64 {cond:.3g}, bound {bound:.3g}, "
          f"iterations {its.tolist()}")
    parity_record("diffpir_cg_rel_l2", err, bound, fp32_to_fp64=cond)
    assert err < bound
    if name == "inpaint":  # the closed form at the same noise: CG is exact after one iteration
        closed = DiffPIRSampler(net)(prob, num_sampling_steps=N, noise_fn=fn, prox="closed_form")
        gap = si.relative_error(out, closed)
        parity_record("diffpir_cg_to_closed_form_rel_l2", gap, 1e-4)
        assert gap < 1e-4


def test_auto_picks_the_closed_form_where_there_is_one(cuda):
    from samplers_amd.samplers import DiffPIRSampler, FusedDiffPIRStep

    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    prob, *_ = _traj_problem("sr", cuda)
    step = FusedDiffPIRStep(net, prob, prob.observation.float(), 1, prox="auto")
    assert not step.cg
    assert FusedDiffPIRStep(net, prob, prob.observation.float(), 1, prox="cg").cg
    auto = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=5, prox="auto")
    assert torch.equal(auto, DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=5))
    net1 = si.make_samplers_amd_net("conv", 1, 0.1, device=cuda)
    prob, *_ = _traj_problem("radon", cuda)
    assert FusedDiffPIRStep(net1, prob, prob.observation.float(), 1, prox="auto").cg
    with pytest.raises(NotImplementedError, match="RadonOperator"):
        DiffPIRSampler(net1)(prob, num_sampling_steps=N, seed=5)
    s = DiffPIRSampler(net1)
    out = s(prob, num_sampling_steps=N, seed=5, prox="auto")
    assert bool(torch.isfinite(out).all()) and s.last_step.cg


def test_philox_trajectory_is_reproducible(cuda):
    from samplers_amd.samplers import DiffPIRSampler

    prob, *_ = _traj_problem("blur", cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    kw = dict(num_sampling_steps=N, prox="cg", cg_iterations=CG_K)
    one = DiffPIRSampler(net)(prob, seed=1234, **kw)
    assert torch.equal(DiffPIRSampler(net)(prob, seed=1234, **kw), one) and bool(torch.isfinite(one).all())
    assert not torch.equal(DiffPIRSampler(net)(prob, seed=1235, **kw), one)
    assert torch.equal(DiffPIRSampler(net)(prob, seed=1234, micro_batch=1, **kw), one)  # any chunking


# --- 7. the bounds-checked library -------------------------------------------------------------------
def debug_sweep(device):
    """Every case through sp_op_prox_cg_ws and both noise forms of sp_diffpir_step_cg_ws, with
    live and stopped samples in one batch; run by the child process under the debug library."""
    lib = _hip.load_library()
    for name in cg.NAMES:
        d = _dev(name, device)
        for batch, ydiv in cg.BATCHES:
            xd, ed, yd = _to(device, d.c.x[:batch], d.c.eps[:batch], d.c.y[:batch // ydiv])
            xi = torch.randn(batch, d.n, device=device)
            outs = [run_prox(lib, d, xd, yd, ydiv, 1.0, 12, 1e-3)[0],
                    run_step(lib, d, xd, ed, yd, None, ydiv, 1.0, 12, 1e-3)[0],
                    run_step(lib, d, xd, ed, yd, xi, ydiv, 1.0, 3, 0.0)[0]]
            assert all(torch.isfinite(t).all() for t in outs)
        xm, ym = _mixed_batch(d, device)
        assert torch.isfinite(run_prox(lib, d, xm, ym, 1, 1.0, 12, 1e-3)[0]).all()
        nv, site = _hip.debug_violations()
        print(name, "violations", nv, site, flush=True)
        assert nv == 0, (name, nv, site)


DEBUG_CHILD = DEBUG_SWEEP_CHILD("test_prox_cg_gpu")


def test_debug_build_has_no_violations(cuda):
    """The new kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library), over every shape of this file."""
    run_debug_child(DEBUG_CHILD)
