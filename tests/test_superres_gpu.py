"""×s super-resolution (SP_OP_SR, csrc/sp_sr.hip) on the GPU: the operator's maps, every fused
entry point against the fp64 semantics of tests/sr_ops.py, and the four samplers against the
oracle loops.

Bounds are the ones the other native operators are held to: 2e-5 x max|reference| per element
and 2e-5 relative on the residual norms for the fused passes (test_hip_kernels.py), 1e-4
relative L2 for the DPS / PSLD trajectories, max(1e-4, 20 x the oracle's own fp32-vs-fp64
distance) for PGDM (test_latent_gpu.py), 1e-5 for graph replay (test_graph_gpu.py)."""

import math
import types

import numpy as np
import pytest
import torch

import sr_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import closed_form, dps_loop
from oracle.latent_loops import pgdm_reference, psld_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise, PoissonNoise
from samplers_amd.operators import SuperResolutionOperator
from samplers_amd.samplers import DPSSampler

pytestmark = pytest.mark.gpu


# shape, factor, batch, y_div
CASES = [
    ((3, 32, 32), 2, 4, 1), ((3, 32, 32), 4, 4, 1), ((3, 32, 32), 8, 4, 1),  # vector path
    ((1, 8, 12), 2, 2, 2), ((1, 8, 12), 4, 2, 2),  # three float4 per row, tiles straddling rows
    ((2, 6, 10), 2, 2, 1),                         # scalar fallback (W % 4 != 0)
    ((3, 40, 72), 8, 6, 3),                        # lane pairs, non-power-of-two rows
    ((1, 8, 8), 8, 2, 1),                          # m = C
    ((1, 2, 2), 2, 1, 1),                          # a single block
    ((3, 64, 128), 4, 2, 1),                       # more than one tile: fixed-order partial sum
]
IDS = [f"{'x'.join(map(str, c[0]))}-s{c[1]}-b{c[2]}-d{c[3]}" for c in CASES]


def _replicate(y, s):
    return y.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1)


@pytest.mark.parametrize("shape,s,batch,ydiv", CASES, ids=IDS)
def test_apply_adjoint_pinv_and_backward(cuda, shape, s, batch, ydiv):
    op = SuperResolutionOperator(shape, s).to(cuda)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(batch, *shape, generator=g)
    y = torch.randn(batch, *op.y_shape, generator=g)
    got = op.apply(x.to(cuda)).cpu()
    assert tuple(got.shape) == (batch, *op.y_shape)
    np.testing.assert_allclose(got.double().numpy(), sr_ops.apply64(x, s).numpy(), rtol=0, atol=2e-5)
    yd = y.to(cuda)
    assert torch.equal(op.apply_transpose(yd).cpu(), _replicate(y, s) / (s * s))
    assert torch.equal(op.apply_pseudo_inverse(yd).cpu(), _replicate(y, s))
    # HipLinearMap: the backward of A is A^T of the cotangent (and of A^T, A)
    xr = x.to(cuda).requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=yd)
    assert torch.equal(gx, op.apply_transpose(yd))
    yr = yd.clone().requires_grad_()
    (gy,) = torch.autograd.grad(op.apply_transpose(yr), yr, grad_outputs=x.to(cuda))
    assert torch.equal(gy, op.apply(x.to(cuda)))


def _dps_passes(cuda, shape, s, batch, ydiv, coefs_tail, seed, record=None):
    """Both DPS passes against oracle.closed_form, with the constants and bounds of
    test_hip_kernels.py::test_fused_dps_passes_match_closed_form."""
    op = SuperResolutionOperator(shape, s).to(cuda)
    apply_np, adjoint_np = sr_ops.sr_ops(shape, s)
    lib = _hip.load_library()
    desc = op.hip_descriptor()
    n, m = math.prod(shape), int(desc.m)
    g = torch.Generator().manual_seed(seed)
    x, eps, w, xi = (torch.randn(batch, n, generator=g) for _ in range(4))
    y = torch.randn(batch // ydiv, m, generator=g)
    a, k, gs = 0.3, math.sqrt(1 - 0.09), 400.0
    c_ell, c_s, std, gamma = coefs_tail
    coefs = _hip.SpDpsCoefs(a, k, gs, c_ell, c_s, std, gamma, 1e-9)
    P = int(lib.sp_rsq_partials(desc))
    assert P > 0
    xd, ed, yd, wd, xid = (t.to(cuda).contiguous() for t in (x, eps, y, w, xi))
    v = torch.full_like(xd, float("nan"))
    part = torch.full((batch, P), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
                                   coefs, v.data_ptr(), part.data_ptr(), _stream()), "residual")
    v_ref, rsq_ref = closed_form.residual_pass(x.numpy(), eps.numpy(), y.numpy(), ydiv, a, k, gs,
                                               apply_np, adjoint_np)
    out_ref = closed_form.update_pass(x.numpy(), eps.numpy(), v_ref, w.numpy(), rsq_ref, xi.numpy(),
                                      a, k, c_ell, c_s, std, gamma)
    out = torch.empty_like(xd)
    _hip.check(lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(),
                                 wd.data_ptr(), part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch,
                                 ydiv, coefs, out.data_ptr(), _stream()), "update")
    v_err = float(np.abs(v.cpu().numpy() - v_ref).max() / np.abs(v_ref).max())
    rsq_err = float(np.abs(part.sum(1).cpu().numpy() / rsq_ref - 1).max())
    out_err = float(np.abs(out.cpu().numpy() - out_ref).max() / np.abs(out_ref).max())
    print(f"sr passes {shape} s={s}: v {v_err:.3g} rsq {rsq_err:.3g} x' {out_err:.3g} P={P}")
    if record is not None:
        record("pass1_v_max_err_over_max", v_err, 2e-5)
        record("pass1_rsq_max_rel_err", rsq_err, 2e-5)
        record("pass2_x_max_err_over_max", out_err, 2e-5)
    np.testing.assert_allclose(v.cpu().numpy(), v_ref, rtol=0, atol=2e-5 * np.abs(v_ref).max())
    np.testing.assert_allclose(part.sum(1).cpu().numpy(), rsq_ref, rtol=2e-5)
    np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=0, atol=2e-5 * np.abs(out_ref).max())
    # SR requires v in pass 2, as BLUR does
    assert lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), None, wd.data_ptr(),
                             part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch, ydiv, coefs,
                             out.data_ptr(), _stream()) == -1
    return P


@pytest.mark.parametrize("shape,s,batch,ydiv", CASES, ids=IDS)
def test_fused_dps_passes_match_closed_form(cuda, shape, s, batch, ydiv):
    P = _dps_passes(cuda, shape, s, batch, ydiv, (0.9, 0.2, 0.1, 0.05), seed=0)
    if shape == (3, 64, 128):
        assert P > 1


def test_dps_passes_full_size(cuda, parity_record):
    _dps_passes(cuda, (3, 256, 256), 4, 4, 2, (0.97, 0.11, 0.05, 1.0), seed=7, record=parity_record)


@pytest.mark.parametrize("shape,s,batch,ydiv", CASES, ids=IDS)
def test_latent_sampler_passes_match_fp64(cuda, shape, s, batch, ydiv):
    """sp_psld_pixel, sp_psld_cotangent (ata_u = NULL) and sp_pixel_opt_step against fp64 torch
    on the helper's maps, at the fused passes' bounds (2e-5 x max|reference|, 2e-5 relative on
    the residual norms); a set stop flag leaves sp_pixel_opt_step's buffers untouched."""
    from samplers_amd.samplers.resample import adamw_coefficients

    op = SuperResolutionOperator(shape, s).to(cuda)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    n, m = math.prod(shape), int(desc.m)
    P = int(lib.sp_rsq_partials(desc))
    g = torch.Generator().manual_seed(11)
    x0, u = (torch.randn(batch, *shape, generator=g) for _ in range(2))
    y = torch.randn(batch // ydiv, *op.y_shape, generator=g)
    rows = torch.arange(batch) // ydiv
    r = y.double()[rows] - sr_ops.apply64(x0, s)
    atr_ref = sr_ops.adjoint64(r, s)
    x_eff_ref = x0.double() + atr_ref
    rsq_ref = r.reshape(batch, -1).square().sum(1)

    def close(got, ref):
        ref = ref.reshape(got.shape).numpy()
        np.testing.assert_allclose(got.cpu().double().numpy(), ref, rtol=0,
                                   atol=2e-5 * np.abs(ref).max())

    x0d, ud, yd = (t.to(cuda).reshape(t.shape[0], -1).contiguous() for t in (x0, u, y))
    x_eff, atr = torch.empty_like(x0d), torch.empty_like(x0d)
    part = torch.full((batch, P), float("nan"), device=cuda)
    _hip.check(lib.sp_psld_pixel(desc, x0d.data_ptr(), yd.data_ptr(), batch, ydiv, x_eff.data_ptr(),
                                 atr.data_ptr(), part.data_ptr(), _stream()), "sp_psld_pixel")
    close(atr, atr_ref)
    close(x_eff, x_eff_ref)
    np.testing.assert_allclose(part.sum(1).cpu().double().numpy(), rsq_ref.numpy(), rtol=2e-5)

    omega = 0.1
    norm_sq = rsq_ref.sum().float().reshape(1).to(cuda)
    out = torch.empty_like(x0d)
    _hip.check(lib.sp_psld_cotangent(desc, atr.data_ptr(), ud.data_ptr(), None, norm_sq.data_ptr(),
                                     omega, batch, out.data_ptr(), _stream()), "sp_psld_cotangent")
    ata_u = sr_ops.adjoint64(sr_ops.apply64(u, s), s)
    close(out, -omega * atr_ref / rsq_ref.sum().sqrt() + (u.double() - ata_u))

    total = batch * m
    gs = float(np.float32(-2.0 / total))
    c = adamw_coefficients(1, 1e-2)
    xd, md, vd = x0d.clone(), torch.zeros_like(x0d), torch.zeros_like(x0d)
    stop = torch.ones(1, dtype=torch.int32, device=cuda)
    part.fill_(float("nan"))
    _hip.check(lib.sp_pixel_opt_step(desc, xd.data_ptr(), md.data_ptr(), vd.data_ptr(), yd.data_ptr(),
                                     batch, ydiv, gs, c, stop.data_ptr(), part.data_ptr(), _stream()),
               "sp_pixel_opt_step")
    assert torch.equal(xd, x0d) and not md.any() and not vd.any() and part.isnan().all()
    stop.zero_()
    _hip.check(lib.sp_pixel_opt_step(desc, xd.data_ptr(), md.data_ptr(), vd.data_ptr(), yd.data_ptr(),
                                     batch, ydiv, gs, c, stop.data_ptr(), part.data_ptr(), _stream()),
               "sp_pixel_opt_step")
    grad = gs * atr_ref  # A^T(gs r)
    m_ref = (1 - c.beta1) * grad
    v_ref = (1 - c.beta2) * grad * grad
    p_ref = x0.double() * c.decay - c.step_size * m_ref / (v_ref.sqrt() / c.bc2_sqrt + c.eps)
    close(md, m_ref)
    close(vd, v_ref)
    close(xd, p_ref)
    np.testing.assert_allclose(part.sum(1).cpu().double().numpy(), rsq_ref.numpy(), rtol=2e-5)


def _sr_problem(shape, s, b, seed, noise, dev):
    op = SuperResolutionOperator(shape, s)
    x_true = si.fixture_x_true(b, shape, seed)
    y = op.apply(x_true)
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return op, y, InverseProblem(op.to(dev), y.to(dev), noise.to(dev))


def test_dps_philox_sharding_and_micro_batch_are_invariant(cuda):
    shape, s, b = (3, 32, 32), 4, 4
    _, _, prob = _sr_problem(shape, s, b, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    kw = dict(num_sampling_steps=8, gamma=1e-2, eta=1.0, rng="philox", seed=11)
    full = DPSSampler(net)(prob, **kw)
    assert torch.isfinite(full).all()
    shards = []
    for b0 in (0, 2):
        p = InverseProblem(prob.operator, prob.observation[b0:b0 + 2], prob.noise)
        shards.append(DPSSampler(net)(p, sample_offset=b0, **kw))
    assert torch.equal(full, torch.cat(shards))
    assert torch.equal(full, DPSSampler(net)(prob, micro_batch=1, **kw))


@pytest.mark.parametrize("noise_kind", ["gauss", "poisson"])
def test_dps_matches_oracle(cuda, noise_kind):
    shape, s, b, N = (3, 32, 32), 4, 2, 8
    noise = GaussianNoise(0.05) if noise_kind == "gauss" else PoissonNoise(1.0)
    _, y, prob = _sr_problem(shape, s, b, 0, noise, cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", 3, 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    lp = dps_loop.gaussian_log_prob(0.05) if noise_kind == "gauss" else dps_loop.poisson_log_prob(1.0)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 lambda x: sr_ops.pool(x, s), lp, y, init, lambda i: steps[i],
                                 gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps sr", noise_kind, err)
    assert err < 1e-4


def test_pgdm_matches_oracle_fused_and_generic(cuda, monkeypatch):
    """The test of the -2 s^2 factor: the fused step (pinv_grad_scale) against the oracle loop,
    which differentiates ||A+ y - A+ A x0||^2 with A+ = replicate, and against GenericDPSStep,
    which differentiates through the operator's own apply_pseudo_inverse."""
    from samplers_amd.samplers import pgdm as pgdm_mod
    from samplers_amd.samplers.dps import FusedDPSStep, GenericDPSStep
    from samplers_amd.samplers.pgdm import PGDMSampler

    shape, s, b, N = (3, 32, 32), 4, 2, 8
    _, y, prob = _sr_problem(shape, s, b, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    init, steps = si.replay_noise(5, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    made = []
    real = pgdm_mod.make_dps_step
    monkeypatch.setattr(pgdm_mod, "make_dps_step",
                        lambda *a, **kw: made.append(real(*a, **kw)) or made[-1])
    out = PGDMSampler(net)(prob, num_sampling_steps=N, guidance_weight=0.05, noise_fn=fn)
    assert type(made[-1]) is FusedDPSStep and made[-1].grad_scale == -2.0 * s * s
    monkeypatch.setattr(pgdm_mod, "make_dps_step", lambda *a, **kw: GenericDPSStep(*a, **kw))
    generic = PGDMSampler(net)(prob, num_sampling_steps=N, guidance_weight=0.05, noise_fn=fn)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)

    def run(dt):
        c = si.EpsCore("conv", 3, 0.1).to(dt)
        return pgdm_reference(lambda x, t: c(x, t), acp.to(dt),
                              si.leading_timesteps_ascending(N).tolist(),
                              lambda x: sr_ops.pool(x, s), lambda v: sr_ops.replicate(v, s),
                              y.to(dt), init.to(dt), lambda i: steps[i].to(dt),
                              guidance_weight=0.05, eta=1.0)

    ref = run(torch.float32)
    cond = si.relative_error(run(torch.float64), ref)
    bound = max(1e-4, 20 * cond)
    err, err_generic = si.relative_error(out.cpu(), ref), si.relative_error(generic.cpu(), out.cpu())
    print("pgdm sr", err, err_generic, "bound", bound)
    assert err < bound
    assert err_generic < bound


def test_psld_matches_oracle(cuda):
    from samplers_amd.samplers.psld import PSLDSampler

    shape, s, b, N = (3, 32, 32), 4, 2, 6
    _, y, prob = _sr_problem(shape, s, b, 4, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    lat = net.get_latent_shape(shape)
    init, steps = si.replay_noise(13, (b, *lat), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = PSLDSampler(net)(prob, num_sampling_steps=N, noise_fn=fn)
    core, vae = si.EpsCore("conv", 4, 0.1), si.LatentCore()
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    ref = psld_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                         lambda x: sr_ops.pool(x, s), lambda v: sr_ops.adjoint_closed(v, s),
                         vae.decode, vae.encode, y, init, lambda i: steps[i])
    err = si.relative_error(out.cpu(), ref)
    print("psld sr", err)
    assert err < 1e-4


@pytest.mark.parametrize("s", [2, 4])
def test_pixel_optimization_device_stop_matches_reference_loop(cuda, s):
    """test_latent_gpu.py's test of the same name for SR (the fused sp_pixel_opt_step): the
    device stopping rule runs exactly the iterations of the torch AdamW + MSELoss loop."""
    from samplers_amd.samplers.resample import ReSampleSampler, _Consistency, _finish_log

    torch.manual_seed(0)
    shape, b = (3, 16, 24), 2
    op = SuperResolutionOperator(shape, s).to(cuda)
    x_true = torch.rand(b, *shape) * 2 - 1
    x0 = torch.randn(b, *shape)
    y = op.apply(x_true.to(cuda)).reshape(b, -1).cpu()
    total = y.numel()

    def reference(n_iter, thr=None):
        opt = x0.clone().requires_grad_()
        adam = torch.optim.AdamW([opt], lr=1e-2)
        losses = []
        for _ in range(n_iter):
            adam.zero_grad()
            loss = torch.nn.MSELoss()(y, op.apply(opt.to(cuda)).reshape(b, -1).cpu())
            loss.backward()
            adam.step()
            losses.append(loss.item())
            if thr is not None and loss.item() < thr:
                break
        return opt.detach(), losses

    _, losses = reference(40)
    stop_at = 22  # 0-based iteration whose loss first falls below the threshold
    assert losses[stop_at] < losses[stop_at - 1]
    thr = 0.5 * (losses[stop_at] + losses[stop_at - 1])
    assert all(v >= thr for v in losses[:stop_at])
    ref, ref_losses = reference(2000, thr)
    assert len(ref_losses) == stop_at + 1
    cons = _Consistency(op, y.to(cuda), 1)
    assert int(cons.desc.kind) == _hip.SP_OP_SR
    holder = types.SimpleNamespace()
    out = ReSampleSampler._pixel_optimization(holder, x0.to(cuda), cons, total, thr ** 0.5, 2000)
    err = float((out.cpu() - ref).norm() / ref.norm())
    _finish_log(holder)
    (rec,) = holder.optimization_log
    assert rec["kind"] == "pixel" and rec["iterations"] == stop_at + 1 and rec["stopped_early"]
    assert abs(rec["final_loss"] - ref_losses[-1]) <= 1e-5 * abs(ref_losses[-1])
    one_more, _ = reference(stop_at + 2)
    assert err < 1e-5, err
    assert float((one_more - ref).norm() / ref.norm()) > 100 * max(err, 1e-7)


def test_graph_replay_matches_eager(cuda):
    """test_graph_gpu.py::test_graph_replay_matches_eager for SR at s = 4 (its small UNet)."""
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.networks.unet2d import UNet2DConfig

    cfg = UNet2DConfig(sample_size=32, block_out_channels=(64, 128), attention_levels=(1,),
                       layers_per_block=1)
    shape, b = (3, 32, 32), 2
    op = SuperResolutionOperator(shape, 4).to(cuda)
    gen = torch.Generator().manual_seed(5)
    x_true = (torch.rand((b, *shape), generator=gen) * 2 - 1).to(cuda)
    y = op.apply(x_true)
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=gen).to(cuda)
    prob = InverseProblem(op, y, GaussianNoise(0.05).to(cuda))
    net = DDPMNetwork.from_config(cfg, seed=0, device=cuda)
    eager = DPSSampler(net)(prob, num_sampling_steps=8, gamma=0.5, seed=1234)
    again = DPSSampler(net)(prob, num_sampling_steps=8, gamma=0.5, seed=1234)
    graphed = DPSSampler(net)(prob, num_sampling_steps=8, gamma=0.5, seed=1234, graph=True)
    assert torch.isfinite(eager).all()
    base = ((again - eager).norm() / eager.norm()).item()
    rel = ((graphed - eager).norm() / eager.norm()).item()
    assert base < 1e-5 and rel < 1e-5, (base, rel)


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
from samplers_amd.operators import SuperResolutionOperator
from samplers_amd.samplers.resample import adamw_coefficients
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
for shape, s in (((3, 40, 72), 8), ((2, 6, 10), 2)):
    op = SuperResolutionOperator(shape, s).to(dev)
    desc = op.hip_descriptor()
    b, n, m = 3, int(desc.n), int(desc.m)
    P = int(lib.sp_rsq_partials(desc))
    x, eps, w, u = (torch.randn(b, n, device=dev) for _ in range(4))
    y = torch.randn(b, m, device=dev)
    ax, aty = torch.empty(b, m, device=dev), torch.empty(b, n, device=dev)
    _hip.check(lib.sp_op_apply(desc, x.data_ptr(), ax.data_ptr(), b, st), "sp_op_apply")
    _hip.check(lib.sp_op_adjoint(desc, y.data_ptr(), aty.data_ptr(), b, st), "sp_op_adjoint")
    c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    v, part, out = torch.empty_like(x), torch.empty(b, P, device=dev), torch.empty_like(x)
    _hip.check(lib.sp_dps_residual(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 1, c,
                                   v.data_ptr(), part.data_ptr(), st), "sp_dps_residual")
    _hip.check(lib.sp_dps_update(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v.data_ptr(),
                                 w.data_ptr(), part.data_ptr(), None, 7, 3, 0, b, 1, c,
                                 out.data_ptr(), st), "sp_dps_update")
    x_eff, atr = torch.empty_like(x), torch.empty_like(x)
    _hip.check(lib.sp_psld_pixel(desc, x.data_ptr(), y.data_ptr(), b, 1, x_eff.data_ptr(),
                                 atr.data_ptr(), part.data_ptr(), st), "sp_psld_pixel")
    norm = torch.ones(1, device=dev)
    _hip.check(lib.sp_psld_cotangent(desc, atr.data_ptr(), u.data_ptr(), None, norm.data_ptr(), 0.1,
                                     b, out.data_ptr(), st), "sp_psld_cotangent")
    mm, vv = torch.zeros_like(x), torch.zeros_like(x)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    _hip.check(lib.sp_pixel_opt_step(desc, x.data_ptr(), mm.data_ptr(), vv.data_ptr(), y.data_ptr(),
                                     b, 1, -2.0 / (b * m), adamw_coefficients(1, 1e-2),
                                     stop.data_ptr(), part.data_ptr(), st), "sp_pixel_opt_step")
    nv, site = _hip.debug_violations()
    print(shape, s, "violations", nv, site, flush=True)
    assert nv == 0, (shape, s, nv, site)
    assert torch.isfinite(out).all() and torch.isfinite(x).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The SR kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library), on the lane-pair and the scalar path."""
    run_debug_child(DEBUG_CHILD)
