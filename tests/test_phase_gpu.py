"""Fourier phase retrieval (SP_OP_PHASE, csrc/sp_phase.hip) on the GPU: the operator's forward map,
its autograd backward and the fused DPS passes against the fp64 semantics of tests/phase_ops.py,
and the samplers against the oracle loop.

Bounds are the native-operator family's (test_psf_gpu.py / test_hip_kernels.py): 2e-5 x
max|reference| per element and 2e-5 relative on the residual norms for the maps and the fused
passes, 1e-4 relative L2 for the DPS trajectories, 1e-5 for graph replay.  The same arithmetic in
fp32 torch on the CPU is within 3.2e-7 x max|v| and 2.8e-7 relative on ||r||^2 of fp64 at all the
shapes below (the smallest |z| down to 2.6e-4 of the largest), so 2e-5 leaves > 60x headroom.

Largest errors measured on an MI355X over CASES (parity_record has every figure): apply 1.9e-7,
backward 3.8e-7, pass-1 v 3.4e-7, ||r||^2 2.6e-7 relative, pass-2 x' 5.9e-7 (all x max|ref|),
DPS trajectories 6.3e-7 relative L2 — at the CPU fp32 figure, well below the 2e-6 that would
point at imprecise twiddles."""

import math

import numpy as np
import pytest
import torch

import phase_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import closed_form, dps_loop
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise, PoissonNoise
from samplers_amd.operators import PhaseRetrievalOperator
from samplers_amd.samplers import DPSSampler
from samplers_amd.samplers.dps import FusedDPSStep, GenericDPSStep, make_dps_step

pytestmark = pytest.mark.gpu


# shape, (pad_h, pad_w), batch, y_div
CASES = [
    ((1, 2, 2), (3, 3), 1, 1),          # 8 x 8: the smallest transform
    ((1, 8, 8), (0, 0), 2, 1),          # no padding
    ((2, 6, 10), (1, 3), 2, 1),         # 8 x 16: W % 4 != 0, odd and unequal pads
    ((1, 12, 20), (6, 2), 2, 2),        # 24 x 24: the radix-3 pass on both axes
    ((3, 16, 16), (8, 8), 4, 1),        # 32 x 32
    ((3, 64, 64), (16, 16), 6, 3),      # 96 x 96: the paper's H/4 geometry, 3 * 2^k
    ((1, 96, 160), (16, 48), 1, 1),     # 128 x 256: several column tiles, rectangular
    ((1, 256, 256), (64, 64), 1, 1),    # 384 x 384: the paper's size
    ((1, 512, 512), (256, 256), 1, 1),  # 1024 x 1024: the largest
]
IDS = [f"{'x'.join(map(str, c[0]))}-p{c[1][0]}x{c[1][1]}-b{c[2]}-d{c[3]}" for c in CASES]


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64).reshape(tuple(got.shape))
    return float(np.abs(got.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())


def _close(got, ref, what, record=None):
    err = _err(got, ref)
    print(f"{what}: max err / max|ref| = {err:.3g}")
    if record is not None:
        record(what, err, 2e-5)
    assert err <= 2e-5, (what, err)


_INPUTS = {}


def _inputs(shape, pad, batch, ydiv):
    """x, eps, w, xi ~ randn (batch, n); y = the amplitude of another random image + 0.05 randn
    (asymmetric: independent noise in both Hermitian halves), (batch / ydiv, m).  Computed once
    per case and shared; never modified."""
    key = (shape, pad, batch, ydiv)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(17)
        n = math.prod(shape)
        x, eps, w, xi = (torch.randn(batch, n, generator=g) for _ in range(4))
        other = torch.randn(batch // ydiv, *shape, generator=g)
        y = phase_ops.amplitude(other, pad)
        y = (y + 0.05 * torch.randn(tuple(y.shape), generator=g)).reshape(batch // ydiv, -1)
        _INPUTS[key] = (x, eps, w, xi, y.contiguous())
    return _INPUTS[key]


@pytest.mark.parametrize("shape,pad,batch,ydiv", CASES, ids=IDS)
def test_apply_and_backward(cuda, parity_record, shape, pad, batch, ydiv):
    op = PhaseRetrievalOperator(shape, pad=pad).to(cuda)
    x, _, _, _, _ = _inputs(shape, pad, batch, ydiv)
    x = x.reshape(batch, *shape)
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(batch, *op.y_shape, generator=g)  # asymmetric cotangent
    xd, cd = x.to(cuda), cot.to(cuda)
    xr = xd.clone().requires_grad_()
    y = op.apply(xr)
    assert tuple(y.shape) == (batch, *op.y_shape) and y.dtype == torch.float32
    _close(y, phase_ops.apply64(x, pad).numpy(), "apply_max_err_over_max", parity_record)
    (gx,) = torch.autograd.grad(y, xr, grad_outputs=cd)
    assert torch.isfinite(gx).all()
    _close(gx, phase_ops.vjp64(x, cot, pad).numpy(), "backward_max_err_over_max", parity_record)
    # every sample is computed alone: the bits do not depend on the batch
    x1 = xd[-1:].clone().requires_grad_()
    y1 = op.apply(x1)
    (g1,) = torch.autograd.grad(y1, x1, grad_outputs=cd[-1:])
    assert torch.equal(y1, y[-1:]) and torch.equal(g1, gx[-1:])
    # no double backward
    xr2 = xd.clone().requires_grad_()
    (gg,) = torch.autograd.grad(op.apply(xr2), xr2, grad_outputs=cd, create_graph=True)
    with pytest.raises(RuntimeError):
        gg.sum().backward()


def _sched_of(coefs, step):
    recs = (_hip.SpStepRec * 2)()
    recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
    recs[1].c, recs[1].step, recs[1].t = coefs, step, 5
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)


@pytest.mark.parametrize("shape,pad,batch,ydiv", CASES, ids=IDS)
def test_fused_dps_passes_match_closed_form(cuda, parity_record, shape, pad, batch, ydiv):
    """Both DPS passes against the fp64 closed form, with the constants of
    test_hip_kernels.py::test_fused_dps_passes_match_closed_form; the _sched forms bit-identical
    to the by-value ones."""
    op = PhaseRetrievalOperator(shape, pad=pad).to(cuda)
    apply_np, vjp_np = phase_ops.phase_ops(shape, pad)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    n, m = math.prod(shape), math.prod(op.y_shape)
    x, eps, w, xi, y = _inputs(shape, pad, batch, ydiv)
    a, k, gs = 0.3, math.sqrt(1 - 0.09), 400.0
    c_ell, c_s, std, gamma = 0.9, 0.2, 0.1, 0.05
    coefs = _hip.SpDpsCoefs(a, k, gs, c_ell, c_s, std, gamma, 1e-9)
    P = int(lib.sp_rsq_partials(desc))
    floats = int(lib.sp_dps_workspace(desc, batch))
    assert P > 0 and floats == 2 * batch * shape[0] * op.y_shape[2] * shape[1]
    xd, ed, yd, wd, xid = (t.to(cuda).contiguous() for t in (x, eps, y, w, xi))
    v = torch.full_like(xd, float("nan"))
    guard = torch.full((batch * P + 16,), float("nan"), device=cuda)  # partials, then a sentinel tail
    part = guard[:batch * P].view(batch, P)
    work = torch.full((floats,), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual_ws(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
                                      coefs, v.data_ptr(), part.data_ptr(), work.data_ptr(),
                                      _stream()), "residual_ws")
    # sp_rsq_partials is the partial count: every one written, none past the last
    assert torch.isfinite(part).all() and torch.isnan(guard[batch * P:]).all()
    v_ref, rsq_ref = phase_ops.residual_pass64(x.numpy(), eps.numpy(), y.numpy(), ydiv, a, k, gs,
                                               apply_np, vjp_np)
    out_ref = closed_form.update_pass(x.numpy(), eps.numpy(), v_ref, w.numpy(), rsq_ref, xi.numpy(),
                                      a, k, c_ell, c_s, std, gamma)
    out = torch.full_like(xd, float("nan"))
    _hip.check(lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(),
                                 wd.data_ptr(), part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch,
                                 ydiv, coefs, out.data_ptr(), _stream()), "update")
    v_err = float(np.abs(v.cpu().numpy() - v_ref).max() / np.abs(v_ref).max())
    rsq_err = float(np.abs(part.sum(1).cpu().double().numpy() / rsq_ref - 1).max())
    out_err = float(np.abs(out.cpu().numpy() - out_ref).max() / np.abs(out_ref).max())
    print(f"phase passes {shape} pad {pad}: v {v_err:.3g} rsq {rsq_err:.3g} x' {out_err:.3g} P={P}")
    parity_record("pass1_v_max_err_over_max", v_err, 2e-5)
    parity_record("pass1_rsq_max_rel_err", rsq_err, 2e-5)
    parity_record("pass2_x_max_err_over_max", out_err, 2e-5)
    assert tuple(part.shape) == (batch, P) and torch.isfinite(part).all()  # every partial written
    np.testing.assert_allclose(v.cpu().numpy(), v_ref, rtol=0, atol=2e-5 * np.abs(v_ref).max())
    np.testing.assert_allclose(part.sum(1).cpu().numpy(), rsq_ref, rtol=2e-5)
    np.testing.assert_allclose(out.cpu().numpy(), out_ref, rtol=0, atol=2e-5 * np.abs(out_ref).max())
    # the samples of a batch are independent: the last one alone gives the same bits
    v1, part1 = torch.full_like(xd[-1:], float("nan")), torch.full((1, P), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual_ws(desc, xd[-1:].data_ptr(), ed[-1:].data_ptr(),
                                      yd[(batch - 1) // ydiv:].data_ptr(), 1, 1, coefs,
                                      v1.data_ptr(), part1.data_ptr(), work.data_ptr(), _stream()),
               "residual_ws")
    assert torch.equal(v1, v[-1:]) and torch.equal(part1, part[-1:])
    # the _sched forms read record 1 through the cursor: the same bits (Philox noise in pass 2)
    sched = _sched_of(coefs, 3).to(cuda)
    cursor = torch.ones(1, dtype=torch.int32, device=cuda)
    vs, parts = torch.full_like(xd, float("nan")), torch.full((batch, P), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual_sched_ws(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch,
                                            ydiv, sched.data_ptr(), cursor.data_ptr(), vs.data_ptr(),
                                            parts.data_ptr(), work.data_ptr(), _stream()),
               "residual_sched_ws")
    assert torch.equal(vs, v) and torch.equal(parts, part)
    o_val, o_sched = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    _hip.check(lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(),
                                 wd.data_ptr(), part.data_ptr(), None, 7, 3, 2, batch, ydiv, coefs,
                                 o_val.data_ptr(), _stream()), "update")
    _hip.check(lib.sp_dps_update_sched(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(),
                                       v.data_ptr(), wd.data_ptr(), part.data_ptr(), 7, 2, batch,
                                       ydiv, sched.data_ptr(), cursor.data_ptr(), o_sched.data_ptr(),
                                       _stream()), "update_sched")
    assert torch.isfinite(o_val).all() and torch.equal(o_val, o_sched)
    # the forms without a workspace do not serve the kind; pass 2 needs v; no linear-kind routes
    args = (desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv, coefs, v.data_ptr(),
            part.data_ptr())
    assert lib.sp_dps_residual(*args, _stream()) == -3
    assert lib.sp_dps_residual_sched(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
                                     sched.data_ptr(), cursor.data_ptr(), v.data_ptr(),
                                     part.data_ptr(), _stream()) == -3
    assert lib.sp_dps_residual_ws(*args, None, _stream()) == -1
    assert lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), None, wd.data_ptr(),
                             part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch, ydiv, coefs,
                             out.data_ptr(), _stream()) == -1
    big = torch.empty(batch, m, device=cuda)
    assert lib.sp_op_apply(desc, xd.data_ptr(), big.data_ptr(), batch, _stream()) == -3
    assert lib.sp_op_adjoint(desc, big.data_ptr(), out.data_ptr(), batch, _stream()) == -3
    assert lib.sp_psld_pixel(desc, xd.data_ptr(), yd.data_ptr(), batch, ydiv, out.data_ptr(),
                             vs.data_ptr(), parts.data_ptr(), _stream()) == -3
    assert lib.sp_psld_cotangent(desc, xd.data_ptr(), ed.data_ptr(), wd.data_ptr(), parts.data_ptr(),
                                 0.1, batch, out.data_ptr(), _stream()) == -3
    from samplers_amd.samplers.resample import adamw_coefficients

    assert lib.sp_pixel_opt_step(desc, out.data_ptr(), vs.data_ptr(), o_val.data_ptr(), yd.data_ptr(),
                                 batch, ydiv, -1.0, adamw_coefficients(1, 1e-2), None,
                                 parts.data_ptr(), _stream()) == -3


def test_linear_kinds_through_the_ws_entry_points(cuda):
    """sp_op_apply_ws forwards to sp_op_apply for the linear kinds, sp_op_vjp_ws refuses them."""
    from samplers_amd.operators import GaussianBlurOperator

    shape, b = (3, 16, 16), 2
    op = GaussianBlurOperator(shape, 5, 1.5).to(cuda)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    x = torch.randn(b, *shape, device=cuda)
    out = torch.full_like(x, float("nan"))
    _hip.check(lib.sp_op_apply_ws(desc, x.data_ptr(), out.data_ptr(), b, None, _stream()), "apply_ws")
    assert torch.equal(out, op.apply(x))
    assert lib.sp_op_vjp_ws(desc, x.data_ptr(), x.data_ptr(), out.data_ptr(), b, None, _stream()) == -3


@pytest.mark.parametrize("shape,pad,batch,ydiv", CASES[:7], ids=IDS[:7])
def test_zero_image(cuda, shape, pad, batch, ydiv):
    """x = eps = 0: z = 0 everywhere, so z / |z| = 0: v is exactly zero and finite, and the
    partials sum to sum y^2."""
    op = PhaseRetrievalOperator(shape, pad=pad).to(cuda)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    b = 2
    _, _, _, _, y = _inputs(shape, pad, batch, ydiv)
    yd = y[:1].to(cuda).contiguous()
    x = torch.zeros(b, math.prod(shape), device=cuda)
    P = int(lib.sp_rsq_partials(desc))
    v, part = torch.full_like(x, float("nan")), torch.full((b, P), float("nan"), device=cuda)
    work = torch.full((int(lib.sp_dps_workspace(desc, b)),), float("nan"), device=cuda)
    coefs = _hip.SpDpsCoefs(0.3, math.sqrt(1 - 0.09), 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    _hip.check(lib.sp_dps_residual_ws(desc, x.data_ptr(), x.data_ptr(), yd.data_ptr(), b, b, coefs,
                                      v.data_ptr(), part.data_ptr(), work.data_ptr(), _stream()),
               "residual_ws")
    assert torch.isfinite(v).all() and torch.equal(v, torch.zeros_like(v))
    ref = float(y[0].double().square().sum())
    np.testing.assert_allclose(part.sum(1).cpu().double().numpy(), [ref, ref], rtol=2e-5)
    xr = x.reshape(b, *shape).clone().requires_grad_()
    yy = op.apply(xr)
    (gx,) = torch.autograd.grad(yy, xr, grad_outputs=torch.ones_like(yy))
    assert torch.equal(yy, torch.zeros_like(yy)) and torch.equal(gx, torch.zeros_like(gx))


def _problem(shape, pad, b, seed, noise, dev):
    op = PhaseRetrievalOperator(shape, pad=pad)
    x_true = si.fixture_x_true(b, shape, seed)
    y = op.apply(x_true)  # torch.fft on the host
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return op, y, InverseProblem(op.to(dev), y.to(dev), noise.to(dev))


def test_make_dps_step_is_the_fused_step(cuda):
    for noise in (GaussianNoise(0.05), PoissonNoise(1.0)):
        _, y, prob = _problem((3, 16, 16), (8, 8), 2, 0, noise, cuda)
        net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
        step = make_dps_step(net, prob, prob.observation.reshape(2, *prob.operator.y_shape), 1)
        assert type(step) is FusedDPSStep and not isinstance(step, GenericDPSStep)
        assert step.needs_v and step.workspace(2, prob.observation) is not None
        with pytest.raises(NotImplementedError):
            FusedDPSStep(net, prob, prob.observation.reshape(2, *prob.operator.y_shape), 1, mode="pgdm")


DPS_CONFIGS = [((3, 16, 16), (8, 8)), ((1, 12, 20), (6, 2)), ((3, 64, 64), (16, 16))]


@pytest.mark.parametrize("shape,pad", DPS_CONFIGS, ids=["32x32", "24x24", "96x96"])
@pytest.mark.parametrize("noise_kind", ["gauss", "poisson"])
def test_dps_matches_oracle(cuda, parity_record, noise_kind, shape, pad):
    b, N = 2, 8
    noise = GaussianNoise(0.05) if noise_kind == "gauss" else PoissonNoise(1.0)
    _, y, prob = _problem(shape, pad, b, 0, noise, cuda)
    net = si.make_samplers_amd_net("conv", shape[0], 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", shape[0], 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    lp = dps_loop.gaussian_log_prob(0.05) if noise_kind == "gauss" else dps_loop.poisson_log_prob(1.0)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 lambda x: phase_ops.amplitude(x, pad), lp, y, init,
                                 lambda i: steps[i], gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps phase", shape, pad, noise_kind, err)
    parity_record("dps_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_dps_philox_sharding_and_micro_batch_are_invariant(cuda):
    """3 x 32 x 32 as in the test of the same name for the PSF blur and super-resolution, so the
    stand-in prior's convolutions run at the shapes (batch 4, 2 and 1) those tests already rely
    on to be bit-identical across batch sizes, and a mismatch here can only come from the passes
    under test; pad 8 gives 48 x 48 planes: radix-4, radix-4 and radix-3 passes on both axes."""
    shape, pad, b = (3, 32, 32), (8, 8), 4
    _, _, prob = _problem(shape, pad, b, 0, GaussianNoise(0.05), cuda)
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


def test_graph_replay_matches_eager(cuda):
    """test_psf_gpu.py::test_graph_replay_matches_eager for phase retrieval: the captured step
    holds the three pass-1 launches and torch's allocation of the work buffer."""
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.networks.unet2d import UNet2DConfig

    cfg = UNet2DConfig(sample_size=32, block_out_channels=(64, 128), attention_levels=(1,),
                       layers_per_block=1)
    shape, b = (3, 32, 32), 2
    op = PhaseRetrievalOperator(shape, pad=8).to(cuda)  # 48 x 48
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


def test_resample_pixel_consistency_is_the_generic_route(cuda, parity_record):
    """make_consistency(...).mse_grad_ss: autograd through the HIP forward and the HIP VJP."""
    from samplers_amd.samplers.resample import _GenericConsistency, make_consistency

    shape, pad, b = (3, 16, 16), (8, 8), 2
    op = PhaseRetrievalOperator(shape, pad=pad).to(cuda)
    x, _, _, _, y = _inputs(shape, pad, 4, 1)
    x, y = x[:b], y[:b]
    cons = make_consistency(op, y.to(cuda), 1)
    assert type(cons) is _GenericConsistency
    total = y.numel()
    grad, ss = cons.mse_grad_ss(x.to(cuda), total)
    x64 = x.reshape(b, *shape).double()
    r = y.reshape(b, *op.y_shape).double() - phase_ops.apply64(x64, pad)
    ref = phase_ops.vjp64(x64, (-2.0 / total) * r, pad)
    _close(grad.reshape(b, *shape), ref.numpy(), "resample_mse_grad_max_err_over_max", parity_record)
    assert abs(float(ss) / float(r.square().sum()) - 1) <= 2e-5


def test_psld_fails_at_apply_transpose(cuda):
    from samplers_amd.samplers.psld import FusedPSLDStep

    shape = (3, 16, 16)
    _, _, prob = _problem(shape, (8, 8), 1, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    with pytest.raises(NotImplementedError, match="Transpose"):
        FusedPSLDStep(net, prob, prob.observation.reshape(1, -1), 1, net.get_latent_shape(shape))


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
from samplers_amd.operators import PhaseRetrievalOperator
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
for shape, pad in (((1, 2, 2), (3, 3)), ((1, 8, 8), (0, 0)), ((2, 6, 10), (1, 3)),
                   ((1, 12, 20), (6, 2)), ((3, 16, 16), (8, 8))):
    op = PhaseRetrievalOperator(shape, pad=pad).to(dev)
    desc = op.hip_descriptor()
    b, n, m = 3, int(desc.n), int(desc.m)
    P = int(lib.sp_rsq_partials(desc))
    x, eps, w = (torch.randn(b, n, device=dev) for _ in range(3))
    y, g = (torch.randn(b, m, device=dev) for _ in range(2))
    ax, dx = torch.empty(b, m, device=dev), torch.empty(b, n, device=dev)
    work = torch.empty(int(lib.sp_op_workspace(desc, b)), device=dev)
    _hip.check(lib.sp_op_apply_ws(desc, x.data_ptr(), ax.data_ptr(), b, work.data_ptr(), st), "apply")
    _hip.check(lib.sp_op_vjp_ws(desc, x.data_ptr(), g.data_ptr(), dx.data_ptr(), b, work.data_ptr(),
                                st), "vjp")
    c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    v, part, out = torch.empty_like(x), torch.empty(b, P, device=dev), torch.empty_like(x)
    _hip.check(lib.sp_dps_residual_ws(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 1, c,
                                      v.data_ptr(), part.data_ptr(), work.data_ptr(), st),
               "sp_dps_residual_ws")
    _hip.check(lib.sp_dps_update(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v.data_ptr(),
                                 w.data_ptr(), part.data_ptr(), None, 7, 3, 0, b, 1, c,
                                 out.data_ptr(), st), "sp_dps_update")
    nv, site = _hip.debug_violations()
    print(shape, pad, "violations", nv, site, flush=True)
    assert nv == 0, (shape, pad, nv, site)
    assert torch.isfinite(out).all() and torch.isfinite(ax).all() and torch.isfinite(dx).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The phase kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library), over the first five table shapes."""
    run_debug_child(DEBUG_CHILD)
