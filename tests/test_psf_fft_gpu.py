"""FFT-domain PSF blur (SP_OP_PSF_FFT, csrc/sp_psf_fft.hip) on the GPU: the operator's maps, their
autograd backward and the fused DPS passes against the fp64 semantics of tests/psf_fft_ops.py, and
the samplers against the oracle loops.

Bounds are the native-operator family's (test_phase_gpu.py runs the same FFT code under them):
2e-5 x max|reference| per element and 2e-5 relative on the residual norms for the maps and the
fused passes, 1e-4 relative L2 for the DPS / PSLD trajectories, 1e-5 for graph replay and the
pixel-optimisation iterate.  The same arithmetic in fp32 torch.fft on the CPU stays within
4.3e-7 x max|ref| of fp64 at all the shapes and modes below, so 2e-5 leaves about 50x headroom.

The fp64 reference takes the helper's direct route where that is quick and its FFT route for the
large cases; tests/test_psf_fft_api.py pins the two to each other.

Largest errors measured on an MI355X over CASES (parity_record has every figure): apply 2.8e-7,
adjoint and backward 3.0e-7, pass-1 v 4.5e-7, pass-2 x' 2.9e-7 (all x max|ref|), ||r||^2 3.9e-7
relative, DPS trajectories 4.6e-7 and PSLD 4.8e-7 relative L2, ReSample's MSE gradient 1.4e-7 and
pixel solve 8.1e-7, 1.7e-6 against the direct SP_OP_PSF kernel at R = 30 — at the CPU fp32
figure."""

import math
import types

import numpy as np
import pytest
import torch

import psf_fft_ops
import psf_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import closed_form, dps_loop
from oracle.latent_loops import psld_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise, PoissonNoise
from samplers_amd.operators import FFTPSFBlurOperator, PSFBlurOperator
from samplers_amd.samplers import DPSSampler
from samplers_amd.samplers.dps import FusedDPSStep, GenericDPSStep, make_dps_step

pytestmark = pytest.mark.gpu


# shape, R, batch, y_div, padding modes
ALL = ("reflect", "circular", "zeros")
SHAPES = [
    ((1, 3, 3), 1, 1, 1, ALL),                           # 5 -> 8 x 8: the smallest transform
    ((2, 7, 10), 3, 2, 1, ALL),                          # W % 4 != 0; exact fits 13 -> 16, 16 -> 16
    ((1, 5, 9), 4, 2, 2, ALL),                           # R = H - 1; radix 3 at 17 -> 24
    ((3, 16, 16), 8, 4, 1, ALL),                         # exact 32
    ((1, 40, 72), 31, 2, 1, ALL),                        # beyond the direct kernel's cap; 128 x 192
    ((3, 64, 64), 16, 6, 3, ALL),                        # 96
    ((1, 96, 160), 30, 1, 1, ALL),                       # several column tiles, rectangular
    ((1, 256, 256), 30, 1, 1, ("reflect", "circular")),  # 316 -> 384: the paper's size
    ((1, 512, 512), 128, 1, 1, ("reflect", "zeros")),    # exact 768
    ((1, 512, 512), 255, 1, 1, ("reflect", "circular")),  # 1022 -> 1024, one line per workgroup
]
CASES = [(s, r, b, d, p) for s, r, b, d, modes in SHAPES for p in modes]
IDS = [f"{'x'.join(map(str, c[0]))}-R{c[1]}-b{c[2]}-d{c[3]}-{c[4]}" for c in CASES]
KERNELS = ("sparse", "randn")


def _kernel(r, kind):
    """An asymmetric sparse PSF with a corner tap, or a signed dense one."""
    if kind == "sparse":
        return psf_ops.random_sparse_kernel(r, seed=100 * r + 1)
    k = 2 * r + 1
    return torch.randn(k, k, generator=torch.Generator().manual_seed(200 * r + 3)) / k


def _route(shape, r):
    """The helper's direct route up to about 2e8 multiply-adds per sample, else its FFT route."""
    return "direct" if math.prod(shape) * (2 * r + 1) ** 2 <= 2e8 else "fft"


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64).reshape(tuple(got.shape))
    return float(np.abs(got.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())


def _close(got, ref, what, record=None, bound=2e-5):
    err = _err(got, ref)
    print(f"{what}: max err / max|ref| = {err:.3g}")
    if record is not None:
        record(what, err, bound)
    assert err <= bound, (what, err)


_INPUTS = {}


def _inputs(shape, batch, ydiv):
    """x, eps, w, xi ~ randn (batch, n), y ~ randn (batch / ydiv, n) and a cotangent (batch, n).
    Computed once per case and shared; never modified."""
    key = (shape, batch, ydiv)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(23)
        n = math.prod(shape)
        x, eps, w, xi, cot = (torch.randn(batch, n, generator=g) for _ in range(5))
        y = torch.randn(batch // ydiv, n, generator=g)
        _INPUTS[key] = (x, eps, w, xi, y, cot)
    return _INPUTS[key]


_MAPS = {}


def _maps64(shape, r, batch, ydiv, padding, kind):
    """A x and A^T cot in fp64, once per case."""
    key = (shape, r, batch, ydiv, padding, kind)
    if key not in _MAPS:
        x, _, _, _, _, cot = _inputs(shape, batch, ydiv)
        h, route = _kernel(r, kind), _route(shape, r)
        _MAPS[key] = (psf_fft_ops.apply64(x.reshape(batch, *shape), h, padding, route).numpy(),
                      psf_fft_ops.adjoint64(cot.reshape(batch, *shape), h, padding, route).numpy())
    return _MAPS[key]


@pytest.mark.parametrize("kind", KERNELS)
@pytest.mark.parametrize("shape,r,batch,ydiv,padding", CASES, ids=IDS)
def test_apply_adjoint_and_backward(cuda, parity_record, shape, r, batch, ydiv, padding, kind):
    h = _kernel(r, kind)
    op = FFTPSFBlurOperator(shape, h, padding=padding).to(cuda)
    x, _, _, _, _, cot = _inputs(shape, batch, ydiv)
    xd, cd = x.reshape(batch, *shape).to(cuda), cot.reshape(batch, *shape).to(cuda)
    ax_ref, atc_ref = _maps64(shape, r, batch, ydiv, padding, kind)
    ax, atc = op.apply(xd), op.apply_transpose(cd)
    assert tuple(ax.shape) == (batch, *shape) and ax.dtype == torch.float32
    assert tuple(atc.shape) == (batch, *shape) and atc.dtype == torch.float32
    _close(ax, ax_ref, "apply_max_err_over_max", parity_record)
    _close(atc, atc_ref, "adjoint_max_err_over_max", parity_record)
    # autograd: the backward of A is A^T of the cotangent, and of A^T, A — the same launches
    xr = xd.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=cd)
    _close(gx, atc_ref, "backward_max_err_over_max", parity_record)
    assert torch.equal(gx, atc)
    cr = cd.clone().requires_grad_()
    (gc,) = torch.autograd.grad(op.apply_transpose(cr), cr, grad_outputs=xd)
    assert torch.equal(gc, ax)
    # every sample is computed alone: the bits do not depend on the batch
    assert torch.equal(op.apply(xd[-1:]), ax[-1:])
    assert torch.equal(op.apply_transpose(cd[-1:]), atc[-1:])
    # leading batch dimensions are kept
    two = op.apply(xd.reshape(batch, 1, *shape))
    assert tuple(two.shape) == (batch, 1, *shape) and torch.equal(two.reshape(ax.shape), ax)


def test_adjoint_identity_on_the_device(cuda):
    """<A x, y> = <x, A^T y> to fp32 accumulation accuracy, for the three modes."""
    shape, r, b = (2, 40, 72), 31, 2
    g = torch.Generator().manual_seed(8)
    x, y = (torch.randn(b, *shape, generator=g).to(cuda) for _ in range(2))
    for padding in ALL:
        op = FFTPSFBlurOperator(shape, _kernel(r, "randn"), padding=padding).to(cuda)
        ax, aty = op.apply(x).double(), op.apply_transpose(y).double()
        lhs, rhs = float((ax * y.double()).sum()), float((x.double() * aty).sum())
        assert abs(lhs - rhs) <= 2e-5 * float(ax.norm() * y.double().norm()), (padding, lhs, rhs)


def test_agrees_with_the_direct_kernel(cuda, parity_record):
    """(1, 96, 160), R = 30, reflect: the new kind's A and A^T against PSFBlurOperator's HIP
    results, within the sum of the two operators' bounds."""
    shape, r, b = (1, 96, 160), 30, 1
    x, _, _, _, _, cot = _inputs(shape, b, 1)
    xd, cd = x.reshape(b, *shape).to(cuda), cot.reshape(b, *shape).to(cuda)
    for kind in KERNELS:
        h = _kernel(r, kind)
        new, direct = FFTPSFBlurOperator(shape, h).to(cuda), PSFBlurOperator(shape, h).to(cuda)
        ax_ref, atc_ref = _maps64(shape, r, b, 1, "reflect", kind)
        for got, want, ref, what in ((new.apply(xd), direct.apply(xd), ax_ref, "apply"),
                                     (new.apply_transpose(cd), direct.apply_transpose(cd), atc_ref,
                                      "adjoint")):
            err = float((got - want).abs().max()) / float(np.abs(ref).max())
            parity_record(f"{what}_vs_direct_kernel_over_max", err, 4e-5)
            assert err <= 4e-5, (kind, what, err)


def _sched_of(coefs, step):
    recs = (_hip.SpStepRec * 2)()
    recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
    recs[1].c, recs[1].step, recs[1].t = coefs, step, 5
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)


def _lines(N):
    NP = (N + N // 16) | 1
    return max(1, min(16, (32000 - 8 * N) // (16 * NP)))


@pytest.mark.parametrize("shape,r,batch,ydiv,padding", CASES, ids=IDS)
def test_fused_dps_passes_match_closed_form(cuda, parity_record, shape, r, batch, ydiv, padding):
    """Both DPS passes against the fp64 closed form, with the constants of
    test_hip_kernels.py::test_fused_dps_passes_match_closed_form; the _sched forms bit-identical
    to the by-value ones."""
    kind = "randn" if (r + len(padding)) % 2 else "sparse"
    h = _kernel(r, kind)
    op = FFTPSFBlurOperator(shape, h, padding=padding).to(cuda)
    apply_np, adjoint_np = psf_fft_ops.psf_ops(shape, h, padding, _route(shape, r))
    lib, desc = _hip.load_library(), op.hip_descriptor()
    n = math.prod(shape)
    x, eps, w, xi, y, _ = _inputs(shape, batch, ydiv)
    a, k, gs = 0.3, math.sqrt(1 - 0.09), 400.0
    c_ell, c_s, std, gamma = 0.9, 0.2, 0.1, 0.05
    coefs = _hip.SpDpsCoefs(a, k, gs, c_ell, c_s, std, gamma, 1e-9)
    P = int(lib.sp_rsq_partials(desc))
    floats = int(lib.sp_dps_workspace(desc, batch))
    Nw = op.padded_shape[1]
    assert P == shape[0] * -(-shape[1] // _lines(Nw))  # one partial per (plane, row tile)
    assert floats == 2 * batch * shape[0] * (Nw // 2 + 1) * shape[1]
    xd, ed, yd, wd, xid = (t.to(cuda).contiguous() for t in (x, eps, y, w, xi))
    v = torch.full_like(xd, float("nan"))
    guard = torch.full((batch * P + 16,), float("nan"), device=cuda)  # partials, then a sentinel tail
    part = guard[:batch * P].view(batch, P)
    wguard = torch.full((floats + 16,), float("nan"), device=cuda)
    work = wguard[:floats]
    _hip.check(lib.sp_dps_residual_ws(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
                                      coefs, v.data_ptr(), part.data_ptr(), work.data_ptr(),
                                      _stream()), "residual_ws")
    # every partial and the whole intermediate written, nothing past their ends
    assert torch.isfinite(part).all() and torch.isnan(guard[batch * P:]).all()
    assert torch.isfinite(work).all() and torch.isnan(wguard[floats:]).all()
    v_ref, rsq_ref = closed_form.residual_pass(x.numpy(), eps.numpy(), y.numpy(), ydiv, a, k, gs,
                                               apply_np, adjoint_np)
    out_ref = closed_form.update_pass(x.numpy(), eps.numpy(), v_ref, w.numpy(), rsq_ref, xi.numpy(),
                                      a, k, c_ell, c_s, std, gamma)
    out = torch.full_like(xd, float("nan"))
    _hip.check(lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(),
                                 wd.data_ptr(), part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch,
                                 ydiv, coefs, out.data_ptr(), _stream()), "update")
    v_err = float(np.abs(v.cpu().numpy() - v_ref).max() / np.abs(v_ref).max())
    rsq_err = float(np.abs(part.sum(1).cpu().double().numpy() / rsq_ref - 1).max())
    out_err = float(np.abs(out.cpu().numpy() - out_ref).max() / np.abs(out_ref).max())
    print(f"psf-fft passes {shape} R={r} {padding}: v {v_err:.3g} rsq {rsq_err:.3g} "
          f"x' {out_err:.3g} P={P}")
    parity_record("pass1_v_max_err_over_max", v_err, 2e-5)
    parity_record("pass1_rsq_max_rel_err", rsq_err, 2e-5)
    parity_record("pass2_x_max_err_over_max", out_err, 2e-5)
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
    assert lib.sp_dps_residual_ws(*args, None, _stream()) == -1
    assert lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), None, wd.data_ptr(),
                             part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch, ydiv, coefs,
                             out.data_ptr(), _stream()) == -1
    assert lib.sp_op_apply(desc, xd.data_ptr(), out.data_ptr(), batch, _stream()) == -3
    assert lib.sp_op_adjoint(desc, xd.data_ptr(), out.data_ptr(), batch, _stream()) == -3
    assert lib.sp_psld_pixel(desc, xd.data_ptr(), yd.data_ptr(), batch, ydiv, out.data_ptr(),
                             vs.data_ptr(), parts.data_ptr(), _stream()) == -3


CONFIGS = {"32x32-R8-reflect": ((3, 32, 32), 8, "reflect"),
           "24x24-R11-circular": ((1, 24, 24), 11, "circular"),
           "24x24-R11-zeros": ((1, 24, 24), 11, "zeros")}


PSLD_CONFIGS = {"32x32-R8-reflect": ((3, 32, 32), 8, "reflect"),
                "24x24-R11-circular": ((3, 24, 24), 11, "circular")}


def _problem(config, b, seed, noise, dev):
    shape, r, padding = CONFIGS[config] if isinstance(config, str) else config
    h = _kernel(r, "sparse")
    op = FFTPSFBlurOperator(shape, h, padding=padding)
    x_true = si.fixture_x_true(b, shape, seed)
    y = op.apply(x_true)  # F.conv2d on the host
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return shape, h, padding, y, InverseProblem(op.to(dev), y.to(dev), noise.to(dev))


def test_make_dps_step_is_the_fused_step(cuda):
    for noise in (GaussianNoise(0.05), PoissonNoise(1.0)):
        shape, _, _, _, prob = _problem("32x32-R8-reflect", 2, 0, noise, cuda)
        net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
        rows = prob.observation.reshape(2, *prob.operator.y_shape)
        step = make_dps_step(net, prob, rows, 1)
        assert type(step) is FusedDPSStep and not isinstance(step, GenericDPSStep)
        assert step.needs_v and step.workspace(2, prob.observation) is not None
        with pytest.raises(NotImplementedError):
            FusedDPSStep(net, prob, rows, 1, mode="pgdm")


def test_pgdm_rejects_the_operator(cuda):
    from samplers_amd.samplers.pgdm import PGDMSampler

    _, _, _, _, prob = _problem("32x32-R8-reflect", 1, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(prob, num_sampling_steps=4)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("noise_kind", ["gauss", "poisson"])
def test_dps_matches_oracle(cuda, parity_record, noise_kind, config):
    b, N = 2, 8
    noise = GaussianNoise(0.05) if noise_kind == "gauss" else PoissonNoise(1.0)
    shape, h, padding, y, prob = _problem(config, b, 0, noise, cuda)
    net = si.make_samplers_amd_net("conv", shape[0], 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", shape[0], 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    lp = dps_loop.gaussian_log_prob(0.05) if noise_kind == "gauss" else dps_loop.poisson_log_prob(1.0)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 lambda x: psf_fft_ops.blur(x, h, padding), lp, y, init,
                                 lambda i: steps[i], gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps psf-fft", config, noise_kind, err)
    parity_record("dps_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_dps_philox_sharding_and_micro_batch_are_invariant(cuda):
    """3 x 32 x 32 as in the test of the same name for the PSF blur, so the stand-in prior's
    convolutions run at the shapes (batch 4, 2 and 1) that test already relies on to be
    bit-identical across batch sizes; R = 8 gives 48 x 48 transforms (radix 4, 4 and 3)."""
    b = 4
    _, _, _, _, prob = _problem("32x32-R8-reflect", b, 0, GaussianNoise(0.05), cuda)
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
    """test_psf_gpu.py::test_graph_replay_matches_eager for the FFT route: the captured step holds
    the five pass-1 launches and torch's allocation of the work buffer."""
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.networks.unet2d import UNet2DConfig

    cfg = UNet2DConfig(sample_size=32, block_out_channels=(64, 128), attention_levels=(1,),
                       layers_per_block=1)
    shape, b = (3, 32, 32), 2
    op = FFTPSFBlurOperator(shape, _kernel(8, "sparse"), padding="circular").to(cuda)
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


@pytest.mark.parametrize("config", list(PSLD_CONFIGS))
def test_psld_matches_oracle_through_the_generic_route(cuda, parity_record, config):
    from samplers_amd.samplers.psld import FusedPSLDStep, PSLDSampler

    b, N = 2, 6
    shape, h, padding, y, prob = _problem(PSLD_CONFIGS[config], b, 4, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    lat = net.get_latent_shape(shape)
    step = FusedPSLDStep(net, prob, prob.observation.reshape(b, -1), 1, lat)
    assert step.generic and step.desc is None  # autograd over apply / apply_transpose, both HIP
    init, steps = si.replay_noise(13, (b, *lat), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = PSLDSampler(net)(prob, num_sampling_steps=N, noise_fn=fn)
    core, vae = si.EpsCore("conv", 4, 0.1), si.LatentCore()
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    ref = psld_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                         lambda x: psf_fft_ops.blur(x.double(), h, padding).float(),
                         lambda v: psf_fft_ops.adjoint(v.double(), h, padding).float(),
                         vae.decode, vae.encode, y, init, lambda i: steps[i])
    err = si.relative_error(out.cpu(), ref)
    print("psld psf-fft", config, err)
    parity_record("psld_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_resample_pixel_consistency_is_the_generic_route(cuda, parity_record):
    """make_consistency(...): autograd through the HIP A with the HIP A^T as its backward.  The
    MSE gradient against fp64, and ReSample's pixel-space solve against the oracle loop's
    (oracle/resample_loop.py: AdamW(lr = 1e-2) on the MSE) for a fixed number of iterations."""
    from samplers_amd.samplers.resample import (ReSampleSampler, _GenericConsistency, _finish_log,
                                                make_consistency)

    shape, r, padding, b = (3, 16, 16), 8, "zeros", 2
    h = _kernel(r, "sparse")
    op = FFTPSFBlurOperator(shape, h, padding=padding).to(cuda)
    x, _, _, _, y, _ = _inputs(shape, 4, 1)
    x, y = x[:b].contiguous(), y[:b].contiguous()
    cons = make_consistency(op, y.to(cuda), 1)
    assert type(cons) is _GenericConsistency
    total = y.numel()
    grad, ss = cons.mse_grad_ss(x.to(cuda), total)
    x64 = x.reshape(b, *shape).double()
    res = y.reshape(b, *shape).double() - psf_fft_ops.apply64(x64, h, padding)
    ref = psf_fft_ops.adjoint64((-2.0 / total) * res, h, padding)
    _close(grad.reshape(b, *shape), ref.numpy(), "resample_mse_grad_max_err_over_max", parity_record)
    assert abs(float(ss) / float(res.square().sum()) - 1) <= 2e-5

    iters = 12
    opt = x.reshape(b, *shape).clone().requires_grad_()
    adam = torch.optim.AdamW([opt], lr=1e-2)
    rows = y.reshape(b, *shape)
    for _ in range(iters):
        adam.zero_grad()
        loss = torch.nn.MSELoss()(rows, psf_fft_ops.blur(opt, h, padding))
        loss.backward()
        adam.step()
    holder = types.SimpleNamespace()
    out = ReSampleSampler._pixel_optimization(holder, x.reshape(b, *shape).to(cuda), cons, total, 0.0,
                                              iters)
    _finish_log(holder)
    (rec,) = holder.optimization_log
    assert rec["kind"] == "pixel" and rec["iterations"] == iters and not rec["stopped_early"]
    err = float((out.cpu().reshape(opt.shape) - opt.detach()).norm() / opt.detach().norm())
    parity_record("resample_pixel_solve_rel_l2", err, 1e-5)
    assert err < 1e-5, err


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
from samplers_amd.operators import FFTPSFBlurOperator
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
gen = torch.Generator().manual_seed(1)
for shape, r in (((1, 3, 3), 1), ((2, 7, 10), 3), ((1, 5, 9), 4), ((3, 16, 16), 8), ((1, 40, 72), 31)):
    for padding in ("reflect", "circular", "zeros"):
        k = 2 * r + 1
        op = FFTPSFBlurOperator(shape, torch.randn(k, k, generator=gen) / k, padding=padding).to(dev)
        desc = op.hip_descriptor()
        b, n = 3, int(desc.n)
        P = int(lib.sp_rsq_partials(desc))
        x, eps, w, y, g = (torch.randn(b, n, device=dev) for _ in range(5))
        ax, dx = torch.empty(b, n, device=dev), torch.empty(b, n, device=dev)
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
        print(shape, r, padding, "violations", nv, site, flush=True)
        assert nv == 0, (shape, r, padding, nv, site)
        assert torch.isfinite(out).all() and torch.isfinite(ax).all() and torch.isfinite(dx).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh child
    process (a process holds one library): the maps and a DPS step over the first five table
    shapes in the three modes."""
    run_debug_child(DEBUG_CHILD)
