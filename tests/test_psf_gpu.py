"""Point-spread-function blur (SP_OP_PSF, csrc/sp_psf.hip) on the GPU: the operator's maps and the
fused DPS passes against the fp64 semantics of tests/psf_ops.py, and the samplers against the
oracle loops.

Bounds are the native-operator family's (test_superres_gpu.py / test_hip_kernels.py): 2e-5 x
max|reference| per element and 2e-5 relative on the residual norms for the maps and the fused
passes, 1e-4 relative L2 for the DPS / PSLD trajectories, 1e-5 for graph replay and the
pixel-optimisation iterate.  The same pass-1 arithmetic in fp32 torch on the CPU is within
8.6e-7 x max|v| of fp64 at R = 30 on 3x64x64 (1e-7 at R = 1), so 2e-5 leaves > 20x headroom."""

import math
import types

import numpy as np
import pytest
import torch

import psf_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import closed_form, dps_loop
from oracle.latent_loops import psld_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise, PoissonNoise
from samplers_amd.operators import GaussianBlurOperator, PSFBlurOperator, motion_blur_kernel
from samplers_amd.samplers import DPSSampler

pytestmark = pytest.mark.gpu



def gappy_kernel(radius: int) -> torch.Tensor:
    """All-zero rows, rows with one tap at either end, and rows with interior zeros: what the
    span sweep (first / last non-zero column per tap row, all-zero rows skipped) must get right."""
    k = 2 * radius + 1
    g = torch.Generator().manual_seed(99)
    h = torch.zeros(k, k, dtype=torch.float64)
    vals = torch.rand(k, k, generator=g, dtype=torch.float64) + 0.1
    h[1, k - 1] = vals[1, k - 1]                     # one tap in the last column
    h[2, 0] = vals[2, 0]                             # one tap in the first column
    h[3, 0], h[3, k - 1] = vals[3, 0], vals[3, k - 1]  # both ends, zeros between
    h[radius, 2:k - 3:3] = vals[radius, 2:k - 3:3]   # interior zeros
    h[radius + 2, radius - 1:radius + 2] = -vals[radius + 2, radius - 1:radius + 2]  # negative taps
    h[k - 2, 5] = vals[k - 2, 5]
    assert not h[0].any() and not h[k - 1].any() and not h[radius + 1].any()  # all-zero rows
    return (h / h.abs().sum()).to(torch.float32)


# shape, R, batch, y_div, kernel
CASES = [
    ((1, 3, 3), 1, 1, 1, "sparse"),      # every pixel on two borders
    ((2, 7, 10), 2, 2, 1, "sparse"),     # odd H, W % 4 != 0: element-wise loads and stores
    ((1, 8, 12), 3, 2, 2, "sparse"),
    ((3, 32, 32), 4, 4, 1, "sparse"),
    ((2, 17, 19), 8, 3, 1, "sparse"),    # H = 2R + 1: folds from both sides on one pixel
    ((3, 32, 40), 15, 2, 1, "sparse"),   # halo wider than the image's half
    ((1, 61, 61), 30, 2, 1, "sparse"),   # smallest image at the largest radius
    ((3, 64, 64), 30, 6, 3, "sparse"),
    ((1, 70, 132), 30, 1, 1, "sparse"),  # 3 x 3 tiles of 32 x 64: interior, edge and corner tiles
    ((2, 40, 70), 10, 2, 1, "gappy"),    # 2 x 2 tiles; all-zero tap rows and interior zeros
]
IDS = [f"{'x'.join(map(str, c[0]))}-R{c[1]}-b{c[2]}-d{c[3]}-{c[4]}" for c in CASES]
MULTI_TILE = {(1, 70, 132): 9, (2, 40, 70): 8}  # sp_rsq_partials of the cases with several tiles


def _kernel(r, kind, seed=0):
    return gappy_kernel(r) if kind == "gappy" else psf_ops.random_sparse_kernel(r, seed=100 * r + seed)


def _close(got, ref, what, record=None):
    ref = np.asarray(ref, dtype=np.float64).reshape(tuple(got.shape))
    err = float(np.abs(got.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())
    print(f"{what}: max err / max|ref| = {err:.3g}")
    if record is not None:
        record(what, err, 2e-5)
    assert err <= 2e-5, (what, err)


@pytest.mark.parametrize("shape,r,batch,ydiv,kind", CASES, ids=IDS)
def test_apply_adjoint_and_backward(cuda, parity_record, shape, r, batch, ydiv, kind):
    h = _kernel(r, kind)
    op = PSFBlurOperator(shape, h).to(cuda)
    g = torch.Generator().manual_seed(0)
    x, y = (torch.randn(batch, *shape, generator=g) for _ in range(2))
    xd, yd = x.to(cuda), y.to(cuda)
    ax, aty = op.apply(xd), op.apply_transpose(yd)
    assert tuple(ax.shape) == (batch, *shape) and tuple(aty.shape) == (batch, *shape)
    _close(ax, psf_ops.apply64(x, h).numpy(), "apply_max_err_over_max", parity_record)
    _close(aty, psf_ops.adjoint64(y, h).numpy(), "adjoint_max_err_over_max", parity_record)
    # every sample is computed alone: the bits do not depend on the batch
    assert torch.equal(op.apply(xd[-1:]), ax[-1:]) and torch.equal(op.apply_transpose(yd[-1:]), aty[-1:])
    # a delta PSF copies (centre) or reflect-shifts (elsewhere) the image: exact
    k = 2 * r + 1
    for u, v in ((r, r), (0, k - 1), (k - 1, r - 1)):
        d = torch.zeros(k, k)
        d[u, v] = 1.0
        got = PSFBlurOperator(shape, d).to(cuda).apply(xd).cpu()
        assert torch.equal(got, psf_ops.shifted(x, u - r, v - r)), (u, v)
    # HipLinearMap: the backward of A is A^T of the cotangent, and of A^T, A
    xr = xd.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=yd)
    assert torch.equal(gx, aty)
    yr = yd.clone().requires_grad_()
    (gy,) = torch.autograd.grad(op.apply_transpose(yr), yr, grad_outputs=xd)
    assert torch.equal(gy, ax)


def test_gaussian_outer_product_matches_the_separable_operator(cuda):
    shape = (3, 32, 32)
    op = PSFBlurOperator.gaussian(shape, 9, 3.0).to(cuda)
    sep = GaussianBlurOperator(shape, 9, 3.0).to(cuda)
    g = torch.Generator().manual_seed(1)
    x, y = (torch.randn(4, *shape, generator=g).to(cuda) for _ in range(2))
    _close(op.apply(x), sep.apply(x).cpu().double().numpy(), "gaussian apply")
    _close(op.apply_transpose(y), sep.apply_transpose(y).cpu().double().numpy(), "gaussian adjoint")


def _dps_passes(cuda, shape, r, batch, ydiv, kind, coefs_tail, seed, record, route="direct"):
    """Both DPS passes against oracle.closed_form, with the constants and bounds of
    test_hip_kernels.py::test_fused_dps_passes_match_closed_form."""
    h = _kernel(r, kind)
    op = PSFBlurOperator(shape, h).to(cuda)
    apply_np, adjoint_np = psf_ops.psf_ops(shape, h, route)
    lib = _hip.load_library()
    desc = op.hip_descriptor()
    n = math.prod(shape)
    g = torch.Generator().manual_seed(seed)
    x, eps, w, xi = (torch.randn(batch, n, generator=g) for _ in range(4))
    y = torch.randn(batch // ydiv, n, generator=g)
    a, k, gs = 0.3, math.sqrt(1 - 0.09), 400.0
    c_ell, c_s, std, gamma = coefs_tail
    coefs = _hip.SpDpsCoefs(a, k, gs, c_ell, c_s, std, gamma, 1e-9)
    P = int(lib.sp_rsq_partials(desc))
    assert P > 0
    floats = int(lib.sp_dps_workspace(desc, batch))
    assert floats == batch * n
    xd, ed, yd, wd, xid = (t.to(cuda).contiguous() for t in (x, eps, y, w, xi))
    v = torch.full_like(xd, float("nan"))
    part = torch.full((batch, P), float("nan"), device=cuda)
    work = torch.full((floats,), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual_ws(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
                                      coefs, v.data_ptr(), part.data_ptr(), work.data_ptr(),
                                      _stream()), "residual_ws")
    v_ref, rsq_ref = closed_form.residual_pass(x.numpy(), eps.numpy(), y.numpy(), ydiv, a, k, gs,
                                               apply_np, adjoint_np)
    out_ref = closed_form.update_pass(x.numpy(), eps.numpy(), v_ref, w.numpy(), rsq_ref, xi.numpy(),
                                      a, k, c_ell, c_s, std, gamma)
    out = torch.full_like(xd, float("nan"))
    _hip.check(lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(),
                                 wd.data_ptr(), part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch,
                                 ydiv, coefs, out.data_ptr(), _stream()), "update")
    v_err = float(np.abs(v.cpu().numpy() - v_ref).max() / np.abs(v_ref).max())
    rsq_err = float(np.abs(part.sum(1).cpu().numpy() / rsq_ref - 1).max())
    out_err = float(np.abs(out.cpu().numpy() - out_ref).max() / np.abs(out_ref).max())
    print(f"psf passes {shape} R={r}: v {v_err:.3g} rsq {rsq_err:.3g} x' {out_err:.3g} P={P}")
    record("pass1_v_max_err_over_max", v_err, 2e-5)
    record("pass1_rsq_max_rel_err", rsq_err, 2e-5)
    record("pass2_x_max_err_over_max", out_err, 2e-5)
    assert torch.isfinite(work).all()  # the whole work buffer is written: g = grad_scale r
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
    # the forms without a workspace do not serve PSF; pass 2 needs v; no fused latent passes
    args = (desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv, coefs, v.data_ptr(),
            part.data_ptr())
    assert lib.sp_dps_residual(*args, _stream()) == -3
    assert lib.sp_dps_residual_ws(*args, None, _stream()) == -1
    assert lib.sp_dps_update(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), None, wd.data_ptr(),
                             part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch, ydiv, coefs,
                             out.data_ptr(), _stream()) == -1
    from samplers_amd.samplers.resample import adamw_coefficients

    assert lib.sp_psld_pixel(desc, xd.data_ptr(), yd.data_ptr(), batch, ydiv, out.data_ptr(),
                             v.data_ptr(), part.data_ptr(), _stream()) == -3
    assert lib.sp_pixel_opt_step(desc, out.data_ptr(), v.data_ptr(), work.data_ptr(), yd.data_ptr(),
                                 batch, ydiv, -1.0, adamw_coefficients(1, 1e-2), None,
                                 part.data_ptr(), _stream()) == -3
    assert lib.sp_psld_cotangent(desc, xd.data_ptr(), ed.data_ptr(), None, part.data_ptr(), 0.1,
                                 batch, out.data_ptr(), _stream()) == -1  # ata_u is required
    return P


@pytest.mark.parametrize("shape,r,batch,ydiv,kind", CASES, ids=IDS)
def test_fused_dps_passes_match_closed_form(cuda, parity_record, shape, r, batch, ydiv, kind):
    P = _dps_passes(cuda, shape, r, batch, ydiv, kind, (0.9, 0.2, 0.1, 0.05), 0, parity_record)
    if shape in MULTI_TILE:
        assert P == MULTI_TILE[shape] and P > 1


def test_dps_passes_full_size(cuda, parity_record):
    """3 x 256 x 256 at R = 30 (the fp64 reference through the helper's FFT route, which
    test_psf_api.py pins to the direct one)."""
    _dps_passes(cuda, (3, 256, 256), 30, 1, 1, "sparse", (0.97, 0.11, 0.05, 1.0), 7, parity_record,
                route="fft")


def test_psld_cotangent_takes_the_elementwise_branch(cuda):
    shape, r, b = (2, 17, 19), 8, 2
    op = PSFBlurOperator(shape, _kernel(r, "sparse")).to(cuda)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    n = math.prod(shape)
    g = torch.Generator().manual_seed(3)
    atr, u, ata_u = (torch.randn(b, n, generator=g) for _ in range(3))
    ad, ud, pd, nd = (t.to(cuda) for t in (atr, u, ata_u, torch.tensor([2.5])))  # kept alive
    out = torch.full((b, n), float("nan"), device=cuda)
    _hip.check(lib.sp_psld_cotangent(desc, ad.data_ptr(), ud.data_ptr(), pd.data_ptr(),
                                     nd.data_ptr(), 0.1, b, out.data_ptr(), _stream()),
               "sp_psld_cotangent")
    ref = -0.1 * atr.double() / math.sqrt(2.5) + (u.double() - ata_u.double())
    _close(out, ref.numpy(), "psld cotangent")


CONFIGS = {"R4": ((3, 32, 32), 4), "R30-motion": ((3, 64, 64), 30)}


def _config_kernel(name):
    shape, r = CONFIGS[name]
    h = motion_blur_kernel(61, 0.5, 0) if name == "R30-motion" else psf_ops.random_sparse_kernel(r, seed=42)
    assert tuple(h.shape) == (2 * r + 1, 2 * r + 1)
    return shape, h


def _psf_problem(shape, h, b, seed, noise, dev):
    op = PSFBlurOperator(shape, h)
    x_true = si.fixture_x_true(b, shape, seed)
    y = op.apply(x_true)
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return op, y, InverseProblem(op.to(dev), y.to(dev), noise.to(dev))


def test_dps_philox_sharding_and_micro_batch_are_invariant(cuda):
    shape, h = _config_kernel("R4")
    b = 4
    _, _, prob = _psf_problem(shape, h, b, 0, GaussianNoise(0.05), cuda)
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


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("noise_kind", ["gauss", "poisson"])
def test_dps_matches_oracle(cuda, parity_record, noise_kind, config):
    shape, h = _config_kernel(config)
    b, N = 2, 8
    noise = GaussianNoise(0.05) if noise_kind == "gauss" else PoissonNoise(1.0)
    _, y, prob = _psf_problem(shape, h, b, 0, noise, cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", 3, 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    lp = dps_loop.gaussian_log_prob(0.05) if noise_kind == "gauss" else dps_loop.poisson_log_prob(1.0)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 lambda x: psf_ops.blur(x, h), lp, y, init, lambda i: steps[i],
                                 gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps psf", config, noise_kind, err)
    parity_record("dps_rel_l2", err, 1e-4)
    assert err < 1e-4


@pytest.mark.parametrize("config", list(CONFIGS))
def test_psld_matches_oracle(cuda, parity_record, config):
    from samplers_amd.samplers.psld import FusedPSLDStep, PSLDSampler

    shape, h = _config_kernel(config)
    b, N = 2, 6
    _, y, prob = _psf_problem(shape, h, b, 4, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    lat = net.get_latent_shape(shape)
    step = FusedPSLDStep(net, prob, prob.observation.reshape(b, -1), 1, lat)
    assert step.blur and not step.generic  # the native composed path, not autograd
    init, steps = si.replay_noise(13, (b, *lat), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = PSLDSampler(net)(prob, num_sampling_steps=N, noise_fn=fn)
    core, vae = si.EpsCore("conv", 4, 0.1), si.LatentCore()
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    ref = psld_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                         lambda x: psf_ops.blur(x.double(), h).float(),
                         lambda v: psf_ops.adjoint(v.double(), h).float(),
                         vae.decode, vae.encode, y, init, lambda i: steps[i])
    err = si.relative_error(out.cpu(), ref)
    print("psld psf", config, err)
    parity_record("psld_rel_l2", err, 1e-4)
    assert err < 1e-4


@pytest.mark.parametrize("config", list(CONFIGS))
def test_pixel_optimization_device_stop_matches_reference_loop(cuda, config):
    """test_latent_gpu.py's test of the same name on its blur path (sp_op_apply /
    sp_residual_grad / sp_op_adjoint / sp_adamw_step_until composed, no fused pass): the device
    stopping rule runs exactly the iterations of the torch AdamW + MSELoss loop."""
    from samplers_amd.samplers.resample import ReSampleSampler, _Consistency, _finish_log

    torch.manual_seed(0)
    shape, h = _config_kernel(config)
    b = 2
    op = PSFBlurOperator(shape, h).to(cuda)
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
    assert int(cons.desc.kind) == _hip.SP_OP_PSF
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


def test_pgdm_rejects_the_operator(cuda):
    from samplers_amd.samplers.pgdm import PGDMSampler

    shape, h = _config_kernel("R4")
    _, _, prob = _psf_problem(shape, h, 1, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(prob, num_sampling_steps=4)


def test_graph_replay_matches_eager(cuda):
    """test_graph_gpu.py::test_graph_replay_matches_eager for the PSF blur (its small UNet): the
    captured step holds both pass-1 launches and torch's allocation of the work buffer."""
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.networks.unet2d import UNet2DConfig

    cfg = UNet2DConfig(sample_size=32, block_out_channels=(64, 128), attention_levels=(1,),
                       layers_per_block=1)
    shape, b = (3, 32, 32), 2
    op = PSFBlurOperator(shape, psf_ops.random_sparse_kernel(4, seed=42)).to(cuda)
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
sys.path.insert(0, sys.argv[1] + "/tests")
import psf_ops
from samplers_amd import _hip
from samplers_amd.operators import PSFBlurOperator
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
for shape, r in (((3, 32, 40), 15), ((2, 7, 10), 2), ((1, 40, 70), 3)):
    op = PSFBlurOperator(shape, psf_ops.random_sparse_kernel(r, seed=r)).to(dev)
    desc = op.hip_descriptor()
    b, n = 3, int(desc.n)
    P = int(lib.sp_rsq_partials(desc))
    x, eps, w, y = (torch.randn(b, n, device=dev) for _ in range(4))
    ax, aty = torch.empty(b, n, device=dev), torch.empty(b, n, device=dev)
    _hip.check(lib.sp_op_apply(desc, x.data_ptr(), ax.data_ptr(), b, st), "sp_op_apply")
    _hip.check(lib.sp_op_adjoint(desc, y.data_ptr(), aty.data_ptr(), b, st), "sp_op_adjoint")
    c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    v, part, out = torch.empty_like(x), torch.empty(b, P, device=dev), torch.empty_like(x)
    work = torch.empty(int(lib.sp_dps_workspace(desc, b)), device=dev)
    _hip.check(lib.sp_dps_residual_ws(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 1, c,
                                      v.data_ptr(), part.data_ptr(), work.data_ptr(), st),
               "sp_dps_residual_ws")
    _hip.check(lib.sp_dps_update(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v.data_ptr(),
                                 w.data_ptr(), part.data_ptr(), None, 7, 3, 0, b, 1, c,
                                 out.data_ptr(), st), "sp_dps_update")
    nv, site = _hip.debug_violations()
    print(shape, r, "violations", nv, site, flush=True)
    assert nv == 0, (shape, r, nv, site)
    assert torch.isfinite(out).all() and torch.isfinite(ax).all() and torch.isfinite(aty).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The PSF kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library): a float4-store case, the element-wise
    (2, 7, 10) case and one with several tiles."""
    run_debug_child(DEBUG_CHILD)
