"""The parallel-beam projector (SP_OP_RADON, csrc/sp_radon.hip) on the GPU: the maps and DPS
pass 1 through the raw entry points, into NaN-filled outputs between guard bands, against
tests/radon_ref.py; then the samplers against the oracle loops.

Which seam of the kernels' tiling each shape of radon_ref.CASES (C, H, W, D, angles) crosses —
`project` sweeps the dominant axis (rows for axis 0, columns for axis 1) in bands of 32, stages per
band the slab of cross indices its chunk of <= 256 rays can touch (at most 400), gathers from
global memory when the slab is wider and skips a band whose slab misses the image; `backproject`
runs one thread per pixel in workgroups of 256 consecutive pixels:
  9x13 (1,9,13,17,5)          one partial band on both axes (9, 13 < 32); a plane of 117 pixels, less
                              than one backproject workgroup
  24x20 (2,24,20,33,7)        two planes: the plane offsets of x, y and the partials
  16x16-short (1,16,16,12,4)  detector shorter than the diagonal: pixels whose candidates
                              floor(s*) - 1 .. + 2 fall off either end of the detector; y_div 2
  40x36 (3,40,36,59,23)       bands 32 + 8 / 32 + 4; batch 3 on one observation row (y_div 3);
                              1440 pixels = 5.6 backproject workgroups per plane
  64x96 (1,64,96,117,1)       exactly 2 and 3 full bands, one angle
  136x72, 72x136              4 full bands + 8 on one axis, 2 + 8 on the other; staged slabs of
  (1,..,155,3)                up to ~250 cross indices, wider than the 128-row image bands the
                              issue names
  200x40 (1,200,40,300,2)     D > 256: two chunks of 150 rays per angle (two partials per angle);
                              rays that miss the image, bands whose slab misses it
  wide-slab (1,16,24,200,3)   |alpha| = 2.5 over 200 rays: slabs wider than 400, the gathered path,
                              beside a staged angle in the same table
  skip-rows / skip-cols       tall / wide thin images under beta = +-1: whole bands off the image
  (1,96,8,16,2), (1,8,96,16,2) on both sides, for either axis
The exact cases (radon_ref.EXACT_SHAPES) add D of equal and different parity to the cross
extent, with two planes and a batch of two.

Bounds.  Per element against dense32: |out - ref| <= n 2^-24 E (radon_ref.rounding_steps: the
kernels sum in the order the issue counts, n = max(H, W) + 4, 2 angles + 4, their sum + 6).
Against dense64: max|out - ref| / max|ref| <= 2 x the CPU emulation's own distance at that shape
(only the order of summation may differ from the emulation).  |r|^2: 2e-5 relative.  Samplers: the
bounds of tests/test_psf_gpu.py (1e-4 relative L2 for DPS / PSLD, 1e-5 for graph replay and the
pixel-optimisation iterate).
Measured on an MI355X (worst case): rho 0.11 (A), 0.39 (A^T), 0.024 (v); against dense64 the
emulation's own distance to three digits (0.50 of the bound; 8.1e-6 / 9.2e-6 / 9.0e-6 at the
largest shapes); |r|^2 4.7e-7; DPS 2.3e-6 (Gaussian), 2.5e-7 (Poisson); PSLD 4.6e-7.
"""

import math
import types

import numpy as np
import pytest
import torch

import exact_cases as ec
import radon_ref as rr
import stand_ins as si
from kind_harness import run_debug_child
from oracle import dps_loop
from oracle.latent_loops import psld_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise, PoissonNoise
from samplers_amd.operators import RadonOperator
from samplers_amd.samplers import DPSSampler

pytestmark = pytest.mark.gpu

NAMES = list(rr.CASES)


class Runner:
    """The raw entry points on a table and a geometry; every output through a Guarded buffer."""

    def __init__(self, cuda, C, H, W, D, table):
        self.lib, self.cuda = _hip.load_library(), cuda
        self.st = torch.cuda.current_stream().cuda_stream
        self.C, self.H, self.W, self.D, self.nA = C, H, W, D, int(table.shape[0])
        self.table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(cuda)
        d = _hip.SpOp()
        d.kind, d.channels, d.height, d.width = _hip.SP_OP_RADON, C, H, W
        d.n, d.m, d.radius, d.factor = C * H * W, C * self.nA * D, self.nA, D
        d.taps = self.table.data_ptr()
        self.desc = d
        self.P = int(self.lib.sp_rsq_partials(d))
        assert self.P == C * self.nA * math.ceil(D / 256)

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.cuda)

    def apply(self, x):
        b = x.shape[0]
        xd = self.dev(x)
        y = ec.Guarded((b, self.C, self.nA, self.D), self.nA * self.D, self.cuda)
        _hip.check(self.lib.sp_op_apply(self.desc, xd.data_ptr(), y.ptr(), b, self.st), "sp_op_apply")
        torch.cuda.synchronize()
        return y.check()

    def adjoint(self, g):
        b = g.shape[0]
        gd = self.dev(g)
        x = ec.Guarded((b, self.C, self.H, self.W), self.H * self.W, self.cuda)
        _hip.check(self.lib.sp_op_adjoint(self.desc, gd.data_ptr(), x.ptr(), b, self.st), "sp_op_adjoint")
        torch.cuda.synchronize()
        return x.check()

    def pass1(self, x, eps, y, y_div, coefs, sched=False):
        """(v, work, partials) of sp_dps_residual_ws (or the _sched_ws form on a two-record
        schedule whose cursor points at `coefs`)."""
        b = x.shape[0]
        xd, ed, yd = self.dev(x), self.dev(eps), self.dev(y)
        floats = int(self.lib.sp_dps_workspace(self.desc, b))
        assert floats == b * self.desc.m
        v = ec.Guarded((b, self.C, self.H, self.W), self.H * self.W, self.cuda)
        work = ec.Guarded((b, self.C, self.nA, self.D), self.nA * self.D, self.cuda)
        part = ec.Guarded((b, self.P), self.P, self.cuda)
        c = _hip.SpDpsCoefs(coefs[0], coefs[1], coefs[2], 0.9, 0.2, 0.1, 0.05, 1e-9)
        if sched:
            recs = (_hip.SpStepRec * 2)()
            recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
            recs[1].c, recs[1].step, recs[1].t = c, 3, 5
            sd = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(self.cuda)
            cursor = torch.ones(1, dtype=torch.int32, device=self.cuda)
            _hip.check(self.lib.sp_dps_residual_sched_ws(self.desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(),
                                                         b, y_div, sd.data_ptr(), cursor.data_ptr(), v.ptr(),
                                                         part.ptr(), work.ptr(), self.st), "residual_sched_ws")
        else:
            _hip.check(self.lib.sp_dps_residual_ws(self.desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), b,
                                                   y_div, c, v.ptr(), part.ptr(), work.ptr(), self.st),
                       "residual_ws")
        torch.cuda.synchronize()
        return v.check(), work.check(), part.check()  # every element of all three was written


# --- bitwise: axis angles and dyadic tables on integers ---------------------------------------
@pytest.mark.parametrize("table_name", ["axis", "dyadic"])
@pytest.mark.parametrize("H,W,D", rr.EXACT_SHAPES)
def test_exact_cases_are_bitwise(cuda, table_name, H, W, D):
    """Integer x, eps, y, g in [-3, 3], a = k = 1/2, grad_scale 4: no fp32 evaluation can round
    (test_radon_ref.py shows it on the emulations), so the kernels return the fp64 products."""
    table = rr.AXIS_TABLE if table_name == "axis" else rr.DYADIC_TABLE
    B, C, nA = 2, 2, table.shape[0]
    run = Runner(cuda, C, H, W, D, table)
    rng = np.random.default_rng(H * 1000 + W * 10 + D)
    x, eps = (rng.integers(-3, 4, size=(B, C, H, W)).astype(np.float64) for _ in range(2))
    g, y = (rng.integers(-3, 4, size=(B, C, nA, D)).astype(np.float64) for _ in range(2))
    A = rr.dense64(table, H, W, D)
    t = torch.from_numpy
    ec.assert_bitwise(run.apply(x), t((x.reshape(B * C, -1) @ A.T).reshape(B, C, nA, D)), "A x")
    ec.assert_bitwise(run.adjoint(g), t((g.reshape(B * C, -1) @ A).reshape(B, C, H, W)), "A^T g")
    v, work, part = run.pass1(x, eps, y, 1, (0.5, 0.5, 4.0))
    x0 = 2.0 * x - eps
    r = y.reshape(B * C, -1) - x0.reshape(B * C, -1) @ A.T
    ec.assert_bitwise(work, t((4.0 * r).reshape(B, C, nA, D)), "work")
    ec.assert_bitwise(v, t((4.0 * r @ A).reshape(B, C, H, W)), "v")
    rsq = (r ** 2).reshape(B, -1).sum(1)
    assert np.abs(part.double().sum(1).cpu().numpy() / rsq - 1).max() <= 2e-5


# --- per element and against fp64 on randn ------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_maps_and_pass1_on_randn(cuda, parity_record, name):
    C, H, W, D, table, batch, y_div = rr.CASES[name]
    run = Runner(cuda, C, H, W, D, table)
    x, eps, g, y = rr.case_inputs(name)
    ref, n, dist = rr.reference64(name), rr.rounding_steps(name), rr.emulation_distance(name)
    v, work, part = run.pass1(x, eps, y, y_div, rr.COEFS)
    got = {"apply": run.apply(x), "adjoint": run.adjoint(g), "v": v}
    for key, out in got.items():
        out = out.cpu().numpy()
        rho = rr.rho(out, ref[key + "32"], ref["E_" + key], n[key])  # and exact zeros where E == 0
        err = rr.max_over_max(out, ref[key + "64"])
        print(f"{name} {key}: rho {rho:.3g} (n = {n[key]}), vs dense64 {err:.3g} "
              f"(emulation {dist[key]:.3g})")
        parity_record(f"{key}_rho", rho, 1.0)
        parity_record(f"{key}_vs_dense64_over_max", err, 2 * dist[key])
        assert rho <= 1.0, (key, rho)
        assert err <= 2 * dist[key], (key, err, dist[key])
    rsq_err = float(np.abs(part.double().sum(1).cpu().numpy() / ref["rsq64"] - 1).max())
    parity_record("pass1_rsq_max_rel_err", rsq_err, 2e-5)
    assert rsq_err <= 2e-5
    # work = grad_scale r: the whole buffer, against the fp32-weight matrix
    werr = rr.max_over_max(work.cpu().numpy(), ref["work32"])
    parity_record("pass1_work_over_max", werr, 2e-5)
    assert werr <= 2e-5


# --- determinism: bitwise -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["40x36", "200x40", "wide-slab"])
def test_pass1_is_deterministic(cuda, name):
    C, H, W, D, table, _, _ = rr.CASES[name]
    run = Runner(cuda, C, H, W, D, table)
    rng = np.random.default_rng(7)
    nA = table.shape[0]
    x, eps = (rng.standard_normal((4, C, H, W)).astype(np.float32) for _ in range(2))
    y = rng.standard_normal((4, C, nA, D)).astype(np.float32)
    first = run.pass1(x, eps, y, 1, rr.COEFS)
    again = run.pass1(x, eps, y, 1, rr.COEFS)
    for a, b in zip(first, again):
        assert torch.equal(a, b)  # the same bits on every run
    for s in (0, 3):  # a sample alone against the same sample in the batch of 4
        alone = run.pass1(x[s:s + 1], eps[s:s + 1], y[s:s + 1], 1, rr.COEFS)
        for a, b in zip(alone, first):
            assert torch.equal(a, b[s:s + 1])
    # y_div 2: samples 2b, 2b + 1 share observation row b
    shared = run.pass1(x, eps, y[:2], 2, rr.COEFS)
    tiled = run.pass1(x, eps, np.repeat(y[:2], 2, axis=0), 1, rr.COEFS)
    for a, b in zip(shared, tiled):
        assert torch.equal(a, b)
    # the device-resident schedule against the by-value call
    for a, b in zip(run.pass1(x, eps, y, 1, rr.COEFS, sched=True), first):
        assert torch.equal(a, b)
    # the maps too
    assert torch.equal(run.apply(x), run.apply(x)) and torch.equal(run.apply(x[1:2]), run.apply(x)[1:2])
    assert torch.equal(run.adjoint(y), run.adjoint(y)) and torch.equal(run.adjoint(y[1:2]), run.adjoint(y)[1:2])


def test_autograd_backward_is_the_other_map(cuda):
    op = RadonOperator((3, 40, 36), angles=rr.case_angles(23), detector_size=59).to(cuda)
    g = torch.Generator().manual_seed(0)
    xd = torch.randn(2, 3, 40, 36, generator=g).to(cuda)
    yd = torch.randn(2, 3, 23, 59, generator=g).to(cuda)
    ax, aty = op.apply(xd), op.apply_transpose(yd)
    assert tuple(ax.shape) == (2, 3, 23, 59) and tuple(aty.shape) == (2, 3, 40, 36)
    xr = xd.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=yd)
    assert torch.equal(gx, aty)
    yr = yd.clone().requires_grad_()
    (gy,) = torch.autograd.grad(op.apply_transpose(yr), yr, grad_outputs=xd)
    assert torch.equal(gy, ax)
    # the device maps are the host form's
    host = RadonOperator((3, 40, 36), angles=rr.case_angles(23), detector_size=59)
    ref = host.apply(xd.cpu().double())
    assert float((ax.cpu().double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    lhs, rhs = float((ax.double() * yd.double()).sum()), float((xd.double() * aty.double()).sum())
    assert abs(lhs - rhs) <= 2e-5 * float(ax.double().norm() * yd.double().norm())


# --- samplers (the cases of tests/test_psf_gpu.py at 1 x 32 x 32, 9 angles) ---------------------
SHAPE, ANGLES = (1, 32, 32), 9


def _problem(b, seed, noise, dev):
    op = RadonOperator(SHAPE, num_angles=ANGLES)
    x_true = si.fixture_x_true(b, SHAPE, seed)
    y = op.apply(x_true)
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return op, y, InverseProblem(RadonOperator(SHAPE, num_angles=ANGLES).to(dev), y.to(dev), noise.to(dev))


def test_dps_philox_sharding_and_micro_batch_are_invariant(cuda):
    b = 4
    _, _, prob = _problem(b, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", SHAPE[0], 0.1, device=cuda)
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
def test_dps_matches_oracle(cuda, parity_record, noise_kind):
    b, N = 2, 8
    noise = GaussianNoise(0.05) if noise_kind == "gauss" else PoissonNoise(1.0)
    host, y, prob = _problem(b, 0, noise, cuda)
    net = si.make_samplers_amd_net("conv", SHAPE[0], 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *SHAPE), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", SHAPE[0], 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    lp = dps_loop.gaussian_log_prob(0.05) if noise_kind == "gauss" else dps_loop.poisson_log_prob(1.0)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 host.apply, lp, y, init, lambda i: steps[i], gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps radon", noise_kind, err)
    parity_record("dps_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_psld_matches_oracle(cuda, parity_record):
    from samplers_amd.samplers.psld import FusedPSLDStep, PSLDSampler

    shape = (3, 32, 32)  # the latent stand-ins decode to three channels
    b, N = 2, 6
    host = RadonOperator(shape, num_angles=ANGLES)
    x_true = si.fixture_x_true(b, shape, 4)
    y = host.apply(x_true)
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(5))
    prob = InverseProblem(RadonOperator(shape, num_angles=ANGLES).to(cuda), y.to(cuda),
                          GaussianNoise(0.05).to(cuda))
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    lat = net.get_latent_shape(shape)
    step = FusedPSLDStep(net, prob, prob.observation.reshape(b, -1), 1, lat)
    assert step.blur and not step.generic  # composed from sp_op_apply / sp_op_adjoint, not autograd
    assert step.m == 3 * ANGLES * host.detector_size and step.m != step.n
    init, steps = si.replay_noise(13, (b, *lat), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = PSLDSampler(net)(prob, num_sampling_steps=N, noise_fn=fn)
    core, vae = si.EpsCore("conv", 4, 0.1), si.LatentCore()
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    ref = psld_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                         lambda x: host.apply(x.double()).float(),
                         lambda v: host.apply_transpose(v.double()).float(),
                         vae.decode, vae.encode, y, init, lambda i: steps[i])
    err = si.relative_error(out.cpu(), ref)
    print("psld radon", err)
    parity_record("psld_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_psld_cotangent_takes_the_ata_u_branch(cuda):
    """c = -omega A^T r / |r| + (u - A^T A u) over n elements with A^T A u from the caller, as for
    the blurs: the kind has no keep_bits for the masked form to read."""
    C, H, W, D, table, _, _ = rr.CASES["24x20"]
    run = Runner(cuda, C, H, W, D, table)
    b, n = 2, C * H * W
    g = torch.Generator().manual_seed(3)
    atr, u, ata_u = (torch.randn(b, n, generator=g) for _ in range(3))
    ad, ud, pd, nd = (t.to(cuda) for t in (atr, u, ata_u, torch.tensor([2.5])))  # kept alive
    out = ec.Guarded((b, n), n, cuda)
    _hip.check(run.lib.sp_psld_cotangent(run.desc, ad.data_ptr(), ud.data_ptr(), pd.data_ptr(),
                                         nd.data_ptr(), 0.1, b, out.ptr(), run.st), "sp_psld_cotangent")
    torch.cuda.synchronize()
    ref = -0.1 * atr.double() / math.sqrt(2.5) + (u.double() - ata_u.double())
    assert rr.max_over_max(out.check().cpu().numpy(), ref.numpy()) <= 2e-5


def test_pixel_optimization_device_stop_matches_reference_loop(cuda):
    """test_psf_gpu.py's test of the same name: ReSample's pixel optimisation on the composed
    path (sp_op_apply / sp_residual_grad over m / sp_op_adjoint / sp_adamw_step_until), with
    m != n: the device stopping rule runs exactly the iterations of the torch AdamW loop."""
    from samplers_amd.samplers.resample import ReSampleSampler, _Consistency, _finish_log

    torch.manual_seed(0)
    shape, b = (3, 32, 32), 2
    op = RadonOperator(shape, num_angles=ANGLES).to(cuda)
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
    assert int(cons.desc.kind) == _hip.SP_OP_RADON and cons.m != cons.n
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

    _, _, prob = _problem(1, 0, GaussianNoise(0.05), cuda)
    net = si.make_samplers_amd_net("conv", SHAPE[0], 0.1, device=cuda)
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(prob, num_sampling_steps=4)


def test_graph_replay_matches_eager(cuda):
    """test_psf_gpu.py::test_graph_replay_matches_eager for the projector: the captured step holds
    both pass-1 launches and torch's allocation of the work buffer."""
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.networks.unet2d import UNet2DConfig

    cfg = UNet2DConfig(sample_size=32, block_out_channels=(64, 128), attention_levels=(1,),
                       layers_per_block=1)
    shape, b = (3, 32, 32), 2
    op = RadonOperator(shape, num_angles=ANGLES).to(cuda)
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
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import radon_ref as rr
from samplers_amd import _hip
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
for name, (C, H, W, D, table, batch, y_div) in rr.CASES.items():
    tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    nA = int(table.shape[0])
    d = _hip.SpOp()
    d.kind, d.channels, d.height, d.width = _hip.SP_OP_RADON, C, H, W
    d.n, d.m, d.radius, d.factor, d.taps = C * H * W, C * nA * D, nA, D, tab.data_ptr()
    b, n, m = 3, int(d.n), int(d.m)
    P = int(lib.sp_rsq_partials(d))
    x, eps, w = (torch.randn(b, n, device=dev) for _ in range(3))
    y, g = (torch.randn(b, m, device=dev) for _ in range(2))
    ax, atg = torch.empty(b, m, device=dev), torch.empty(b, n, device=dev)
    _hip.check(lib.sp_op_apply(d, x.data_ptr(), ax.data_ptr(), b, st), "sp_op_apply")
    _hip.check(lib.sp_op_adjoint(d, g.data_ptr(), atg.data_ptr(), b, st), "sp_op_adjoint")
    c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    v, part, out = torch.empty_like(x), torch.empty(b, P, device=dev), torch.empty_like(x)
    work = torch.empty(int(lib.sp_dps_workspace(d, b)), device=dev)
    _hip.check(lib.sp_dps_residual_ws(d, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 1, c,
                                      v.data_ptr(), part.data_ptr(), work.data_ptr(), st),
               "sp_dps_residual_ws")
    _hip.check(lib.sp_dps_update(d, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v.data_ptr(),
                                 w.data_ptr(), part.data_ptr(), None, 7, 3, 0, b, 1, c,
                                 out.data_ptr(), st), "sp_dps_update")
    nv, site = _hip.debug_violations()
    print(name, "violations", nv, site, flush=True)
    assert nv == 0, (name, nv, site)
    assert torch.isfinite(out).all() and torch.isfinite(ax).all() and torch.isfinite(atg).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The projector kernels' SP_DCHECK index invariants under the bounds-checked library, in a
    fresh child process (a process holds one library), over every shape of the kernel cases."""
    run_debug_child(DEBUG_CHILD)
