"""What the operator kinds' tests share: the raw entry points into guarded buffers (`KindDevice`), the
four reference loops and sampler calls behind one name each, the host-sampler checks and the
debug-library child.  A plain module: the calling test hands in `cuda`, `parity_record` and the like.

A new kind's test file subclasses `KindDevice` (descriptor, traits, expected sizes), keeps its own
cases, bounds and `debug_sweep`, and calls the functions below for everything else."""

import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import prox_ref as pr
import stand_ins as si
from oracle import dps_loop
from oracle.latent_loops import pgdm_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise

ROOT = Path(__file__).resolve().parents[1]
GUARD = 16                   # NaNs on each side of a guarded buffer
SEED, OFFSET = 77, 5         # seed and sample_offset of the Philox calls
GAMMA, GUIDANCE, ETA = 1e-2, 0.05, 1.0   # DPS and PGDM settings of the trajectory tests
# the scalars of the raw passes: DPS pass 1, the prox / DiffPIR step, DDRM in the DDRM suite's regimes
DPS = dict(a=0.3, k=math.sqrt(1 - 0.09), gs=400.0)
PROX = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)
DDRM = {"big": dr.make_coefs(3.0, 0.05, 0.85, 1.0), "blend": dr.make_coefs(0.5, 0.05, 0.5, 0.5),
        "small": dr.make_coefs(0.041, 0.05, 0.85, 1.0), "sig_y=0": dr.make_coefs(0.23, 0.0, 0.85, 1.0),
        "sig_prev=0": dr.make_coefs(0.0, 0.05, 0.85, 1.0)}


# --- small helpers ------------------------------------------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


def f32(d):
    return {k: float(np.float32(v)) for k, v in d.items()}


def acp(dtype=torch.float32):
    return torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).to(dtype)


def counting_net(kind, channels, scale, device=None):
    """(net, flags): the stand-in prior; flags gets one bool per network call, whether the call was
    building an autograd graph.  Also kept as `net.graph_flags`."""
    net = si.make_samplers_amd_net(kind, channels, scale, device=device)
    flags, inner = [], net.forward

    def forward(x, t):
        e = inner(x, t)
        flags.append(bool(e.requires_grad) or torch.is_grad_enabled())
        return e

    net.forward = forward
    net.graph_flags = flags
    return net, flags


def _loop_distance(run):
    """(fp32 reference loop, its relative distance to the fp64 run, the bound that follows)."""
    ref32 = run(torch.float32)
    cond = si.relative_error(run(torch.float64), ref32)
    return ref32, cond, max(1e-4, 20 * cond)


def loop_bound(run):
    """(fp32 reference loop, max(1e-4, 20 x its distance to the fp64 run))."""
    ref32, _, bound = _loop_distance(run)
    return ref32, bound


def bound_check(out, run, what, record):
    ref32, cond, bound = _loop_distance(run)
    err = si.relative_error(out.reshape(ref32.shape).cpu(), ref32)
    print(f"{what}: rel l2 {err:.3g}, fp32 reference to fp64 {cond:.3g}, bound {bound:.3g}")
    record(f"{what}_rel_l2", err, bound, fp32_to_fp64=cond)
    assert err < bound


def rounding_check(got, ref64, env, n_r, what, record=None):
    """max over the elements of |got - ref64| / (n_r · 2⁻²⁴ · E) ≤ 1, E the pass's envelope."""
    ratio = float(((got.detach().cpu().double() - ref64).abs() / (n_r * 2.0 ** -24 * env)).max())
    print(f"{what}: worst |err| / (n_r 2^-24 E) = {ratio:.3g} (n_r = {n_r})")
    if record is not None:
        record(f"{what}_err_over_bound", ratio, 1.0, n_r=n_r)
    assert ratio <= 1.0, (what, ratio)
    return ratio


def make_descriptor(kind, n, m, c=0, h=0, w=0, radius=0, factor=0, taps=None, keep=None, rank=None):
    d = _hip.SpOp()
    d.kind, d.n, d.m, d.channels, d.height, d.width = kind, n, m, c, h, w
    d.radius, d.factor, d.taps, d.keep_bits, d.word_rank = radius, factor, taps, keep, rank
    return d


# --- guarded buffers ----------------------------------------------------------------------------------------
def guarded(floats, device):
    """`floats` NaNs between two guard bands of 16 NaNs; (whole, view)."""
    whole = torch.full((floats + 2 * GUARD,), float("nan"), device=device)
    return whole, whole[GUARD:GUARD + floats]


def check_guards(whole, floats):
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + floats:]).all()


def _ptr(t):
    return None if t is None else t.data_ptr()


class KindDevice:
    """A kind's descriptor on the device and every entry point into guarded buffers.

    A subclass builds its tables and descriptor, calls ``super().__init__`` and supplies TRAITS,
    `check_workspace`, `partials` and, where it prepares a q, `Q_ROW` and `check_q`."""

    TRAITS = None            # sp_op_traits of the descriptor
    WORKSPACE_FORMS = True   # the maps and DPS pass 1 through the _ws entry points, or the plain ones
    Q_PASSES = frozenset()   # of "prox" (the map and the DiffPIR step) and "ddrm": the passes that read
    #                          a prepared q where the others read the observation rows y
    Q_ROW = None             # floats in a row of q

    def __init__(self, device, desc, xs, ys, name=""):
        self.lib = _hip.load_library()
        self.device, self.desc, self.xs, self.ys, self.name = device, desc, tuple(xs), tuple(ys), name
        assert (desc.n, desc.m) == (int(np.prod(xs)), int(np.prod(ys)))
        self.n, self.m = desc.n, desc.m
        assert self.lib.sp_op_traits(desc) == self.TRAITS

    def check_workspace(self, floats, batch):
        """Assert on the float count a size function gave for `batch`."""
        raise NotImplementedError

    def partials(self):
        """The expected sp_rsq_partials."""
        raise NotImplementedError

    def check_q(self, q, y):
        """Assert on a prepared q (rows, Q_ROW)."""

    def _run(self, size_fn, batch, out_shape, call):
        """call(out, work pointer) into a guarded output and a guarded workspace (NULL where the
        kind takes none): status, both guard bands, a finite output."""
        floats = int(size_fn(self.desc, batch))
        self.check_workspace(floats, batch)
        whole, work = guarded(floats, self.device)
        count = int(np.prod(out_shape))
        owhole, out = guarded(count, self.device)
        out = out.view(out_shape)
        _hip.check(call(out, work.data_ptr() if floats else None), f"{self.name} entry")
        check_guards(whole, floats)
        check_guards(owhole, count)
        assert torch.isfinite(out).all()
        return out

    # the four maps
    def apply(self, x):
        b = x.shape[0]

        def call(o, w):
            if self.WORKSPACE_FORMS:
                return self.lib.sp_op_apply_ws(self.desc, x.data_ptr(), o.data_ptr(), b, w, stream())
            return self.lib.sp_op_apply(self.desc, x.data_ptr(), o.data_ptr(), b, stream())

        return self._run(self.lib.sp_op_workspace, b, (b, *self.ys), call)

    def adjoint(self, g):
        b = g.shape[0]

        def call(o, w):
            if self.WORKSPACE_FORMS:
                return self.lib.sp_op_vjp_ws(self.desc, g.data_ptr(), g.data_ptr(), o.data_ptr(), b, w, stream())
            return self.lib.sp_op_adjoint(self.desc, g.data_ptr(), o.data_ptr(), b, stream())

        return self._run(self.lib.sp_op_workspace, b, (b, *self.xs), call)

    def pinv(self, t, transpose=0):
        b = t.shape[0]
        return self._run(self.lib.sp_op_workspace, b, (b, *(self.ys if transpose else self.xs)),
                         lambda o, w: self.lib.sp_op_pinv_ws(self.desc, t.data_ptr(), o.data_ptr(), b, transpose, w,
                                                             stream()))

    def prepare(self, y, prox=False):
        """q of the PGDM / DDRM passes, or of the prox: (rows, Q_ROW)."""
        rows = y.shape[0]
        size = self.lib.sp_prox_prepare_size if prox else self.lib.sp_op_workspace
        floats = int(size(self.desc, rows))
        assert floats == rows * self.Q_ROW
        whole, q = guarded(floats, self.device)
        fn = self.lib.sp_prox_prepare if prox else self.lib.sp_pgdm_prepare
        _hip.check(fn(self.desc, y.data_ptr(), rows, q.data_ptr(), stream()), "prepare")
        check_guards(whole, floats)
        q = q.view(rows, self.Q_ROW)
        self.check_q(q, y)
        return q

    # pass 1 of DPS and PGDM
    def dps(self, x, eps, y, ydiv, c, sched=False):
        b, P = x.shape[0], int(self.lib.sp_rsq_partials(self.desc))
        assert P == self.partials()
        pwhole, part = guarded(b * P, self.device)
        coefs = _hip.SpDpsCoefs(c["a"], c["k"], c["gs"], 0.9, 0.2, 0.1, 0.05, 1e-9)
        plain, sched_fn = ((self.lib.sp_dps_residual_ws, self.lib.sp_dps_residual_sched_ws) if self.WORKSPACE_FORMS
                           else (self.lib.sp_dps_residual, self.lib.sp_dps_residual_sched))

        def call(o, w):
            tail = (o.data_ptr(), part.data_ptr()) + ((w,) if self.WORKSPACE_FORMS else ()) + (stream(),)
            if not sched:
                return plain(self.desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, ydiv, coefs, *tail)
            recs = (_hip.SpStepRec * 2)()
            recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
            recs[1].c, recs[1].step, recs[1].t = coefs, 3, 5
            self._sched = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(self.device)
            self._cursor = torch.ones(1, dtype=torch.int32, device=self.device)
            return sched_fn(self.desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, ydiv, self._sched.data_ptr(),
                            self._cursor.data_ptr(), *tail)

        v = self._run(self.lib.sp_dps_workspace, b, (b, *self.xs), call)
        check_guards(pwhole, b * P)
        assert torch.isfinite(part).all()
        return v, part.view(b, P)

    def pgdm(self, x, eps, q, ydiv, c):
        b = x.shape[0]
        coefs = _hip.SpDpsCoefs(c["a"], c["k"], c["gs"], 0.9, 0.2, 0.1, 0.05, 1e-9)
        return self._run(self.lib.sp_op_workspace, b, (b, *self.xs),
                         lambda o, w: self.lib.sp_pgdm_residual_ws(self.desc, x.data_ptr(), eps.data_ptr(),
                                                                   q.data_ptr(), b, ydiv, coefs, o.data_ptr(), w,
                                                                   stream()))

    # the proximal map and the two steps; `obs` is y, or q for the passes in Q_PASSES
    def _y_q(self, key, obs):
        return (None, obs.data_ptr()) if key in self.Q_PASSES else (obs.data_ptr(), None)

    def prox(self, x0, obs, ydiv, rho):
        b = x0.shape[0]
        y, q = self._y_q("prox", obs)
        return self._run(self.lib.sp_prox_workspace, b, (b, *self.xs),
                         lambda o, w: self.lib.sp_op_prox_ws(self.desc, x0.data_ptr(), y, q, b, ydiv, rho,
                                                             o.data_ptr(), w, stream()))

    def _step(self, entry, size_fn, key, x, eps, obs, xi, ydiv, coefs, alias, step):
        b = x.shape[0]
        src = x.clone() if alias else x
        y, q = self._y_q(key, obs)

        def call(o, w):
            dst = src if alias else o
            rc = entry(self.desc, src.data_ptr(), eps.data_ptr(), y, q, _ptr(xi), SEED, step, OFFSET, b, ydiv,
                       coefs, dst.data_ptr(), w, stream())
            if alias:
                o.copy_(src)
            return rc

        return self._run(size_fn, b, (b, *self.xs), call)

    def diffpir(self, x, eps, obs, xi, ydiv, c, alias=False, step=3):
        coefs = _hip.SpProxCoefs(c["a"], c["k"], c["rho"], c["a_prev"], c["c_eps"], c["c_xi"])
        return self._step(self.lib.sp_diffpir_step_ws, self.lib.sp_prox_workspace, "prox", x, eps, obs, xi, ydiv,
                          coefs, alias, step)

    def ddrm(self, x, eps, obs, xi, ydiv, c, alias=False, step=3):
        coefs = _hip.SpDdrmCoefs(*[c[k] for k in dr.KEYS])
        return self._step(self.lib.sp_ddrm_step_ws, self.lib.sp_ddrm_workspace, "ddrm", x, eps, obs, xi, ydiv,
                          coefs, alias, step)

    def randn(self, b, step=3):
        out = torch.empty(b, *self.xs, device=self.device)
        _hip.check(self.lib.sp_randn(out.data_ptr(), b, self.n, SEED, step, OFFSET, stream()), "sp_randn")
        return out

    def x0(self, x, eps, a, k):
        out = torch.empty_like(x)
        _hip.check(self.lib.sp_predict_x0(x.data_ptr(), eps.data_ptr(), x.numel(), a, k, out.data_ptr(),
                                          stream()), "sp_predict_x0")
        return out


# --- reference loops and sampler calls ----------------------------------------------------------------------
def reference_loop(sampler, S, eps_fn, acp, ts, y, init, noise, dt, sigma):
    """The plain loop of `sampler` in `dt` on a reference object S (apply, pinv, prox, ddrm)."""
    y, init = y.to(dt), init.to(dt)
    if sampler == "dps":
        return dps_loop.dps_reference(eps_fn, acp, ts, S.apply, dps_loop.gaussian_log_prob(sigma), y, init, noise,
                                      gamma=GAMMA, eta=ETA)
    if sampler == "pgdm":
        return pgdm_reference(eps_fn, acp, ts, S.apply, S.pinv, y, init, noise, guidance_weight=GUIDANCE, eta=ETA)
    if sampler == "diffpir":
        return pr.diffpir_reference(eps_fn, acp, ts, S.apply, lambda x0, yy, rho: S.prox(x0, yy, float(rho)),
                                    y, init, noise, sigma=sigma)
    assert sampler == "ddrm", sampler
    step = lambda x, e, yy, xi, c: S.ddrm(x, e, yy, xi, dr.round32(c) if dt == torch.float32 else c)  # noqa: E731
    return dr.ddrm_reference(eps_fn, acp, ts, step, y, init, noise, sigma_y=sigma)


def run_sampler(sampler, net, prob, kind, **kw):
    """The sampler on the device, and that it took the fused HIP path of `kind`."""
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler, DPSSampler, PGDMSampler

    if sampler == "dps":
        return DPSSampler(net)(prob, gamma=GAMMA, eta=ETA, **kw)
    if sampler == "pgdm":
        return PGDMSampler(net)(prob, guidance_weight=GUIDANCE, **kw)
    smp = DiffPIRSampler(net) if sampler == "diffpir" else DDRMSampler(net)
    out = smp(prob, **kw)
    if sampler == "diffpir":
        assert not smp.last_step.cg and not smp.last_step.host
    else:
        assert smp.last_step.fused
    assert smp.last_step.desc.kind == kind  # the HIP path ran
    assert len(net.graph_flags) >= 2 and not any(net.graph_flags)  # no network call builds an autograd graph
    return out


def check_trajectory(cuda, record, sampler, kind, prob, y, make_S, shape, n_steps, sigma, recon, what):
    """`sampler` on the device over replayed noise against its plain loop on make_S(dt), under
    `bound_check`'s rule; y holds the host observation rows."""
    B = y.shape[0]
    net, _ = counting_net("conv", shape[0], 0.1, cuda)
    init, steps = si.replay_noise(17, (B * recon, *shape), n_steps)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    ts = si.leading_timesteps_ascending(n_steps).tolist()
    yr = y.repeat_interleave(recon, dim=0)

    def loop(dt):
        core = si.EpsCore("conv", shape[0], 0.1).to(dt)
        return reference_loop(sampler, make_S(dt), lambda x, tt: core(x, tt), acp(dt), ts, yr, init,
                              lambda i: steps[i].to(dt), dt, sigma)

    out = run_sampler(sampler, net, prob, kind, num_sampling_steps=n_steps, num_reconstructions=recon, noise_fn=fn,
                      micro_batch=2 if recon == 2 else None)
    assert tuple(out.shape) == ((B, *shape) if recon == 1 else (B, recon, *shape))
    bound_check(out, loop, what, record)


def check_fused_path_and_reproduce(net, prob, rows, kind, n_steps, expect_q):
    """Every sampler's step on the kind's descriptor (`expect_q`: the DDRM step holds a prepared q),
    and the seeded samplers: the same seed bit for bit, another seed not, micro_batch=1 bit for bit.
    Returns the steps it built, for what a kind has to say about them."""
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler, DPSSampler, PGDMSampler
    from samplers_amd.samplers.ddrm import FusedDDRMStep
    from samplers_amd.samplers.diffpir import FusedDiffPIRStep
    from samplers_amd.samplers.dps import FusedDPSStep, make_dps_step

    steps = {"ddrm": FusedDDRMStep(net, prob, rows, 1)}
    assert steps["ddrm"].fused and (steps["ddrm"].q is not None) == expect_q and steps["ddrm"].desc.kind == kind
    for mode in ("closed_form", "auto"):
        steps[mode] = st = FusedDiffPIRStep(net, prob, rows, 1, prox=mode)
        assert not st.cg and st.desc.kind == kind
    assert FusedDiffPIRStep(net, prob, rows, 1, prox="cg").cg
    for mode in ("dps", "pgdm"):  # DPS and PGDM: the fused step on the kind's descriptor, q for PGDM
        steps[mode] = st = make_dps_step(net, prob, rows, 1, mode=mode)
        assert isinstance(st, FusedDPSStep) and st.desc.kind == kind
        assert st.needs_v and (st.q is not None) == (mode == "pgdm")
    for cls in (DPSSampler, PGDMSampler, DDRMSampler, DiffPIRSampler):
        one = cls(net)(prob, num_sampling_steps=n_steps, seed=1234)
        assert torch.equal(cls(net)(prob, num_sampling_steps=n_steps, seed=1234), one) and torch.isfinite(one).all()
        assert not torch.equal(cls(net)(prob, num_sampling_steps=n_steps, seed=1235), one)
        assert torch.equal(cls(net)(prob, num_sampling_steps=n_steps, seed=1234, micro_batch=1), one)
    # conjugate gradients run through the kind's maps (their agreement with the closed form is
    # test_conjugate_gradients_reach_the_closed_form's)
    out = DiffPIRSampler(net)(prob, num_sampling_steps=n_steps, seed=3, prox="cg", cg_iterations=8)
    assert torch.isfinite(out).all() and tuple(out.shape) == tuple(one.shape)
    return steps


# --- host_sampler_checks: the samplers on host tensors are the plain loops --------------------------------
HOST_STEPS, HOST_CG_ITERATIONS = 6, 16


def _host_noise(y, shape, recon):
    init, steps = si.replay_noise(21, (y.shape[0] * recon, *shape), HOST_STEPS)
    return init, steps, lambda kind, i, sh: init.clone() if kind == "init" else steps[i]


def _host_loop(sampler, make_S, y, shape, sigma, recon, init, steps):
    def run(dt):
        core = si.EpsCore("conv", shape[0], 0.1).to(dt)
        return reference_loop(sampler, make_S(dt), lambda x, tt: core(x, tt), acp(dt),
                              si.leading_timesteps_ascending(HOST_STEPS).tolist(), y.repeat_interleave(recon, dim=0),
                              init, lambda i: steps[i].to(dt), dt, sigma)
    return run


def host_ddrm_check(op, S64, y, shape, sigma, recon):
    """DDRMSampler on host tensors (ddrm_step_svd through the host maps) against the fp64 loop on S64."""
    from samplers_amd.samplers import DDRMSampler

    N, B = HOST_STEPS, y.shape[0]
    net, calls = counting_net("conv", shape[0], 0.1)
    init, steps, fn = _host_noise(y, shape, recon)
    smp = DDRMSampler(net)
    out = smp(InverseProblem(op, y, GaussianNoise(sigma)), num_sampling_steps=N, num_reconstructions=recon,
              noise_fn=fn, micro_batch=2 if recon == 2 else None)
    assert not smp.last_step.fused
    assert tuple(out.shape) == ((B, *shape) if recon == 1 else (B, recon, *shape))
    assert len(calls) >= N - 1 and not any(calls)  # every network call under no_grad
    ref = _host_loop("ddrm", lambda dt: S64, y, shape, sigma, recon, init, steps)(torch.float64)
    err = si.relative_error(out.reshape(ref.shape), ref)
    print(f"host DDRM C={shape[0]} R={recon}: rel l2 {err:.3g}")
    assert err <= 1e-4  # fp32 plain torch against the fp64 loop over N - 2 steps


def host_refusals(op, y, shape, sigma):
    """DPS has no host form (its fused step needs a device), and the host DDRM path draws no
    Philox noise."""
    from samplers_amd.samplers import DDRMSampler, DPSSampler

    net = si.make_samplers_amd_net("conv", shape[0], 0.1)
    with pytest.raises(_hip.HipLibraryError):
        DPSSampler(net)(InverseProblem(op, y, GaussianNoise(sigma)), num_sampling_steps=4)
    with pytest.raises((ValueError, _hip.HipLibraryError)):
        DDRMSampler(net)(InverseProblem(op, y, GaussianNoise(sigma)), num_sampling_steps=4, seed=1)


def host_pgdm_check(op, make_S, y, shape, sigma, recon):
    from samplers_amd.samplers import PGDMSampler

    B = y.shape[0]
    net = si.make_samplers_amd_net("conv", shape[0], 0.1)
    init, steps, fn = _host_noise(y, shape, recon)
    out = PGDMSampler(net)(InverseProblem(op, y, GaussianNoise(sigma)), num_sampling_steps=HOST_STEPS,
                           num_reconstructions=recon, guidance_weight=GUIDANCE, noise_fn=fn,
                           micro_batch=2 if recon == 2 else None)
    assert tuple(out.shape) == ((B, *shape) if recon == 1 else (B, recon, *shape))
    ref, bound = loop_bound(_host_loop("pgdm", make_S, y, shape, sigma, recon, init, steps))
    err = si.relative_error(out.reshape(ref.shape), ref)
    print(f"host PGDM R={recon}: rel l2 {err:.3g} bound {bound:.3g}")
    assert err <= bound


def host_diffpir_check(op, make_S, y, shape, sigma, prox, tol):
    """DiffPIRSampler on host tensors against the plain loop with make_S(dt).prox as its data step;
    returns the sampler."""
    from samplers_amd.samplers import DiffPIRSampler

    N, B = HOST_STEPS, y.shape[0]
    net, calls = counting_net("conv", shape[0], 0.1)
    init, steps, fn = _host_noise(y, shape, 1)
    sampler = DiffPIRSampler(net)
    out = sampler(InverseProblem(op, y, GaussianNoise(sigma)), num_sampling_steps=N, noise_fn=fn, prox=prox,
                  cg_iterations=HOST_CG_ITERATIONS, cg_tol=tol)
    assert sampler.last_step.host and len(calls) >= N - 1 and not any(calls)  # every network call under no_grad
    if prox == "cg":
        assert tuple(sampler.last_step.iterations.shape) == (N - 2, B)
    ref, bound = loop_bound(_host_loop("diffpir", make_S, y, shape, sigma, 1, init, steps))
    err = si.relative_error(out.reshape(ref.shape), ref)
    print(f"host DiffPIR {prox}: rel l2 {err:.3g} bound {bound:.3g}")
    assert err <= bound
    return sampler


# --- the debug-library child --------------------------------------------------------------------------------
def DEBUG_SWEEP_CHILD(module_name):
    """The child's script for a test module whose `debug_sweep(device)` asserts per case."""
    return f"""
import sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from samplers_amd import _hip
assert _hip.load_library().sp_debug_build() == 1, "not the debug library"
import {module_name} as T
_hip.debug_violations()  # clear
T.debug_sweep(torch.device("cuda:0"))
print("debug build: clean", flush=True)
"""


def run_debug_child(script, timeout=240):
    """`script` in a fresh child process under the bounds-checked library (a process holds one
    library); it has to end clean and print the marker."""
    if not _hip.DEBUG_LIB_PATH.exists():
        pytest.fail(f"{_hip.DEBUG_LIB_PATH} missing: run `make` (builds the debug library too)")
    env = dict(os.environ, SAMPLERS_HIP_LIB=str(_hip.DEBUG_LIB_PATH))
    out = subprocess.run([sys.executable, "-c", script, str(ROOT)], env=env,
                         capture_output=True, text=True, timeout=timeout)
    print(out.stdout[-4000:], out.stderr[-4000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build: clean" in out.stdout
