"""The channel-mixing kind (SP_OP_CHANNEL_MIX, csrc/sp_chanmix.hip) on the GPU, through the raw entry
points into NaN-filled outputs between guard bands (the kind takes no workspace: every `work` is
NULL): A, Aᵀ, A⁺, A⁺ᵀ, DPS pass 1, PGDM pass 1, the proximal map, the DiffPIR step and the DDRM step
against the fp64 evaluation of tests/chanmix_ref.py, every case at (batch 3, y_div 3) and
(batch 4, y_div 2).

Bounds.  Exact cases (dyadic tables, integer data in [−3, 3], dyadic scalars: tests/test_chanmix_ref.py
shows that the fp32 evaluation does not round): bit for bit.  ``randn`` data, per element:
``|err| ≤ n_r · 2⁻²⁴ · E`` with E the same pass on absolute values with absolute tables and n_r the
roundings of the pass's longest path (``chanmix_ref.roundings``); ‖r‖² relative to its own envelope.
The compositions from the device maps, ``sp_predict_x0`` and ``sp_randn`` are held to the same
bounds.  Conjugate gradients against the closed form: max(2e-5, 4 × the CPU fp32 emulation's own
distance) × max|ref| (the rule of tests/test_prox_cg_gpu.py).  Trajectories: max(1e-4, 20 × the fp32
reference loop's distance to its fp64 run); PSLD 1e-4 (tests/test_superres_gpu.py).

Largest errors measured on an MI355X are recorded in README.md ("Channel-mixing operator")."""

import numpy as np
import pytest
import torch

import chanmix_ref as cr
import ddrm_ref as dr
import stand_ins as si
from kind_harness import (DDRM, DEBUG_SWEEP_CHILD, DPS, PROX, KindDevice, acp as _acp,
                          check_fused_path_and_reproduce, check_guards, check_trajectory, counting_net,
                          f32 as _f32, guarded, rounding_check as _check, run_debug_child, stream as _stream)
from oracle.latent_loops import psld_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import ChannelMixOperator, IdentityOperator

pytestmark = pytest.mark.gpu

CASE_IDS = [c[0] for c in cr.CASES]
FORMS = [(i, f) for i in range(len(cr.CASES)) for f in cr.FORMS]
FORM_IDS = [f"{CASE_IDS[i]}-b{f[0]}-d{f[1]}" for i, f in FORMS]


# --- a descriptor on the device -----------------------------------------------------------------------------
class Dev(KindDevice):
    """The tables on the device and the descriptor.  The kind takes no workspace (every `work` is
    NULL), its maps run through the plain entry points, and every pass reads the observation rows."""

    TRAITS = _hip.SP_TRAIT_LINEAR | _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_NEEDS_ATA_U | _hip.SP_TRAIT_PINV
    WORKSPACE_FORMS = False

    def __init__(self, shape, tab32, device, name=""):
        self.C, self.Cy, self.H, self.W = self.shape = shape
        self.hw = self.H * self.W
        self.taps = torch.from_numpy(cr.flat_tables(tab32)).to(device)
        assert self.taps.numel() == 2 * self.C * self.Cy + self.Cy ** 2 + self.C ** 2 + 2 * self.Cy
        s = _hip.SpOp()
        s.kind, s.channels, s.height, s.width = _hip.SP_OP_CHANNEL_MIX, self.C, self.H, self.W
        s.n, s.m, s.radius, s.factor = self.C * self.hw, self.Cy * self.hw, self.Cy, 0
        s.taps = self.taps.data_ptr()
        super().__init__(device, s, (self.C, self.H, self.W), (self.Cy, self.H, self.W), name)
        for size in (self.lib.sp_op_workspace, self.lib.sp_dps_workspace, self.lib.sp_prox_workspace,
                     self.lib.sp_ddrm_workspace, self.lib.sp_prox_prepare_size):
            assert size(s, 4) == 0

    def check_workspace(self, floats, batch):
        assert floats == 0

    def partials(self):
        return cr.partials(self.shape)

    def pgdm(self, x, eps, y, ydiv, c):
        """The observation rows themselves are the q of the pass; sp_pgdm_prepare writes nothing."""
        qwhole, q = guarded(4, self.device)
        assert self.lib.sp_pgdm_prepare(self.desc, y.data_ptr(), y.shape[0], q.data_ptr(), _stream()) == 0
        out = super().pgdm(x, eps, y, ydiv, c)
        assert torch.isnan(qwhole).all()
        return out

    def prox(self, x0, y, ydiv, rho):
        assert self.lib.sp_prox_prepare(self.desc, y.data_ptr(), y.shape[0], None, _stream()) == 0
        return super().prox(x0, y, ydiv, rho)

    def prox_cg(self, x0, y, ydiv, rho, iters=64, tol=1e-6):
        b = x0.shape[0]
        floats = int(self.lib.sp_prox_cg_workspace(self.desc, b, 0))
        assert floats > 0
        wwhole, work = guarded(floats, self.device)
        it = torch.full((b,), -1, dtype=torch.int32, device=self.device)
        out = self._run(self.lib.sp_op_workspace, b, (b, *self.xs), lambda o, w: self.lib.sp_op_prox_cg_ws(
            self.desc, x0.data_ptr(), y.data_ptr(), b, ydiv, rho, iters, tol, o.data_ptr(), it.data_ptr(),
            work.data_ptr(), _stream()))
        check_guards(wwhole, floats)
        return out, it


def _dev(i, device):
    name, shape, tab, _ = cr.case(i)
    t32 = cr.round32(tab)
    return Dev(shape, t32, device, name), cr.Mix(shape, t32), t32


_DATA = {}


def _randn_case(i):
    """randn inputs for the largest batch of the case; computed once, never modified."""
    if i not in _DATA:
        c, cy, h, w = cr.CASES[i][1]
        g = torch.Generator().manual_seed(300 + i)
        x, eps, xi = (torch.randn(4, c, h, w, generator=g) for _ in range(3))
        _DATA[i] = (x, eps, xi, torch.randn(2, cy, h, w, generator=g))
    return _DATA[i]


def test_tile_counts():
    """The vector case of several tiles with a partial last one, and the ragged scalar case."""
    lib = _hip.load_library()
    assert cr.partials(cr.CASES[6][1]) == 3 and cr.CASES[6][1][2:] == (64, 36)   # 576 groups of 4: 256 + 256 + 64
    assert cr.partials(cr.CASES[3][1]) == 5 and cr.CASES[3][1][2:] == (33, 35)   # 1155 pixels: 4 x 256 + 131
    assert lib.sp_version() >= 115


# --- exact cases: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cr.FORMS, ids=[f"b{f[0]}-d{f[1]}" for f in cr.FORMS])
@pytest.mark.parametrize("name,shape,tab,passes", cr.EXACT_CASES, ids=[c[0] for c in cr.EXACT_CASES])
def test_exact_cases_are_bitwise(cuda, name, shape, tab, passes, form):
    batch, ydiv = form
    t32 = cr.round32(tab)
    d, S = Dev(shape, t32, cuda, name), cr.Mix(shape, t32)
    x, eps, xi, y = cr.exact_data(shape, batch, ydiv)
    ye = cr.expand(y, batch, ydiv)
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    e, px = cr.EXACT_DPS, cr.EXACT_PROX
    v, part = d.dps(xd, ed, yd, ydiv, e)
    got = {"apply": d.apply(xd), "adjoint": d.adjoint(yed), "pinv": d.pinv(yed), "pinv_t": d.pinv(xd, 1), "dps": v,
           "pgdm": d.pgdm(xd, ed, yd, ydiv, dict(e, gs=-2.0)), "prox": d.prox(xd, yd, ydiv, px["rho"]),
           "diffpir": d.diffpir(xd, ed, yd, xid, ydiv, px)}
    for regime in ("big", "small"):
        got["ddrm"] = d.ddrm(xd, ed, yd, xid, ydiv, cr.EXACT_DDRM[regime])
        want = cr.run_passes(S, x.double(), eps.double(), ye.double(), xi.double(), regime)
        for key in passes:
            assert torch.equal(got[key].cpu().double(), want[key]), (name, key, regime)
    rsq = S.dps(x.double(), eps.double(), ye.double(), e["a"], e["k"], e["gs"])[1]
    assert torch.equal(part.double().sum(1).cpu(), rsq)  # sums of small dyadic numbers: no rounding


# --- every pass under the bound ----------------------------------------------------------------------------
@pytest.mark.parametrize("i,form", FORMS, ids=FORM_IDS)
def test_every_pass_against_fp64(cuda, parity_record, i, form):
    batch, ydiv = form
    d, S, t32 = _dev(i, cuda)
    shape = cr.CASES[i][1]
    x, eps, xi, y = _randn_case(i)
    x, eps, xi, y = x[:batch], eps[:batch], xi[:batch], y[: -(-batch // ydiv)]
    ye = cr.expand(y, batch, ydiv)
    nr = lambda what: cr.roundings(what, d.C, d.Cy)  # noqa: E731
    env = lambda what, **kw: cr.envelope(shape, t32, what, **kw)  # noqa: E731
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    x6, e6, n6, y6 = x.double(), eps.double(), xi.double(), ye.double()
    rec = parity_record
    _check(d.apply(xd), S.apply(x6), env("apply", x=x), nr("apply"), "apply", rec)
    _check(d.adjoint(yed), S.adjoint(y6), env("adjoint", y=ye), nr("adjoint"), "adjoint", rec)
    _check(d.pinv(yed), S.pinv(y6), env("pinv", y=ye), nr("pinv"), "pinv", rec)
    _check(d.pinv(xd, 1), S.pinv_t(x6), env("pinv_t", x=x), nr("pinv_t"), "pinv_t", rec)
    # DPS pass 1, its _sched form and its composition from the maps
    c = _f32(DPS)
    v, part = d.dps(xd, ed, yd, ydiv, c)
    v64, rsq64 = S.dps(x6, e6, y6, c["a"], c["k"], c["gs"])
    envd = env("dps", x=x, eps=eps, y=ye, c=c)
    _check(v, v64, envd, nr("dps"), "dps_v", rec)
    ratio = float(((part.double().sum(1).cpu() - rsq64).abs()
                   / (nr("rsq") * cr.U24 * env("rsq", x=x, eps=eps, y=ye, c=c))).max())
    rec("dps_rsq_err_over_bound", ratio, 1.0)
    assert ratio <= 1.0, ("rsq", ratio)
    vs, parts = d.dps(xd, ed, yd, ydiv, c, sched=True)
    assert torch.equal(vs, v) and torch.equal(parts, part)
    x0d = d.x0(xd, ed, c["a"], c["k"])
    comp = d.adjoint((c["gs"] * (yed - d.apply(x0d))).contiguous())
    _check(comp, v64, envd, nr("dps"), "dps_v_composed", rec)
    # PGDM pass 1 against fp64 and against -2 A^+ (y - A x0) from the maps
    cp = dict(c, gs=-2.0)
    p64, envp = S.pgdm(x6, e6, y6, cp["a"], cp["k"], cp["gs"]), env("pgdm", x=x, eps=eps, y=ye, c=cp)
    _check(d.pgdm(xd, ed, yd, ydiv, cp), p64, envp, nr("pgdm"), "pgdm_v", rec)
    comp = -2.0 * d.pinv((yed - d.apply(x0d)).contiguous())
    _check(comp, p64, envp, nr("pgdm"), "pgdm_v_composed", rec)
    # the proximal map and the DiffPIR step (xi given), and their composition
    px = _f32(PROX)
    for rho in (1e-4, px["rho"], 50.0):
        rho = float(np.float32(rho))
        _check(d.prox(xd, yd, ydiv, rho), S.prox(x6, y6, rho), env("prox", x=x, y=ye, c=dict(rho=rho)),
               nr("prox"), f"prox_rho{rho:.3g}", rec)
    s64, envs = S.diffpir(x6, e6, y6, n6, px), env("diffpir", x=x, eps=eps, y=ye, xi=xi, c=px)
    _check(d.diffpir(xd, ed, yd, xid, ydiv, px), s64, envs, nr("diffpir"), "diffpir", rec)
    z = d.prox(d.x0(xd, ed, px["a"], px["k"]), yd, ydiv, px["rho"])
    comp = px["a_prev"] * z + (px["c_eps"] * ((xd - px["a"] * z) / px["k"]) + px["c_xi"] * xid)
    _check(comp, s64, envs, nr("diffpir"), "diffpir_composed", rec)
    # DDRM in the DDRM suite's scalar regimes (the reference is given the fp32 class mask), and its
    # composition from the maps in the blend regime: x' = a' [x0 + c1 s' eps + eta s' xi + A^+(...)]
    for regime, cc in DDRM.items():
        cc = dr.round32(cc)
        big = cr.big_mask32(t32, cc)
        r64 = S.ddrm(x6, e6, y6, n6, cc, big=big)
        envr = env("ddrm", x=x, eps=eps, y=ye, xi=xi, c=cc, big=big)
        _check(d.ddrm(xd, ed, yd, xid, ydiv, cc), r64, envr, nr("ddrm"), f"ddrm_{regime}", rec)
    drawn = d.randn(batch)
    cc = dr.round32(DDRM["blend"])
    big = cr.big_mask32(t32, cc)
    r64 = S.ddrm(x6, e6, y6, drawn.cpu().double(), cc, big=big)
    envr = env("ddrm", x=x, eps=eps, y=ye, xi=drawn.cpu(), c=cc, big=big)
    fused = d.ddrm(xd, ed, yd, None, ydiv, cc)
    _check(fused, r64, envr, nr("ddrm"), "ddrm_philox", rec)
    # The DDRM step composes from the device maps A and A^+ only when every kept component takes
    # the same coefficients (A^+ A is then the one projector involved); components of mixed classes
    # or singular values need V itself, which no device map exposes.  So: the cases with Cy = 1.
    if d.Cy == 1:
        s2 = torch.from_numpy(np.float32(t32["S"] * t32["S"]))
        fo = [float(v) for v in dr.coefficients(s2, torch.tensor([True]), big, cc, torch.float32)]
        fu = [float(v) for v in dr.coefficients(s2, torch.tensor([False]), torch.tensor([False]), cc, torch.float32)]
        x0d = d.x0(xd, ed, cc["a"], cc["k"])
        w = ((fo[0] - fu[0]) * x0d + (fo[1] - fu[1]) * ed) + (fo[3] - fu[3]) * drawn
        comp = cc["a_prev"] * ((x0d + (fu[1] * ed + fu[3] * drawn))
                               + d.pinv((fo[2] * yed + d.apply(w.contiguous())).contiguous()))
        _check(comp, r64, envr, nr("ddrm"), "ddrm_composed", rec)


# --- bitwise properties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=CASE_IDS)
def test_bitwise_properties(cuda, i):
    d, _, _ = _dev(i, cuda)
    x, eps, xi, y = _randn_case(i)
    xd, ed, xid, yd = (v.to(cuda).contiguous() for v in (x, eps, xi, y))
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])

    def passes(xs, es, xis, ys, ydiv, alias=False):
        v, part = d.dps(xs, es, ys, ydiv, c)
        vs, parts = d.dps(xs, es, ys, ydiv, c, sched=True)
        ax = d.apply(xs)
        return {"A": ax, "AT": d.adjoint(ax), "N": d.pinv(ax), "NT": d.pinv(xs, 1), "v": v, "part": part,
                "v_sched": vs, "part_sched": parts, "pgdm": d.pgdm(xs, es, ys, ydiv, dict(c, gs=-2.0)),
                "prox": d.prox(xs, ys, ydiv, px["rho"]),
                "diffpir": d.diffpir(xs, es, ys, xis, ydiv, px, alias=alias),
                "ddrm": d.ddrm(xs, es, ys, xis, ydiv, cc, alias=alias)}

    one = passes(xd, ed, xid, yd, 2)
    two = passes(xd, ed, xid, yd, 2, alias=True)          # the same bits twice, and x_out = x
    for key in one:
        assert torch.equal(one[key], two[key]), key
    assert torch.equal(one["v"], one["v_sched"]) and torch.equal(one["part"], one["part_sched"])
    # a sample alone against the batch of 4 (sample 3 reads observation row 1)
    alone = passes(xd[3:], ed[3:], xid[3:], yd[1:], 1)
    for key in one:
        assert torch.equal(alone[key], one[key][3:]), key
    # y_div = 2 against repeated rows
    rows = passes(xd, ed, xid, cr.expand(y, 4, 2).to(cuda).contiguous(), 1)
    for key in one:
        assert torch.equal(rows[key], one[key]), key
    # xi = NULL draws sp_randn's plane
    drawn = d.randn(4)
    given = passes(xd, ed, drawn, yd, 2)
    null = passes(xd, ed, None, yd, 2)
    for key in ("diffpir", "ddrm"):
        assert torch.equal(given[key], null[key]), key
        assert not torch.equal(null[key], one[key])


# --- cross-checks against existing kinds ------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (8, 12)], ids=["scalar", "vector"])
def test_identity_matrix_is_the_identity_kind(cuda, hw):
    """M = I₃: A is a copy and DPS v has the identity kind's bits (adding a product by 0 is exact)."""
    shape = (3, 3, *hw)
    d = Dev(shape, cr.round32(cr.svd_tables(np.eye(3))), cuda)
    ident = IdentityOperator((3, *hw)).hip_descriptor()
    g = torch.Generator().manual_seed(8)
    x, eps, y = (torch.randn(4, 3, *hw, generator=g).to(cuda) for _ in range(3))
    assert torch.equal(d.apply(x), x) and torch.equal(d.adjoint(x), x)
    c = _f32(DPS)
    v, part = d.dps(x, eps, y[:2], 2, c)
    lib = d.lib
    P = int(lib.sp_rsq_partials(ident))
    vi, pi = torch.empty_like(x), torch.empty(4, P, device=cuda)
    coefs = _hip.SpDpsCoefs(c["a"], c["k"], c["gs"], 0.9, 0.2, 0.1, 0.05, 1e-9)
    _hip.check(lib.sp_dps_residual(ident, x.data_ptr(), eps.data_ptr(), y[:2].data_ptr(), 4, 2, coefs,
                                   vi.data_ptr(), pi.data_ptr(), _stream()), "identity residual")
    assert torch.equal(v, vi)
    assert float((part.double().sum(1) / pi.double().sum(1) - 1).abs().max()) <= 64 * cr.U24


@pytest.mark.parametrize("i", [1, 3, 4, 7], ids=[CASE_IDS[i] for i in (1, 3, 4, 7)])
def test_conjugate_gradients_reach_the_closed_form(cuda, parity_record, i):
    """sp_op_prox_cg_ws (K = 64, tol 1e-6) through the kind's apply / adjoint against sp_op_prox_ws,
    under max(2e-5, 4 x the CPU fp32 emulation's own distance to fp64) x max|ref|."""
    d, S, t32 = _dev(i, cuda)
    x, _, _, y = _randn_case(i)
    emu = cr.Emu(cr.CASES[i][1], t32)
    for batch, ydiv in cr.FORMS:
        x0, yy = x[:batch], y[: -(-batch // ydiv)]
        ye = cr.expand(yy, batch, ydiv)
        for rho in (1e-2, 1.0):
            rho = float(np.float32(rho))
            ref = S.prox(x0.double(), ye.double(), rho)
            scale = float(ref.abs().max())
            z32 = emu.prox(x0.reshape(batch, -1).numpy(), ye.reshape(batch, -1).numpy(), rho)
            yard = float(np.abs(z32.astype(np.float64) - ref.reshape(batch, -1).numpy()).max()) / scale
            closed = d.prox(x0.to(cuda), yy.to(cuda), ydiv, rho)
            z, it = d.prox_cg(x0.to(cuda), yy.to(cuda), ydiv, rho)
            err = float((z - closed).abs().max()) / scale
            bound = max(2e-5, 4 * yard)
            print(f"{d.name} rho={rho:g} b{batch}: cg to closed form {err:.3g} emulation {yard:.3g} "
                  f"bound {bound:.3g} iters {it.tolist()}")
            parity_record("cg_to_closed_form_max_err_over_max", err, bound, rho=rho, emulation=yard)
            assert err <= bound and 1 <= int(it.min()) and int(it.max()) < 64


def test_autograd_of_the_four_device_maps(cuda):
    name, shape, tab, rtol = cr.case(7)
    xs = (shape[0], *shape[2:])
    op = ChannelMixOperator(xs, cr.CASES[7][2], rtol=rtol).to(cuda)
    host = ChannelMixOperator(xs, cr.CASES[7][2], rtol=rtol)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, *xs, generator=g)
    y = torch.randn(3, *op.y_shape, generator=g)
    xd, yd = x.to(cuda), y.to(cuda)
    ax, aty, py, ptx = op.apply(xd), op.apply_transpose(yd), op.apply_pseudo_inverse(yd), op.apply_pseudo_inverse_transpose(xd)
    assert tuple(ax.shape) == (3, *op.y_shape) and tuple(py.shape) == (3, *xs)
    for fn, arg, cot, want in ((op.apply, xd, yd, aty), (op.apply_transpose, yd, xd, ax),
                               (op.apply_pseudo_inverse, yd, xd, ptx), (op.apply_pseudo_inverse_transpose, xd, yd, py)):
        r = arg.clone().requires_grad_()
        (gr,) = torch.autograd.grad(fn(r), r, grad_outputs=cot)
        assert torch.equal(gr, want)  # the backward of a map is its transpose: the same launch
    t32 = dict(M=host.matrix.numpy(), N=host.pinv_matrix.numpy(), U=host.U.numpy(), V=host.V.numpy(),
               S=host.singular_values_full.numpy(), P=host.pinv_multiplier.numpy())
    env = lambda what, **kw: cr.envelope(shape, t32, what, **kw)  # noqa: E731
    nr = lambda what: cr.roundings(what, shape[0], shape[1])  # noqa: E731
    for got, want, what, kw in ((ax, host.apply(x.double()), "apply", dict(x=x)),
                                (aty, host.apply_transpose(y.double()), "adjoint", dict(y=y)),
                                (py, host.apply_pseudo_inverse(y.double()), "pinv", dict(y=y)),
                                (ptx, host.apply_pseudo_inverse_transpose(x.double()), "pinv_t", dict(x=x))):
        _check(got, want, env(what, **kw), nr(what), f"operator_{what}")
    z = op.apply_prox(xd, yd, 0.3)
    _check(z, host.apply_prox(x.double(), y.double(), 0.3), env("prox", x=x, y=y, c=dict(rho=0.3)), nr("prox"),
           "operator_prox")
    assert tuple(op.apply(xd.reshape(1, 3, *xs)).shape) == (1, 3, *op.y_shape)  # leading batch dimensions


# --- trajectories ---------------------------------------------------------------------------------------------
SHAPE, B, N, SIGMA = (3, 32, 32), 2, 8, 0.05
FULL = (3, 1, 32, 32)


def _tables_of(op):
    return dict(M=op.matrix.numpy(), N=op.pinv_matrix.numpy(), U=op.U.numpy(), V=op.V.numpy(),
                S=op.singular_values_full.numpy(), P=op.pinv_multiplier.numpy())


def _traj(weights, cuda):
    host = ChannelMixOperator.colorization(SHAPE, weights)
    g = torch.Generator().manual_seed(41)
    x_true = si.fixture_x_true(B, SHAPE, seed=9)
    y = cr.Mix(FULL, _tables_of(host)).apply(x_true.double()).float()
    y = y + SIGMA * torch.randn(y.shape, generator=g)
    op = ChannelMixOperator.colorization(SHAPE, weights).to(cuda)
    return op, _tables_of(host), y, InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))


@pytest.mark.parametrize("recon", [1, 2])
@pytest.mark.parametrize("weights", ["mean", "luma"])
@pytest.mark.parametrize("sampler", ["dps", "pgdm", "diffpir", "ddrm"])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, sampler, weights, recon):
    op, tab, y, prob = _traj(weights, cuda)
    check_trajectory(cuda, parity_record, sampler, _hip.SP_OP_CHANNEL_MIX, prob, y,
                     lambda dt: cr.Mix(FULL, tab, dtype=dt), SHAPE, N, SIGMA, recon, f"{sampler}_{weights}_R{recon}")


def test_psld_matches_the_reference_loop(cuda, parity_record):
    """PSLD takes the maps-plus-cotangent route (no fused-latent trait), as the Gaussian blur does."""
    from samplers_amd.samplers.psld import FusedPSLDStep, PSLDSampler

    op, tab, y, prob = _traj("luma", cuda)
    net = si.make_samplers_amd_latent_net("conv", 0.1, device=cuda)
    lat = net.get_latent_shape(SHAPE)
    n_steps = 6
    init, steps = si.replay_noise(13, (B, *lat), n_steps)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    step = FusedPSLDStep(net, prob, y.to(cuda), 1, lat)
    assert step.blur and not step.generic
    out = PSLDSampler(net)(prob, num_sampling_steps=n_steps, noise_fn=fn)
    core, vae, S = si.EpsCore("conv", 4, 0.1), si.LatentCore(), cr.Mix(FULL, tab, dtype=torch.float32)
    ref = psld_reference(lambda x, t: core(x, t), _acp(), si.leading_timesteps_ascending(n_steps).tolist(),
                         S.apply, S.adjoint, vae.decode, vae.encode, y, init, lambda i: steps[i])
    err = si.relative_error(out.cpu(), ref)
    print("psld channel mix", err)
    parity_record("psld_rel_l2", err, 1e-4)
    assert err < 1e-4


def test_samplers_take_the_fused_path_and_reproduce(cuda):
    op, _, y, prob = _traj("mean", cuda)
    net, _ = counting_net("conv", 3, 0.1, cuda)
    steps = check_fused_path_and_reproduce(net, prob, y.to(cuda), _hip.SP_OP_CHANNEL_MIX, N, expect_q=False)
    assert steps["closed_form"].q is None and steps["auto"].q is None
    assert steps["pgdm"].q.data_ptr() == steps["pgdm"].y.data_ptr()  # the observation rows themselves: no copy of y


# --- the bounds-checked library ------------------------------------------------------------------------------
def debug_sweep(device):
    """Every pass over every shape of this file; run by the child process under the debug library."""
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])
    cases = [(cr.CASES[i][0], cr.CASES[i][1], cr.round32(cr.case(i)[2])) for i in range(len(cr.CASES))]
    cases += [(n, s, cr.round32(t)) for n, s, t, _ in cr.EXACT_CASES]
    for name, shape, t32 in cases:
        d = Dev(shape, t32, device, name)
        for batch, ydiv in cr.FORMS:
            g = torch.Generator().manual_seed(1)
            x, eps, xi = (torch.randn(batch, *d.xs, generator=g).to(device) for _ in range(3))
            y = torch.randn(-(-batch // ydiv), *d.ys, generator=g).to(device)
            ye = cr.expand(y, batch, ydiv).contiguous()
            d.apply(x), d.adjoint(ye), d.pinv(ye), d.pinv(x, 1)
            d.dps(x, eps, y, ydiv, c), d.dps(x, eps, y, ydiv, c, sched=True)
            d.pgdm(x, eps, y, ydiv, c), d.prox(x, y, ydiv, px["rho"])
            for noise in (xi, None):
                d.diffpir(x, eps, y, noise, ydiv, px), d.ddrm(x, eps, y, noise, ydiv, cc)
        nv, site = _hip.debug_violations()
        print(name, "violations", nv, site, flush=True)
        assert nv == 0, (name, nv, site)


DEBUG_CHILD = DEBUG_SWEEP_CHILD("test_chanmix_gpu")


def test_debug_build_has_no_violations(cuda):
    """The kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh child
    process (a process holds one library), over every shape of this file."""
    run_debug_child(DEBUG_CHILD)
