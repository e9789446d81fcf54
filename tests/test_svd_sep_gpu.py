"""The separable-SVD kind (SP_OP_SVD_SEPARABLE, csrc/sp_svd_sep.hip) on the GPU, through the raw entry
points into NaN-filled outputs and a NaN-filled workspace between guard bands: A, Aᵀ, A⁺, A⁺ᵀ, DPS
pass 1, PGDM pass 1, the proximal map, the DiffPIR step and the DDRM step against the fp64
evaluation of tests/svd_sep_ref.py on the same fp32 tables, every case at (batch 3, y_div 3) and
(batch 4, y_div 2).

Bounds.  Exact cases (Hadamard tables, dyadic scalars, integer data: tests/test_svd_sep_ref.py shows
that no fp32 evaluation order rounds): bit for bit.  Every other case: max(2e-5, 4 x the distance of
the fp32 ``torch.matmul`` evaluation of the same pass to fp64) x max|ref|, the project's rule for its
transform kinds; ||r||^2 relative under the same rule.  Trajectories: max(1e-4, 20 x the fp32
reference loop's distance to its fp64 run).

Largest errors measured on an MI355X are recorded in README.md ("Separable-SVD operator")."""

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import stand_ins as si
import svd_sep_ref as sr
from kind_harness import (DDRM, DEBUG_SWEEP_CHILD, DPS, PROX, KindDevice, check_fused_path_and_reproduce,
                          check_trajectory, counting_net, f32 as _f32, run_debug_child)
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import GaussianBlurOperator, SeparableSVDOperator
from samplers_amd.operators.base import _host_prox_cg

pytestmark = pytest.mark.gpu

FLOOR = 2e-5
FACTOR_IDS = [c[0] for c in sr.FACTOR_CASES]
EXACT_IDS = [c[0] for c in sr.EXACT_CASES]
FORM_IDS = [f"b{b}-d{d}" for b, d in sr.BATCH_FORMS]


# --- a descriptor on the device -----------------------------------------------------------------------------
class Dev(KindDevice):
    """The tables on the device and the descriptor; the prox and DDRM each read a prepared q."""

    TRAITS = _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_PINV
    Q_PASSES = frozenset({"prox", "ddrm"})

    def __init__(self, t: sr.Tables, C: int, device):
        self.t, self.C = t, C
        self.H, self.W, self.Hy, self.Wy = t.dims
        self.tables = t.flat32().to(device)
        d = _hip.SpOp()
        d.kind, d.channels, d.height, d.width = _hip.SP_OP_SVD_SEPARABLE, C, self.H, self.W
        d.n, d.m, d.radius, d.factor = C * self.H * self.W, C * self.Hy * self.Wy, self.Hy, self.Wy
        d.taps = self.tables.data_ptr()
        super().__init__(device, d, (C, self.H, self.W), (C, self.Hy, self.Wy), "svd_separable")
        self.Q_ROW = 2 * self.n  # P T_y(y) for PGDM / DDRM, S T_y(y) for the prox: m floats of it used

    def check_workspace(self, floats, batch):
        assert floats > 0

    def partials(self):
        return self.C * -(-self.Hy // 64) * -(-self.Wy // 64)

    def check_q(self, q, y):
        assert torch.isfinite(q[:, :self.m]).all()


_FACTOR = {}


def _factor_case(i):
    """The case's operator (host: its fp32 tables define the map), inputs for the larger batch and
    nothing else; computed once, never modified."""
    if i not in _FACTOR:
        name, C, make, rtol, _ = sr.FACTOR_CASES[i]
        ah, aw = make()
        op = SeparableSVDOperator((C, ah.shape[1], aw.shape[1]), ah, aw, rtol=rtol)
        t = sr.Tables.from_flat(op.tables, ah.shape[1], aw.shape[1], ah.shape[0], aw.shape[0])
        g = torch.Generator().manual_seed(300 + i)
        H, W, Hy, Wy = t.dims
        x, eps, xi, cot = (torch.randn(4, C, H, W, generator=g) for _ in range(4))
        y = torch.randn(2, C, Hy, Wy, generator=g)
        _FACTOR[i] = (op, t, (x, eps, xi, cot, y))
    return _FACTOR[i]


def _rows(y, batch, ydiv):
    return y[: -(-batch // ydiv)]


def _expand(y, batch, ydiv):
    return y[torch.arange(batch) // ydiv]


def _check(got, ref64, ref32, what, record=None):
    """max|got - ref64| <= max(2e-5, 4 x max|ref32 - ref64|) x max|ref64|."""
    scale = float(ref64.abs().max())
    yard = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
    bound = max(FLOOR, 4 * yard)
    print(f"{what}: err {err:.3g} fp32 matmul {yard:.3g} bound {bound:.3g}")
    if record is not None:
        record(f"{what}_max_err_over_max", err, bound, fp32_matmul=yard)
    assert err <= bound, (what, err, bound)
    return err


# --- exact cases: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sr.BATCH_FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(sr.EXACT_CASES)), ids=EXACT_IDS)
def test_exact_cases_are_bitwise(cuda, i, form):
    name, C, H, W, bh, bw, amp = sr.EXACT_CASES[i]
    batch, ydiv = form
    t, tp = sr.exact_tables(i), sr.exact_tables(i, prox=True)
    x, eps, xi, y, ye = sr.exact_form(i, batch, ydiv)
    S, Sp = sr.Sep(t), sr.Sep(tp)
    d, dp = Dev(t, C, cuda), Dev(tp, C, cuda)
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    e, px = sr.EXACT_DPS, sr.EXACT_PROX
    x6, e6, xi6, ye6 = x.double(), eps.double(), xi.double(), ye.double()
    eq = lambda got, want, what: (torch.equal(got.cpu().double(), want) or pytest.fail(f"{name} {what}"))  # noqa: E731
    eq(d.apply(xd), S.apply(x6), "A")
    eq(d.adjoint(yed), S.adjoint(ye6), "A^T")
    eq(d.pinv(yed), S.pinv(ye6), "A^+")
    eq(d.pinv(xd, 1), S.pinv_t(x6), "A^+T")
    v, part = d.dps(xd, ed, yd, ydiv, e)
    vref, rsq = S.dps(x6, e6, ye6, e["a"], e["k"], e["gs"])
    eq(v, vref, "DPS v")
    assert float((part.double().sum(1).cpu() / rsq - 1).abs().max()) <= FLOOR
    q = d.prepare(yd)
    eq(q[:, :d.m].reshape(y.shape), S.q_pgdm(y.double()), "q")
    eq(d.pgdm(xd, ed, q, ydiv, dict(e, gs=-e["gs"])), S.pgdm(x6, e6, ye6, e["a"], e["k"], -e["gs"]), "PGDM v")
    qp = dp.prepare(yd, prox=True)
    eq(dp.prox(xd, qp, ydiv, px["rho"]), Sp.prox(x6, ye6, px["rho"]), "prox z")
    eq(dp.diffpir(xd, ed, qp, xid, ydiv, px), Sp.diffpir(x6, e6, ye6, xi6, px), "DiffPIR x'")
    for regime in ("big", "small"):
        c = dr.exact_coefs(regime, 1)
        eq(d.ddrm(xd, ed, q, xid, ydiv, c), S.ddrm(x6, e6, ye6, xi6, c), f"DDRM x' {regime}")


# --- every pass under the bound ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", sr.BATCH_FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("i", range(len(sr.FACTOR_CASES)), ids=FACTOR_IDS)
def test_every_pass_against_fp64(cuda, parity_record, i, form):
    name, C = sr.FACTOR_CASES[i][:2]
    batch, ydiv = form
    op, t, (x, eps, xi, cot, y) = _factor_case(i)
    x, eps, xi = x[:batch], eps[:batch], xi[:batch]
    y = _rows(y, batch, ydiv)
    ye = _expand(y, batch, ydiv)
    S64, S32 = sr.Sep(t), sr.Sep(t, dtype=torch.float32)
    d = Dev(t, C, cuda)
    assert torch.equal(d.tables.cpu(), op.tables)
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    ref = lambda fn, *a: (fn(S64, *[v.double() if torch.is_tensor(v) else v for v in a]),  # noqa: E731
                          fn(S32, *a))
    rec = parity_record
    ax = d.apply(xd)
    _check(ax, *ref(sr.Sep.apply, x), "apply", rec)
    _check(d.adjoint(yed), *ref(sr.Sep.adjoint, ye), "adjoint", rec)
    _check(d.pinv(yed), *ref(sr.Sep.pinv, ye), "pinv", rec)
    _check(d.pinv(xd, 1), *ref(sr.Sep.pinv_t, x), "pinv_transpose", rec)
    # DPS pass 1, its _sched_ws form and its composition from the maps
    c = _f32(DPS)
    v, part = d.dps(xd, ed, yd, ydiv, c)
    (v64, rsq64), (v32, rsq32) = ref(sr.Sep.dps, x, eps, ye, c["a"], c["k"], c["gs"])
    _check(v, v64, v32, "dps_v", rec)
    _check(part.double().sum(1), rsq64, rsq32, "dps_rsq", rec)
    vs, parts = d.dps(xd, ed, yd, ydiv, c, sched=True)
    assert torch.equal(vs, v) and torch.equal(parts, part)
    x0d = d.x0(xd, ed, c["a"], c["k"])
    comp = d.adjoint((c["gs"] * (yed - d.apply(x0d))).contiguous())
    _check(comp, v64, v32, "dps_v_composed", rec)
    # PGDM pass 1 against fp64 and against A^+ y - A^+ A x0
    q = d.prepare(yd)
    cp = dict(c, gs=-2.0)
    vp = d.pgdm(xd, ed, q, ydiv, cp)
    p64, p32 = ref(sr.Sep.pgdm, x, eps, ye, cp["a"], cp["k"], cp["gs"])
    _check(vp, p64, p32, "pgdm_v", rec)
    comp = -2.0 * (d.pinv(yed) - d.pinv(d.apply(x0d)))
    _check(comp, p64, p32, "pgdm_v_composed", rec)
    # the proximal map and the DiffPIR step (xi given), and their composition
    px = _f32(PROX)
    qp = d.prepare(yd, prox=True)
    for rho in (1e-4, px["rho"], 50.0):
        rho = float(np.float32(rho))
        _check(d.prox(xd, qp, ydiv, rho), *ref(sr.Sep.prox, x, ye, rho), f"prox_rho{rho:.3g}", rec)
    xp = d.diffpir(xd, ed, qp, xid, ydiv, px)
    s64, s32 = ref(sr.Sep.diffpir, x, eps, ye, xi, px)
    _check(xp, s64, s32, "diffpir", rec)
    z = d.prox(d.x0(xd, ed, px["a"], px["k"]), qp, ydiv, px["rho"])
    comp = px["a_prev"] * z + (px["c_eps"] * ((xd - px["a"] * z) / px["k"]) + px["c_xi"] * xid)
    _check(comp, s64, s32, "diffpir_composed", rec)
    # DDRM in the DDRM suite's scalar regimes
    for regime, cc in DDRM.items():
        cc = dr.round32(cc)
        _check(d.ddrm(xd, ed, q, xid, ydiv, cc), *ref(sr.Sep.ddrm, x, eps, ye, xi, cc), f"ddrm_{regime}", rec)


# --- bitwise properties -----------------------------------------------------------------------------------
SMALL = [i for i, c in enumerate(sr.FACTOR_CASES) if "256" not in c[0]]


@pytest.mark.parametrize("i", SMALL, ids=[FACTOR_IDS[i] for i in SMALL])
def test_bitwise_properties(cuda, i):
    name, C = sr.FACTOR_CASES[i][:2]
    op, t, (x, eps, xi, cot, y) = _factor_case(i)
    d = Dev(t, C, cuda)
    xd, ed, xid, yd = (v.to(cuda).contiguous() for v in (x, eps, xi, y))
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])
    q, qp = d.prepare(yd), d.prepare(yd, prox=True)

    def passes(xs, es, xis, ys, qs, qps, ydiv, alias=False, xi_none=False):
        v, part = d.dps(xs, es, ys, ydiv, c)
        n = None if xi_none else xis
        return {"A": d.apply(xs), "AT": d.adjoint(d.apply(xs)), "pinv": d.pinv(d.apply(xs)), "v": v, "part": part,
                "pgdm": d.pgdm(xs, es, qs, ydiv, dict(c, gs=-2.0)), "prox": d.prox(xs, qps, ydiv, px["rho"]),
                "diffpir": d.diffpir(xs, es, qps, n, ydiv, px, alias=alias),
                "ddrm": d.ddrm(xs, es, qs, n, ydiv, cc, alias=alias)}

    one = passes(xd, ed, xid, yd, q, qp, 2)
    two = passes(xd, ed, xid, yd, q, qp, 2, alias=True)          # the same bits twice, and x_out = x
    for key in one:
        assert torch.equal(one[key], two[key]), key
    # a sample alone against the batch of 4 (sample 3 reads observation row 1)
    alone = passes(xd[3:], ed[3:], xid[3:], yd[1:], q[1:], qp[1:], 1)
    for key in one:
        assert torch.equal(alone[key], one[key][3:]), key
    # y_div = 2 against repeated rows
    rep = _expand(y, 4, 2).to(cuda).contiguous()
    rows = passes(xd, ed, xid, rep, d.prepare(rep), d.prepare(rep, prox=True), 1)
    for key in one:
        assert torch.equal(rows[key], one[key]), key
    # xi = NULL draws sp_randn's plane
    drawn = d.randn(4)
    given = passes(xd, ed, drawn, yd, q, qp, 2)
    null = passes(xd, ed, None, yd, q, qp, 2, xi_none=True)
    for key in ("diffpir", "ddrm"):
        assert torch.equal(given[key], null[key]), key
        assert not torch.equal(null[key], one[key])


# --- against the other kinds -------------------------------------------------------------------------------
def test_gaussian_blur_against_the_blur_kind(cuda, parity_record):
    shape = (3, 33, 35)
    new, old = SeparableSVDOperator.gaussian_blur(shape).to(cuda), GaussianBlurOperator(shape).to(cuda)
    g = torch.Generator().manual_seed(4)
    x, cot = (torch.randn(2, *shape, generator=g).to(cuda) for _ in range(2))
    for got, want, what in ((new.apply(x), old.apply(x), "apply"),
                            (new.apply_transpose(cot), old.apply_transpose(cot), "adjoint")):
        err = float((got - want).abs().max() / want.abs().max())
        parity_record(f"{what}_vs_blur_kind_over_max", err, FLOOR)
        assert err <= FLOOR, (what, err)


@pytest.mark.parametrize("i", [1, 5], ids=[FACTOR_IDS[1], FACTOR_IDS[5]])
def test_conjugate_gradients_reach_the_closed_form(cuda, parity_record, i):
    """sp_op_prox_cg_ws (K = 64, tol 1e-6) through the kind's apply_ws / vjp_ws against sp_op_prox_ws,
    under tests/test_prox_cg_gpu.py's rule: max(2e-5, 4 x the host fp32 recurrence's distance to fp64)."""
    name, C = sr.FACTOR_CASES[i][:2]
    op, t, (x, eps, xi, cot, y) = _factor_case(i)
    S64 = sr.Sep(t)
    dev_op = SeparableSVDOperator((C, *t.dims[:2]), *sr.FACTOR_CASES[i][2](), rtol=sr.FACTOR_CASES[i][3]).to(cuda)
    assert torch.equal(dev_op.tables.cpu(), op.tables)
    for rho in (1e-2, 1.0):
        x0, yy = x[:2], y[:2]
        ref = S64.prox(x0.double(), yy.double(), rho)
        host, _ = _host_prox_cg(op, x0, yy, rho, 64, 1e-6)
        yard = float((host.double() - ref).abs().max() / ref.abs().max())
        bound = max(FLOOR, 4 * yard)
        z, iters = dev_op.apply_prox_cg(x0.to(cuda), yy.to(cuda), rho, iterations=64, tol=1e-6,
                                        return_iterations=True)
        closed = dev_op.apply_prox(x0.to(cuda), yy.to(cuda), rho)
        err = float((z - closed).abs().max() / closed.abs().max())
        print(f"{name} rho={rho}: cg to closed form {err:.3g} bound {bound:.3g} iters {iters.tolist()}")
        parity_record("cg_to_closed_form_max_err_over_max", err, bound, rho=rho)
        assert err <= bound and int(iters.min()) >= 1


def test_autograd_of_the_four_device_maps(cuda):
    shape = (2, 24, 16)
    op = SeparableSVDOperator.bicubic_sr(shape, 4, rtol=0.7).to(cuda)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, *shape, generator=g).to(cuda)
    y = torch.randn(3, *op.y_shape, generator=g).to(cuda)
    ax, aty, py, ptx = op.apply(x), op.apply_transpose(y), op.apply_pseudo_inverse(y), op.apply_pseudo_inverse_transpose(x)
    assert tuple(ax.shape) == (3, *op.y_shape) and tuple(py.shape) == (3, *shape)
    for fn, arg, cot, want in ((op.apply, x, y, aty), (op.apply_transpose, y, x, ax),
                               (op.apply_pseudo_inverse, y, x, ptx), (op.apply_pseudo_inverse_transpose, x, y, py)):
        r = arg.clone().requires_grad_()
        (gr,) = torch.autograd.grad(fn(r), r, grad_outputs=cot)
        assert torch.equal(gr, want)  # the backward of a map is its transpose: the same launches
    host = SeparableSVDOperator.bicubic_sr(shape, 4, rtol=0.7)
    for got, want in ((ax, host.apply(x.cpu().double())), (py, host.apply_pseudo_inverse(y.cpu().double()))):
        assert float((got.cpu().double() - want).abs().max() / want.abs().max()) <= FLOOR
    lhs, rhs = float((ax.double() * y.double()).sum()), float((x.double() * aty.double()).sum())
    assert abs(lhs - rhs) <= FLOOR * float(ax.double().norm() * y.double().norm())


# --- trajectories ---------------------------------------------------------------------------------------------
SHAPE, B, N, SIGMA = (3, 32, 32), 2, 8, 0.05


def _traj(name, cuda):
    host = (SeparableSVDOperator.gaussian_blur(SHAPE, 9, 3.0) if name == "blur"
            else SeparableSVDOperator.bicubic_sr(SHAPE, 4))
    t = sr.Tables.from_flat(host.tables, 32, 32, host.y_shape[1], host.y_shape[2])
    g = torch.Generator().manual_seed(41)
    x_true = si.fixture_x_true(B, SHAPE, seed=9)
    y = sr.Sep(t).apply(x_true.double()).float()
    y = y + SIGMA * torch.randn(y.shape, generator=g)
    op = (SeparableSVDOperator.gaussian_blur(SHAPE, 9, 3.0) if name == "blur"
          else SeparableSVDOperator.bicubic_sr(SHAPE, 4)).to(cuda)
    return op, t, y, InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))


@pytest.mark.parametrize("recon", [1, 2])
@pytest.mark.parametrize("name", ["blur", "sr"])
@pytest.mark.parametrize("sampler", ["dps", "pgdm", "diffpir", "ddrm"])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, sampler, name, recon):
    op, t, y, prob = _traj(name, cuda)
    check_trajectory(cuda, parity_record, sampler, _hip.SP_OP_SVD_SEPARABLE, prob, y,
                     lambda dt: sr.Sep(t, dtype=dt), SHAPE, N, SIGMA, recon, f"{sampler}_{name}_R{recon}")


def test_samplers_take_the_fused_path_and_reproduce(cuda):
    op, t, y, prob = _traj("blur", cuda)
    net, _ = counting_net("conv", 3, 0.1, cuda)
    steps = check_fused_path_and_reproduce(net, prob, y.to(cuda), _hip.SP_OP_SVD_SEPARABLE, N, expect_q=True)
    assert steps["closed_form"].q is not None and steps["auto"].q is not None  # S T_y(y), prepared once


# --- the bounds-checked library ------------------------------------------------------------------------------
def debug_sweep(device):
    """Every pass over every shape of this file; run by the child process under the debug library."""
    cases = [(sr.exact_tables(i), sr.EXACT_CASES[i][1], sr.EXACT_CASES[i][0]) for i in range(len(sr.EXACT_CASES))]
    for i in range(len(sr.FACTOR_CASES)):
        _, t, _ = _factor_case(i)
        cases.append((t, sr.FACTOR_CASES[i][1], sr.FACTOR_CASES[i][0]))
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])
    for t, C, name in cases:
        d = Dev(t, C, device)
        for batch, ydiv in sr.BATCH_FORMS:
            g = torch.Generator().manual_seed(1)
            x, eps, xi = (torch.randn(batch, C, d.H, d.W, generator=g).to(device) for _ in range(3))
            y = torch.randn(-(-batch // ydiv), C, d.Hy, d.Wy, generator=g).to(device)
            ye = _expand(y, batch, ydiv).contiguous()
            q, qp = d.prepare(y), d.prepare(y, prox=True)
            d.apply(x), d.adjoint(ye), d.pinv(ye), d.pinv(x, 1)
            d.dps(x, eps, y, ydiv, c), d.dps(x, eps, y, ydiv, c, sched=True)
            d.pgdm(x, eps, q, ydiv, c), d.prox(x, qp, ydiv, px["rho"])
            for noise in (xi, None):
                d.diffpir(x, eps, qp, noise, ydiv, px), d.ddrm(x, eps, q, noise, ydiv, cc)
        nv, site = _hip.debug_violations()
        print(name, "violations", nv, site, flush=True)
        assert nv == 0, (name, nv, site)


DEBUG_CHILD = DEBUG_SWEEP_CHILD("test_svd_sep_gpu")


def test_debug_build_has_no_violations(cuda):
    """The kernel's SP_DCHECK index invariants under the bounds-checked library, in a fresh child
    process (a process holds one library), over every shape of this file."""
    run_debug_child(DEBUG_CHILD)
