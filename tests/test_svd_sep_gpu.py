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
import svd_sep_ref as sr
from oracle import dps_loop
from oracle.latent_loops import pgdm_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import GaussianBlurOperator, SeparableSVDOperator
from samplers_amd.operators.base import _host_prox_cg

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FLOOR = 2e-5
OFFSET = 5  # sample_offset of the Philox calls
FACTOR_IDS = [c[0] for c in sr.FACTOR_CASES]
EXACT_IDS = [c[0] for c in sr.EXACT_CASES]
FORM_IDS = [f"b{b}-d{d}" for b, d in sr.BATCH_FORMS]
DPS = dict(a=0.3, k=math.sqrt(1 - 0.09), gs=400.0)
PROX = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)
DDRM = {"big": dr.make_coefs(3.0, 0.05, 0.85, 1.0), "blend": dr.make_coefs(0.5, 0.05, 0.5, 0.5),
        "small": dr.make_coefs(0.041, 0.05, 0.85, 1.0), "sig_y=0": dr.make_coefs(0.23, 0.0, 0.85, 1.0),
        "sig_prev=0": dr.make_coefs(0.0, 0.05, 0.85, 1.0)}


def _f32(d):
    return {k: float(np.float32(v)) for k, v in d.items()}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --- a descriptor on the device and the raw calls ---------------------------------------------------------
class Dev:
    """The tables on the device, the descriptor and every entry point into guarded buffers."""

    def __init__(self, t: sr.Tables, C: int, device):
        self.lib = _hip.load_library()
        self.t, self.C, self.device = t, C, device
        self.H, self.W, self.Hy, self.Wy = t.dims
        self.n, self.m = C * self.H * self.W, C * self.Hy * self.Wy
        self.tables = t.flat32().to(device)
        d = _hip.SpOp()
        d.kind, d.channels, d.height, d.width = _hip.SP_OP_SVD_SEPARABLE, C, self.H, self.W
        d.n, d.m, d.radius, d.factor, d.taps = self.n, self.m, self.Hy, self.Wy, self.tables.data_ptr()
        self.desc = d
        assert self.lib.sp_op_traits(d) == (_hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE
                                            | _hip.SP_TRAIT_PINV)

    def guarded(self, floats):
        """`floats` NaNs between two guard bands of 16 NaNs; (whole, view)."""
        whole = torch.full((floats + 32,), float("nan"), device=self.device)
        return whole, whole[16:16 + floats]

    def check_guards(self, whole, floats):
        assert torch.isnan(whole[:16]).all() and torch.isnan(whole[16 + floats:]).all()

    def _run(self, size_fn, batch, out_shape, call):
        floats = int(size_fn(self.desc, batch))
        assert floats > 0
        whole, work = self.guarded(floats)
        out = torch.full(out_shape, float("nan"), device=self.device)
        _hip.check(call(out, work), "svd_separable entry")
        self.check_guards(whole, floats)
        assert torch.isfinite(out).all()
        return out

    def apply(self, x):
        b = x.shape[0]
        return self._run(self.lib.sp_op_workspace, b, (b, self.C, self.Hy, self.Wy),
                         lambda o, w: self.lib.sp_op_apply_ws(self.desc, x.data_ptr(), o.data_ptr(), b,
                                                              w.data_ptr(), _stream()))

    def adjoint(self, g):
        b = g.shape[0]
        return self._run(self.lib.sp_op_workspace, b, (b, self.C, self.H, self.W),
                         lambda o, w: self.lib.sp_op_vjp_ws(self.desc, g.data_ptr(), g.data_ptr(), o.data_ptr(),
                                                            b, w.data_ptr(), _stream()))

    def pinv(self, y, transpose=0):
        b = y.shape[0]
        shape = (b, self.C, self.Hy, self.Wy) if transpose else (b, self.C, self.H, self.W)
        return self._run(self.lib.sp_op_workspace, b, shape,
                         lambda o, w: self.lib.sp_op_pinv_ws(self.desc, y.data_ptr(), o.data_ptr(), b, transpose,
                                                             w.data_ptr(), _stream()))

    def prepare(self, y, prox=False):
        """q of the PGDM / DDRM passes (P T_y(y)) or of the prox (S T_y(y)): (rows, 2 n), m used."""
        rows = y.shape[0]
        size = self.lib.sp_prox_prepare_size if prox else self.lib.sp_op_workspace
        floats = int(size(self.desc, rows))
        assert floats == 2 * rows * self.n
        whole, q = self.guarded(floats)
        fn = self.lib.sp_prox_prepare if prox else self.lib.sp_pgdm_prepare
        _hip.check(fn(self.desc, y.data_ptr(), rows, q.data_ptr(), _stream()), "prepare")
        self.check_guards(whole, floats)
        q = q.view(rows, 2 * self.n)
        assert torch.isfinite(q[:, :self.m]).all()
        return q

    def dps(self, x, eps, y, ydiv, c, sched=False):
        b, P = x.shape[0], int(self.lib.sp_rsq_partials(self.desc))
        assert P == self.C * -(-self.Hy // 64) * -(-self.Wy // 64)
        pwhole, part = self.guarded(b * P)
        coefs = _hip.SpDpsCoefs(c["a"], c["k"], c["gs"], 0.9, 0.2, 0.1, 0.05, 1e-9)

        def call(o, w):
            if not sched:
                return self.lib.sp_dps_residual_ws(self.desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b,
                                                   ydiv, coefs, o.data_ptr(), part.data_ptr(), w.data_ptr(),
                                                   _stream())
            recs = (_hip.SpStepRec * 2)()
            recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
            recs[1].c, recs[1].step, recs[1].t = coefs, 3, 5
            self._sched = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(self.device)
            self._cursor = torch.ones(1, dtype=torch.int32, device=self.device)
            return self.lib.sp_dps_residual_sched_ws(self.desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b,
                                                     ydiv, self._sched.data_ptr(), self._cursor.data_ptr(),
                                                     o.data_ptr(), part.data_ptr(), w.data_ptr(), _stream())

        v = self._run(self.lib.sp_dps_workspace, b, (b, self.C, self.H, self.W), call)
        self.check_guards(pwhole, b * P)
        assert torch.isfinite(part).all()
        return v, part.view(b, P)

    def pgdm(self, x, eps, q, ydiv, c):
        b = x.shape[0]
        coefs = _hip.SpDpsCoefs(c["a"], c["k"], c["gs"], 0.9, 0.2, 0.1, 0.05, 1e-9)
        return self._run(self.lib.sp_op_workspace, b, (b, self.C, self.H, self.W),
                         lambda o, w: self.lib.sp_pgdm_residual_ws(self.desc, x.data_ptr(), eps.data_ptr(),
                                                                   q.data_ptr(), b, ydiv, coefs, o.data_ptr(),
                                                                   w.data_ptr(), _stream()))

    def prox(self, x0, q, ydiv, rho):
        b = x0.shape[0]
        return self._run(self.lib.sp_prox_workspace, b, (b, self.C, self.H, self.W),
                         lambda o, w: self.lib.sp_op_prox_ws(self.desc, x0.data_ptr(), None, q.data_ptr(), b, ydiv,
                                                             rho, o.data_ptr(), w.data_ptr(), _stream()))

    def diffpir(self, x, eps, q, xi, ydiv, c, alias=False, step=3):
        b = x.shape[0]
        coefs = _hip.SpProxCoefs(c["a"], c["k"], c["rho"], c["a_prev"], c["c_eps"], c["c_xi"])
        src = x.clone() if alias else x

        def call(o, w):
            dst = src if alias else o
            rc = self.lib.sp_diffpir_step_ws(self.desc, src.data_ptr(), eps.data_ptr(), None, q.data_ptr(),
                                             None if xi is None else xi.data_ptr(), 77, step, OFFSET, b, ydiv,
                                             coefs, dst.data_ptr(), w.data_ptr(), _stream())
            if alias:
                o.copy_(src)
            return rc

        return self._run(self.lib.sp_prox_workspace, b, (b, self.C, self.H, self.W), call)

    def ddrm(self, x, eps, q, xi, ydiv, c, alias=False, step=3):
        b = x.shape[0]
        coefs = _hip.SpDdrmCoefs(*[c[k] for k in dr.KEYS])
        src = x.clone() if alias else x

        def call(o, w):
            dst = src if alias else o
            rc = self.lib.sp_ddrm_step_ws(self.desc, src.data_ptr(), eps.data_ptr(), None, q.data_ptr(),
                                          None if xi is None else xi.data_ptr(), 77, step, OFFSET, b, ydiv,
                                          coefs, dst.data_ptr(), w.data_ptr(), _stream())
            if alias:
                o.copy_(src)
            return rc

        return self._run(self.lib.sp_ddrm_workspace, b, (b, self.C, self.H, self.W), call)

    def randn(self, b, step=3):
        out = torch.empty(b, self.C, self.H, self.W, device=self.device)
        _hip.check(self.lib.sp_randn(out.data_ptr(), b, self.n, 77, step, OFFSET, _stream()), "sp_randn")
        return out

    def x0(self, x, eps, a, k):
        out = torch.empty_like(x)
        _hip.check(self.lib.sp_predict_x0(x.data_ptr(), eps.data_ptr(), x.numel(), a, k, out.data_ptr(),
                                          _stream()), "sp_predict_x0")
        return out


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


def _acp(dt=torch.float32):
    return torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).to(dt)


def _net(cuda):
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    grads, inner = [], net.forward

    def forward(x, t):
        e = inner(x, t)
        grads.append(bool(e.requires_grad) or torch.is_grad_enabled())
        return e

    net.forward = forward
    return net, grads


def _bound_check(out, run, what, record):
    ref32 = run(torch.float32)
    cond = si.relative_error(run(torch.float64), ref32)
    bound = max(1e-4, 20 * cond)
    err = si.relative_error(out.reshape(ref32.shape).cpu(), ref32)
    print(f"{what}: rel l2 {err:.3g}, fp32 reference to fp64 {cond:.3g}, bound {bound:.3g}")
    record(f"{what}_rel_l2", err, bound, fp32_to_fp64=cond)
    assert err < bound


@pytest.mark.parametrize("recon", [1, 2])
@pytest.mark.parametrize("name", ["blur", "sr"])
@pytest.mark.parametrize("sampler", ["dps", "pgdm", "diffpir", "ddrm"])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, sampler, name, recon):
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler, DPSSampler, PGDMSampler

    op, t, y, prob = _traj(name, cuda)
    net, grads = _net(cuda)
    init, steps = si.replay_noise(17, (B * recon, *SHAPE), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    ts = si.leading_timesteps_ascending(N).tolist()
    yr = y.repeat_interleave(recon, dim=0)
    kw = dict(num_sampling_steps=N, num_reconstructions=recon, noise_fn=fn,
              micro_batch=2 if recon == 2 else None)

    def loop(dt):
        core, S = si.EpsCore("conv", 3, 0.1).to(dt), sr.Sep(t, dtype=dt)
        eps_fn = lambda x, tt: core(x, tt)  # noqa: E731
        noise = lambda i: steps[i].to(dt)  # noqa: E731
        if sampler == "dps":
            return dps_loop.dps_reference(eps_fn, _acp(dt), ts, S.apply, dps_loop.gaussian_log_prob(SIGMA),
                                          yr.to(dt), init.to(dt), noise, gamma=1e-2, eta=1.0)
        if sampler == "pgdm":
            return pgdm_reference(eps_fn, _acp(dt), ts, S.apply, S.pinv, yr.to(dt), init.to(dt), noise,
                                  guidance_weight=0.05, eta=1.0)
        if sampler == "diffpir":
            return pr.diffpir_reference(eps_fn, _acp(dt), ts, S.apply, lambda x0, yy, rho: S.prox(x0, yy, float(rho)),
                                        yr.to(dt), init.to(dt), noise, sigma=SIGMA)
        step = lambda x, e, yy, xi, c: S.ddrm(x, e, yy, xi, dr.round32(c) if dt == torch.float32 else c)  # noqa: E731
        return dr.ddrm_reference(eps_fn, _acp(dt), ts, step, yr.to(dt), init.to(dt), noise, sigma_y=SIGMA)

    if sampler == "dps":
        out = DPSSampler(net)(prob, gamma=1e-2, eta=1.0, **kw)
    elif sampler == "pgdm":
        out = PGDMSampler(net)(prob, guidance_weight=0.05, **kw)
    elif sampler == "diffpir":
        out = DiffPIRSampler(net)(prob, **kw)
    else:
        out = DDRMSampler(net)(prob, **kw)
    assert tuple(out.shape) == ((B, *SHAPE) if recon == 1 else (B, recon, *SHAPE))
    if sampler in ("diffpir", "ddrm"):
        assert len(grads) >= 2 and not any(grads)  # no network call builds an autograd graph
    _bound_check(out, loop, f"{sampler}_{name}_R{recon}", parity_record)


def test_samplers_take_the_fused_path_and_reproduce(cuda):
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler
    from samplers_amd.samplers.ddrm import FusedDDRMStep
    from samplers_amd.samplers.diffpir import FusedDiffPIRStep

    op, t, y, prob = _traj("blur", cuda)
    net, _ = _net(cuda)
    rows = y.to(cuda)
    step = FusedDDRMStep(net, prob, rows, 1)
    assert step.fused and step.q is not None
    for mode in ("closed_form", "auto"):
        st = FusedDiffPIRStep(net, prob, rows, 1, prox=mode)
        assert not st.cg and st.q is not None
    assert FusedDiffPIRStep(net, prob, rows, 1, prox="cg").cg
    for cls in (DDRMSampler, DiffPIRSampler):
        one = cls(net)(prob, num_sampling_steps=N, seed=1234)
        assert torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1234), one) and torch.isfinite(one).all()
        assert not torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1235), one)
        assert torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1234, micro_batch=1), one)
    # conjugate gradients run through the kind's apply_ws / vjp_ws (the maps' agreement with the
    # closed form is test_conjugate_gradients_reach_the_closed_form's)
    out = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=3, prox="cg", cg_iterations=8)
    assert torch.isfinite(out).all() and tuple(out.shape) == (B, *SHAPE)


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


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from samplers_amd import _hip
assert _hip.load_library().sp_debug_build() == 1, "not the debug library"
import test_svd_sep_gpu as T
_hip.debug_violations()  # clear
T.debug_sweep(torch.device("cuda:0"))
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The kernel's SP_DCHECK index invariants under the bounds-checked library, in a fresh child
    process (a process holds one library), over every shape of this file."""
    if not _hip.DEBUG_LIB_PATH.exists():
        pytest.fail(f"{_hip.DEBUG_LIB_PATH} missing: run `make` (builds the debug library too)")
    env = dict(os.environ, SAMPLERS_HIP_LIB=str(_hip.DEBUG_LIB_PATH))
    out = subprocess.run([sys.executable, "-c", DEBUG_CHILD, str(ROOT)], env=env,
                         capture_output=True, text=True, timeout=240)
    print(out.stdout[-4000:], out.stderr[-4000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "debug build: clean" in out.stdout
