"""The Walsh–Hadamard compressed-sensing kind (SP_OP_HADAMARD, csrc/sp_hadamard.hip) on the GPU,
through the raw entry points into NaN-filled outputs and a NaN-filled workspace between guard bands:
A, Aᵀ, A⁺, A⁺ᵀ, DPS pass 1, PGDM pass 1, the proximal map, the DiffPIR step and the DDRM step against
the fp64 evaluation of tests/hadamard_ref.py, every case at (batch 3, y_div 3) and (batch 4, y_div 2),
the 2^20 plane at batch 1.

Bounds.  Exact cases (even k, integer data in [−3, 3], dyadic scalars: tests/test_hadamard_ref.py
shows that no fp32 evaluation order rounds): bit for bit.  ``randn`` data, per element:
``|err| ≤ n_r · 2⁻²⁴ · E`` with E the same pass on absolute values and n_r the roundings of the
algorithm's longest path (``hadamard_ref.roundings``: k + 2 per transform plus the elementwise
steps); ‖r‖² relative, ``(k + log₂ m + 4) · 2⁻²⁴`` times its absolute-value envelope ratio.  The
compositions from the device maps are held to the same bounds.  Conjugate gradients: the prox bound
once per application of A and Aᵀ, ``(1 + iterations)`` times.  Trajectories: max(1e-4, 20 × the fp32
reference loop's distance to its fp64 run).

Largest errors measured on an MI355X are recorded in README.md ("Hadamard operator")."""

import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import hadamard_ref as hr
import prox_ref as pr
import stand_ins as si
from oracle import dps_loop
from oracle.latent_loops import pgdm_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import HadamardOperator
from samplers_amd.operators.inpainting import keep_bitmask

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
OFFSET = 5  # sample_offset of the Philox calls
CASE_IDS = [c[0] for c in hr.CASES]
DPS = dict(a=0.3, k=math.sqrt(1 - 0.09), gs=400.0)
PROX = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)
DDRM = {"big": dr.make_coefs(3.0, 0.05, 0.85, 1.0), "blend": dr.make_coefs(0.5, 0.05, 0.5, 0.5),
        "small": dr.make_coefs(0.041, 0.05, 0.85, 1.0), "sig_y=0": dr.make_coefs(0.23, 0.0, 0.85, 1.0),
        "sig_prev=0": dr.make_coefs(0.0, 0.05, 0.85, 1.0)}
FORMS = [(i, f) for i in range(len(hr.CASES)) for f in hr.forms_of(i)]
FORM_IDS = [f"{CASE_IDS[i]}-b{f[0]}-d{f[1]}" for i, f in FORMS]
EXACT_FORMS = [(i, f) for i, f in FORMS if i in hr.EXACT]
EXACT_IDS = [f"{CASE_IDS[i]}-b{f[0]}-d{f[1]}" for i, f in EXACT_FORMS]


def _f32(d):
    return {k: float(np.float32(v)) for k, v in d.items()}


def _stream():
    return torch.cuda.current_stream().cuda_stream


# --- a descriptor on the device and the raw calls ---------------------------------------------------------
class Dev:
    """keep_bits, word_rank and the signs on the device, the descriptor and every entry point into
    guarded buffers."""

    def __init__(self, i: int, device):
        self.lib = _hip.load_library()
        self.name, (self.C, self.H, self.W), keep, d = hr.case(i)
        self.device = device
        self.np_, self.mp = self.H * self.W, int(keep.sum())
        self.n, self.m = self.C * self.np_, self.C * self.mp
        self.k = self.np_.bit_length() - 1
        bits, rank = keep_bitmask(keep)
        self.bits = torch.from_numpy(bits.view(np.int64)).to(device)
        self.rank = torch.from_numpy(rank).to(device)
        self.signs = None if d is None else torch.from_numpy(d).to(device)
        s = _hip.SpOp()
        s.kind, s.channels, s.height, s.width = _hip.SP_OP_HADAMARD, self.C, self.H, self.W
        s.n, s.m, s.radius, s.factor = self.n, self.m, 0, 0
        s.keep_bits, s.word_rank = self.bits.data_ptr(), self.rank.data_ptr()
        s.taps = None if d is None else self.signs.data_ptr()
        self.desc = s
        assert self.lib.sp_op_traits(s) == (_hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE
                                            | _hip.SP_TRAIT_PINV)

    def guarded(self, floats):
        """`floats` NaNs between two guard bands of 16 NaNs; (whole, view)."""
        whole = torch.full((floats + 32,), float("nan"), device=self.device)
        return whole, whole[16:16 + floats]

    def check_guards(self, whole, floats):
        assert torch.isnan(whole[:16]).all() and torch.isnan(whole[16 + floats:]).all()

    def _run(self, size_fn, batch, out_shape, call):
        floats = int(size_fn(self.desc, batch))
        assert floats == batch * self.n
        whole, work = self.guarded(floats)
        owhole, out = self.guarded(int(np.prod(out_shape)))
        out = out.view(out_shape)
        _hip.check(call(out, work), "hadamard entry")
        self.check_guards(whole, floats)
        self.check_guards(owhole, out.numel())
        assert torch.isfinite(out).all()
        return out

    def apply(self, x):
        b = x.shape[0]
        return self._run(self.lib.sp_op_workspace, b, (b, self.C, self.mp),
                         lambda o, w: self.lib.sp_op_apply_ws(self.desc, x.data_ptr(), o.data_ptr(), b,
                                                              w.data_ptr(), _stream()))

    def adjoint(self, g):
        b = g.shape[0]
        return self._run(self.lib.sp_op_workspace, b, (b, self.C, self.H, self.W),
                         lambda o, w: self.lib.sp_op_vjp_ws(self.desc, g.data_ptr(), g.data_ptr(), o.data_ptr(),
                                                            b, w.data_ptr(), _stream()))

    def pinv(self, y, transpose=0):
        b = y.shape[0]
        shape = (b, self.C, self.mp) if transpose else (b, self.C, self.H, self.W)
        return self._run(self.lib.sp_op_workspace, b, shape,
                         lambda o, w: self.lib.sp_op_pinv_ws(self.desc, y.data_ptr(), o.data_ptr(), b, transpose,
                                                             w.data_ptr(), _stream()))

    def prepare(self, y):
        """q of the PGDM / DDRM passes: y itself, a row every n floats."""
        rows = y.shape[0]
        floats = int(self.lib.sp_op_workspace(self.desc, rows))
        assert floats == rows * self.n
        whole, q = self.guarded(floats)
        _hip.check(self.lib.sp_pgdm_prepare(self.desc, y.data_ptr(), rows, q.data_ptr(), _stream()), "prepare")
        self.check_guards(whole, floats)
        q = q.view(rows, self.n)
        assert torch.equal(q[:, :self.m], y.reshape(rows, self.m))
        return q

    def dps(self, x, eps, y, ydiv, c, sched=False):
        b, P = x.shape[0], int(self.lib.sp_rsq_partials(self.desc))
        hb = self.k - 12  # one partial per mid tile: the plane, or the high stage's tiles of max(2^12, 2^hb * 32)
        assert P == self.C * (1 if hb <= 0 else self.np_ >> max(12, hb + 5))
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

    def prox(self, x0, y, ydiv, rho):
        b = x0.shape[0]
        return self._run(self.lib.sp_prox_workspace, b, (b, self.C, self.H, self.W),
                         lambda o, w: self.lib.sp_op_prox_ws(self.desc, x0.data_ptr(), y.data_ptr(), None, b, ydiv,
                                                             rho, o.data_ptr(), w.data_ptr(), _stream()))

    def _step(self, entry, size_fn, x, eps, y, q, xi, ydiv, coefs, alias, step):
        b = x.shape[0]
        src = x.clone() if alias else x

        def call(o, w):
            dst = src if alias else o
            rc = entry(self.desc, src.data_ptr(), eps.data_ptr(), None if y is None else y.data_ptr(),
                       None if q is None else q.data_ptr(), None if xi is None else xi.data_ptr(), 77, step,
                       OFFSET, b, ydiv, coefs, dst.data_ptr(), w.data_ptr(), _stream())
            if alias:
                o.copy_(src)
            return rc

        return self._run(size_fn, b, (b, self.C, self.H, self.W), call)

    def diffpir(self, x, eps, y, xi, ydiv, c, alias=False, step=3):
        coefs = _hip.SpProxCoefs(c["a"], c["k"], c["rho"], c["a_prev"], c["c_eps"], c["c_xi"])
        return self._step(self.lib.sp_diffpir_step_ws, self.lib.sp_prox_workspace, x, eps, y, None, xi, ydiv,
                          coefs, alias, step)

    def ddrm(self, x, eps, q, xi, ydiv, c, alias=False, step=3):
        coefs = _hip.SpDdrmCoefs(*[c[k] for k in dr.KEYS])
        return self._step(self.lib.sp_ddrm_step_ws, self.lib.sp_ddrm_workspace, x, eps, None, q, xi, ydiv,
                          coefs, alias, step)

    def randn(self, b, step=3):
        out = torch.empty(b, self.C, self.H, self.W, device=self.device)
        _hip.check(self.lib.sp_randn(out.data_ptr(), b, self.n, 77, step, OFFSET, _stream()), "sp_randn")
        return out

    def x0(self, x, eps, a, k):
        out = torch.empty_like(x)
        _hip.check(self.lib.sp_predict_x0(x.data_ptr(), eps.data_ptr(), x.numel(), a, k, out.data_ptr(),
                                          _stream()), "sp_predict_x0")
        return out


_DATA = {}


def _randn_case(i):
    """randn inputs for the largest batch of the case; computed once, never modified."""
    if i not in _DATA:
        _, (C, H, W), keep, _ = hr.case(i)
        b = max(f[0] for f in hr.forms_of(i))
        g = torch.Generator().manual_seed(300 + i)
        x, eps, xi = (torch.randn(b, C, H, W, generator=g) for _ in range(3))
        y = torch.randn(2 if b > 1 else 1, C, int(keep.sum()), generator=g)
        _DATA[i] = (x, eps, xi, y)
    return _DATA[i]


def _rows(y, batch, ydiv):
    return y[: -(-batch // ydiv)]


def _check(got, ref64, env, n_r, what, record=None):
    """max over the elements of |got − ref64| / (n_r · 2⁻²⁴ · E) ≤ 1."""
    ratio = float(((got.detach().cpu().double() - ref64).abs() / (n_r * hr.U24 * env)).max())
    print(f"{what}: worst |err| / (n_r 2^-24 E) = {ratio:.3g} (n_r = {n_r})")
    if record is not None:
        record(f"{what}_err_over_bound", ratio, 1.0, n_r=n_r)
    assert ratio <= 1.0, (what, ratio)
    return ratio


# --- exact cases: bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("i,form", EXACT_FORMS, ids=EXACT_IDS)
def test_exact_cases_are_bitwise(cuda, i, form):
    name, shape, keep, sg = hr.case(i)
    batch, ydiv = form
    x, eps, xi, y = hr.exact_data(i, batch, ydiv)
    ye = hr.expand(y, batch, ydiv)
    S, d = hr.Had(shape, keep, sg), Dev(i, cuda)
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    e, px, cc = hr.EXACT_DPS, hr.EXACT_PROX, hr.EXACT_DDRM
    eq = lambda got, want, what: (torch.equal(got.cpu().double(), want) or pytest.fail(f"{name} {what}"))  # noqa: E731
    eq(d.apply(xd), S.apply(x), "A")
    eq(d.adjoint(yed), S.adjoint(ye), "A^T")
    eq(d.pinv(yed), S.pinv(ye), "A^+")
    eq(d.pinv(xd, 1), S.pinv_t(x), "A^+T")
    v, part = d.dps(xd, ed, yd, ydiv, e)
    vref, rsq = S.dps(x, eps, ye, e["a"], e["k"], e["gs"])
    eq(v, vref, "DPS v")
    rel = (d.k + math.ceil(math.log2(max(d.m, 2))) + 4) * hr.U24
    assert float((part.double().sum(1).cpu() / rsq - 1).abs().max()) <= rel
    q = d.prepare(yd)
    eq(d.pgdm(xd, ed, q, ydiv, dict(e, gs=-e["gs"])), S.pgdm(x, eps, ye, e["a"], e["k"], -e["gs"]), "PGDM v")
    eq(d.prox(xd, yd, ydiv, px["rho"]), S.prox(x, ye, px["rho"]), "prox z")
    eq(d.diffpir(xd, ed, yd, xid, ydiv, px), S.diffpir(x, eps, ye, xi, px), "DiffPIR x'")
    eq(d.ddrm(xd, ed, q, xid, ydiv, cc), S.ddrm(x, eps, ye, xi, cc), "DDRM x'")


# --- every pass under the bound ----------------------------------------------------------------------------
@pytest.mark.parametrize("i,form", FORMS, ids=FORM_IDS)
def test_every_pass_against_fp64(cuda, parity_record, i, form):
    name, shape, keep, sg = hr.case(i)
    batch, ydiv = form
    x, eps, xi, y = _randn_case(i)
    x, eps, xi = x[:batch], eps[:batch], xi[:batch]
    y = _rows(y, batch, ydiv)
    ye = hr.expand(y, batch, ydiv)
    S, d = hr.Had(shape, keep, sg), Dev(i, cuda)
    k, nr = d.k, lambda what: hr.roundings(what, d.k)  # noqa: E731
    xd, ed, xid, yd, yed = (v.to(cuda).contiguous() for v in (x, eps, xi, y, ye))
    rec = parity_record
    ax = d.apply(xd)
    _check(ax, S.apply(x), S.envelope("apply", x=x), nr("apply"), "apply", rec)
    _check(d.adjoint(yed), S.adjoint(ye), S.envelope("adjoint", y=ye), nr("adjoint"), "adjoint", rec)
    assert torch.equal(d.pinv(yed), d.adjoint(yed)) and torch.equal(d.pinv(xd, 1), ax)  # the same launches
    # DPS pass 1, its _sched_ws form and its composition from the maps
    c = _f32(DPS)
    v, part = d.dps(xd, ed, yd, ydiv, c)
    v64, rsq64 = S.dps(x, eps, ye, c["a"], c["k"], c["gs"])
    env = S.envelope("dps", x=x, eps=eps, y=ye, c=c)
    _check(v, v64, env, nr("dps"), "dps_v", rec)
    ratio = float(((part.double().sum(1).cpu() - rsq64).abs()
                   / (hr.roundings("rsq", k, d.m) * hr.U24 * S.envelope("rsq", x=x, eps=eps, y=ye, c=c))).max())
    rec("dps_rsq_err_over_bound", ratio, 1.0)
    assert ratio <= 1.0, ("rsq", ratio)
    vs, parts = d.dps(xd, ed, yd, ydiv, c, sched=True)
    assert torch.equal(vs, v) and torch.equal(parts, part)
    x0d = d.x0(xd, ed, c["a"], c["k"])
    comp = d.adjoint((c["gs"] * (yed - d.apply(x0d))).contiguous())
    _check(comp, v64, env, nr("dps"), "dps_v_composed", rec)
    # PGDM pass 1 against fp64 and against A^+ y - A^+ A x0
    q = d.prepare(yd)
    cp = dict(c, gs=-2.0)
    p64, envp = S.pgdm(x, eps, ye, cp["a"], cp["k"], cp["gs"]), S.envelope("pgdm", x=x, eps=eps, y=ye, c=cp)
    _check(d.pgdm(xd, ed, q, ydiv, cp), p64, envp, nr("pgdm"), "pgdm_v", rec)
    comp = -2.0 * (d.pinv(yed) - d.pinv(d.apply(x0d)))
    _check(comp, p64, envp, nr("pgdm"), "pgdm_v_composed", rec)
    # the proximal map and the DiffPIR step (xi given), and their composition
    px = _f32(PROX)
    for rho in (1e-4, px["rho"], 50.0):
        rho = float(np.float32(rho))
        _check(d.prox(xd, yd, ydiv, rho), S.prox(x, ye, rho), S.envelope("prox", x=x, y=ye, c=dict(rho=rho)),
               nr("prox"), f"prox_rho{rho:.3g}", rec)
    s64, envs = S.diffpir(x, eps, ye, xi, px), S.envelope("diffpir", x=x, eps=eps, y=ye, xi=xi, c=px)
    _check(d.diffpir(xd, ed, yd, xid, ydiv, px), s64, envs, nr("diffpir"), "diffpir", rec)
    z = d.prox(d.x0(xd, ed, px["a"], px["k"]), yd, ydiv, px["rho"])
    comp = px["a_prev"] * z + (px["c_eps"] * ((xd - px["a"] * z) / px["k"]) + px["c_xi"] * xid)
    _check(comp, s64, envs, nr("diffpir"), "diffpir_composed", rec)
    # DDRM in the DDRM suite's scalar regimes, and its composition (the blend regime)
    for regime, cc in DDRM.items():
        cc = dr.round32(cc)
        r64, envd = S.ddrm(x, eps, ye, xi, cc), S.envelope("ddrm", x=x, eps=eps, y=ye, xi=xi, c=cc)
        _check(d.ddrm(xd, ed, q, xid, ydiv, cc), r64, envd, nr("ddrm"), f"ddrm_{regime}", rec)
        if regime == "blend":
            one = torch.ones((), dtype=torch.float32)
            fo = [float(v) for v in dr.coefficients(one, torch.tensor(True), dr.big_mask32(one, cc), cc, torch.float32)]
            fu = [float(v) for v in dr.coefficients(one, torch.tensor(False), torch.tensor(False), cc, torch.float32)]
            x0d = d.x0(xd, ed, cc["a"], cc["k"])
            w = ((fo[0] - fu[0]) * x0d + (fo[1] - fu[1]) * ed) + (fo[3] - fu[3]) * xid
            comp = cc["a_prev"] * ((x0d + (fu[1] * ed + fu[3] * xid))
                                   + d.adjoint((fo[2] * yed + d.apply(w.contiguous())).contiguous()))
            _check(comp, r64, envd, nr("ddrm"), "ddrm_composed", rec)


# --- bitwise properties -----------------------------------------------------------------------------------
SMALL = [i for i, c in enumerate(hr.CASES) if c[1][1] * c[1][2] <= 1 << 16]


@pytest.mark.parametrize("i", SMALL, ids=[CASE_IDS[i] for i in SMALL])
def test_bitwise_properties(cuda, i):
    d = Dev(i, cuda)
    x, eps, xi, y = _randn_case(i)
    xd, ed, xid, yd = (v.to(cuda).contiguous() for v in (x, eps, xi, y))
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])
    q = d.prepare(yd)

    def passes(xs, es, xis, ys, qs, ydiv, alias=False, xi_none=False):
        v, part = d.dps(xs, es, ys, ydiv, c)
        n = None if xi_none else xis
        return {"A": d.apply(xs), "AT": d.adjoint(d.apply(xs)), "v": v, "part": part,
                "pgdm": d.pgdm(xs, es, qs, ydiv, dict(c, gs=-2.0)), "prox": d.prox(xs, ys, ydiv, px["rho"]),
                "diffpir": d.diffpir(xs, es, ys, n, ydiv, px, alias=alias),
                "ddrm": d.ddrm(xs, es, qs, n, ydiv, cc, alias=alias)}

    one = passes(xd, ed, xid, yd, q, 2)
    two = passes(xd, ed, xid, yd, q, 2, alias=True)          # the same bits twice, and x_out = x
    for key in one:
        assert torch.equal(one[key], two[key]), key
    # a sample alone against the batch of 4 (sample 3 reads observation row 1)
    alone = passes(xd[3:], ed[3:], xid[3:], yd[1:], q[1:], 1)
    for key in one:
        assert torch.equal(alone[key], one[key][3:]), key
    # y_div = 2 against repeated rows
    rep = hr.expand(y, 4, 2).to(cuda).contiguous()
    rows = passes(xd, ed, xid, rep, d.prepare(rep), 1)
    for key in one:
        assert torch.equal(rows[key], one[key]), key
    # xi = NULL draws sp_randn's plane
    drawn = d.randn(4)
    given = passes(xd, ed, drawn, yd, q, 2)
    null = passes(xd, ed, None, yd, q, 2, xi_none=True)
    for key in ("diffpir", "ddrm"):
        assert torch.equal(given[key], null[key]), key
        assert not torch.equal(null[key], one[key])


# --- conjugate gradients, autograd -------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 4], ids=[CASE_IDS[1], CASE_IDS[4]])
def test_conjugate_gradients_reach_the_closed_form(cuda, parity_record, i):
    """sp_op_prox_cg_ws (K = 64, tol 1e-6) through the kind's apply_ws / vjp_ws: A Aᵀ = I, so the
    recurrence stops within two iterations, on sp_op_prox_ws's point."""
    name, shape, keep, sg = hr.case(i)
    op = HadamardOperator(shape, kept=keep, signs=sg if sg is not None else False).to(cuda)
    S = hr.Had(shape, keep, sg)
    x, _, _, y = _randn_case(i)
    x0, yy = x[:2], y[:2]
    for rho in (1e-2, 1.0):
        z, iters = op.apply_prox_cg(x0.to(cuda), yy.to(cuda), rho, iterations=64, tol=1e-6, return_iterations=True)
        closed = op.apply_prox(x0.to(cuda), yy.to(cuda), rho)
        env = S.envelope("prox", x=x0, y=yy, c=dict(rho=rho))
        n_r = (1 + int(iters.max())) * hr.roundings("prox", S.k)
        ratio = float(((z - closed).cpu().double().abs() / (n_r * hr.U24 * env)).max())
        print(f"{name} rho={rho}: cg to closed form {ratio:.3g} of the bound, iters {iters.tolist()}")
        parity_record("cg_to_closed_form_err_over_bound", ratio, 1.0, rho=rho)
        assert 1 <= int(iters.min()) and int(iters.max()) <= 2 and ratio <= 1.0
        _check(closed, S.prox(x0, yy, rho), env, hr.roundings("prox", S.k), "apply_prox", parity_record)


def test_autograd_of_the_four_device_maps(cuda):
    name, shape, keep, sg = hr.case(4)
    op = HadamardOperator(shape, kept=keep, signs=sg).to(cuda)
    S = hr.Had(shape, keep, sg)
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
    _check(ax, S.apply(x.cpu()), S.envelope("apply", x=x.cpu()), hr.roundings("apply", S.k), "operator_apply")
    _check(py, S.adjoint(y.cpu()), S.envelope("adjoint", y=y.cpu()), hr.roundings("adjoint", S.k), "operator_pinv")
    assert torch.equal(op.apply_V_transpose(x), ax) and torch.equal(op.apply_V(y), aty)
    assert op.apply_U(y) is y and op.apply_U_transpose(y) is y


# --- trajectories ---------------------------------------------------------------------------------------------
SHAPE, B, N, SIGMA = (3, 32, 32), 2, 8, 0.05


def _traj(ratio, cuda):
    host = HadamardOperator(SHAPE, ratio=ratio, seed=3)
    keep, sg = host.keep.numpy(), host.signs.numpy()
    g = torch.Generator().manual_seed(41)
    x_true = si.fixture_x_true(B, SHAPE, seed=9)
    y = hr.Had(SHAPE, keep, sg).apply(x_true.double()).float()
    y = y + SIGMA * torch.randn(y.shape, generator=g)
    op = HadamardOperator(SHAPE, ratio=ratio, seed=3).to(cuda)
    return op, (keep, sg), y, InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))


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
@pytest.mark.parametrize("ratio", [0.25, 0.5])
@pytest.mark.parametrize("sampler", ["dps", "pgdm", "diffpir", "ddrm"])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, sampler, ratio, recon):
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler, DPSSampler, PGDMSampler

    op, (keep, sg), y, prob = _traj(ratio, cuda)
    net, grads = _net(cuda)
    init, steps = si.replay_noise(17, (B * recon, *SHAPE), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    ts = si.leading_timesteps_ascending(N).tolist()
    yr = y.repeat_interleave(recon, dim=0)
    kw = dict(num_sampling_steps=N, num_reconstructions=recon, noise_fn=fn,
              micro_batch=2 if recon == 2 else None)

    def loop(dt):
        core, S = si.EpsCore("conv", 3, 0.1).to(dt), hr.Had(SHAPE, keep, sg, dtype=dt)
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
        smp = DPSSampler(net)
        out = smp(prob, gamma=1e-2, eta=1.0, **kw)
    elif sampler == "pgdm":
        smp = PGDMSampler(net)
        out = smp(prob, guidance_weight=0.05, **kw)
    elif sampler == "diffpir":
        smp = DiffPIRSampler(net)
        out = smp(prob, **kw)
        assert not smp.last_step.cg and not smp.last_step.host
    else:
        smp = DDRMSampler(net)
        out = smp(prob, **kw)
        assert smp.last_step.fused
    if sampler in ("diffpir", "ddrm"):
        assert smp.last_step.desc.kind == _hip.SP_OP_HADAMARD  # the HIP path ran
    assert tuple(out.shape) == ((B, *SHAPE) if recon == 1 else (B, recon, *SHAPE))
    if sampler in ("diffpir", "ddrm"):
        assert len(grads) >= 2 and not any(grads)  # no network call builds an autograd graph
    _bound_check(out, loop, f"{sampler}_r{ratio}_R{recon}", parity_record)


def test_samplers_take_the_fused_path_and_reproduce(cuda):
    from samplers_amd.samplers import DDRMSampler, DiffPIRSampler, DPSSampler, PGDMSampler
    from samplers_amd.samplers.ddrm import FusedDDRMStep
    from samplers_amd.samplers.diffpir import FusedDiffPIRStep
    from samplers_amd.samplers.dps import FusedDPSStep, make_dps_step

    op, _, y, prob = _traj(0.25, cuda)
    net, _ = _net(cuda)
    rows = y.to(cuda)
    step = FusedDDRMStep(net, prob, rows, 1)
    assert step.fused and step.q is not None
    for mode in ("closed_form", "auto"):
        assert not FusedDiffPIRStep(net, prob, rows, 1, prox=mode).cg
    assert FusedDiffPIRStep(net, prob, rows, 1, prox="cg").cg
    for mode in ("dps", "pgdm"):  # DPS and PGDM: the fused step on the kind's descriptor, q for PGDM
        st = make_dps_step(net, prob, rows, 1, mode=mode)
        assert isinstance(st, FusedDPSStep) and st.desc.kind == _hip.SP_OP_HADAMARD
        assert st.needs_v and (st.q is not None) == (mode == "pgdm")
    for cls in (DPSSampler, PGDMSampler, DDRMSampler, DiffPIRSampler):
        one = cls(net)(prob, num_sampling_steps=N, seed=1234)
        assert torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1234), one) and torch.isfinite(one).all()
        assert not torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1235), one)
        assert torch.equal(cls(net)(prob, num_sampling_steps=N, seed=1234, micro_batch=1), one)
    out = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=3, prox="cg", cg_iterations=8)
    assert torch.isfinite(out).all() and tuple(out.shape) == (B, *SHAPE)


# --- the bounds-checked library ------------------------------------------------------------------------------
def debug_sweep(device):
    """Every pass over every shape of this file; run by the child process under the debug library."""
    c, px, cc = _f32(DPS), _f32(PROX), dr.round32(DDRM["blend"])
    for i in range(len(hr.CASES)):
        d = Dev(i, device)
        for batch, ydiv in hr.forms_of(i):
            g = torch.Generator().manual_seed(1)
            x, eps, xi = (torch.randn(batch, d.C, d.H, d.W, generator=g).to(device) for _ in range(3))
            y = torch.randn(-(-batch // ydiv), d.C, d.mp, generator=g).to(device)
            ye = hr.expand(y, batch, ydiv).contiguous()
            q = d.prepare(y)
            d.apply(x), d.adjoint(ye), d.pinv(ye), d.pinv(x, 1)
            d.dps(x, eps, y, ydiv, c), d.dps(x, eps, y, ydiv, c, sched=True)
            d.pgdm(x, eps, q, ydiv, c), d.prox(x, y, ydiv, px["rho"])
            for noise in (xi, None):
                d.diffpir(x, eps, y, noise, ydiv, px), d.ddrm(x, eps, q, noise, ydiv, cc)
        nv, site = _hip.debug_violations()
        print(d.name, "violations", nv, site, flush=True)
        assert nv == 0, (d.name, nv, site)


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from samplers_amd import _hip
assert _hip.load_library().sp_debug_build() == 1, "not the debug library"
import test_hadamard_gpu as T
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
