"""Periodic blur with a spectral pseudo-inverse (SP_OP_PSF_PERIODIC, csrc/sp_psf_fft.hip) on the
GPU: the four maps A, A^T, A^+, A^+T and their autograd backwards, the fused DPS passes and the
fused PGDM pass 1 against the fp64 semantics of tests/periodic_ops.py, and PGDMSampler / DPSSampler
against the oracle loops.

Bounds are the native-operator family's: 2e-5 x max|reference| per element and 2e-5 relative on
||r||^2 for the maps and the fused passes, 1e-4 relative L2 for the DPS trajectory,
max(1e-4, 20 x the fp32 oracle's distance to its fp64 run) for the PGDM trajectory.  The same
arithmetic in fp32 torch.fft on the CPU stays within 2.5e-7 x max|ref| of fp64 on A^+ y and on the
PGDM gradient for these kernels although P reaches 1 / rtol = 33, so 2e-5 leaves about 80x
headroom.  The helper takes the operator's own keep mask: a frequency at the threshold is never
decided differently by the test and by the code.

Largest errors measured on an MI355X over CASES (parity_record has every figure): A 2.6e-7, A^T
2.6e-7, A^+ 2.5e-7, A^+T 2.3e-7, DPS pass-1 v 3.4e-7, pass-2 x' 3.0e-7 (all x max|ref|), ||r||^2
1.6e-7 relative, the fused PGDM v 2.4e-7, the composed one 3.9e-7, fused against composed 3.3e-7,
3.3e-7 against the circular SP_OP_PSF_FFT pass, the DPS trajectory 4.0e-7 relative L2 - at the CPU
fp32 figure.  The PGDM trajectory: 9.0e-4 from the fp32 oracle, the generic step 2.5e-3 from the
fused one, bound 2.2e-2 (the fp32 oracle lies 1.1e-3 from its fp64 run: the truncated inverse
amplifies by up to 1 / rtol)."""

import math

import numpy as np
import pytest
import torch

import periodic_ops as po
import psf_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import closed_form, dps_loop
from oracle.latent_loops import pgdm_reference
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import FFTPSFBlurOperator, PeriodicBlurOperator, PhaseRetrievalOperator
from samplers_amd.operators.blur import gaussian_taps
from samplers_amd.samplers import DPSSampler
from samplers_amd.samplers.dps import FusedDPSStep, GenericDPSStep, make_dps_step

pytestmark = pytest.mark.gpu



def _gauss(k, sigma):
    t = gaussian_taps(k, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


def _randn(k, seed):
    return torch.randn(k, k, generator=torch.Generator().manual_seed(seed)) / k


# shape (C, H, W), R, batch, y_div, PSF
CASES = [
    ((1, 8, 8), 1, 1, 1, lambda: _gauss(3, 0.8)),                # the smallest transform
    ((2, 8, 24), 1, 2, 1, lambda: torch.ones(1, 3) / 3),         # radix 3, rectangular, spectral zeros
    ((3, 16, 16), 4, 4, 2, lambda: _gauss(9, 1.5)),
    ((1, 24, 24), 3, 2, 1, lambda: _randn(7, 3)),                # signed kernel
    ((1, 32, 48), 7, 2, 2, lambda: psf_ops.random_sparse_kernel(7, seed=701)),  # asymmetric, corner tap
    ((1, 64, 96), 16, 3, 3, lambda: _gauss(33, 2.5)),            # several column tiles
    ((3, 256, 256), 30, 1, 1, lambda: _gauss(61, 3.0)),          # the paper's size
    ((1, 512, 1024), 30, 1, 1, lambda: _gauss(61, 3.0)),         # one line per workgroup
]
IDS = [f"{'x'.join(map(str, c[0]))}-R{c[1]}-b{c[2]}-d{c[3]}" for c in CASES]
BOUND = 2e-5


def _route(shape, r):
    """The helper's direct route up to about 2e8 multiply-adds per sample, else its FFT route
    (tests/test_periodic_api.py pins the two to each other)."""
    return "direct" if math.prod(shape) * (2 * r + 1) ** 2 <= 2e8 else "fft"


def _err(got, ref):
    ref = np.asarray(ref, dtype=np.float64).reshape(tuple(got.shape))
    return float(np.abs(got.detach().cpu().double().numpy() - ref).max() / np.abs(ref).max())


def _close(got, ref, what, record=None, bound=BOUND):
    err = _err(got, ref)
    print(f"{what}: max err / max|ref| = {err:.3g}")
    if record is not None:
        record(what, err, bound)
    assert err <= bound, (what, err)


_CACHE = {}


def _case(i):
    """The case's operator (host), PSF, inputs and fp64 references; computed once and shared,
    never modified."""
    if i not in _CACHE:
        shape, r, batch, ydiv, make = CASES[i]
        op = PeriodicBlurOperator(shape, make())
        assert op.radius == r
        kept = float(op.keep.float().mean())
        assert 0.0 < kept < 1.0, kept  # a projection that is neither the identity nor zero
        g = torch.Generator().manual_seed(23 + i)
        n = math.prod(shape)
        x, eps, w, xi, cot = (torch.randn(batch, n, generator=g) for _ in range(5))
        y = torch.randn(batch // ydiv, n, generator=g)
        h, keep, route = op.kernel, op.keep, _route(shape, r)
        x4, c4 = x.reshape(batch, *shape), cot.reshape(batch, *shape)
        refs = {"A": po.apply64(x4, h, route).numpy(), "AT": po.adjoint64(c4, h, route).numpy(),
                "pinv": po.pinv(c4.double(), h, keep).numpy(),
                "pinvT": po.pinv(x4.double(), h, keep, transpose=True).numpy()}
        _CACHE[i] = (op, h, (x, eps, w, xi, y, cot), refs, route)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_four_maps_and_their_backwards(cuda, parity_record, i):
    shape, r, batch, ydiv, _ = CASES[i]
    host_op, h, (x, _, _, _, _, cot), refs, _ = _case(i)
    op = PeriodicBlurOperator(shape, h).to(cuda)
    assert torch.equal(op.keep.cpu(), host_op.keep)
    xd, cd = x.reshape(batch, *shape).to(cuda), cot.reshape(batch, *shape).to(cuda)
    ax, atc = op.apply(xd), op.apply_transpose(cd)
    pc = op.apply_pseudo_inverse(cd)
    for t in (ax, atc, pc):
        assert tuple(t.shape) == (batch, *shape) and t.dtype == torch.float32
    _close(ax, refs["A"], "apply_max_err_over_max", parity_record)
    _close(atc, refs["AT"], "adjoint_max_err_over_max", parity_record)
    _close(pc, refs["pinv"], "pinv_max_err_over_max", parity_record)
    # autograd: the backward of each map is its transpose - the same launches, the same bits
    xr = xd.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=cd)
    assert torch.equal(gx, atc)
    cr = cd.clone().requires_grad_()
    (gc,) = torch.autograd.grad(op.apply_transpose(cr), cr, grad_outputs=xd)
    assert torch.equal(gc, ax)
    cr = cd.clone().requires_grad_()
    (ptx,) = torch.autograd.grad(op.apply_pseudo_inverse(cr), cr, grad_outputs=xd)   # A^+T x
    _close(ptx, refs["pinvT"], "pinv_transpose_max_err_over_max", parity_record)
    # ... to any order: the backward of the backward is A^+ again
    xr = xd.clone().requires_grad_()
    cr = cd.clone().requires_grad_()
    (inner,) = torch.autograd.grad(op.apply_pseudo_inverse(cr), cr, grad_outputs=xr,
                                   create_graph=True)
    (back,) = torch.autograd.grad(inner, xr, grad_outputs=cd)
    assert torch.equal(back, pc)
    # every sample is computed alone: the bits do not depend on the batch
    assert torch.equal(op.apply(xd[-1:]), ax[-1:])
    assert torch.equal(op.apply_transpose(cd[-1:]), atc[-1:])
    assert torch.equal(op.apply_pseudo_inverse(cd[-1:]), pc[-1:])
    # leading batch dimensions are kept
    two = op.apply_pseudo_inverse(cd.reshape(batch, 1, *shape))
    assert tuple(two.shape) == (batch, 1, *shape) and torch.equal(two.reshape(pc.shape), pc)


def test_adjoint_identities_on_the_device(cuda):
    """<A x, y> = <x, A^T y> and <A^+ x, y> = <x, A^+T y> to fp32 accumulation accuracy."""
    shape, b = (2, 32, 48), 2
    g = torch.Generator().manual_seed(8)
    x, y = (torch.randn(b, *shape, generator=g).to(cuda) for _ in range(2))
    op = PeriodicBlurOperator(shape, psf_ops.random_sparse_kernel(7, seed=701)).to(cuda)
    ax, aty = op.apply(x).double(), op.apply_transpose(y).double()
    lhs, rhs = float((ax * y.double()).sum()), float((x.double() * aty).sum())
    assert abs(lhs - rhs) <= 2e-5 * float(ax.norm() * y.double().norm()), (lhs, rhs)
    px = op.apply_pseudo_inverse(x).double()
    yr = y.clone().requires_grad_()
    (pty,) = torch.autograd.grad(op.apply_pseudo_inverse(yr), yr, grad_outputs=y)   # A^+T y
    lhs, rhs = float((px * y.double()).sum()), float((x.double() * pty.double()).sum())
    assert abs(lhs - rhs) <= 2e-5 * float(px.norm() * y.double().norm()), (lhs, rhs)


@pytest.mark.parametrize("i", [4, 5], ids=[IDS[4], IDS[5]])
def test_agrees_with_the_fft_kind_on_circular_padding(cuda, parity_record, i):
    """apply, A^T and DPS pass 1 against FFTPSFBlurOperator(padding="circular") on the device (the
    same map through padded_size(H + 2R) transforms), within the sum of the two bounds."""
    shape, r, batch, ydiv, _ = CASES[i]
    _, h, (x, eps, _, _, y, cot), refs, _ = _case(i)
    new = PeriodicBlurOperator(shape, h).to(cuda)
    old = FFTPSFBlurOperator(shape, h, padding="circular").to(cuda)
    xd, cd = x.reshape(batch, *shape).to(cuda), cot.reshape(batch, *shape).to(cuda)
    for got, want, ref, what in ((new.apply(xd), old.apply(xd), refs["A"], "apply"),
                                 (new.apply_transpose(cd), old.apply_transpose(cd), refs["AT"],
                                  "adjoint")):
        err = float((got - want).abs().max()) / float(np.abs(ref).max())
        parity_record(f"{what}_vs_fft_kind_over_max", err, 4e-5)
        assert err <= 4e-5, (what, err)
    lib = _hip.load_library()
    coefs = _hip.SpDpsCoefs(0.3, math.sqrt(1 - 0.09), 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    xf, ef, yf = (t.to(cuda).contiguous() for t in (x, eps, y))
    vs, rsqs = [], []
    for op in (new, old):
        desc = op.hip_descriptor()
        P = int(lib.sp_rsq_partials(desc))
        v, part = torch.empty_like(xf), torch.empty(batch, P, device=cuda)
        work = torch.empty(int(lib.sp_dps_workspace(desc, batch)), device=cuda)
        _hip.check(lib.sp_dps_residual_ws(desc, xf.data_ptr(), ef.data_ptr(), yf.data_ptr(), batch,
                                          ydiv, coefs, v.data_ptr(), part.data_ptr(),
                                          work.data_ptr(), _stream()), "residual_ws")
        vs.append(v)
        rsqs.append(part.double().sum(1))
    err = float((vs[0] - vs[1]).abs().max() / vs[1].abs().max())
    parity_record("pass1_v_vs_fft_kind_over_max", err, 4e-5)
    assert err <= 4e-5, err
    assert float((rsqs[0] / rsqs[1] - 1).abs().max()) <= 4e-5


def _sched_of(coefs, step):
    recs = (_hip.SpStepRec * 2)()
    recs[0].c, recs[0].step, recs[0].t = _hip.SpDpsCoefs(0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1
    recs[1].c, recs[1].step, recs[1].t = coefs, step, 5
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8)


def _lines(N):
    NP = (N + N // 16) | 1
    return max(1, min(16, (32000 - 8 * N) // (16 * NP)))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fused_dps_passes_match_closed_form(cuda, parity_record, i):
    """Both DPS passes against the fp64 closed form, with the constants of
    test_psf_fft_gpu.py::test_fused_dps_passes_match_closed_form; the _sched_ws form bit-identical
    to the by-value one."""
    shape, r, batch, ydiv, _ = CASES[i]
    _, h, (x, eps, w, xi, y, _), _, route = _case(i)
    op = PeriodicBlurOperator(shape, h).to(cuda)
    apply_np, adjoint_np = po.periodic_ops(shape, h, route)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    a, k, gs = 0.3, math.sqrt(1 - 0.09), 400.0
    c_ell, c_s, std, gamma = 0.9, 0.2, 0.1, 0.05
    coefs = _hip.SpDpsCoefs(a, k, gs, c_ell, c_s, std, gamma, 1e-9)
    P = int(lib.sp_rsq_partials(desc))
    floats = int(lib.sp_dps_workspace(desc, batch))
    assert P == shape[0] * -(-shape[1] // _lines(shape[2]))  # one partial per (plane, row tile)
    assert floats == 2 * batch * shape[0] * (shape[2] // 2 + 1) * shape[1]
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
    print(f"periodic passes {shape} R={r}: v {v_err:.3g} rsq {rsq_err:.3g} x' {out_err:.3g} P={P}")
    parity_record("pass1_v_max_err_over_max", v_err, BOUND)
    parity_record("pass1_rsq_max_rel_err", rsq_err, BOUND)
    parity_record("pass2_x_max_err_over_max", out_err, BOUND)
    assert v_err <= BOUND and rsq_err <= BOUND and out_err <= BOUND
    # the samples of a batch are independent: the last one alone gives the same bits
    v1, part1 = torch.full_like(xd[-1:], float("nan")), torch.full((1, P), float("nan"), device=cuda)
    _hip.check(lib.sp_dps_residual_ws(desc, xd[-1:].data_ptr(), ed[-1:].data_ptr(),
                                      yd[(batch - 1) // ydiv:].data_ptr(), 1, 1, coefs,
                                      v1.data_ptr(), part1.data_ptr(), work.data_ptr(), _stream()),
               "residual_ws")
    assert torch.equal(v1, v[-1:]) and torch.equal(part1, part[-1:])
    # the _sched_ws form reads record 1 through the cursor: the same bits
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
    # the form without a workspace does not serve the kind
    assert lib.sp_dps_residual(desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv, coefs,
                               v.data_ptr(), part.data_ptr(), _stream()) == -3


def _pgdm_v(lib, op, x, eps, y, ydiv, coefs, cuda, guard=False):
    """sp_pgdm_prepare + sp_pgdm_residual_ws on flat device tensors."""
    desc = op.hip_descriptor()
    batch, rows = x.shape[0], y.shape[0]
    qf = int(lib.sp_op_workspace(desc, rows))
    wf = int(lib.sp_op_workspace(desc, batch))
    qg = torch.full((qf + 16,), float("nan"), device=cuda)
    wg = torch.full((wf + 16,), float("nan"), device=cuda)
    q, work = qg[:qf], wg[:wf]
    _hip.check(lib.sp_pgdm_prepare(desc, y.data_ptr(), rows, q.data_ptr(), _stream()), "prepare")
    v = torch.full_like(x, float("nan"))
    _hip.check(lib.sp_pgdm_residual_ws(desc, x.data_ptr(), eps.data_ptr(), q.data_ptr(), batch, ydiv,
                                       coefs, v.data_ptr(), work.data_ptr(), _stream()),
               "pgdm_residual_ws")
    if guard:  # Q and the intermediate written whole, nothing past their ends
        assert torch.isfinite(q).all() and torch.isnan(qg[qf:]).all()
        assert torch.isfinite(work).all() and torch.isnan(wg[wf:]).all()
    return v


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fused_pgdm_pass(cuda, parity_record, i):
    """v = grad_scale (A^+ y - Pi x0), x0 = (x - k eps) / a, against the fp64 closed form and
    against the same v composed from sp_op_apply_ws and sp_op_pinv_ws."""
    shape, r, batch, ydiv, _ = CASES[i]
    host_op, h, (x, eps, _, _, y, _), _, route = _case(i)
    op = PeriodicBlurOperator(shape, h).to(cuda)
    lib, desc = _hip.load_library(), op.hip_descriptor()
    a, k, gs = 0.3, math.sqrt(1 - 0.09), -2.0
    coefs = _hip.SpDpsCoefs(a, k, gs, 0.9, 0.2, 0.1, 0.05, 1e-9)
    xd, ed, yd = (t.to(cuda).contiguous() for t in (x, eps, y))
    v = _pgdm_v(lib, op, xd, ed, yd, ydiv, coefs, cuda, guard=True)
    x0 = ((x.double() - k * eps.double()) / a).reshape(batch, *shape)
    rows = y.double().reshape(batch // ydiv, *shape).repeat_interleave(ydiv, dim=0)
    ref = po.pgdm_grad(x0, rows, h, host_op.keep).numpy()
    _close(v.reshape(batch, *shape), ref, "pgdm_v_max_err_over_max", parity_record)
    if batch <= 4 and math.prod(shape) <= 4096:  # the autograd form of the reference's loss
        auto = po.pgdm_grad_autograd(x0, rows, h, host_op.keep, route).numpy()
        assert np.abs(auto - ref).max() <= 1e-12 * np.abs(ref).max()
    # composed: x0, A x0, y - A x0, A^+ of it, the scale
    x0d = torch.empty_like(xd)
    _hip.check(lib.sp_predict_x0(xd.data_ptr(), ed.data_ptr(), xd.numel(), a, k, x0d.data_ptr(),
                                 _stream()), "predict_x0")
    work = torch.empty(int(lib.sp_op_workspace(desc, batch)), device=cuda)
    ax, comp = torch.empty_like(xd), torch.empty_like(xd)
    _hip.check(lib.sp_op_apply_ws(desc, x0d.data_ptr(), ax.data_ptr(), batch, work.data_ptr(),
                                  _stream()), "apply_ws")
    res = (yd.repeat_interleave(ydiv, dim=0) - ax).contiguous()
    _hip.check(lib.sp_op_pinv_ws(desc, res.data_ptr(), comp.data_ptr(), batch, 0, work.data_ptr(),
                                 _stream()), "pinv_ws")
    _close((gs * comp).reshape(batch, *shape), ref, "pgdm_v_composed_max_err_over_max", parity_record)
    err = float((v - gs * comp).abs().max()) / float(np.abs(ref).max())
    parity_record("pgdm_v_fused_vs_composed_over_max", err, BOUND)
    assert err <= BOUND, err


def test_pgdm_pass_is_batch_invariant(cuda):
    """The fused PGDM v of a sample is bitwise the same alone, in a batch of 4 and at y_div = 2."""
    shape = (3, 16, 16)
    op = PeriodicBlurOperator(shape, _gauss(9, 1.5)).to(cuda)
    lib = _hip.load_library()
    g = torch.Generator().manual_seed(31)
    n = math.prod(shape)
    x, eps = (torch.randn(4, n, generator=g).to(cuda) for _ in range(2))
    y2 = torch.randn(2, n, generator=g).to(cuda)
    coefs = _hip.SpDpsCoefs(0.3, math.sqrt(1 - 0.09), -2.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    paired = _pgdm_v(lib, op, x, eps, y2, 2, coefs, cuda)                              # y_div = 2
    four = _pgdm_v(lib, op, x, eps, y2.repeat_interleave(2, dim=0).contiguous(), 1, coefs, cuda)
    assert torch.isfinite(paired).all() and torch.equal(paired, four)
    for b in range(4):
        alone = _pgdm_v(lib, op, x[b:b + 1].contiguous(), eps[b:b + 1].contiguous(),
                        y2[b // 2:b // 2 + 1].contiguous(), 1, coefs, cuda)
        assert torch.equal(alone, four[b:b + 1]), b


def _problem(shape, r, b, seed, dev):
    h = psf_ops.random_sparse_kernel(r, seed=100 * r + 1)
    op = PeriodicBlurOperator(shape, h)
    assert 0.0 < float(op.keep.float().mean()) < 1.0
    x_true = si.fixture_x_true(b, shape, seed)
    y = op.apply(x_true)  # F.conv2d on the host
    y = y + 0.05 * torch.randn(tuple(y.shape), generator=torch.Generator().manual_seed(seed + 1))
    return h, op.keep.clone(), y, InverseProblem(op.to(dev), y.to(dev), GaussianNoise(0.05).to(dev))


def test_make_dps_step_is_the_fused_step_in_both_modes(cuda):
    shape = (3, 32, 32)
    _, _, _, prob = _problem(shape, 4, 2, 0, cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    rows = prob.observation.reshape(2, *shape)
    step = make_dps_step(net, prob, rows, 1)
    assert type(step) is FusedDPSStep and step.mode == "dps" and step.q is None
    assert step.needs_v and step.workspace(2, prob.observation) is not None
    step = make_dps_step(net, prob, rows, 1, mode="pgdm", guidance_weight=0.05)
    assert type(step) is FusedDPSStep and step.mode == "pgdm" and step.grad_scale == -2.0
    assert step.q is not None and tuple(step.q.shape) == (2, 2 * 3 * 17 * 32)


def test_pgdm_is_still_rejected_for_the_other_fft_kinds(cuda):
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    for op in (FFTPSFBlurOperator((3, 32, 32), psf_ops.random_sparse_kernel(4, seed=1)),
               PhaseRetrievalOperator((3, 16, 16), pad=8)):
        op = op.to(cuda)
        y = torch.zeros(2, *op.y_shape, device=cuda)
        prob = InverseProblem(op, y, GaussianNoise(0.05).to(cuda))
        with pytest.raises(NotImplementedError):
            FusedDPSStep(net, prob, y, 1, mode="pgdm")


def test_pgdm_matches_oracle_fused_and_generic(cuda, parity_record, monkeypatch):
    """The test of every layer: PGDMSampler on the fused step (sp_pgdm_prepare once,
    sp_pgdm_residual_ws per step) against the oracle loop, which differentiates
    ||A^+ y - A^+ A x0||^2 through the helper's maps, and against GenericDPSStep, which
    differentiates through the operator's own HIP apply and apply_pseudo_inverse."""
    from samplers_amd.samplers import pgdm as pgdm_mod
    from samplers_amd.samplers.pgdm import PGDMSampler

    shape, r, b, N = (3, 32, 32), 4, 2, 8
    h, keep, y, prob = _problem(shape, r, b, 0, cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    init, steps = si.replay_noise(5, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    made = []
    real = pgdm_mod.make_dps_step
    monkeypatch.setattr(pgdm_mod, "make_dps_step",
                        lambda *a, **kw: made.append(real(*a, **kw)) or made[-1])
    out = PGDMSampler(net)(prob, num_sampling_steps=N, guidance_weight=0.05, noise_fn=fn)
    assert type(made[-1]) is FusedDPSStep and made[-1].grad_scale == -2.0
    assert made[-1].q is not None
    monkeypatch.setattr(pgdm_mod, "make_dps_step", lambda *a, **kw: GenericDPSStep(*a, **kw))
    generic = PGDMSampler(net)(prob, num_sampling_steps=N, guidance_weight=0.05, noise_fn=fn)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)

    def run(dt):
        c = si.EpsCore("conv", 3, 0.1).to(dt)
        return pgdm_reference(lambda x, t: c(x, t), acp.to(dt),
                              si.leading_timesteps_ascending(N).tolist(),
                              lambda x: po.blur(x, h), lambda v: po.pinv(v, h, keep),
                              y.to(dt), init.to(dt), lambda i: steps[i].to(dt),
                              guidance_weight=0.05, eta=1.0)

    ref = run(torch.float32)
    cond = si.relative_error(run(torch.float64), ref)
    bound = max(1e-4, 20 * cond)
    err, err_generic = si.relative_error(out.cpu(), ref), si.relative_error(generic.cpu(), out.cpu())
    print("pgdm periodic", err, err_generic, "bound", bound)
    parity_record("pgdm_rel_l2", err, bound)
    parity_record("pgdm_generic_vs_fused_rel_l2", err_generic, bound)
    assert err < bound
    assert err_generic < bound


def test_dps_matches_oracle(cuda, parity_record):
    shape, r, b, N = (3, 32, 32), 4, 2, 8
    h, _, y, prob = _problem(shape, r, b, 0, cuda)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    init, steps = si.replay_noise(21, (b, *shape), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DPSSampler(net)(prob, num_sampling_steps=N, gamma=1e-2, eta=1.0, noise_fn=fn)
    core = si.EpsCore("conv", 3, 0.1)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1)
    ref = dps_loop.dps_reference(lambda x, t: core(x, t), acp,
                                 si.leading_timesteps_ascending(N).tolist(),
                                 lambda x: po.blur(x, h), dps_loop.gaussian_log_prob(0.05), y, init,
                                 lambda i: steps[i], gamma=1e-2, eta=1.0)
    err = si.relative_error(out.cpu(), ref)
    print("dps periodic", err)
    parity_record("dps_rel_l2", err, 1e-4)
    assert err < 1e-4


DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import psf_ops
from samplers_amd import _hip
from samplers_amd.operators import PeriodicBlurOperator
from samplers_amd.operators.blur import gaussian_taps
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
gen = torch.Generator().manual_seed(1)
def gauss(k, s):
    t = gaussian_taps(k, s).double()
    return torch.outer(t, t).float()
cases = (((1, 8, 8), gauss(3, 0.8)), ((2, 8, 24), torch.ones(1, 3) / 3), ((3, 16, 16), gauss(9, 1.5)),
         ((1, 24, 24), torch.randn(7, 7, generator=gen) / 7),
         ((1, 32, 48), psf_ops.random_sparse_kernel(7, seed=701)))
for shape, h in cases:
    op = PeriodicBlurOperator(shape, h).to(dev)
    desc = op.hip_descriptor()
    b, n = 4, int(desc.n)
    P = int(lib.sp_rsq_partials(desc))
    x, eps, w, g = (torch.randn(b, n, device=dev) for _ in range(4))
    y = torch.randn(b // 2, n, device=dev)
    outs = [torch.empty(b, n, device=dev) for _ in range(4)]
    work = torch.empty(int(lib.sp_op_workspace(desc, b)), device=dev)
    _hip.check(lib.sp_op_apply_ws(desc, x.data_ptr(), outs[0].data_ptr(), b, work.data_ptr(), st), "apply")
    _hip.check(lib.sp_op_vjp_ws(desc, x.data_ptr(), g.data_ptr(), outs[1].data_ptr(), b, work.data_ptr(),
                                st), "vjp")
    for tr in (0, 1):
        _hip.check(lib.sp_op_pinv_ws(desc, g.data_ptr(), outs[2 + tr].data_ptr(), b, tr, work.data_ptr(),
                                     st), "pinv")
    c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    v, part, out = torch.empty_like(x), torch.empty(b, P, device=dev), torch.empty_like(x)
    _hip.check(lib.sp_dps_residual_ws(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 2, c,
                                      v.data_ptr(), part.data_ptr(), work.data_ptr(), st),
               "sp_dps_residual_ws")
    _hip.check(lib.sp_dps_update(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v.data_ptr(),
                                 w.data_ptr(), part.data_ptr(), None, 7, 3, 0, b, 2, c,
                                 out.data_ptr(), st), "sp_dps_update")
    c = _hip.SpDpsCoefs(0.3, 0.95, -2.0, 0.9, 0.2, 0.1, -0.05, 1e-9)
    q = torch.empty(int(lib.sp_op_workspace(desc, b // 2)), device=dev)
    v2, out2 = torch.empty_like(x), torch.empty_like(x)
    _hip.check(lib.sp_pgdm_prepare(desc, y.data_ptr(), b // 2, q.data_ptr(), st), "sp_pgdm_prepare")
    _hip.check(lib.sp_pgdm_residual_ws(desc, x.data_ptr(), eps.data_ptr(), q.data_ptr(), b, 2, c,
                                       v2.data_ptr(), work.data_ptr(), st), "sp_pgdm_residual_ws")
    _hip.check(lib.sp_dps_update(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), v2.data_ptr(),
                                 w.data_ptr(), None, None, 7, 3, 0, b, 2, c, out2.data_ptr(), st),
               "sp_dps_update (pgdm)")
    nv, site = _hip.debug_violations()
    print(shape, "violations", nv, site, flush=True)
    assert nv == 0, (shape, nv, site)
    for t in outs + [out, out2]:
        assert torch.isfinite(t).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh child
    process (a process holds one library): the four maps, a DPS step and a PGDM step over the
    first five cases."""
    run_debug_child(DEBUG_CHILD)
