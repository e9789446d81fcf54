"""The proximal data step and the DiffPIR step on the GPU (sp_op_prox_ws, sp_diffpir_step_ws,
sp_prox_prepare; csrc/sp_dps.hip, sp_sr.hip, sp_psf_fft.hip), through the raw entry points into
NaN-filled outputs between guard bands, against the fp64 semantics of tests/prox_ref.py; then
Operator.apply_prox on device tensors and DiffPIRSampler against the reference loop.

Shapes are the smallest at which each kernel can go wrong: a scalar tail only, two keep words,
the vector body, several workgroups with n % 4 != 0; every SR patch shape (scalar, two blocks per
patch, one, a lane pair) with one and several blocks; periodic transforms of both radices, one and
several column tiles, several planes.  Every case runs at (batch 3, y_div 3) and (batch 4, y_div 2).

Bounds.  Exact cases (integer data, a = k = 1/2, 1 + rho s^2 = 2): torch.equal, every element -
tests/test_prox_ref.py shows that no fp32 evaluation can round there.  randn data, elementwise
kinds and SR: per element |err| <= n * 2^-24 * E, n the rounding steps of the longest path through
the kernel's arithmetic (counted in ``_roundings``), E the same expression on absolute values.
Periodic: max|err| <= max(2e-5, 4 x the distance of prox_ref's fp32 torch.fft evaluation from fp64
at that shape and rho) x max|ref|; 2e-5 is the periodic suite's bound, the second term is there
because |M| / (|M|^2 + rho) amplifies transform error by up to 1 / (2 sqrt(rho)).
Trajectories: max(1e-4, 20 x the fp32 reference loop's distance to its fp64 run), the rule of
test_pgdm_matches_oracle_fused_and_generic.

Measured on an MI355X: see README.md "DiffPIR" (parity_record has every figure)."""

import math

import pytest
import torch

import periodic_ops as po
import prox_ref as pr
import psf_ops
import stand_ins as si
from exact_cases import Guarded, assert_bitwise
from kind_harness import DEBUG_SWEEP_CHILD, run_debug_child, stream as _stream
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import (IdentityOperator, InpaintingOperator, PeriodicBlurOperator,
                                    RandomInpaintingOperator, SuperResolutionOperator)
from samplers_amd.operators.blur import gaussian_taps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BATCHES = [(3, 3), (4, 2)]  # (batch, y_div)
SEED, STEP, OFFSET = 11, 5, 7


# --- the cases ----------------------------------------------------------------------------------
def _keep(n, mask):
    g = torch.Generator().manual_seed(n)
    if mask == "all":
        return torch.ones(n, dtype=torch.bool)
    if mask == "word":  # one whole keep word dropped
        k = torch.ones(n, dtype=torch.bool)
        k[:64] = False
        if not k.any():
            k[n - 1] = True
        return k
    if mask == "one":  # m = 1
        k = torch.zeros(n, dtype=torch.bool)
        k[n // 2] = True
        return k
    k = torch.rand(n, generator=g) < 0.5
    k[0] = True
    return k


def _gauss(k, sigma):
    t = gaussian_taps(k, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


NS = (3, 65, 768, 3 * 33 * 35, 5000)  # the last: several workgroups on the vector path
ELEMENTWISE = ([("identity", n, "all") for n in NS] + [("mask", n, "half") for n in NS]
               + [("inpaint", n, m) for n in NS for m in ("all", "word", "half", "one")])
SR = [((1, 2, 2), 2), ((1, 8, 8), 8), ((3, 16, 24), 2), ((3, 16, 24), 4), ((2, 32, 40), 8),
      ((1, 6, 10), 2)]  # the last: W % 4 != 0, the scalar patch
PERIODIC = [((1, 8, 8), lambda: _gauss(3, 0.8)), ((1, 8, 12), lambda: torch.ones(1, 3) / 3),
            ((1, 24, 16), lambda: _gauss(9, 1.5)),
            ((1, 32, 64), lambda: psf_ops.random_sparse_kernel(7, seed=701)),
            ((3, 64, 48), lambda: _gauss(33, 2.5))]
CASES = ([("ew",) + c for c in ELEMENTWISE] + [("sr",) + c for c in SR]
         + [("periodic", c[0], i) for i, c in enumerate(PERIODIC)])
IDS = ["-".join(str(p).replace(" ", "") for p in c) for c in CASES]
ONE_LAUNCH = [i for i, c in enumerate(CASES) if c[0] != "periodic"]
FFT = [i for i, c in enumerate(CASES) if c[0] == "periodic"]


class Case:
    """The operator (device), its descriptor, and its fp64 / fp32 closed form on flat rows."""

    def __init__(self, case, device):
        fam = case[0]
        self.fam, self.h = fam, None
        if fam == "ew":
            _, kind, n, mask = case
            keep = _keep(n, mask)
            self.keep = keep
            if kind == "identity":
                self.op = IdentityOperator((n,))
            else:
                self.op = InpaintingOperator((n,), ~keep, flatten=kind == "inpaint")
            packed = kind != "mask"
            self.prox = lambda x0, y, rho: pr.mask_prox(x0, y, keep, rho, packed)
            self.s = 1
        elif fam == "sr":
            _, shape, s = case
            self.op = SuperResolutionOperator(shape, s)
            ys = self.op.y_shape
            self.prox = lambda x0, y, rho: pr.sr_prox(x0.reshape(-1, *shape), y.reshape(-1, *ys), s,
                                                      rho).reshape(x0.shape)
            self.s = s
        else:
            _, shape, i = case
            h = PERIODIC[i][1]()
            self.op = PeriodicBlurOperator(shape, h)
            kept = float(self.op.keep.float().mean())
            assert 0.0 < kept < 1.0, kept  # some frequencies kept, some dropped
            self.h = self.op.kernel.clone()
            hh = self.h
            self.prox = lambda x0, y, rho: pr.periodic_prox(x0.reshape(-1, *shape),
                                                            y.reshape(-1, *shape), hh, rho).reshape(x0.shape)
            self.s = 1
        self.op = self.op.to(device)
        self.desc = self.op.hip_descriptor()
        self.n, self.m = int(self.desc.n), int(self.desc.m)


_CASES = {}


def _case(i, device):
    if i not in _CASES:
        _CASES[i] = Case(CASES[i], device)
    return _CASES[i]


def _prepare(lib, c, y):
    """q of the kinds that prepare (written whole, nothing past its ends), else None."""
    rows = y.shape[0]
    size = int(lib.sp_prox_prepare_size(c.desc, rows))
    assert size >= 0
    q = Guarded((size,), 64, y.device) if size else None
    _hip.check(lib.sp_prox_prepare(c.desc, y.data_ptr(), rows, q.ptr() if q else None, _stream()),
               "sp_prox_prepare")
    return q.check() if q else None


def _work(lib, c, batch, device):
    floats = int(lib.sp_prox_workspace(c.desc, batch))
    assert floats >= 0
    return Guarded((floats,), 64, device) if floats else None


def run_prox(lib, c, x0, y, ydiv, rho, q=None):
    batch = x0.shape[0]
    q = _prepare(lib, c, y) if q is None else q
    work, out = _work(lib, c, batch, x0.device), Guarded((batch, c.n), 64, x0.device)
    _hip.check(lib.sp_op_prox_ws(c.desc, x0.data_ptr(), y.data_ptr(), q.data_ptr() if q is not None else None,
                                 batch, ydiv, rho, out.ptr(), work.ptr() if work else None, _stream()),
               "sp_op_prox_ws")
    if work:
        work.check()
    return out.check()


def run_step(lib, c, x, eps, y, xi, ydiv, coefs, alias=False, offset=OFFSET, q=None):
    batch = x.shape[0]
    q = _prepare(lib, c, y) if q is None else q
    work, out = _work(lib, c, batch, x.device), Guarded((batch, c.n), 64, x.device)
    if alias:
        out.t.copy_(x)
    src = out.t if alias else x
    _hip.check(lib.sp_diffpir_step_ws(c.desc, src.data_ptr(), eps.data_ptr(), y.data_ptr(),
                                      q.data_ptr() if q is not None else None,
                                      xi.data_ptr() if xi is not None else None, SEED, STEP, offset,
                                      batch, ydiv, coefs, out.ptr(), work.ptr() if work else None,
                                      _stream()), "sp_diffpir_step_ws")
    if work:
        work.check()
    return out.check()


def _randn(lib, batch, n, device, offset=OFFSET):
    xi = torch.empty(batch, n, device=device)
    _hip.check(lib.sp_randn(xi.data_ptr(), batch, n, SEED, STEP, offset, _stream()), "sp_randn")
    return xi


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _coefs(rho, exact=False):
    if exact:
        return _hip.SpProxCoefs(0.5, 0.5, rho, 0.5, 0.25, 0.125), dict(pr.EXACT)
    vals = dict(a=_f32(0.8), k=_f32(0.6), a_prev=_f32(0.9), c_eps=_f32(0.35), c_xi=_f32(0.25))
    return _hip.SpProxCoefs(vals["a"], vals["k"], rho, vals["a_prev"], vals["c_eps"], vals["c_xi"]), vals


def _rows(y, ydiv):
    return y.repeat_interleave(ydiv, dim=0)


# --- bitwise: exact cases, Philox, aliasing, composition ------------------------------------------
@pytest.mark.parametrize("batch,ydiv", BATCHES)
@pytest.mark.parametrize("i", ONE_LAUNCH, ids=[IDS[i] for i in ONE_LAUNCH])
def test_exact_cases_are_bitwise(cuda, i, batch, ydiv):
    lib, c = _hip.load_library(), _case(i, cuda)
    rho = pr.exact_rho(c.s)
    x, eps, xi, y = pr.exact_inputs(batch, c.n, batch // ydiv, c.m, 100 + i)
    z64, out64 = pr.step_from_prox(x.double(), eps.double(), xi.double(), _rows(y, ydiv).double(),
                                   c.prox, rho)
    x0 = pr.predict_x0(x, eps, 0.5, 0.5)
    xd, ed, xid, yd, x0d = (t.to(cuda).contiguous() for t in (x, eps, xi, y, x0))
    coefs, _ = _coefs(rho, exact=True)
    z = run_prox(lib, c, x0d, yd, ydiv, rho)
    assert_bitwise(z, z64, "z")
    out = run_step(lib, c, xd, ed, yd, xid, ydiv, coefs)
    assert_bitwise(out, out64, "x'")
    assert torch.equal(run_step(lib, c, xd, ed, yd, xid, ydiv, coefs, alias=True), out)  # x_out = x
    # composition: sp_predict_x0 -> sp_op_prox_ws -> the update in torch
    p0 = torch.empty_like(xd)
    _hip.check(lib.sp_predict_x0(xd.data_ptr(), ed.data_ptr(), xd.numel(), 0.5, 0.5, p0.data_ptr(),
                                 _stream()), "sp_predict_x0")
    zc = run_prox(lib, c, p0, yd, ydiv, rho)
    comp = pr.diffpir_update(xd, zc, xid, **pr.EXACT)
    assert torch.equal(comp, out)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_philox_is_sp_randn_and_aliasing(cuda, i):
    """xi = NULL draws the bits of sp_randn(seed, step, offset) at the flat element index, for all
    five kinds; x_out = x gives the same bits."""
    lib, c = _hip.load_library(), _case(i, cuda)
    batch, ydiv = 4, 2
    g = torch.Generator().manual_seed(200 + i)
    x, eps = (torch.randn(batch, c.n, generator=g).to(cuda) for _ in range(2))
    y = torch.randn(batch // ydiv, c.m, generator=g).to(cuda)
    coefs, _ = _coefs(_f32(0.37))
    q = _prepare(lib, c, y)
    given = run_step(lib, c, x, eps, y, _randn(lib, batch, c.n, cuda), ydiv, coefs, q=q)
    drawn = run_step(lib, c, x, eps, y, None, ydiv, coefs, q=q)
    assert torch.equal(drawn, given)
    assert torch.equal(run_step(lib, c, x, eps, y, None, ydiv, coefs, alias=True, q=q), drawn)
    other = run_step(lib, c, x, eps, y, None, ydiv, coefs, offset=OFFSET + 1, q=q)
    assert not torch.equal(other, drawn)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_batch_invariance(cuda, i):
    """A sample alone, in a batch of 4 and at y_div = 2: the same bits, and the same bits twice."""
    lib, c = _hip.load_library(), _case(i, cuda)
    g = torch.Generator().manual_seed(300 + i)
    x, eps = (torch.randn(4, c.n, generator=g).to(cuda) for _ in range(2))
    y = torch.randn(2, c.m, generator=g).to(cuda)
    rho = _f32(0.02)
    coefs, _ = _coefs(rho)
    full = run_step(lib, c, x, eps, y, None, 2, coefs)
    assert torch.equal(run_step(lib, c, x, eps, y, None, 2, coefs), full)
    zfull = run_prox(lib, c, x, y, 2, rho)
    assert torch.equal(run_prox(lib, c, x, y, 2, rho), zfull)
    for b in (0, 3):
        alone = run_step(lib, c, x[b:b + 1].contiguous(), eps[b:b + 1].contiguous(),
                         y[b // 2:b // 2 + 1].contiguous(), None, 1, coefs, offset=OFFSET + b)
        assert torch.equal(alone, full[b:b + 1]), b
        zalone = run_prox(lib, c, x[b:b + 1].contiguous(), y[b // 2:b // 2 + 1].contiguous(), 1, rho)
        assert torch.equal(zalone, zfull[b:b + 1]), b


# --- error bounds on randn data ---------------------------------------------------------------------
def _roundings(c):
    """Rounding steps of the longest path through the kernels' arithmetic (csrc/sp_dps.hip k_prox,
    csrc/sp_sr.hip k_sr_prox), for z given x0 and for x' given x, eps:
      x0 = (x - k eps) * (1 / a)             k eps, the difference, 1 / a, the product      4
      mean of the block                      a balanced tree over s^2 terms: log2(s^2)      (SR)
      d = (y - A x0) * (1 / (1 + rho s^2))   the difference, 1 + rho s^2, its reciprocal,
                                             the product                                    4
      z = x0 + d                                                                            1
      eps_hat = (x - a z) * (1 / k)          a z, the difference, 1 / k, the product        4
      x' = a_prev z + (c_eps eps_hat + c_xi xi)   c_eps eps_hat, the inner sum, the outer   3
    A product by a rounded reciprocal carries the reciprocal's steps too (relative errors of the
    two factors add), a sum carries the longer of its two operands' paths.  a, k, rho and the
    other scalars are fp32 numbers that the fp64 reference takes as they are.
    """
    tree = int(math.log2(c.s * c.s))
    return tree + 5, 4 + tree + 5 + 4 + 3


def _abs_expression(c, x, eps, xi, y_rows, rho, v):
    """The step's expression on absolute values, in fp64: (E of z given x0, E of x')."""
    ax0 = (x.abs() + v["k"] * eps.abs()) / v["a"]

    def e_of_z(a0):
        zero = torch.zeros_like(a0)
        # prox of |.|: x0 + A^T(|y| + A|x0|) / (1 + rho s^2) = |x0| + (prox(0, |y|) + prox(|x0|, 0) ...)
        d_y = c.prox(zero, y_rows.abs(), rho)            # A^T |y| / (gram + rho)
        d_x = a0 - c.prox(a0, torch.zeros_like(y_rows), rho)  # A^T A |x0| / (gram + rho)
        return a0 + d_y + d_x

    ez_prox = e_of_z(x.abs())  # the prox form takes x as x0
    ez = e_of_z(ax0)
    eeh = (x.abs() + v["a"] * ez) / v["k"]
    return ez_prox, v["a_prev"] * ez + v["c_eps"] * eeh + v["c_xi"] * xi.abs()


@pytest.mark.parametrize("rho", pr.RHOS)
@pytest.mark.parametrize("i", ONE_LAUNCH, ids=[IDS[i] for i in ONE_LAUNCH])
def test_error_bound_one_launch_kinds(cuda, parity_record, i, rho):
    lib, c = _hip.load_library(), _case(i, cuda)
    rho = _f32(rho)
    coefs, v = _coefs(rho)
    n_z, n_out = _roundings(c)
    worst = [0.0, 0.0]
    for batch, ydiv in BATCHES:
        g = torch.Generator().manual_seed(400 + i)
        x, eps, xi = (torch.randn(batch, c.n, generator=g) for _ in range(3))
        y = torch.randn(batch // ydiv, c.m, generator=g)
        yr = _rows(y, ydiv).double()
        z64 = c.prox(x.double(), yr, rho)
        _, out64 = pr.step_from_prox(x.double(), eps.double(), xi.double(), yr, c.prox, rho, v)
        ez, eout = _abs_expression(c, x.double(), eps.double(), xi.double(), yr, rho, v)
        xd, ed, xid, yd = (t.to(cuda).contiguous() for t in (x, eps, xi, y))
        z = run_prox(lib, c, xd, yd, ydiv, rho).cpu().double()
        out = run_step(lib, c, xd, ed, yd, xid, ydiv, coefs).cpu().double()
        worst[0] = max(worst[0], float(((z - z64).abs() / (n_z * U * ez)).max()))
        worst[1] = max(worst[1], float(((out - out64).abs() / (n_out * U * eout)).max()))
        # composition on randn: sp_predict_x0 -> sp_op_prox_ws -> torch, within the same bound
        p0 = torch.empty_like(xd)
        _hip.check(lib.sp_predict_x0(xd.data_ptr(), ed.data_ptr(), xd.numel(), v["a"], v["k"],
                                     p0.data_ptr(), _stream()), "sp_predict_x0")
        comp = pr.diffpir_update(xd, run_prox(lib, c, p0, yd, ydiv, rho), xid, **v).cpu().double()
        worst.append(float(((comp - out64).abs() / (n_out * U * eout)).max()))
    print(f"{IDS[i]} rho={rho:g}: z {worst[0]:.3f} x' {worst[1]:.3f} composed {max(worst[2:]):.3f} (bound 1)")
    parity_record("prox_err_over_bound", worst[0], 1.0, rho=rho)
    parity_record("step_err_over_bound", worst[1], 1.0, rho=rho)
    parity_record("composed_err_over_bound", max(worst[2:]), 1.0, rho=rho)
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and max(worst[2:]) <= 1.0, worst


@pytest.mark.parametrize("rho", pr.RHOS)
@pytest.mark.parametrize("i", FFT, ids=[IDS[i] for i in FFT])
def test_error_bound_periodic(cuda, parity_record, i, rho):
    lib, c = _hip.load_library(), _case(i, cuda)
    rho = _f32(rho)
    coefs, v = _coefs(rho)
    for batch, ydiv in BATCHES:
        g = torch.Generator().manual_seed(500 + i)
        x, eps, xi = (torch.randn(batch, c.n, generator=g) for _ in range(3))
        y = torch.randn(batch // ydiv, c.m, generator=g)
        yr = _rows(y, ydiv)
        z64 = c.prox(x.double(), yr.double(), rho)
        z64s, out64 = pr.step_from_prox(x.double(), eps.double(), xi.double(), yr.double(), c.prox, rho, v)
        z32 = c.prox(x, yr, rho)
        _, out32 = pr.step_from_prox(x, eps, xi, yr, c.prox, rho, v)
        xd, ed, xid, yd = (t.to(cuda).contiguous() for t in (x, eps, xi, y))
        z = run_prox(lib, c, xd, yd, ydiv, rho).cpu().double()
        out = run_step(lib, c, xd, ed, yd, xid, ydiv, coefs).cpu().double()
        p0 = torch.empty_like(xd)
        _hip.check(lib.sp_predict_x0(xd.data_ptr(), ed.data_ptr(), xd.numel(), v["a"], v["k"],
                                     p0.data_ptr(), _stream()), "sp_predict_x0")
        comp = pr.diffpir_update(xd, run_prox(lib, c, p0, yd, ydiv, rho), xid, **v).cpu().double()
        for what, got, ref, ref32 in (("prox", z, z64, z32), ("step", out, out64, out32),
                                      ("composed", comp, out64, out32)):
            scale = float(ref.abs().max())
            yard = float((ref32.double() - ref).abs().max()) / scale
            bound = max(2e-5, 4 * yard)
            err = float((got - ref).abs().max()) / scale
            print(f"{IDS[i]} rho={rho:g} b{batch}: {what} err {err:.3g} torch.fft fp32 {yard:.3g} bound {bound:.3g}")
            parity_record(f"periodic_{what}_max_err_over_max", err, bound, rho=rho, fp32_fft=yard)
            assert err <= bound, (what, err, bound)


# --- Operator.apply_prox on device tensors ----------------------------------------------------------
@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c[0] != "ew" or c[2] == 3 * 33 * 35],
                         ids=lambda i: IDS[i])
def test_device_apply_prox_matches_the_host(cuda, parity_record, i):
    lib, c = _hip.load_library(), _case(i, cuda)
    host = type(c.op).__name__
    g = torch.Generator().manual_seed(600 + i)
    x0 = torch.randn(2, 2, *c.op.x_shape, generator=g)  # two leading batch dimensions
    y = torch.randn(2, 2, *c.op.y_shape, generator=g)
    for rho in pr.RHOS:
        got = c.op.apply_prox(x0.to(cuda), y.to(cuda), rho)
        assert got.shape == x0.shape and got.is_cuda and got.dtype == torch.float32
        ref = c.prox(x0.reshape(4, -1).double(), y.reshape(4, -1).double(), _f32(rho)).reshape(x0.shape)
        err = (got.cpu().double() - ref).abs()
        if c.fam == "periodic":
            ref32 = c.prox(x0.reshape(4, -1), y.reshape(4, -1), _f32(rho)).reshape(x0.shape)
            scale = float(ref.abs().max())
            bound = max(2e-5, 4 * float((ref32.double() - ref).abs().max()) / scale)
            assert float(err.max()) / scale <= bound, (host, rho)
        else:
            ez, _ = _abs_expression(c, x0.reshape(4, -1).double(), x0.reshape(4, -1).double(),
                                    x0.reshape(4, -1).double(), y.reshape(4, -1).double(), _f32(rho),
                                    _coefs(rho)[1])
            worst = float((err.reshape(4, -1) / (_roundings(c)[0] * U * ez)).max())
            parity_record("apply_prox_err_over_bound", worst, 1.0, rho=rho)
            assert worst <= 1.0, (host, rho, worst)


# --- trajectories -----------------------------------------------------------------------------------
SHAPE, B, N, SIGMA = (3, 32, 32), 2, 8, 0.05


def _traj_problem(name, cuda, rows):
    g = torch.Generator().manual_seed(41)
    x_true = si.fixture_x_true(rows, SHAPE, seed=9)
    if name == "inpaint":
        op = RandomInpaintingOperator(SHAPE, 0.5, seed=3)
        keep = ~op.mask.reshape(-1)
        apply = lambda x: x.reshape(x.shape[0], -1)[:, keep]  # noqa: E731
        prox = lambda x0, y, rho: pr.mask_prox(x0.reshape(x0.shape[0], -1), y, keep,  # noqa: E731
                                               rho).reshape(x0.shape)
    elif name == "sr":
        op = SuperResolutionOperator(SHAPE, 4)
        apply = lambda x: torch.nn.functional.avg_pool2d(x, 4)  # noqa: E731
        prox = lambda x0, y, rho: pr.sr_prox(x0, y, 4, rho)  # noqa: E731
    else:
        h = _gauss(9, 1.5)
        op = PeriodicBlurOperator(SHAPE, h)
        hk = op.kernel.clone()
        apply = lambda x: po.blur(x, hk)  # noqa: E731
        prox = lambda x0, y, rho: pr.periodic_prox(x0, y, hk, rho)  # noqa: E731
    y = apply(x_true.double()).float()
    y = y + SIGMA * torch.randn(y.shape, generator=g)
    op = op.to(cuda)
    prob = InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))
    return prob, y, apply, prox


def _reference(dt, y, apply, prox, init, steps, ydiv):
    core = si.EpsCore("conv", 3, 0.1).to(dt)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).to(dt)
    return pr.diffpir_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                                apply, prox, _rows(y, ydiv).to(dt), init.to(dt),
                                lambda i: steps[i].to(dt), sigma=SIGMA)


@pytest.mark.parametrize("name,recon", [("inpaint", 1), ("sr", 1), ("periodic", 1), ("sr", 2)])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, name, recon):
    from samplers_amd.samplers import DiffPIRSampler

    prob, y, apply, prox = _traj_problem(name, cuda, B)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    grads = []
    inner = net.forward

    def forward(x, t):
        e = inner(x, t)
        grads.append(bool(e.requires_grad) or torch.is_grad_enabled())
        return e

    net.forward = forward
    init, steps = si.replay_noise(17, (B * recon, *SHAPE), N)
    fn = lambda kind, i, sh: (init if kind == "init" else steps[i]).to(cuda)  # noqa: E731
    out = DiffPIRSampler(net)(prob, num_sampling_steps=N, num_reconstructions=recon, noise_fn=fn)
    assert tuple(out.shape) == ((B, *SHAPE) if recon == 1 else (B, recon, *SHAPE))
    assert len(grads) >= 2 and not any(grads)  # every network call ran under no_grad: no graph
    ref32 = _reference(torch.float32, y, apply, prox, init, steps, recon)
    cond = si.relative_error(_reference(torch.float64, y, apply, prox, init, steps, recon), ref32)
    bound = max(1e-4, 20 * cond)
    err = si.relative_error(out.reshape(ref32.shape).cpu(), ref32)
    print(f"diffpir {name} R={recon}: rel l2 {err:.3g}, fp32 reference to fp64 {cond:.3g}, bound {bound:.3g}")
    parity_record("diffpir_rel_l2", err, bound, fp32_to_fp64=cond)
    assert err < bound


def test_philox_trajectory_is_reproducible(cuda):
    from samplers_amd.samplers import DiffPIRSampler

    prob, *_ = _traj_problem("inpaint", cuda, B)
    net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
    one = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=1234)
    two = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=1234)
    assert torch.equal(one, two) and torch.isfinite(one).all()
    assert not torch.equal(DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=1235), one)
    halves = DiffPIRSampler(net)(prob, num_sampling_steps=N, seed=1234, micro_batch=1)
    assert torch.equal(halves, one)  # the bits do not depend on the chunking


# --- the bounds-checked library -----------------------------------------------------------------------
def debug_sweep(device):
    """Every case through sp_prox_prepare, sp_op_prox_ws and both noise forms of
    sp_diffpir_step_ws; run by the child process under the debug library."""
    lib = _hip.load_library()
    for i in range(len(CASES)):
        c = _case(i, device)
        for batch, ydiv in BATCHES:
            x, eps = (torch.randn(batch, c.n, device=device) for _ in range(2))
            y = torch.randn(batch // ydiv, c.m, device=device)
            coefs, _ = _coefs(_f32(0.05))
            outs = [run_prox(lib, c, x, y, ydiv, _f32(0.05)),
                    run_step(lib, c, x, eps, y, None, ydiv, coefs),
                    run_step(lib, c, x, eps, y, _randn(lib, batch, c.n, device), ydiv, coefs)]
            assert all(torch.isfinite(t).all() for t in outs)
        nv, site = _hip.debug_violations()
        print(IDS[i], "violations", nv, site, flush=True)
        assert nv == 0, (IDS[i], nv, site)


DEBUG_CHILD = DEBUG_SWEEP_CHILD("test_diffpir_gpu")


def test_debug_build_has_no_violations(cuda):
    """The new kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library), over every shape of this file."""
    run_debug_child(DEBUG_CHILD)
