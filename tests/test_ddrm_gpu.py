"""The DDRM step on the GPU (sp_ddrm_step_ws; csrc/sp_dps.hip k_ddrm, sp_sr.hip k_sr_ddrm,
sp_psf_fft.hip k_pf_rows_ddrm / k_pf_cols_ddrm), through the raw entry point into NaN-filled
outputs and a NaN-filled workspace between guard bands, against the fp64 forms of
tests/ddrm_ref.py; then DDRMSampler against the reference loop.

Shapes: identity n = 3 (a scalar tail only), 4099 (several workgroups, n % 4 != 0), 5000 (the
vector body); inpainting n = 5000 with every element kept, alternating and a random half, the mask
kind with none kept (the packed kind has no descriptor with m = 0) and at 3x8x8; every SR patch
shape of tests/test_diffpir_gpu.py; periodic transforms of both radices, one and several column
tiles, several planes.  Every case runs at (batch 3, y_div 3) and (batch 4, y_div 2).

Scalar regimes: every observed component big, every one small, sig_y = 0, sig_prev = 0; for the
periodic kind also a threshold that cuts the kept spectrum with at least 10 % of it in each class
(asserted on the host).  The A A^T = g I cases keep sig_prev^2 g a factor >= 2 from sig_y^2: near
equality f_xi is a difference of nearly equal squares, a property of the map.

Bounds.  Exact cases (tests/ddrm_ref.py: integer data, dyadic scalars): every element equal to the
fp64 result.  randn data, one-launch kinds: per element |err| <= n_r * 2^-24 * E, n_r the rounding
steps of the longest path through the kernel (12; SR 15 + log2 s^2, counted in the kernels'
comments), E the kernel's expression on absolute values (1 - r -> 1 + r, the difference under the
square root a sum).  Periodic: max|err| <= max(2e-5, 4 x the distance of the fp32 torch.fft
evaluation from fp64) x max|ref|, the reference given the fp32 class mask.  Trajectories:
max(1e-4, 20 x the fp32 reference loop's distance to its fp64 run).

Measured on an MI355X: see README.md "DDRM" (parity_record has every figure)."""

import math

import pytest
import torch

import ddrm_ref as dr
import periodic_ops as po
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
    if mask == "all":
        return torch.ones(n, dtype=torch.bool)
    if mask == "none":
        return torch.zeros(n, dtype=torch.bool)
    if mask == "alternating":
        return torch.arange(n) % 2 == 0
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5


def _gauss(k, sigma):
    t = gaussian_taps(k, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


def _dense(k, seed):
    h = torch.rand(k, k, generator=torch.Generator().manual_seed(seed))
    return h / h.sum()


ELEMENTWISE = ([("identity", (n,), "all") for n in (3, 4099, 5000)]
               + [("inpaint", (5000,), m) for m in ("all", "alternating", "half")]
               + [("mask", (5000,), "none"), ("mask", (3, 8, 8), "half")])
SR = [((1, 2, 2), 2), ((1, 8, 8), 8), ((3, 16, 24), 2), ((3, 16, 24), 4), ((2, 32, 40), 8),
      ((1, 6, 10), 2)]  # the last: W % 4 != 0, the scalar patch
PERIODIC = [((1, 8, 8), lambda: _gauss(3, 0.8)), ((1, 8, 12), lambda: _gauss(5, 1.0)),
            ((2, 32, 32), lambda: _dense(15, 77)), ((3, 64, 48), lambda: _gauss(11, 2.0))]
CASES = ([("ew",) + c for c in ELEMENTWISE] + [("sr",) + c for c in SR]
         + [("periodic", c[0], i) for i, c in enumerate(PERIODIC)])
IDS = ["-".join(str(p).replace(" ", "") for p in c) for c in CASES]
ONE_LAUNCH = [i for i, c in enumerate(CASES) if c[0] != "periodic"]
FFT = [i for i, c in enumerate(CASES) if c[0] == "periodic"]


class Case:
    """The operator (device), its descriptor, and what its fp64 / fp32 form needs, on flat rows."""

    def __init__(self, case, device):
        self.fam = case[0]
        self.s = 1
        if self.fam == "ew":
            _, kind, shape, mask = case
            n = math.prod(shape)
            self.keep = _keep(n, mask)
            self.packed = kind != "mask"
            if kind == "identity":
                self.op = IdentityOperator(shape)
            else:
                self.op = InpaintingOperator(shape, ~self.keep.reshape(shape), flatten=self.packed)
            self.proj, self.up = dr.mask_ops(self.keep, self.packed)
        elif self.fam == "sr":
            _, shape, s = case
            self.op, self.s = SuperResolutionOperator(shape, s), s
            self.proj, self.up = dr.sr_ops(shape, s)
        else:
            _, shape, i = case
            self.op = PeriodicBlurOperator(shape, PERIODIC[i][1]())
            self.shape = shape
            self.keep = self.op.keep.clone()
            self.M32 = po.transfer(self.op.kernel, *shape[1:]).to(torch.complex64)  # what the kernel reads
            self.s2 = dr.s2_of_spectrum32(self.M32)
        self.g = 1.0 / (self.s * self.s)
        self.op = self.op.to(device)
        self.desc = self.op.hip_descriptor()
        self.n, self.m = int(self.desc.n), int(self.desc.m)

    def y_device(self, y, device):
        """y on the device; the mask kind's unobserved entries are NaN (the step must not use them)."""
        yd = y.clone()
        if self.fam == "ew" and not self.packed:
            yd[:, ~self.keep] = float("nan")
        return yd.to(device).contiguous()

    def reference(self, x, eps, y_rows, xi, c, dtype=torch.float64):
        """The step in ``dtype`` (fp32: plain torch / torch.fft), the class mask the fp32 one."""
        t = lambda v: v.to(dtype)  # noqa: E731
        if self.fam == "periodic":
            r = lambda v: t(v).reshape(-1, *self.shape)  # noqa: E731
            big = dr.big_mask32(self.s2, c)
            return dr.dft_step(r(x), r(eps), r(y_rows), r(xi), c, self.M32, self.keep, big).reshape(x.shape)
        big = dr.big_mask32(torch.tensor(self.g, dtype=torch.float32), c)
        return dr.projector_step(t(x), t(eps), self.up(t(y_rows)), t(xi), c, self.g, self.proj, big)


_CASES = {}


def _case(i, device):
    if i not in _CASES:
        _CASES[i] = Case(CASES[i], device)
    return _CASES[i]


def _prepare(lib, c, y):
    """q of the periodic kind (sp_pgdm_prepare's, written whole), else None."""
    if c.fam != "periodic":
        return None
    rows = y.shape[0]
    size = int(lib.sp_op_workspace(c.desc, rows))
    assert size > 0
    q = Guarded((size,), 64, y.device)
    _hip.check(lib.sp_pgdm_prepare(c.desc, y.data_ptr(), rows, q.ptr(), _stream()), "sp_pgdm_prepare")
    return q.check()


def _spcoefs(c):
    return _hip.SpDdrmCoefs(*(c[f] for f, _ in _hip.SpDdrmCoefs._fields_))


def run_step(lib, c, x, eps, y, xi, ydiv, coefs, alias=False, offset=OFFSET, q=None):
    batch = x.shape[0]
    q = _prepare(lib, c, y) if q is None else q
    floats = int(lib.sp_ddrm_workspace(c.desc, batch))
    assert floats >= 0 and (floats > 0) == (c.fam == "periodic")
    work = Guarded((floats,), 64, x.device) if floats else None
    out = Guarded((batch, c.n), 64, x.device)
    if alias:
        out.t.copy_(x)
    src = out.t if alias else x
    _hip.check(lib.sp_ddrm_step_ws(c.desc, src.data_ptr(), eps.data_ptr(), y.data_ptr(),
                                   q.data_ptr() if q is not None else None,
                                   xi.data_ptr() if xi is not None else None, SEED, STEP, offset,
                                   batch, ydiv, _spcoefs(coefs), out.ptr(), work.ptr() if work else None,
                                   _stream()), "sp_ddrm_step_ws")
    if work:
        work.check(nan_ok=True)
    return out.check()


def _randn(lib, batch, n, device, offset=OFFSET):
    xi = torch.empty(batch, n, device=device)
    _hip.check(lib.sp_randn(xi.data_ptr(), batch, n, SEED, STEP, offset, _stream()), "sp_randn")
    return xi


def _rows(y, ydiv):
    return y.repeat_interleave(ydiv, dim=0)


def _inputs(c, batch, ydiv, seed):
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randn(batch, c.n, generator=g) for _ in range(3))
    return x, eps, xi, torch.randn(batch // ydiv, c.m, generator=g)


# --- the scalar regimes ---------------------------------------------------------------------------
def _cut(c):
    """sig_y / sig_prev between two distinct kept |M| next to the median, so no frequency sits on
    the threshold."""
    vals = torch.sort(torch.sqrt(c.s2.double())[c.keep]).values
    k = vals.numel() // 2
    while k + 1 < vals.numel() and vals[k] - vals[k - 1] <= 1e-4 * vals[k]:
        k += 1
    return float(torch.sqrt(vals[k - 1] * vals[k]))


def regimes(c):
    """name -> the eight scalars, rounded to fp32 (what the kernel is given)."""
    rt = math.sqrt(c.g)
    out = {
        "big": dr.make_coefs(0.5, 0.05 * rt, 0.85, 1.0),
        "big_blend": dr.make_coefs(0.5, 0.05 * rt, 0.5, 0.5),
        "small": dr.make_coefs(0.041, 0.5 * rt, 0.85, 1.0),
        "sig_y=0": dr.make_coefs(0.23, 0.0, 0.85, 1.0),
        "sig_prev=0": dr.make_coefs(0.0, 0.05, 0.85, 1.0),
    }
    if c.fam == "periodic":
        out["big"] = dr.make_coefs(3.0, 0.05, 0.85, 1.0)       # kept |M| > 0.03: 3 |M| > 0.05
        out["big_blend"] = dr.make_coefs(3.0, 0.05, 0.5, 0.5)
        out["small"] = dr.make_coefs(0.041, 0.05, 0.85, 1.0)   # |M| <= 1
        out["cut"] = dr.make_coefs(0.5, 0.5 * _cut(c), 0.85, 0.75)
    return {k: dr.round32(v) for k, v in out.items()}


REGIMES = ("big", "big_blend", "small", "sig_y=0", "sig_prev=0")


def test_regimes_are_what_they_say(cuda):
    dropping = 0
    for i in range(len(CASES)):
        c = _case(i, cuda)
        rg = regimes(c)
        if c.fam != "periodic":
            g32 = torch.tensor(c.g, dtype=torch.float32)
            for name in ("big", "big_blend", "small"):
                v = rg[name]
                ratio = v["sig_prev"] ** 2 * c.g / v["sig_y"] ** 2
                assert (ratio >= 2 or ratio <= 0.5) and bool(dr.big_mask32(g32, v)) == (ratio > 1), name
            continue
        kept = c.keep
        dropping += int(not bool(kept.all()))
        assert bool(kept.any())
        for name, want in (("big", 1.0), ("big_blend", 1.0), ("small", 0.0)):
            assert float(dr.big_mask32(c.s2, rg[name])[kept].float().mean()) == want, (IDS[i], name)
        share = float(dr.big_mask32(c.s2, rg["cut"])[kept].float().mean())
        assert 0.1 <= share <= 0.9, (IDS[i], share)  # each class holds >= 10 % of the kept spectrum
        far = (rg["cut"]["sig_prev"] ** 2 * c.s2.double() / rg["cut"]["sig_y"] ** 2 - 1).abs() > 1e-5
        assert bool(far[kept].all())  # and nothing sits on the threshold
    assert dropping >= 2  # at least two of the PSFs drop frequencies


# --- bitwise: exact cases, Philox, aliasing, batch invariance ---------------------------------------
@pytest.mark.parametrize("regime", ["big", "small"])
@pytest.mark.parametrize("i", ONE_LAUNCH, ids=[IDS[i] for i in ONE_LAUNCH])
def test_exact_cases_are_bitwise(cuda, i, regime):
    lib, c = _hip.load_library(), _case(i, cuda)
    coefs = dr.exact_coefs(regime, c.s)
    for batch, ydiv in BATCHES:
        x, eps, xi, y = dr.exact_inputs(batch, c.n, batch // ydiv, c.m, 100 + i)
        ref = c.reference(x, eps, _rows(y, ydiv), xi, coefs)
        xd, ed, xid = (t.to(cuda).contiguous() for t in (x, eps, xi))
        out = run_step(lib, c, xd, ed, c.y_device(y, cuda), xid, ydiv, coefs)
        assert_bitwise(out, ref, f"x' b{batch}")
        assert torch.equal(run_step(lib, c, xd, ed, c.y_device(y, cuda), xid, ydiv, coefs, alias=True), out)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_philox_is_sp_randn_and_aliasing(cuda, i):
    """xi = NULL draws the bits of sp_randn(seed, step, offset) at the flat element index, for all
    five kinds; x_out = x gives the same bits."""
    lib, c = _hip.load_library(), _case(i, cuda)
    batch, ydiv = 4, 2
    x, eps, _, y = _inputs(c, batch, ydiv, 200 + i)
    xd, ed, yd = x.to(cuda), eps.to(cuda), c.y_device(y, cuda)
    q = _prepare(lib, c, yd)
    for name in ("big", "small") + (("cut",) if c.fam == "periodic" else ()):
        coefs = regimes(c)[name]
        given = run_step(lib, c, xd, ed, yd, _randn(lib, batch, c.n, cuda), ydiv, coefs, q=q)
        drawn = run_step(lib, c, xd, ed, yd, None, ydiv, coefs, q=q)
        assert torch.equal(drawn, given), name
        assert torch.equal(run_step(lib, c, xd, ed, yd, None, ydiv, coefs, alias=True, q=q), drawn)
        other = run_step(lib, c, xd, ed, yd, None, ydiv, coefs, offset=OFFSET + 1, q=q)
        assert not torch.equal(other, drawn)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_batch_invariance(cuda, i):
    """A sample alone against a batch of 4, y_div = 2 against repeated rows, and the same bits
    twice."""
    lib, c = _hip.load_library(), _case(i, cuda)
    x, eps, _, y = _inputs(c, 4, 2, 300 + i)
    xd, ed, yd = x.to(cuda), eps.to(cuda), c.y_device(y, cuda)
    coefs = regimes(c)["cut" if c.fam == "periodic" else "big_blend"]
    full = run_step(lib, c, xd, ed, yd, None, 2, coefs)
    assert torch.equal(run_step(lib, c, xd, ed, yd, None, 2, coefs), full)
    rep = run_step(lib, c, xd, ed, _rows(yd, 2).contiguous(), None, 1, coefs)
    assert torch.equal(rep, full)
    for b in (0, 3):
        alone = run_step(lib, c, xd[b:b + 1].contiguous(), ed[b:b + 1].contiguous(),
                         yd[b // 2:b // 2 + 1].contiguous(), None, 1, coefs, offset=OFFSET + b)
        assert torch.equal(alone, full[b:b + 1]), b


# --- error bounds on randn data ---------------------------------------------------------------------
def _abs_coefficients(v, g):
    """(|f_th|, f_y, |f_xi|, c1 sig_prev, eta sig_prev) of the observed set with every difference
    taken as a sum: what the kernels' expression gives on absolute values."""
    sp, sy, eb = v["sig_prev"], v["sig_y"], v["eta_b"]
    ce, es = v["c1"] * sp, v["eta"] * sp
    if bool(dr.big_mask32(torch.tensor(g, dtype=torch.float32), v)):
        return 1 + eb, eb, math.sqrt(sp * sp + (eb * sy) ** 2 / g), ce, es
    r = ce * math.sqrt(g) / sy
    return 1 + r, r, es, ce, es


def _roundings(c):
    """k_ddrm: 12; k_sr_ddrm: 15 + log2 s^2 (the kernels' comments count them)."""
    return 12 if c.fam == "ew" else 15 + int(math.log2(c.s * c.s))


def _abs_expression(c, x, eps, xi, y_rows, v):
    ath, fy, axi, ce, es = _abs_coefficients(v, c.g)
    ax0 = (x.abs() + v["k"] * eps.abs()) / v["a"]
    yu = c.up(y_rows.abs())
    if c.fam == "ew":  # observed: f_th x0 + f_y y + f_xi xi; unobserved: x0 + c1 sig' eps + eta sig' xi
        obs = ath * ax0 + fy * yu + axi * xi.abs()
        uno = ax0 + ce * eps.abs() + es * xi.abs()
        return v["a_prev"] * torch.where(c.keep, obs, uno)
    tail = c.proj((ath + 1) * ax0 + ce * eps.abs() + (axi + es) * xi.abs())
    return v["a_prev"] * (ax0 + ce * eps.abs() + es * xi.abs() + tail + fy * yu)


def _composed(lib, c, xd, ed, yd, ydiv, v):
    """The same x' from the existing entry points: sp_predict_x0, sp_randn, the operator's device
    maps (or torch.fft on the device for the periodic kind) and torch elementwise ops."""
    x0 = torch.empty_like(xd)
    _hip.check(lib.sp_predict_x0(xd.data_ptr(), ed.data_ptr(), xd.numel(), v["a"], v["k"], x0.data_ptr(),
                                 _stream()), "sp_predict_x0")
    xi = _randn(lib, xd.shape[0], c.n, xd.device)
    yr = _rows(torch.nan_to_num(yd), ydiv)
    dev = xd.device
    if c.fam == "periodic":
        r = lambda t: t.reshape(-1, *c.shape)  # noqa: E731
        big = dr.big_mask32(c.s2, v).to(dev)
        return dr.dft_step(r(xd), r(ed), r(yr), r(xi), v, c.M32.to(dev), c.keep.to(dev), big,
                           x0=r(x0)).reshape(xd.shape)
    shape = (-1, *c.op.x_shape)
    at = lambda t: c.op.apply_transpose(t.reshape(-1, *c.op.y_shape)).reshape(xd.shape[0], -1)  # noqa: E731
    proj = lambda t: at(c.op.apply(t.reshape(shape))) / c.g  # noqa: E731
    big = dr.big_mask32(torch.tensor(c.g, dtype=torch.float32), v)
    return dr.projector_step(xd, ed, at(yr) / c.g, xi, v, c.g, proj, big, x0=x0)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("i", ONE_LAUNCH, ids=[IDS[i] for i in ONE_LAUNCH])
def test_error_bound_one_launch_kinds(cuda, parity_record, i, regime):
    lib, c = _hip.load_library(), _case(i, cuda)
    v = regimes(c)[regime]
    n_r = _roundings(c)
    worst, worst_c = 0.0, 0.0
    for batch, ydiv in BATCHES:
        x, eps, _, y = _inputs(c, batch, ydiv, 400 + i)
        xd, ed, yd = x.to(cuda), eps.to(cuda), c.y_device(y, cuda)
        xi = _randn(lib, batch, c.n, cuda).cpu()  # the composition draws the same plane
        yr = _rows(y, ydiv)
        ref = c.reference(x, eps, yr, xi, v)
        e = _abs_expression(c, x.double(), eps.double(), xi.double(), yr.double(), v)
        out = run_step(lib, c, xd, ed, yd, None, ydiv, v).cpu().double()
        comp = _composed(lib, c, xd, ed, yd, ydiv, v).cpu().double()
        tiny = 1e-300  # sig_prev = 0 and an unobserved element: E = a_prev |x0| > 0 still
        worst = max(worst, float(((out - ref).abs() / (n_r * U * e + tiny)).max()))
        worst_c = max(worst_c, float(((comp - ref).abs() / (n_r * U * e + tiny)).max()))
    print(f"{IDS[i]} {regime}: x' {worst:.3f} composed {worst_c:.3f} (bound 1, n_r {n_r})")
    parity_record("ddrm_step_err_over_bound", worst, 1.0, regime=regime)
    parity_record("ddrm_composed_err_over_bound", worst_c, 1.0, regime=regime)
    assert worst <= 1.0 and worst_c <= 1.0, (worst, worst_c)


@pytest.mark.parametrize("regime", REGIMES + ("cut",))
@pytest.mark.parametrize("i", FFT, ids=[IDS[i] for i in FFT])
def test_error_bound_periodic(cuda, parity_record, i, regime):
    lib, c = _hip.load_library(), _case(i, cuda)
    v = regimes(c)[regime]
    for batch, ydiv in BATCHES:
        x, eps, _, y = _inputs(c, batch, ydiv, 500 + i)
        xd, ed, yd = x.to(cuda), eps.to(cuda), c.y_device(y, cuda)
        xi = _randn(lib, batch, c.n, cuda).cpu()
        yr = _rows(y, ydiv)
        ref = c.reference(x, eps, yr, xi, v)
        ref32 = c.reference(x, eps, yr, xi, v, torch.float32).double()
        out = run_step(lib, c, xd, ed, yd, None, ydiv, v).cpu().double()
        comp = _composed(lib, c, xd, ed, yd, ydiv, v).cpu().double()
        scale = float(ref.abs().max())
        yard = float((ref32 - ref).abs().max()) / scale
        bound = max(2e-5, 4 * yard)
        for what, got in (("step", out), ("composed", comp)):
            err = float((got - ref).abs().max()) / scale
            print(f"{IDS[i]} {regime} b{batch}: {what} err {err:.3g} torch.fft fp32 {yard:.3g} bound {bound:.3g}")
            parity_record(f"ddrm_periodic_{what}_max_err_over_max", err, bound, regime=regime, fp32_fft=yard)
            assert err <= bound, (what, err, bound)


# --- trajectories -----------------------------------------------------------------------------------
SHAPE, B, N, SIGMA = (3, 32, 32), 2, 8, 0.05


def _traj_problem(name, cuda, rows):
    """(problem, y, step_fn(dtype)) for the reference loop."""
    g = torch.Generator().manual_seed(41)
    x_true = si.fixture_x_true(rows, SHAPE, seed=9)
    flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
    if name == "inpaint":
        op = RandomInpaintingOperator(SHAPE, 0.5, seed=3)
        keep = ~op.mask.reshape(-1)
        y = flat(x_true)[:, keep]
        proj, up = dr.mask_ops(keep)
        gain = 1.0
    elif name == "sr":
        op = SuperResolutionOperator(SHAPE, 4)
        y = torch.nn.functional.avg_pool2d(x_true, 4)
        proj, up = dr.sr_ops(SHAPE, 4)
        gain = 1.0 / 16
    else:
        op = PeriodicBlurOperator(SHAPE, _gauss(9, 1.5))
        y = po.blur(x_true.double(), op.kernel).float()
        M32 = po.transfer(op.kernel, 32, 32).to(torch.complex64)
        keep, s2 = op.keep.clone(), dr.s2_of_spectrum32(M32)
    y = y + SIGMA * torch.randn(y.shape, generator=g)

    def step_fn(x, eps, yy, xi, c):
        c32 = dr.round32(c)
        if name == "periodic":
            return dr.dft_step(x, eps, yy, xi, c, M32, keep, dr.big_mask32(s2, c32))
        big = dr.big_mask32(torch.tensor(gain, dtype=torch.float32), c32)
        out = dr.projector_step(flat(x), flat(eps), up(flat(yy)), flat(xi), c, gain, proj, big)
        return out.reshape(x.shape)

    return op.to(cuda), y, step_fn


def _reference(dt, y, step_fn, init, steps, ydiv, sigma_y):
    core = si.EpsCore("conv", 3, 0.1).to(dt)
    acp = torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).to(dt)
    return dr.ddrm_reference(lambda x, t: core(x, t), acp, si.leading_timesteps_ascending(N).tolist(),
                             step_fn, _rows(y, ydiv).to(dt), init.to(dt), lambda i: steps[i].to(dt),
                             sigma_y=sigma_y)


@pytest.mark.parametrize("name,recon,noise_std", [("inpaint", 1, None), ("sr", 1, None), ("sr", 2, None),
                                                  ("periodic", 1, None), ("sr", 1, 0.0)])
def test_trajectory_matches_the_reference_loop(cuda, parity_record, name, recon, noise_std):
    from samplers_amd.samplers import DDRMSampler

    op, y, step_fn = _traj_problem(name, cuda, B)
    prob = InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))
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
    out = DDRMSampler(net)(prob, num_sampling_steps=N, num_reconstructions=recon, noise_std=noise_std,
                           noise_fn=fn)
    assert tuple(out.shape) == ((B, *SHAPE) if recon == 1 else (B, recon, *SHAPE))
    assert len(grads) >= 2 and not any(grads)  # every network call ran under no_grad: no graph
    sy = SIGMA if noise_std is None else noise_std
    ref32 = _reference(torch.float32, y, step_fn, init, steps, recon, sy)
    cond = si.relative_error(_reference(torch.float64, y, step_fn, init, steps, recon, sy), ref32)
    bound = max(1e-4, 20 * cond)
    err = si.relative_error(out.reshape(ref32.shape).cpu(), ref32)
    print(f"ddrm {name} R={recon} noise_std={noise_std}: rel l2 {err:.3g}, fp32 reference to fp64 "
          f"{cond:.3g}, bound {bound:.3g}")
    parity_record("ddrm_rel_l2", err, bound, fp32_to_fp64=cond)
    assert err < bound


def test_philox_trajectory_is_reproducible(cuda):
    from samplers_amd.samplers import DDRMSampler

    for name in ("inpaint", "periodic"):
        op, y, _ = _traj_problem(name, cuda, B)
        prob = InverseProblem(op, y.to(cuda), GaussianNoise(SIGMA).to(cuda))
        net = si.make_samplers_amd_net("conv", 3, 0.1, device=cuda)
        one = DDRMSampler(net)(prob, num_sampling_steps=N, seed=1234)
        two = DDRMSampler(net)(prob, num_sampling_steps=N, seed=1234)
        assert torch.equal(one, two) and torch.isfinite(one).all()
        assert not torch.equal(DDRMSampler(net)(prob, num_sampling_steps=N, seed=1235), one)
        halves = DDRMSampler(net)(prob, num_sampling_steps=N, seed=1234, micro_batch=1)
        assert torch.equal(halves, one)  # the bits do not depend on the chunking


# --- the bounds-checked library -----------------------------------------------------------------------
def debug_sweep(device):
    """Every case and regime through both noise forms of sp_ddrm_step_ws; run by the child process
    under the debug library."""
    lib = _hip.load_library()
    for i in range(len(CASES)):
        c = _case(i, device)
        for batch, ydiv in BATCHES:
            x, eps, _, y = _inputs(c, batch, ydiv, 700 + i)
            xd, ed, yd = x.to(device), eps.to(device), c.y_device(y, device)
            for name, v in regimes(c).items():
                outs = [run_step(lib, c, xd, ed, yd, None, ydiv, v),
                        run_step(lib, c, xd, ed, yd, _randn(lib, batch, c.n, device), ydiv, v)]
                assert all(torch.isfinite(t).all() for t in outs), (IDS[i], name)
        nv, site = _hip.debug_violations()
        print(IDS[i], "violations", nv, site, flush=True)
        assert nv == 0, (IDS[i], nv, site)


DEBUG_CHILD = DEBUG_SWEEP_CHILD("test_ddrm_gpu")


def test_debug_build_has_no_violations(cuda):
    """The new kernels' SP_DCHECK index invariants under the bounds-checked library, in a fresh
    child process (a process holds one library), over every shape of this file."""
    run_debug_child(DEBUG_CHILD)
