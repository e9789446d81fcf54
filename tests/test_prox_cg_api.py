"""The conjugate-gradient proximal map on the host: ``Operator.apply_prox_cg`` of every operator
class against the dense solve, what raises and by which name, the new keywords of the DiffPIR
sampler, and the return codes and workspace sizes of sp_prox_cg_workspace, sp_op_prox_cg_ws and
sp_diffpir_step_cg_ws before any launch.

No GPU: the library loads without one and every call here returns before a launch."""

import inspect

import pytest
import torch

import prox_cg_ref as cg
import prox_ref as pr
import stand_ins as si
import test_diffpir_api as D
from samplers_amd import _hip, operators as ops
from samplers_amd.operators.sr_filter import gaussian_filter_taps
from samplers_amd.samplers import DiffPIRSampler, FusedDiffPIRStep

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
PTR = D.PTR

LINEAR = dict(D.WITH_PROX)
LINEAR.update({k: v for k, v in D.WITHOUT_PROX.items() if k != "phase"})
LINEAR["sr_periodic"] = D.make(_hip.SP_OP_SR_PERIODIC, 256, 64, 1, 16, 16, radius=4, factor=2, taps=PTR)
PHASE = D.WITHOUT_PROX["phase"]


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def r4(v):
    return (v + 3) // 4 * 4


def expected_floats(lib, d, batch, step):
    pn, pm = lib.sp_vec_partials(d.n), lib.sp_vec_partials(d.m)
    return ((3 + step) * r4(batch * d.n) + 2 * r4(batch * d.m) + r4(batch * (3 * pn + pm))
            + 4 * batch + lib.sp_op_workspace(d, batch))


def prox_call(lib, d, *, x0=PTR, y=PTR, batch=3, y_div=1, rho=1.0, k=8, tol=1e-6, out=PTR,
              iters=PTR, work=PTR):
    return lib.sp_op_prox_cg_ws(d, x0, y, batch, y_div, rho, k, tol, out, iters, work, None)


def step_call(lib, d, *, x=PTR, eps=PTR, y=PTR, xi=None, batch=3, y_div=1, c="default", k=8,
              tol=1e-4, out=PTR, iters=PTR, work=PTR):
    c = D.coefs() if c == "default" else c
    return lib.sp_diffpir_step_cg_ws(d, x, eps, y, xi, 7, 3, 0, batch, y_div, c, k, tol, out,
                                     iters, work, None)


# --- the library, before any launch ---------------------------------------------------------------
def test_version_and_exports(lib):
    assert lib.sp_version() >= 111
    for name in ("sp_prox_cg_workspace", "sp_op_prox_cg_ws", "sp_diffpir_step_cg_ws"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("name", list(LINEAR))
def test_workspace_is_the_header_formula(lib, name):
    d = LINEAR[name]
    for batch in (1, 3, 64):
        for step in (0, 1):
            assert lib.sp_prox_cg_workspace(d, batch, step) == expected_floats(lib, d, batch, step)
    assert lib.sp_prox_cg_workspace(d, 3, 1) - lib.sp_prox_cg_workspace(d, 3, 0) == r4(3 * d.n)


def test_workspace_figures(lib):
    d = LINEAR["identity"]  # n = m = 12: one partial each, nothing for the maps
    assert lib.sp_prox_cg_workspace(d, 1, 0) == 3 * 12 + 2 * 12 + 4 + 4 == 68
    assert lib.sp_prox_cg_workspace(d, 1, 1) == 80
    big = D.plane(_hip.SP_OP_BLUR, 3, 256, 256, radius=4, taps=PTR)  # the benchmark's shape
    n = 3 * 256 * 256
    assert lib.sp_vec_partials(n) == 96
    assert lib.sp_prox_cg_workspace(big, 64, 1) == 6 * 64 * n + 64 * 4 * 96 + 4 * 64
    fft = LINEAR["periodic"]  # the maps' own workspace last
    assert lib.sp_prox_cg_workspace(fft, 5, 0) == expected_floats(lib, fft, 5, 0)
    assert lib.sp_op_workspace(fft, 5) == 6240


@pytest.mark.parametrize("name", list(LINEAR))
def test_argument_checks(lib, name):
    d = LINEAR[name]
    for bad in ((d, 0, 0), (d, -1, 0), (d, 65536, 0), (d, 3, 2), (d, 3, -1)):
        assert lib.sp_prox_cg_workspace(*bad) == EINVAL, bad[1:]
    nan, inf = float("nan"), float("inf")
    common = (dict(y=None), dict(out=None), dict(work=None), dict(batch=0), dict(batch=65536),
              dict(y_div=0), dict(k=0), dict(k=-3), dict(tol=-1e-9), dict(tol=nan), dict(tol=inf))
    for bad in common + (dict(x0=None), dict(rho=0.0), dict(rho=-1.0), dict(rho=inf), dict(rho=nan)):
        assert prox_call(lib, d, **bad) == EINVAL, bad
    for bad in common + (dict(x=None), dict(eps=None), dict(c=None), dict(c=D.coefs(rho=0.0)),
                         dict(c=D.coefs(rho=-2.0)), dict(c=D.coefs(rho=inf)),
                         dict(c=D.coefs(rho=nan)), dict(c=D.coefs(k=0.0))):
        assert step_call(lib, d, **bad) == EINVAL, bad


@pytest.mark.parametrize("what", list(D.REJECTED))
def test_rejected_descriptor_is_einval(lib, what):
    d = D.REJECTED[what]
    assert lib.sp_prox_cg_workspace(d, 3, 0) == EINVAL and lib.sp_prox_cg_workspace(d, 3, 1) == EINVAL
    assert prox_call(lib, d) == EINVAL and step_call(lib, d) == EINVAL


def test_phase_is_unsupported_after_the_argument_checks(lib):
    assert lib.sp_rsq_partials(PHASE) > 0, "the descriptor itself is valid"
    assert lib.sp_prox_cg_workspace(PHASE, 3, 0) == EUNSUPPORTED
    assert lib.sp_prox_cg_workspace(PHASE, 3, 1) == EUNSUPPORTED
    assert prox_call(lib, PHASE) == EUNSUPPORTED and step_call(lib, PHASE) == EUNSUPPORTED
    assert prox_call(lib, PHASE, iters=None) == EUNSUPPORTED  # iters_out may be NULL
    assert lib.sp_prox_cg_workspace(PHASE, 0, 0) == EINVAL
    assert prox_call(lib, PHASE, rho=0.0) == EINVAL and step_call(lib, PHASE, k=0) == EINVAL


def test_the_closed_form_probe_is_unchanged(lib):
    for name, d in D.WITHOUT_PROX.items():
        assert lib.sp_prox_workspace(d, 3) == EUNSUPPORTED, name
    for name, d in D.WITH_PROX.items():
        assert lib.sp_prox_workspace(d, 3) >= 0, name


# --- apply_prox_cg on host tensors ------------------------------------------------------------------
SHAPE = (3, 8, 16)


def _svd_operator():
    g = torch.Generator().manual_seed(8)
    u, s, vh = torch.linalg.svd(torch.randn(6, 10, generator=g).double(), full_matrices=False)
    # the constructor infers y_shape in fp32; the buffers go to fp64 afterwards
    return ops.GeneralSVDOperator(u.float(), s.float(), vh.float()).double()


def _host_operators():
    mask = D._mask(SHAPE)
    h3 = cg._psf3()
    return {
        "identity": lambda: ops.IdentityOperator(SHAPE),
        "identity_flat": lambda: ops.IdentityOperator(SHAPE, flatten=True),
        "inpaint": lambda: ops.InpaintingOperator(SHAPE, mask),
        "mask": lambda: ops.InpaintingOperator(SHAPE, mask, flatten=False),
        "center": lambda: ops.CenterInpaintingOperator(SHAPE, 0.5),
        "outpaint": lambda: ops.CenterOutpaintingOperator(SHAPE, 0.5),
        "side": lambda: ops.SidePaintingOperator(SHAPE, 0.25),
        "random": lambda: ops.RandomInpaintingOperator(SHAPE, 0.5, seed=3),
        "sr2": lambda: ops.SuperResolutionOperator(SHAPE, 2),
        "sr8": lambda: ops.SuperResolutionOperator(SHAPE, 8),
        "gaussian_blur": lambda: ops.GaussianBlurOperator(SHAPE, 5, 1.0),
        "psf": lambda: ops.PSFBlurOperator(SHAPE, h3),
        "motion": lambda: ops.MotionBlurOperator((1, 16, 16), kernel_size=5, seed=2),
        "psf_fft": lambda: ops.FFTPSFBlurOperator(SHAPE, h3),
        "periodic": lambda: ops.PeriodicBlurOperator((2, 8, 24), h3),
        "sr_periodic": lambda: ops.PeriodicSuperResolutionOperator((1, 16, 16),
                                                                   gaussian_filter_taps(4, 1.0), 2),
        "radon": lambda: ops.RadonOperator((1, 16, 12), num_angles=5),
        "filtered_sr": lambda: ops.FilteredSuperResolutionOperator.gaussian((2, 8, 16), 2, 6, 1.2),
        "bicubic_sr": lambda: ops.BicubicSuperResolutionOperator((1, 16, 16), 2),
        "svd": _svd_operator,
    }


CLOSED = ("identity", "identity_flat", "inpaint", "mask", "center", "outpaint", "side", "random",
          "sr2", "sr8", "periodic", "sr_periodic")


@pytest.mark.parametrize("name", list(_host_operators()))
def test_host_apply_prox_cg_against_the_dense_solve(name):
    op = _host_operators()[name]()
    A = cg.dense(op)
    g = torch.Generator().manual_seed(21)
    x0 = torch.randn(2, *op.x_shape, generator=g).double()
    y = torch.randn(2, *op.y_shape, generator=g).double()
    for rho in pr.RHOS if name in CLOSED else (1.0, 50.0):
        z, iters = op.apply_prox_cg(x0, y, rho, iterations=2000, tol=1e-13, return_iterations=True)
        assert z.shape == x0.shape and z.dtype == torch.float64
        assert iters.shape == (2,) and iters.dtype == torch.int32 and int(iters.max()) < 2000
        want = cg.solve(A, x0.reshape(2, -1), y.reshape(2, -1), rho)
        assert cg.distance(z.reshape(2, -1), want) <= 1e-10, (name, rho)
        # the independent restatement, sample by sample
        ref, _ = cg.cgls(A, x0.reshape(2, -1), y.reshape(2, -1), rho, 2000, 1e-13)
        assert cg.distance(z.reshape(2, -1), ref) <= 1e-10
        if name in CLOSED:  # and the closed forms; the periodic ones divide by an fp32 spectrum,
            # whose rounding reaches z amplified by |M| / (|M|^2 + rho) <= 1 / (2 sqrt(rho))
            # (test_diffpir_api.test_periodic_apply_prox_on_the_host)
            bound = 8 * 2.0 ** -24 * (1 + 1 / (2 * rho ** 0.5)) if "periodic" in name else 1e-9
            assert cg.distance(z, op.apply_prox(x0, y, rho)) <= bound, (name, rho)
    one = op.apply_prox_cg(x0[0], y[0], 1.0, iterations=2000, tol=1e-13)  # no batch dimension
    assert one.shape == x0.shape[1:]
    assert cg.distance(one, op.apply_prox_cg(x0, y, 1.0, iterations=2000, tol=1e-13)[0]) <= 1e-12


def test_host_recurrence_in_fp32_and_the_stop_rule():
    op = ops.GaussianBlurOperator(SHAPE, 5, 1.0)
    A = cg.dense(op)
    g = torch.Generator().manual_seed(22)
    x0, y = torch.randn(3, *SHAPE, generator=g), torch.randn(3, *SHAPE, generator=g)
    y[1] = op.apply(x0[1:2])[0]  # a sample with no residual: stops at once, returns x0 itself
    z, iters = op.apply_prox_cg(x0, y, 50.0, iterations=300, return_iterations=True)
    assert z.dtype == torch.float32 and bool(torch.isfinite(z).all())
    assert iters[1] == 0 and torch.equal(z[1], x0[1])
    assert 1 <= int(iters[0]) <= 5 and 1 <= int(iters[2]) <= 5
    want = cg.solve(A, x0.reshape(3, -1), y.reshape(3, -1), 50.0)
    assert cg.distance(z.reshape(3, -1), want) <= 2e-5
    # a sample's result does not depend on its neighbours' stops
    alone = op.apply_prox_cg(x0[2:], y[2:], 50.0, iterations=300)
    assert torch.equal(alone[0], z[2])
    emu, emu_iters = cg.cgls(A, x0.reshape(3, -1), y.reshape(3, -1), 50.0, 300, 1e-6, torch.float32)
    assert cg.distance(z.reshape(3, -1), emu) <= 2e-6


def test_apply_prox_cg_raises():
    phase = ops.PhaseRetrievalOperator(SHAPE, pad=4)
    with pytest.raises(NotImplementedError, match="PhaseRetrievalOperator"):
        phase.apply_prox_cg(torch.zeros(1, *phase.x_shape), torch.zeros(1, *phase.y_shape), 1.0)
    op = ops.IdentityOperator(SHAPE)
    x0 = torch.zeros(1, *SHAPE)
    for rho in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="rho"):
            op.apply_prox_cg(x0, x0, rho)
    for bad in (dict(iterations=0), dict(iterations=-2), dict(iterations=1.5)):
        with pytest.raises(ValueError, match="iterations"):
            op.apply_prox_cg(x0, x0, 1.0, **bad)
    for bad in (dict(tol=-1e-3), dict(tol=float("nan")), dict(tol=float("inf"))):
        with pytest.raises(ValueError, match="tol"):
            op.apply_prox_cg(x0, x0, 1.0, **bad)
    with pytest.raises(ValueError, match="batch"):
        op.apply_prox_cg(torch.zeros(2, *SHAPE), torch.zeros(3, *SHAPE), 1.0)


def test_apply_prox_is_untouched():
    """The closed-form entry keeps its operators and its errors (test_diffpir_api has the list)."""
    for op in (ops.GaussianBlurOperator(SHAPE, 3, 1.0), ops.RadonOperator((1, 16, 16), num_angles=5)):
        with pytest.raises(NotImplementedError, match=f"{type(op).__name__} has no closed-form"):
            op.apply_prox(torch.zeros(1, *op.x_shape), torch.zeros(1, *op.y_shape), 1.0)


# --- the keywords -----------------------------------------------------------------------------------
def test_keyword_defaults():
    p = inspect.signature(ops.Operator.apply_prox_cg).parameters
    assert list(p)[1:] == ["x0", "y", "rho", "iterations", "tol", "return_iterations"]
    assert p["iterations"].default == 32 and p["tol"].default == 1e-6
    assert p["return_iterations"].default is False
    for fn in (DiffPIRSampler.__call__, FusedDiffPIRStep.__init__):
        p = inspect.signature(fn).parameters
        assert p["prox"].default == "closed_form"
        assert p["cg_iterations"].default == 16 and p["cg_tol"].default == 1e-4
        for kw in ("prox", "cg_iterations", "cg_tol"):
            assert p[kw].kind is inspect.Parameter.KEYWORD_ONLY


def _problem(op):
    return D._problem(op)


def test_sampler_modes_raise_by_name():
    net = si.make_samplers_amd_net("conv", 3, 0.1)
    shape = (3, 16, 16)
    blur, radon = ops.GaussianBlurOperator(shape, 3, 1.0), ops.RadonOperator((3, 16, 16), num_angles=5)
    for op in (blur, radon, ops.FFTPSFBlurOperator(shape, torch.ones(3, 3) / 9)):
        for kw in (dict(), dict(prox="closed_form")):  # exactly as before
            with pytest.raises(NotImplementedError, match=f"{type(op).__name__} has no closed-form"):
                DiffPIRSampler(net)(_problem(op), num_sampling_steps=4, **kw)
        for mode in ("cg", "auto"):  # accepted, up to the device check
            with pytest.raises(_hip.HipLibraryError, match="MI355X"):
                DiffPIRSampler(net)(_problem(op), num_sampling_steps=4, prox=mode)
    for mode in ("cg", "auto"):  # no descriptor, or nonlinear: by name
        for op in (ops.BicubicSuperResolutionOperator(shape, 2), ops.PhaseRetrievalOperator(shape, pad=4)):
            with pytest.raises(NotImplementedError, match=type(op).__name__):
                DiffPIRSampler(net)(_problem(op), num_sampling_steps=4, prox=mode)
    good = ops.SuperResolutionOperator(shape, 4)
    for mode in ("closed_form", "cg", "auto"):
        with pytest.raises(_hip.HipLibraryError, match="MI355X"):
            DiffPIRSampler(net)(_problem(good), num_sampling_steps=4, prox=mode)
    for bad in (dict(prox="fft"), dict(prox=None), dict(prox="cg", cg_iterations=0),
                dict(prox="cg", cg_iterations=2.5), dict(prox="cg", cg_tol=-1.0),
                dict(prox="cg", cg_tol=float("nan"))):
        with pytest.raises(ValueError):
            DiffPIRSampler(net)(_problem(good), num_sampling_steps=4, **bad)
