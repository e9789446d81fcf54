"""PeriodicBlurOperator on the host: the fp64 helper against itself (direct route = FFT route), the
operator's host maps against the helper, the algebra of the truncated pseudo-inverse, the layout
of the descriptor's spectra, the constructor's and the library's rules.  No GPU: the library loads
without one and every call here returns before a launch.

Every PSF here keeps some frequencies and drops some (0 < keep.mean() < 1 is asserted), so the
projection is neither the identity nor zero."""

import ctypes
import math

import numpy as np
import pytest
import torch

import periodic_ops as po
from kind_harness import make_descriptor as make
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import (FFTPSFBlurOperator, PeriodicBlurOperator,
                                    pseudo_inverse_spectrum, transfer_function)
from samplers_amd.operators.blur import gaussian_taps

OK, EINVAL, EUNSUPPORTED = 0, -1, -3


def _gauss(k, sigma):
    t = gaussian_taps(k, sigma).to(torch.float64)
    return torch.outer(t, t).to(torch.float32)


def _signed():
    return torch.randn(7, 7, generator=torch.Generator().manual_seed(3)) / 7


# name -> (x_shape, kernel, share of the frequencies kept at rtol = 3e-2)
PSFS = {
    "8x8-gauss3": ((1, 8, 8), _gauss(3, 0.8), 0.86),
    "8x24-box3": ((2, 8, 24), torch.ones(1, 3) / 3, 0.917),  # exact spectral zeros at kw = 8, 16
    "16x16-gauss9": ((3, 16, 16), _gauss(9, 1.5), 0.27),
    "24x24-signed7": ((1, 24, 24), _signed(), None),
    "256x256-gauss61": ((1, 256, 256), _gauss(61, 3.0), 0.062),
}
SMALL = [n for n in PSFS if not n.startswith("256")]


def _op(name):
    shape, h, share = PSFS[name]
    op = PeriodicBlurOperator(shape, h)
    kept = float(op.keep.float().mean())
    assert 0.0 < kept < 1.0, (name, kept)
    if share is not None:
        assert abs(kept - share) < 0.01, (name, kept)
    return op, shape, op.kernel


def _x(shape, seed, b=2, dtype=torch.float64):
    return torch.randn(b, *shape, dtype=dtype, generator=torch.Generator().manual_seed(seed))


def _close(got, ref, tol):
    cast = (lambda t: t.to(torch.complex128)) if got.is_complex() else (lambda t: t.double())
    err = float((cast(got) - cast(ref)).abs().max() / cast(ref).abs().max())
    assert err <= tol, err


@pytest.mark.parametrize("name", list(PSFS))
def test_helper_direct_route_equals_fft_route(name):
    op, shape, h = _op(name)
    x = _x(shape, 1, b=1)
    _close(po.blur(x, h, "fft"), po.blur(x, h, "direct"), 1e-12)
    _close(po.adjoint(x, h, "fft"), po.adjoint(x, h, "direct"), 1e-12)
    _close(transfer_function(h, *shape[1:]), po.transfer(h, *shape[1:]), 1e-14)


@pytest.mark.parametrize("name", list(PSFS))
def test_host_maps_match_the_helper(name):
    op, shape, h = _op(name)
    x, y = _x(shape, 2, dtype=torch.float32), _x(shape, 3, dtype=torch.float32)
    route = "fft" if name.startswith("256") else "direct"
    _close(op.apply(x), po.apply64(x, h, route), 2e-6)
    _close(op.apply_transpose(y), po.adjoint64(y, h, route), 2e-6)
    # P reaches 1 / rtol = 33: fp32 torch.fft stays within 2.5e-7 x max of fp64 (measured)
    _close(op.apply_pseudo_inverse(y), po.pinv(y.double(), h, op.keep), 2e-6)
    # fp64 in, fp64 out, with the fp32-rounded P
    out = op.apply_pseudo_inverse(y.double())
    assert out.dtype == torch.float64
    _close(out, po.pinv(y.double(), h, op.keep), 2e-6)
    # the same map as the FFT operator with circular padding
    _close(op.apply(x), FFTPSFBlurOperator(shape, h, padding="circular").apply(x), 1e-6)
    # differentiable on the host: the backward of A^+ is A^+T
    yr = y.clone().requires_grad_()
    (g,) = torch.autograd.grad(op.apply_pseudo_inverse(yr), yr, grad_outputs=x)
    _close(g, po.pinv(x.double(), h, op.keep, transpose=True), 2e-6)
    assert tuple(op.y_shape) == tuple(op.x_shape) == shape and op.hip_linear is False
    assert op.pinv_grad_scale == 2.0


@pytest.mark.parametrize("name", SMALL)
def test_adjoint_identity(name):
    op, shape, h = _op(name)
    x, y = _x(shape, 4), _x(shape, 5)
    lhs = float((po.blur(x, h) * y).sum())
    rhs = float((x * po.adjoint(y, h)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(x.norm() * y.norm())
    x32, y32 = x.float(), y.float()
    lhs = float((op.apply(x32).double() * y).sum())
    rhs = float((x * op.apply_transpose(y32).double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(x.norm() * y.norm())


@pytest.mark.parametrize("name", SMALL)
def test_projection_and_pseudo_inverse_algebra(name):
    op, shape, h = _op(name)
    keep = op.keep
    x, z = _x(shape, 6), _x(shape, 7)
    pi = lambda t: po.pinv(po.blur(t, h), h, keep)  # noqa: E731
    _close(pi(x), po.projection(x, keep), 1e-12)
    _close(pi(pi(x)), pi(x), 1e-12)  # idempotent
    assert abs(float((pi(x) * z).sum() - (x * pi(z)).sum())) <= 1e-12 * float(x.norm() * z.norm())
    _close(po.pinv(pi(x), h, keep), po.pinv(x, h, keep), 1e-12)  # A^+ A A^+ = A^+ (A, A^+ commute)
    # A A^+ A = A does not hold: what the blur passes below the threshold is gone (the box's
    # dropped frequencies are its exact zeros: there, and only there, nothing is lost)
    diff = po.blur(pi(x), h) - po.blur(x, h)
    passed_below = float(po.transfer(h, *shape[1:]).abs()[~keep].max())
    if name == "8x24-box3":
        assert passed_below < 1e-15
        assert float(diff.abs().max()) <= 1e-12 * float(po.blur(x, h).abs().max())
    else:
        assert passed_below > 1e-4
        assert float(diff.abs().max()) > 1e-6 * float(po.blur(x, h).abs().max())


@pytest.mark.parametrize("name", list(PSFS))
def test_keep_is_symmetric_and_thresholded(name):
    op, shape, h = _op(name)
    keep = op.keep.numpy()
    neg = np.roll(np.flip(keep, (0, 1)), 1, (0, 1))
    assert keep.dtype == np.bool_ and keep.shape == shape[1:] and np.array_equal(keep, neg)
    m = transfer_function(h, *shape[1:])
    p, k2 = pseudo_inverse_spectrum(m, op.rtol)
    assert torch.equal(k2, op.keep)
    mag = m.abs().numpy()
    assert (mag[keep] > op.rtol * mag.max()).all()
    assert (np.minimum(mag, np.roll(np.flip(mag, (0, 1)), 1, (0, 1)))[~keep]
            <= op.rtol * mag.max()).all()
    pn = p.numpy()
    assert np.array_equal(pn != 0, keep) and np.allclose(pn[keep] * m.numpy()[keep], 1.0)
    # Hermitian: the maps take real images to real images
    assert np.allclose(np.roll(np.flip(pn, (0, 1)), 1, (0, 1)), pn.conj())


@pytest.mark.parametrize("name", SMALL)
def test_pgdm_gradient_identity(name):
    """d/dx0 ||A^+ y - A^+ A x0||^2 = -2 (A^+ y - Pi x0), against autograd of the loss."""
    op, shape, h = _op(name)
    x0, y = _x(shape, 8), _x(shape, 9)
    closed = po.pgdm_grad(x0, y, h, op.keep)
    auto = po.pgdm_grad_autograd(x0, y, h, op.keep)
    _close(closed, auto, 1e-12)
    # and through the operator's own host maps, as GenericDPSStep differentiates
    xr = x0.float().requires_grad_()
    loss = (op.apply_pseudo_inverse(y.float()) - op.apply_pseudo_inverse(op.forward(xr))).pow(2).sum()
    (g,) = torch.autograd.grad(loss, xr)
    _close(g, closed, 2e-5)


@pytest.mark.parametrize("name", list(PSFS))
def test_descriptor_and_taps_layout(name):
    """taps = M then P, each (re, im) pairs [W / 2 + 1][H], fp64 rounded to fp32."""
    op, shape, h = _op(name)
    c, H, W = shape
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width) == (_hip.SP_OP_PSF_PERIODIC, c, H, W)
    assert d.n == d.m == math.prod(shape) and d.radius == op.radius and d.factor == 0
    assert d.taps == op.spectra.data_ptr() and not d.keep_bits and not d.word_rank
    assert tuple(op.spectra.shape) == (2, W // 2 + 1, H, 2) and op.spectra.dtype == torch.float32
    assert op.spectra.is_contiguous()
    m = po.transfer(h, H, W)
    p = po.pinv_spectrum(h, op.keep)
    for i, spec in enumerate((m, p)):
        want = spec[:, : W // 2 + 1].T
        got = torch.view_as_complex(op.spectra[i])
        # fp32 rounding of each entry (the floor: the fp64 transforms' own round-off)
        tol = 1e-7 * want.abs() + 1e-13 * float(want.abs().max())
        assert bool(((got - want).abs() <= tol).all())
    kept_half = op.keep[:, : W // 2 + 1].T
    assert torch.equal(torch.view_as_complex(op.spectra[1]) != 0, kept_half)


def test_rectangular_and_gaussian_constructors():
    op = PeriodicBlurOperator((1, 8, 24), torch.ones(1, 3) / 3)
    assert tuple(op.kernel.shape) == (3, 3) and op.radius == 1
    assert torch.equal(op.kernel[1], torch.full((3,), 1 / 3)) and float(op.kernel[0].abs().sum()) == 0
    g = PeriodicBlurOperator.gaussian((3, 64, 64), 9, 1.5, rtol=0.1)
    assert torch.equal(g.kernel, _gauss(9, 1.5)) and g.rtol == 0.1
    assert torch.equal(PeriodicBlurOperator.gaussian((1, 256, 256)).kernel, _gauss(61, 3.0))


def test_constructor_errors():
    k3 = torch.ones(3, 3)
    for bad in ((1, 20, 16), (1, 16, 20), (1, 4, 8), (1, 2048, 8), (16, 16)):
        with pytest.raises(ValueError):
            PeriodicBlurOperator(bad, k3)
    with pytest.raises(ValueError):
        PeriodicBlurOperator((1, 16, 16), torch.ones(4, 4))           # even
    with pytest.raises(ValueError):
        PeriodicBlurOperator((1, 16, 16), torch.ones(1, 1))           # R = 0
    with pytest.raises(ValueError):
        PeriodicBlurOperator((1, 8, 16), torch.ones(9, 9))            # 2R + 1 > min(H, W)
    with pytest.raises(ValueError):
        PeriodicBlurOperator((1, 16, 16), torch.full((3, 3), float("nan")))
    PeriodicBlurOperator((1, 8, 16), torch.ones(7, 7))                # 2R + 1 = 7 <= 8
    for rtol in (0.0, 1.0, -0.1, 2.0):
        with pytest.raises(ValueError):
            PeriodicBlurOperator((1, 16, 16), k3, rtol=rtol)
        with pytest.raises(ValueError):
            pseudo_inverse_spectrum(transfer_function(k3, 16, 16), rtol)
    with pytest.raises(ValueError):
        PeriodicBlurOperator.gaussian((1, 16, 16), 4, 1.0)
    with pytest.raises(ValueError):
        PeriodicBlurOperator.gaussian((1, 16, 16), 5, 0.0)


# --- the library's table row, as tests/test_op_table.py reads the other kinds -------------------

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def periodic(c=1, h=8, w=8, r=1, **kw):
    args = dict(radius=r, taps=PTR)
    args.update(kw)
    return make(_hip.SP_OP_PSF_PERIODIC, c * h * w, c * h * w, c, h, w, **args)


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def new_entries(lib, d, *, work=PTR):
    c = _hip.SpDpsCoefs()
    return {
        "sp_op_pinv_ws": lambda: lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, work, None),
        "sp_pgdm_prepare": lambda: lib.sp_pgdm_prepare(d, PTR, 3, PTR, None),
        "sp_pgdm_residual_ws": lambda: lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, work,
                                                              None),
    }


def test_version_and_constants(lib):
    assert lib.sp_version() >= 107
    assert _hip.SP_OP_PSF_PERIODIC == 8 and _hip.SP_TRAIT_PINV == 32


def _lines(N):
    NP = (N + N // 16) | 1
    return max(1, min(16, (32000 - 8 * N) // (16 * NP)))


@pytest.mark.parametrize("c,h,w,r", [(1, 8, 8, 1), (2, 8, 24, 1), (3, 256, 256, 30),
                                     (1, 512, 1024, 30), (1, 1024, 8, 3)])
def test_counts_follow_the_fft_kind_at_exact_sizes(lib, c, h, w, r):
    d = periodic(c, h, w, r)
    assert lib.sp_rsq_partials(d) == c * -(-h // _lines(w))
    floats = 2 * 3 * c * (w // 2 + 1) * h
    assert lib.sp_dps_workspace(d, 3) == floats and lib.sp_op_workspace(d, 3) == floats
    assert lib.sp_dps_workspace(d, 0) == EINVAL and lib.sp_op_workspace(d, 0) == EINVAL


def test_traits(lib):
    t = lib.sp_op_traits(periodic())
    assert t == (_hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_PINV)
    op, _, _ = _op("8x8-gauss3")
    assert lib.sp_op_traits(op.hip_descriptor()) == t


def test_descriptor_rules(lib):
    bad = [periodic(1, 20, 16), periodic(1, 16, 20), periodic(1, 4, 8), periodic(1, 2048, 8),
           periodic(1, 8, 8, 0), periodic(1, 8, 8, 4), periodic(1, 8, 16, 4), periodic(1, 16, 16, -1),
           periodic(1, 8, 8, taps=None), periodic(1, 8, 8, factor=1), periodic(1, 8, 8, keep=PTR),
           periodic(1, 8, 8, rank=PTR), periodic(0, 8, 8),
           make(_hip.SP_OP_PSF_PERIODIC, 64, 32, 1, 8, 8, radius=1, taps=PTR),
           make(_hip.SP_OP_PSF_PERIODIC, 65, 65, 1, 8, 8, radius=1, taps=PTR),
           make(9, 64, 64, 1, 8, 8, radius=1, taps=PTR)]
    for d in bad:
        assert lib.sp_rsq_partials(d) == EINVAL, (d.height, d.width, d.radius, d.factor)
        assert lib.sp_op_traits(d) == 0
        for name, call in new_entries(lib, d).items():
            assert call() == EINVAL, name
    ok = [periodic(1, 8, 8, 3), periodic(1, 8, 16, 3), periodic(1, 1024, 768, 383),
          periodic(2, 24, 48, 11)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.height, d.width, d.radius)
    for name, call in new_entries(lib, None).items():
        assert call() == EINVAL, name


def test_new_entries_argument_checks(lib):
    d, c = periodic(), _hip.SpDpsCoefs()
    assert lib.sp_op_pinv_ws(d, None, PTR, 3, 0, PTR, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, None, 3, 0, PTR, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, None, None) == EINVAL       # work == NULL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 0, 0, PTR, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 65536, 0, PTR, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 2, PTR, None) == EINVAL        # transpose is 0 or 1
    assert lib.sp_pgdm_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 0, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 65536, PTR, None) == EINVAL
    args = [d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None]
    for i, v in ((1, None), (2, None), (3, None), (4, 0), (4, 65536), (5, 0), (6, None), (7, None),
                 (8, None)):
        a = list(args)
        a[i] = v
        assert lib.sp_pgdm_residual_ws(*a) == EINVAL, i
    # the existing columns answer as for the FFT kind
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None, None) == EINVAL
    assert lib.sp_op_apply(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_op_adjoint(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_op_apply_ws(d, PTR, PTR, 3, None, None) == EINVAL
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, None, None) == EINVAL
    assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_dps_update(d, PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR,
                             None) == EINVAL                                 # pass 2 needs v


def test_other_kinds_have_no_pseudo_inverse_columns(lib):
    n = 64
    others = [make(_hip.SP_OP_IDENTITY, 12, 12), make(_hip.SP_OP_INPAINT, 128, 64, keep=PTR, rank=PTR),
              make(_hip.SP_OP_BLUR, n, n, 1, 8, 8, radius=1, taps=PTR), make(_hip.SP_OP_MASK, 128, 128, keep=PTR),
              make(_hip.SP_OP_SR, n, n // 4, 1, 8, 8, factor=2),
              make(_hip.SP_OP_PSF, n, n, 1, 8, 8, radius=1, taps=PTR), make(_hip.SP_OP_PHASE, n, n, 1, 8, 8),
              make(_hip.SP_OP_PSF_FFT, n, n, 1, 8, 8, radius=1, taps=PTR)]
    for d in others:
        assert lib.sp_rsq_partials(d) > 0, d.kind
        assert not lib.sp_op_traits(d) & _hip.SP_TRAIT_PINV
        for name, call in new_entries(lib, d).items():
            assert call() == EUNSUPPORTED, (d.kind, name)
        # a null buffer is SP_EINVAL before the kind is looked at
        assert lib.sp_op_pinv_ws(d, None, PTR, 3, 0, PTR, None) == EINVAL


def test_pgdm_probe_accepts_the_operator():
    """PGDMSampler's pseudo-inverse probe (a host tensor of y_shape) must not raise; the call then
    stops at the device check, since this observation lives on the host."""
    import stand_ins as si
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = PeriodicBlurOperator((3, 32, 32), _gauss(9, 1.5))
    assert 0.0 < float(op.keep.float().mean()) < 1.0
    assert tuple(op.apply_pseudo_inverse(torch.zeros(1, *op.y_shape)).shape) == (1, 3, 32, 32)
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(_hip.HipLibraryError, match="HIP"):
        PGDMSampler(net)(ip, num_sampling_steps=4)
