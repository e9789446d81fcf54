"""FilteredSuperResolutionOperator and BicubicSuperResolutionOperator on the host: the constructor's
rules, the shapes, both maps against the fp64 matrices of tests/sr_filter_ref.py, and what the
samplers answer for an operator the library has no kind for (no GPU)."""

import numpy as np
import pytest
import torch

import sr_filter_ref as sf
from samplers_amd import operators
from samplers_amd.operators import (BicubicSuperResolutionOperator, FilteredSuperResolutionOperator,
                                    LinearOperator, bicubic_taps)


def test_exported():
    for name in ("FilteredSuperResolutionOperator", "BicubicSuperResolutionOperator", "bicubic_taps"):
        assert name in operators.__all__
    assert issubclass(BicubicSuperResolutionOperator, FilteredSuperResolutionOperator)
    assert issubclass(FilteredSuperResolutionOperator, LinearOperator)


# --- the Python class -----------------------------------------------------------------------------
@pytest.mark.parametrize("args,kwargs,rule", [
    (((24, 16), [0.5, 0.5]), {"factor": 2}, "x_shape"),
    (((1, 24, 16), [0.5, 0.5]), {"factor": 3}, "factor"),
    (((1, 24, 16), [[0.5, 0.5]]), {"factor": 2}, "1-D"),
    (((1, 24, 16), [0.5]), {"factor": 2}, "number of taps"),
    (((1, 24, 16), [0.1] * 34), {"factor": 2}, "number of taps"),
    (((1, 24, 16), [0.2] * 5), {"factor": 2}, "parity"),
    (((1, 24, 16), [0.5, float("nan")]), {"factor": 2}, "finite"),
    (((1, 26, 16), [0.25] * 4), {"factor": 4}, "multiples"),
    (((1, 24, 18), [0.25] * 4), {"factor": 4}, "multiples"),
    (((0, 24, 16), [0.25] * 4), {"factor": 4}, "multiples"),
    (((1, 14, 32), [1 / 32] * 32), {"factor": 2}, "pad"),
    (((1, 32, 14), [1 / 32] * 32), {"factor": 2}, "pad"),
])
def test_bad_arguments_raise_naming_the_rule(args, kwargs, rule):
    with pytest.raises(ValueError, match=rule):
        FilteredSuperResolutionOperator(*args, **kwargs)


def test_other_constructors():
    with pytest.raises(ValueError, match="factor"):
        BicubicSuperResolutionOperator((1, 24, 24), factor=3)
    with pytest.raises(ValueError, match="parity"):
        FilteredSuperResolutionOperator.gaussian((1, 24, 24), factor=4, kernel_size=9, sigma=2.0)
    with pytest.raises(ValueError, match="sigma"):
        FilteredSuperResolutionOperator.gaussian((1, 24, 24), factor=4, kernel_size=8, sigma=0.0)
    op = FilteredSuperResolutionOperator.gaussian((3, 24, 32), factor=4, kernel_size=12, sigma=2.0)
    i = np.arange(12) - 5.5
    k = np.exp(-i ** 2 / 8.0)
    assert op.y_shape == (3, 6, 8) and op.kernel_size == 12 and op.pad == 4
    assert np.array_equal(op.taps.numpy(), (k / k.sum()).astype(np.float32))
    bic = BicubicSuperResolutionOperator((3, 32, 32))
    assert bic.factor == 4 and bic.kernel_size == 16 and bic.pad == 6 and bic.y_shape == (3, 8, 8)
    assert torch.equal(bic.taps, bicubic_taps(4))
    with pytest.raises(NotImplementedError):
        bic.apply_pseudo_inverse(torch.zeros(1, 3, 8, 8))


def test_no_descriptor_and_no_device_maps():
    """The library has no kind for the operator: no descriptor, and a device tensor is an error,
    not eager torch on the device."""
    op = BicubicSuperResolutionOperator((3, 40, 36), factor=2)
    assert op.hip_descriptor() is None

    class DeviceTensor:
        is_cuda = True

    for fn in (op.apply, op.apply_transpose):
        with pytest.raises(NotImplementedError, match="no native"):
            fn(DeviceTensor())


@pytest.mark.parametrize("s,K,H,W", [(2, 8, 4, 12), (4, 16, 8, 24), (8, 32, 16, 32), (4, 6, 12, 8), (2, 32, 16, 32)])
def test_host_maps_against_the_reference_matrices(s, K, H, W):
    k = sf.bicubic_taps64(s).astype(np.float32) if K == 4 * s else sf.random_taps(K)
    op = FilteredSuperResolutionOperator((2, H, W), k, factor=s)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 2, H, W))  # two leading batch dimensions
    g = rng.standard_normal((2, 3, 2, H // s, W // s))
    ax, atg = op.apply(torch.from_numpy(x)), op.apply_transpose(torch.from_numpy(g))
    assert tuple(ax.shape) == g.shape and tuple(atg.shape) == x.shape
    assert np.abs(ax.numpy() - sf.apply64(x, k, s)).max() <= 1e-12
    assert np.abs(atg.numpy() - sf.adjoint64(g, k, s)).max() <= 1e-12
    x32 = torch.from_numpy(x).float()
    assert op.apply(x32).dtype == torch.float32
    assert float((op.apply(x32).double() - ax).abs().max()) <= 2e-5 * float(ax.abs().max())
    # differentiable on the host: the gradient of <A x, g> is A^T g
    xr = torch.from_numpy(x).requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=torch.from_numpy(g))
    assert float((gx - atg).abs().max()) <= 1e-12


def test_no_pseudo_inverse_so_pgdm_raises():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = BicubicSuperResolutionOperator((3, 32, 32))
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(ip, num_sampling_steps=4)


def test_fused_dps_refuses_an_operator_without_a_descriptor_by_name():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.dps import FusedDPSStep

    op = BicubicSuperResolutionOperator((3, 32, 32))
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="BicubicSuperResolutionOperator has no native"):
        FusedDPSStep(net, ip, torch.zeros(1, *op.y_shape), 1)
