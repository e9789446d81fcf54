"""SuperResolutionOperator on the host and the library's SP_OP_SR descriptor rules (no GPU)."""

import pytest
import torch
import torch.nn.functional as F

import sr_ops
from samplers_amd import _hip
from samplers_amd import operators
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import LinearOperator, SuperResolutionOperator

CASES = [((3, 32, 32), 2), ((3, 32, 32), 4), ((3, 32, 32), 8), ((1, 8, 12), 4), ((2, 6, 10), 2),
         ((3, 40, 72), 8), ((1, 2, 2), 2)]


def test_exported():
    assert "SuperResolutionOperator" in operators.__all__
    assert issubclass(SuperResolutionOperator, LinearOperator)


@pytest.mark.parametrize("shape,s", CASES)
def test_host_apply_is_avg_pool(shape, s):
    op = SuperResolutionOperator(shape, s)
    c, h, w = shape
    assert op.x_shape == shape and op.y_shape == (c, h // s, w // s)
    x = torch.randn(3, *shape, generator=torch.Generator().manual_seed(0))
    y = op.apply(x)
    assert tuple(y.shape) == (3, *op.y_shape)
    assert torch.equal(y, F.avg_pool2d(x, s))
    assert torch.equal(op(x), y)
    two = op.apply(x.reshape(3, 1, *shape))  # leading batch dimensions are kept
    assert tuple(two.shape) == (3, 1, *op.y_shape) and torch.equal(two.reshape(y.shape), y)


@pytest.mark.parametrize("shape,s", CASES)
def test_adjoint_identity_in_fp64(shape, s):
    op = SuperResolutionOperator(shape, s)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, *shape, dtype=torch.float64, generator=g)
    y = torch.randn(2, *op.y_shape, dtype=torch.float64, generator=g)
    lhs = (op.apply(x) * y).sum()
    rhs = (x * op.apply_transpose(y)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(lhs)))
    # the class's maps are the helper's fp64 semantics (autograd adjoint of avg_pool2d)
    assert torch.equal(op.apply(x), sr_ops.apply64(x, s))
    torch.testing.assert_close(op.apply_transpose(y), sr_ops.adjoint64(y, s), rtol=0, atol=1e-15)
    assert torch.equal(sr_ops.adjoint_closed(y, s), op.apply_transpose(y))


@pytest.mark.parametrize("shape,s", CASES)
def test_pseudo_inverse(shape, s):
    op = SuperResolutionOperator(shape, s)
    y = torch.randn(2, *op.y_shape, generator=torch.Generator().manual_seed(2))
    pinv = op.apply_pseudo_inverse(y)
    assert torch.equal(pinv, y.repeat_interleave(s, dim=-2).repeat_interleave(s, dim=-1))
    assert torch.equal(op.apply_transpose(y) * (s * s), pinv)  # A+ = s^2 A^T, exact scaling
    y64 = y.double()
    torch.testing.assert_close(op.apply(op.apply_pseudo_inverse(y64)), y64, rtol=0, atol=1e-15)
    x = torch.randn(2, *shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    proj = op.apply_pseudo_inverse(op.apply(x))  # A+ A is a projection
    torch.testing.assert_close(op.apply_pseudo_inverse(op.apply(proj)), proj, rtol=0, atol=1e-15)


@pytest.mark.parametrize("shape,s", [((3, 8, 8), 2), ((2, 8, 16), 4), ((1, 8, 8), 8)])
def test_pgdm_gradient_factor_matches_autograd(shape, s):
    """d/dx0 ||A+ y - A+ A x0||^2 = -pinv_grad_scale * A^T (y - A x0), pinv_grad_scale = 2 s^2."""
    op = SuperResolutionOperator(shape, s)
    assert op.pinv_grad_scale == 2.0 * s * s
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(2, *shape, dtype=torch.float64, generator=g).requires_grad_()
    y = torch.randn(2, *op.y_shape, dtype=torch.float64, generator=g)
    loss = (op.apply_pseudo_inverse(y) - op.apply_pseudo_inverse(op.apply(x0))).pow(2).sum()
    (grad,) = torch.autograd.grad(loss, x0)
    closed = -op.pinv_grad_scale * op.apply_transpose(y - op.apply(x0.detach()))
    torch.testing.assert_close(grad, closed, rtol=0, atol=1e-12)


def test_existing_operators_keep_the_partial_isometry_factor():
    from samplers_amd.operators import IdentityOperator, RandomInpaintingOperator

    assert IdentityOperator((3, 4, 4)).pinv_grad_scale == 2.0
    assert RandomInpaintingOperator((3, 4, 4), 0.5, seed=0).pinv_grad_scale == 2.0


@pytest.mark.parametrize("shape,s", [((3, 32, 32), 3), ((3, 32, 32), 1), ((3, 32, 32), 16),
                                     ((3, 30, 32), 4), ((3, 32, 30), 4), ((3, 12, 8), 8),
                                     ((32, 32), 2)])
def test_bad_arguments_raise(shape, s):
    with pytest.raises(ValueError):
        SuperResolutionOperator(shape, s)


def test_descriptor_fields():
    d = SuperResolutionOperator((3, 40, 72), 8).hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width) == (_hip.SP_OP_SR, 3, 40, 72)
    assert _hip.SP_OP_SR == 4
    assert d.n == 3 * 40 * 72 and d.m == 3 * 5 * 9 and d.factor == 8
    assert not d.keep_bits and not d.word_rank and not d.taps and d.radius == 0
    ident = operators.IdentityOperator((3, 4, 4)).hip_descriptor()
    assert ident.factor == 0  # the other kinds leave it 0


def test_library_accepts_only_valid_sr_descriptors():
    lib = _hip.load_library()
    assert lib.sp_version() >= 102
    for shape, s in CASES:
        assert lib.sp_rsq_partials(SuperResolutionOperator(shape, s).hip_descriptor()) > 0
    # 6 tiles of 256 4x4 blocks: the fixed-order partial sum has more than one term
    assert lib.sp_rsq_partials(SuperResolutionOperator((3, 64, 128), 4).hip_descriptor()) > 1

    def rejected(**fields):
        d = SuperResolutionOperator((3, 32, 32), 4).hip_descriptor()
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.sp_rsq_partials(d)

    assert rejected() > 0
    assert rejected(factor=3) == -1
    assert rejected(factor=0) == -1
    assert rejected(m=3 * 8 * 8 + 1) == -1            # m * s^2 != n
    assert rejected(factor=2) == -1                   # m * s^2 != n for the other factor
    assert rejected(height=30, n=3 * 30 * 32, m=3 * 30 * 32 // 16) == -1  # 30 % 4 != 0
    assert rejected(width=30, n=3 * 32 * 30, m=3 * 32 * 30 // 16) == -1
    assert rejected(n=3 * 32 * 32 + 16, m=3 * 8 * 8 + 1) == -1  # C * H * W != n


def test_pgdm_probe_accepts_the_operator():
    """PGDMSampler's pseudo-inverse probe (a host tensor of y_shape) must not raise; the call
    then stops at the device check, since this observation lives on the host."""
    import stand_ins as si
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = SuperResolutionOperator((3, 32, 32), 4)
    assert tuple(op.apply_pseudo_inverse(torch.zeros(1, *op.y_shape)).shape) == (1, 3, 32, 32)
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(_hip.HipLibraryError, match="HIP"):
        PGDMSampler(net)(ip, num_sampling_steps=4)
