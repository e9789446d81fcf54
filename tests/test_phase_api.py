"""PhaseRetrievalOperator on the host and the library's SP_OP_PHASE descriptor rules (no GPU).
The semantics are those of tests/phase_ops.py (fp64)."""

import ctypes

import numpy as np
import pytest
import torch

import phase_ops
from samplers_amd import _hip
from samplers_amd import operators
from samplers_amd.operators import NonlinearOperator, Operator, PhaseRetrievalOperator

# shape, (pad_h, pad_w)
CASES = [((1, 2, 2), (3, 3)), ((1, 8, 8), (0, 0)), ((2, 6, 10), (1, 3)), ((1, 12, 20), (6, 2)),
         ((3, 16, 16), (8, 8)), ((3, 64, 64), (16, 16)), ((1, 96, 160), (16, 48))]


def test_exported():
    assert "PhaseRetrievalOperator" in operators.__all__
    assert issubclass(PhaseRetrievalOperator, NonlinearOperator)
    assert PhaseRetrievalOperator.hip_linear is False and Operator.hip_linear is True
    assert operators.GaussianBlurOperator.hip_linear is True


@pytest.mark.parametrize("shape,pad", CASES + [((1, 256, 256), (64, 64))])
def test_closed_form_vjp_is_fp64_autograd(shape, pad):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, *shape, dtype=torch.float64, generator=g)
    cot = torch.randn(2, shape[0], shape[1] + 2 * pad[0], shape[2] + 2 * pad[1], dtype=torch.float64,
                      generator=g)
    xr = x.clone().requires_grad_()
    (ref,) = torch.autograd.grad(phase_ops.amplitude(xr, pad), xr, grad_outputs=cot)
    got = phase_ops.vjp64(x, cot, pad)
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    apply, vjp = phase_ops.phase_ops(shape, pad)
    np.testing.assert_allclose(vjp(x.reshape(2, -1).numpy(), cot.reshape(2, -1).numpy()),
                               ref.reshape(2, -1).numpy(), rtol=0, atol=1e-13 * float(ref.abs().max()))
    assert apply(x.reshape(2, -1).numpy()).shape == (2, cot[0].numel())


@pytest.mark.parametrize("shape,pad", CASES)
def test_host_apply_and_autograd(shape, pad):
    op = PhaseRetrievalOperator(shape, pad=pad)
    c, h, w = shape
    assert op.x_shape == shape and op.y_shape == (c, h + 2 * pad[0], w + 2 * pad[1])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, *shape, generator=g)
    y = op.apply(x)
    assert tuple(y.shape) == (2, *op.y_shape) and y.dtype == torch.float32
    ref = torch.fft.fft2(torch.nn.functional.pad(x, (pad[1], pad[1], pad[0], pad[0])), norm="ortho").abs()
    assert torch.equal(y, ref) and torch.equal(op(x), y)
    r64 = phase_ops.apply64(x, pad)
    assert float((y.double() - r64).abs().max()) <= 2e-5 * float(r64.abs().max())
    cot = torch.randn(tuple(y.shape), generator=g)
    xr = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(op.apply(xr), xr, grad_outputs=cot)
    v64 = phase_ops.vjp64(x, cot, pad)
    assert float((gx.double() - v64).abs().max()) <= 2e-5 * float(v64.abs().max())
    two = op.apply(x.reshape(2, 1, *shape))  # leading batch dimensions are kept
    assert tuple(two.shape) == (2, 1, *op.y_shape)


def test_pad_rule_and_forms():
    assert PhaseRetrievalOperator((3, 256, 256)).y_shape == (3, 384, 384)
    assert PhaseRetrievalOperator((3, 256, 256)).pad_h == 64
    big = PhaseRetrievalOperator((1, 512, 512))
    assert (big.pad_h, big.pad_w) == (128, 128) and big.y_shape == (1, 768, 768)
    assert PhaseRetrievalOperator((1, 512, 512), pad=256).y_shape == (1, 1024, 1024)
    assert PhaseRetrievalOperator((1, 64, 32), oversample=4.0).y_shape == (1, 128, 64)
    assert PhaseRetrievalOperator((1, 8, 16), pad=0).y_shape == (1, 8, 16)
    assert PhaseRetrievalOperator((2, 6, 10), pad=(1, 3)).y_shape == (2, 8, 16)
    assert PhaseRetrievalOperator((1, 12, 12), pad=6).y_shape == (1, 24, 24)


@pytest.mark.parametrize("shape,kw", [
    ((1, 16, 16), dict(pad=2)),            # 20
    ((1, 16, 32), dict(pad=(8, 4))),       # width 40
    ((1, 1024, 1024), dict(pad=512)),      # 2048
    ((1, 2, 2), dict(pad=1)),              # 4
    ((1, 16, 16), dict(pad=-4)),           # negative, though 8 is a valid size
    ((1, 16, 16), dict(pad=(8, -4))),
    ((1, 40, 40), dict()),                 # the rule gives pad 10: 60
    ((16, 16), dict(pad=8)),               # x_shape not (C, H, W)
])
def test_bad_arguments_raise(shape, kw):
    with pytest.raises(ValueError):
        PhaseRetrievalOperator(shape, **kw)


def test_error_names_the_nearest_valid_pads():
    with pytest.raises(ValueError, match=r"\[0, 4\]"):
        PhaseRetrievalOperator((1, 16, 16), pad=2)  # 16 -> 16 (pad 0) or 24 (pad 4)


def test_zero_image():
    op = PhaseRetrievalOperator((2, 6, 10), pad=(1, 3))
    x = torch.zeros(1, 2, 6, 10, requires_grad=True)
    y = op.apply(x)
    assert torch.equal(y, torch.zeros_like(y))
    (gx,) = torch.autograd.grad(y, x, grad_outputs=torch.ones_like(y))
    assert torch.isfinite(gx).all() and torch.equal(gx, torch.zeros_like(gx))
    v = phase_ops.vjp64(x.detach(), torch.ones_like(y), (1, 3))
    assert torch.equal(v, torch.zeros_like(v))


def test_no_transpose_no_pseudo_inverse_so_pgdm_raises():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = PhaseRetrievalOperator((3, 16, 16), pad=8)
    with pytest.raises(NotImplementedError):
        op.apply_transpose(torch.zeros(1, *op.y_shape))
    with pytest.raises(NotImplementedError):
        op.apply_pseudo_inverse(torch.zeros(1, *op.y_shape))
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(ip, num_sampling_steps=4)


def test_make_consistency_picks_the_generic_class():
    from samplers_amd.samplers import resample

    op = PhaseRetrievalOperator((3, 16, 16), pad=8)
    cons = resample.make_consistency(op, torch.zeros(2, *op.y_shape), 1)
    assert type(cons) is resample._GenericConsistency and cons.desc is None
    assert (cons.m, cons.n) == (3 * 32 * 32, 3 * 16 * 16)
    lin = operators.IdentityOperator((3, 16, 16))
    assert type(resample.make_consistency(lin, torch.zeros(2, 3, 16, 16), 1)) is resample._Consistency


def test_descriptor_fields():
    op = PhaseRetrievalOperator((2, 6, 10), pad=(1, 3))
    d = op.hip_descriptor()
    assert _hip.SP_OP_PHASE == 6 and ctypes.sizeof(_hip.SpOp) == 64
    assert (d.kind, d.channels, d.height, d.width) == (6, 2, 6, 10)
    assert d.n == 2 * 6 * 10 and d.m == 2 * 8 * 16
    assert (d.radius, d.factor) == (1, 3)  # pad_h, pad_w
    assert not d.taps and not d.keep_bits and not d.word_rank


def test_library_abi():
    lib = _hip.load_library()
    assert lib.sp_version() >= 104
    for name in ("sp_op_workspace", "sp_op_apply_ws", "sp_op_vjp_ws"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)


def test_library_accepts_only_valid_phase_descriptors():
    lib = _hip.load_library()
    for shape, pad in CASES + [((1, 256, 256), (64, 64)), ((1, 512, 512), (256, 256)),
                               ((3, 512, 512), (128, 128))]:
        op = PhaseRetrievalOperator(shape, pad=pad)
        d = op.hip_descriptor()
        c, nh, nw = op.y_shape
        # one partial per (plane, column tile): at least one tile, at most one per column
        assert c <= lib.sp_rsq_partials(d) <= c * nw and lib.sp_rsq_partials(d) % c == 0, (shape, pad)
        for batch in (1, 5):
            floats = 2 * batch * c * nw * shape[1]
            assert lib.sp_dps_workspace(d, batch) == floats
            assert lib.sp_op_workspace(d, batch) == floats
    # the linear kinds need no operator workspace
    ident = operators.IdentityOperator((3, 16, 16)).hip_descriptor()
    assert lib.sp_op_workspace(ident, 3) == 0

    base = PhaseRetrievalOperator((3, 16, 16), pad=8)
    keep = torch.zeros(64)  # any non-NULL pointer; the host-only calls never read it

    def rejected(**fields):
        d = base.hip_descriptor()
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.sp_rsq_partials(d), lib.sp_dps_workspace(d, 2), lib.sp_op_workspace(d, 2)

    assert all(v > 0 for v in rejected())
    bad = (-1, -1, -1)
    assert rejected(radius=2, m=3 * 20 * 32) == bad                    # Nh = 20
    assert rejected(factor=12, m=3 * 32 * 40) == bad                   # Nw = 40
    assert rejected(height=1024, radius=512, n=3 * 1024 * 16, m=3 * 2048 * 32) == bad  # 2048
    assert rejected(height=2, radius=1, n=3 * 2 * 16, m=3 * 4 * 32) == bad             # 4
    assert rejected(radius=-4, m=3 * 8 * 32) == bad                    # negative pad, Nh = 8
    assert rejected(factor=-4, m=3 * 32 * 8) == bad
    assert rejected(m=3 * 32 * 32 - 1) == bad                          # m != C Nh Nw
    assert rejected(n=3 * 16 * 16 + 4) == bad                          # n != C H W
    assert rejected(taps=keep.data_ptr()) == bad
    assert rejected(keep_bits=keep.data_ptr()) == bad
    assert rejected(word_rank=keep.data_ptr()) == bad
    assert lib.sp_dps_workspace(base.hip_descriptor(), 0) == -1
    assert lib.sp_op_workspace(base.hip_descriptor(), 0) == -1
