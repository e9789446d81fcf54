"""RadonOperator on the host and the library's SP_OP_RADON descriptor rules, counts, traits and
entry-point forms (no GPU: the library loads and answers these without one)."""

import math

import numpy as np
import pytest
import torch

import radon_ref as rr
from samplers_amd import _hip, operators
from samplers_amd.operators import LinearOperator, RadonOperator, radon_table

EINVAL, EUNSUPPORTED = -1, -3
PTR = 0x1000  # a non-null dummy: these calls return before any launch


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def make(c=2, h=24, w=20, angles=7, d=33, **fields):
    desc = _hip.SpOp()
    desc.kind = _hip.SP_OP_RADON
    desc.channels, desc.height, desc.width = c, h, w
    desc.n, desc.m = c * h * w, c * angles * d
    desc.radius, desc.factor = angles, d
    desc.taps = PTR
    for k, v in fields.items():
        setattr(desc, k, v)
    return desc


def test_exported_and_version(lib):
    assert _hip.SP_OP_RADON == 9
    assert "RadonOperator" in operators.__all__ and "radon_table" in operators.__all__
    assert issubclass(RadonOperator, LinearOperator) and RadonOperator.hip_linear is True
    assert lib.sp_version() >= 108


def test_descriptor_rules(lib):
    assert lib.sp_rsq_partials(make()) > 0
    bad = {
        "null taps": make(taps=None),
        "0 angles": make(angles=0), "513 angles": make(angles=513),
        "D = 0": make(d=0), "D = 1025": make(d=1025),
        "H = 7": make(h=7), "H = 513": make(h=513), "W = 7": make(w=7), "W = 513": make(w=513),
        "m mismatched": make(m=2 * 7 * 33 + 1), "n mismatched": make(n=2 * 24 * 20 - 1),
        "m == n, not the sinogram's": make(m=2 * 24 * 20),
        "keep_bits": make(keep_bits=PTR), "word_rank": make(word_rank=PTR),
        "no channels": make(c=0),
    }
    for what, d in bad.items():
        assert lib.sp_rsq_partials(d) == EINVAL, what
        assert lib.sp_dps_workspace(d, 2) == EINVAL, what
        assert lib.sp_op_traits(d) == 0, what
    for d in (make(angles=1), make(angles=512, d=1), make(d=1), make(d=1024), make(h=8, w=8),
              make(h=512, w=512, c=1)):
        assert lib.sp_rsq_partials(d) > 0


@pytest.mark.parametrize("c,angles,d", [(1, 5, 17), (2, 7, 33), (3, 23, 59), (1, 2, 256), (1, 2, 257),
                                        (1, 3, 300), (2, 512, 1024), (1, 1, 1)])
def test_counts(lib, c, angles, d):
    desc = make(c=c, angles=angles, d=d)
    assert lib.sp_rsq_partials(desc) == c * angles * math.ceil(d / 256)  # workgroups of `project`
    for batch in (1, 3, 64):
        assert lib.sp_dps_workspace(desc, batch) == batch * desc.m
        assert lib.sp_op_workspace(desc, batch) == 0
    assert lib.sp_dps_workspace(desc, 0) == EINVAL


def test_traits(lib):
    t = lib.sp_op_traits(make())
    assert t == (_hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_LINEAR
                 | _hip.SP_TRAIT_NEEDS_ATA_U)
    assert not t & (_hip.SP_TRAIT_FUSED_LATENT | _hip.SP_TRAIT_PINV)


def test_entry_point_forms(lib):
    d, c, a = make(), _hip.SpDpsCoefs(), _hip.SpAdamWCoefs()
    # pass 1 runs in the _ws forms only, and needs its workspace
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_dps_residual_sched(d, PTR, PTR, PTR, 3, 1, PTR, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None, None) == EINVAL
    assert lib.sp_dps_residual_sched_ws(d, PTR, PTR, PTR, 3, 1, PTR, PTR, PTR, PTR, None, None) == EINVAL
    # pass 2 cannot re-derive v
    assert lib.sp_dps_update(d, PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR, None) == EINVAL
    assert lib.sp_dps_update_sched(d, PTR, PTR, PTR, None, PTR, PTR, 0, 0, 3, 1, PTR, PTR, PTR,
                                   None) == EINVAL
    # no pseudo-inverse, no fused latent passes, no VJP through a workspace; A^T A u is required
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, PTR, None) == EUNSUPPORTED
    assert lib.sp_pgdm_prepare(d, PTR, 3, PTR, None) == EUNSUPPORTED
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, PTR, None) == EUNSUPPORTED
    assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 3, 1, 1.0, a, None, PTR, None) == EUNSUPPORTED
    assert lib.sp_psld_cotangent(d, PTR, PTR, None, PTR, 0.1, 3, PTR, None) == EINVAL
    # null arguments of the maps
    assert lib.sp_op_apply(d, None, PTR, 3, None) == EINVAL
    assert lib.sp_op_adjoint(d, PTR, None, 3, None) == EINVAL


def test_table_against_an_independent_fp64_computation():
    angles = [0.0, math.pi / 2, math.pi, 3 * math.pi / 2, math.pi / 4, 3 * math.pi / 4, 0.3, 1.1, 2.0,
              -0.7, 5.5, math.pi / 4 + 1e-9, math.pi / 4 - 1e-9]
    t = radon_table(angles)
    assert t.dtype == torch.float32 and tuple(t.shape) == (len(angles), 4)
    assert np.array_equal(t.numpy(), rr.table_of(angles))
    # the snapped axis angles: exact rows
    assert t[:4].tolist() == [[1, 0, 1, 0], [1, 0, 1, 1], [-1, 0, 1, 0], [-1, 0, 1, 1]]
    # the tie: |cos| >= |sin| is axis 0 (in fp64 cos(pi/4) > sin(pi/4) by one ulp)
    assert math.cos(math.pi / 4) >= math.sin(math.pi / 4) and t[4, 3] == 0
    r2 = np.float32(math.sqrt(2.0))
    assert abs(float(t[4, 0]) - r2) <= 1e-6 and abs(float(t[4, 1]) + 1) <= 1e-6 and abs(float(t[4, 2]) - r2) <= 1e-6
    assert t[5, 3] == 1  # 3 pi / 4 in fp64: |cos| < |sin|
    for row, th in zip(t.double().tolist(), angles):  # each row is its own angle's
        c, s = math.cos(th), math.sin(th)
        dom = s if row[3] else c
        assert abs(row[0] - 1 / dom) <= 1e-6 and abs(row[2] - 1 / abs(dom)) <= 1e-6
    # the preconditions the library states for a table
    assert float(t[:, 0].abs().min()) >= 1 and float(t[:, 1].abs().max()) <= 1 + 1e-7
    assert torch.equal(radon_table(torch.tensor(angles, dtype=torch.float64)), t)
    assert torch.equal(radon_table(np.asarray(angles)), t)


def test_constructor_defaults_and_shapes():
    op = RadonOperator((3, 40, 36))
    assert op.x_shape == (3, 40, 36) and op.num_angles == 23
    d = 2 * math.ceil(math.sqrt(40 * 40 + 36 * 36) / 2) + 1
    assert d == 55 and op.detector_size == d and op.y_shape == (3, 23, d)
    assert np.array_equal(op.table.numpy(), rr.table_of([math.pi * a / 23 for a in range(23)]))
    assert RadonOperator((1, 256, 256)).detector_size == 365
    assert RadonOperator((1, 512, 512)).detector_size == 727
    op = RadonOperator((2, 24, 20), angles=[0.1, 0.2, 2.0], detector_size=12)
    assert op.y_shape == (2, 3, 12) and op.angles == (0.1, 0.2, 2.0)
    lim = RadonOperator.limited_angle((1, 16, 16), 6, math.pi / 2)
    assert lim.num_angles == 6
    assert np.array_equal(lim.table.numpy(), rr.table_of([math.pi / 2 * a / 6 for a in range(6)]))
    x = torch.zeros(2, 2, 24, 20)
    assert tuple(op.apply(x).shape) == (2, 2, 3, 12)
    assert tuple(op.apply_transpose(torch.zeros(5, 1, 2, 3, 12)).shape) == (5, 1, 2, 24, 20)
    with pytest.raises(NotImplementedError):
        op.apply_pseudo_inverse(torch.zeros(1, 2, 3, 12))


@pytest.mark.parametrize("args,kwargs", [
    (((24, 20),), {}),                                   # not (C, H, W)
    (((1, 2, 24, 20),), {}),
    (((1, 7, 20),), {}), (((1, 24, 513),), {}), (((0, 24, 20),), {}),
    (((1, 24, 20),), {"angles": []}),
    (((1, 24, 20),), {"angles": [0.1, float("nan")]}),
    (((1, 24, 20),), {"angles": [float("inf")]}),
    (((1, 24, 20),), {"angles": [0.01 * a for a in range(513)]}),
    (((1, 24, 20),), {"num_angles": 0}), (((1, 24, 20),), {"num_angles": 513}),
    (((1, 24, 20),), {"detector_size": 0}), (((1, 24, 20),), {"detector_size": 1025}),
])
def test_bad_arguments_raise(args, kwargs):
    with pytest.raises(ValueError):
        RadonOperator(*args, **kwargs)


def test_descriptor_fields(lib):
    op = RadonOperator((3, 40, 36), num_angles=9, detector_size=61)
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width) == (_hip.SP_OP_RADON, 3, 40, 36)
    assert d.n == 3 * 40 * 36 and d.m == 3 * 9 * 61 and d.radius == 9 and d.factor == 61
    assert d.taps == op.table.data_ptr() and not d.keep_bits and not d.word_rank
    assert lib.sp_rsq_partials(d) == 3 * 9
    op.table = op.table.clone()  # the pointer is read at call time (e.g. after .to(device))
    assert op.hip_descriptor().taps == op.table.data_ptr()


def test_dot_product_identity_on_the_host():
    op = RadonOperator((2, 24, 20), num_angles=7, detector_size=33)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 2, 24, 20, dtype=torch.float64, generator=g)
    y = torch.randn(3, 2, 7, 33, dtype=torch.float64, generator=g)
    lhs, rhs = (op.apply(x) * y).sum(), (x * op.apply_transpose(y)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    x32 = x.float()
    assert op.apply(x32).dtype == torch.float32
    assert float((op.apply(x32).double() - op.apply(x)).abs().max()) <= 2e-5 * float(op.apply(x).abs().max())


def test_no_pseudo_inverse_so_pgdm_raises():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = RadonOperator((3, 32, 32), num_angles=9)
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(ip, num_sampling_steps=4)


def test_fused_dps_refuses_an_operator_without_a_descriptor_by_name():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.dps import FusedDPSStep

    class Plain(RadonOperator):
        def hip_descriptor(self):
            return None

    op = Plain((3, 32, 32), num_angles=4)
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="RadonOperator"):
        FusedDPSStep(net, ip, torch.zeros(1, *op.y_shape), 1)
