"""SP_OP_SR_PERIODIC on the host: the constructor's rules by name, the descriptor, and the library's
table row (geometry rules, traits, workspace / partial / prepare sizes, return codes), as
tests/test_periodic_api.py and tests/test_diffpir_api.py read theirs.  No GPU: the library loads
without one and every call here returns before a launch."""

import ctypes
import math

import pytest
import torch

from kind_harness import make_descriptor as make
from samplers_amd import _hip
from samplers_amd.inverse_problem import InverseProblem
from samplers_amd.noise import GaussianNoise
from samplers_amd.operators import PeriodicSuperResolutionOperator, bicubic_taps
from samplers_amd.operators.sr_filter import gaussian_filter_taps

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
KIND = 10

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def srp(c=1, h=8, w=8, s=2, k=None, **kw):
    args = dict(radius=s if k is None else k, factor=s, taps=PTR)
    args.update(kw)
    return make(KIND, c * h * w, c * h * w // (s * s), c, h, w, **args)


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def test_version_and_constants(lib):
    assert lib.sp_version() >= 110
    assert _hip.SP_OP_SR_PERIODIC == KIND


def test_constructor_rules_by_name():
    k8 = bicubic_taps(2)
    rules = [
        (dict(x_shape=(1, 16, 16), taps=k8, factor=3), "factor must be one of"),
        (dict(x_shape=(16, 16), taps=k8, factor=2), "x_shape must be"),
        (dict(x_shape=(1, 20, 16), taps=k8, factor=2), "2\\^k or 3\\*2\\^k"),
        (dict(x_shape=(1, 16, 4), taps=k8, factor=2), "2\\^k or 3\\*2\\^k"),
        (dict(x_shape=(1, 2048, 16), taps=k8, factor=2), "2\\^k or 3\\*2\\^k"),
        (dict(x_shape=(1, 12, 16), taps=torch.ones(8), factor=8), "multiples of the factor"),
        (dict(x_shape=(1, 16, 16), taps=torch.ones(2), factor=4), "number of taps must be in"),
        (dict(x_shape=(1, 8, 16), taps=torch.ones(10), factor=2), "number of taps must be in"),
        (dict(x_shape=(1, 16, 16), taps=torch.ones(5), factor=2), "parity of the factor"),
        (dict(x_shape=(1, 16, 16), taps=torch.ones(4, 6), factor=2), "1-D or a square 2-D"),
        (dict(x_shape=(1, 16, 16), taps=torch.ones(2, 2, 2), factor=2), "1-D or a square 2-D"),
        (dict(x_shape=(1, 16, 16), taps=torch.tensor([1.0, float("nan")]), factor=2), "finite"),
        (dict(x_shape=(1, 16, 16), taps=k8, factor=2, rtol=0.0), "rtol must be in"),
        (dict(x_shape=(1, 16, 16), taps=k8, factor=2, rtol=1.0), "rtol must be in"),
    ]
    for kwargs, text in rules:
        with pytest.raises(ValueError, match=text):
            PeriodicSuperResolutionOperator(**kwargs)
    PeriodicSuperResolutionOperator((1, 8, 16), torch.ones(8), factor=2)   # K = min(H, W)
    PeriodicSuperResolutionOperator((1, 8, 8), torch.ones(8), factor=8)    # a 1 x 1 observation


def test_classmethods():
    b = PeriodicSuperResolutionOperator.bicubic((3, 32, 32), 4)
    want = torch.outer(bicubic_taps(4).double(), bicubic_taps(4).double())
    assert torch.equal(b.kernel, want) and (b.factor, b.kernel_size, b.pad) == (4, 16, 6)
    g = PeriodicSuperResolutionOperator.gaussian((3, 32, 32), 4, 16, 3.0, rtol=0.1)
    t = gaussian_filter_taps(16, 3.0).double()
    assert torch.equal(g.kernel, torch.outer(t, t)) and g.rtol == 0.1
    assert tuple(g.y_shape) == (3, 8, 8)
    with pytest.raises(ValueError):
        PeriodicSuperResolutionOperator.gaussian((3, 32, 32), 4, 15, 3.0)


def test_descriptor(lib):
    op = PeriodicSuperResolutionOperator.bicubic((2, 16, 24), 2)
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width) == (KIND, 2, 16, 24)
    assert d.n == 2 * 16 * 24 and d.m == 2 * 8 * 12 and (d.radius, d.factor) == (8, 2)
    assert d.taps == op.spectra.data_ptr() and not d.keep_bits and not d.word_rank
    t = _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_PINV
    assert lib.sp_op_traits(d) == t and lib.sp_op_traits(srp()) == t
    assert not t & _hip.SP_TRAIT_LINEAR


def _lines(N):
    NP = (N + N // 16) | 1
    return max(1, min(16, (32000 - 8 * N) // (16 * NP)))


@pytest.mark.parametrize("c,h,w,s,k", [(1, 8, 8, 2, 2), (2, 16, 24, 2, 8), (3, 256, 256, 4, 16),
                                       (1, 512, 1024, 4, 16), (1, 1024, 8, 8, 8), (1, 48, 96, 8, 32)])
def test_sizes(lib, c, h, w, s, k):
    d = srp(c, h, w, s, k)
    # one r^2 partial per (plane, tile of lattice rows)
    t = min(_lines(w), h // s)
    assert lib.sp_rsq_partials(d) == c * -(-(h // s) // t)
    floats = 2 * 3 * c * (w // 2 + 1) * h
    for size in (lib.sp_dps_workspace, lib.sp_op_workspace, lib.sp_prox_workspace,
                 lib.sp_prox_prepare_size):
        assert size(d, 3) == floats and size(d, 0) == EINVAL
    assert floats // 3 >= d.m  # a row of q holds a row of y


def test_descriptor_rules(lib):
    bad = [srp(1, 20, 16), srp(1, 16, 20), srp(1, 4, 8), srp(1, 2048, 8), srp(0, 8, 8),
           srp(1, 8, 8, 3), srp(1, 8, 8, 1), srp(1, 8, 8, 16),
           make(KIND, 12 * 16, 3, 1, 12, 16, radius=8, factor=8, taps=PTR),     # 8 does not divide 12
           srp(1, 8, 8, 2, 1), srp(1, 8, 8, 2, 3), srp(1, 8, 8, 2, 10), srp(1, 8, 16, 2, 10),
           srp(1, 8, 8, 4, 2), srp(1, 8, 8, taps=None), srp(1, 8, 8, keep=PTR), srp(1, 8, 8, rank=PTR),
           make(KIND, 64, 64, 1, 8, 8, radius=2, factor=2, taps=PTR),           # m != n / s^2
           make(KIND, 65, 16, 1, 8, 8, radius=2, factor=2, taps=PTR),
           make(KIND, 64, 64, 1, 8, 8),                                         # no taps, factor 0
           make(11, 64, 16, 1, 8, 8, radius=2, factor=2, taps=PTR)]             # past the table
    c = _hip.SpDpsCoefs()
    for d in bad:
        assert lib.sp_rsq_partials(d) == EINVAL, (d.height, d.width, d.radius, d.factor)
        assert lib.sp_op_traits(d) == 0
        assert lib.sp_op_workspace(d, 1) == EINVAL and lib.sp_prox_workspace(d, 1) == EINVAL
        assert lib.sp_op_apply_ws(d, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, PTR, None) == EINVAL
        assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
    ok = [srp(1, 8, 8, 2, 8), srp(1, 8, 16, 2, 8), srp(1, 8, 8, 8, 8), srp(2, 24, 48, 8, 24),
          srp(1, 1024, 768, 4, 768), srp(1, 12, 16, 4, 12)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.height, d.width, d.radius, d.factor)


def test_argument_checks_and_return_codes(lib):
    d, c, pc = srp(), _hip.SpDpsCoefs(), _hip.SpProxCoefs(1.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    # the maps run through the workspace forms only
    assert lib.sp_op_apply(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_op_adjoint(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_op_apply_ws(d, PTR, PTR, 3, None, None) == EINVAL          # work == NULL
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, None, None) == EINVAL
    assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, None, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 2, PTR, None) == EINVAL         # transpose is 0 or 1
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 65536, 0, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, None, 3, 1, c, PTR, PTR, None) == EINVAL
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, None, None) == EINVAL
    assert lib.sp_dps_update(d, PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR,
                             None) == EINVAL                                  # pass 2 needs v
    # the proximal entries: a kind that prepares needs q and work, y may be NULL
    assert lib.sp_prox_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_prox_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, None, 3, 1, 0.5, PTR, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, 0.5, PTR, None, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, 0.0, PTR, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, float("nan"), PTR, PTR, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, pc, PTR, PTR,
                                  None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, pc, PTR, None,
                                  None) == EINVAL


def test_samplers_accept_the_operator_up_to_the_device_check():
    """PGDMSampler's pseudo-inverse probe and DiffPIR's proximal probe must not raise; the calls
    then stop at the device check, since this observation lives on the host."""
    import stand_ins as si
    from samplers_amd.samplers.diffpir import prox_descriptor
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = PeriodicSuperResolutionOperator.gaussian((3, 32, 32), 4, 16, 3.0)
    assert 0 < int(op.keep.sum()) < op.keep.numel()
    assert tuple(op.apply_pseudo_inverse(torch.zeros(1, *op.y_shape)).shape) == (1, 3, 32, 32)
    assert prox_descriptor(op).kind == KIND
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, *op.y_shape), GaussianNoise(0.05))
    with pytest.raises(_hip.HipLibraryError, match="HIP"):
        PGDMSampler(net)(ip, num_sampling_steps=4)
    assert math.prod(op.y_shape) * 16 == math.prod(op.x_shape)
