"""The channel-mixing kind's C API and Python surface on the host (no GPU): the constant, traits,
descriptor rules by violation, sizes against the header, the return code of every entry point, the
constructor's errors by name, the host maps against tests/chanmix_ref.py, and DDRMSampler,
PGDMSampler and DiffPIRSampler (closed form, conjugate gradients, auto) on host tensors against the
plain loops (DPS has no host form for any operator: its step needs a device)."""

import ctypes

import numpy as np
import pytest
import torch

import chanmix_ref as cr
import samplers_amd
from kind_harness import host_ddrm_check, host_diffpir_check, host_pgdm_check, host_refusals
from samplers_amd import _hip
from samplers_amd.operators import ChannelMixOperator, SVDOperator

KIND, EINVAL, EUNSUPPORTED = 13, -1, -3
_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it
TRAITS = (_hip.SP_TRAIT_LINEAR | _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_NEEDS_ATA_U
          | _hip.SP_TRAIT_PINV)


def make(c=3, cy=1, h=8, w=8, n=None, m=None, taps=PTR, keep=None, rank=None, factor=0):
    d = _hip.SpOp()
    d.kind, d.channels, d.height, d.width, d.radius, d.factor = KIND, c, h, w, cy, factor
    d.n = c * h * w if n is None else n
    d.m = cy * h * w if m is None else m
    d.taps, d.keep_bits, d.word_rank = taps, keep, rank
    return d


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def test_version_constant_and_traits(lib):
    assert _hip.SP_OP_CHANNEL_MIX == KIND and lib.sp_version() >= 115
    assert samplers_amd.ChannelMixOperator is ChannelMixOperator
    for d in (make(), make(8, 8), make(1, 1, 1, 1), make(4, 2, 3, 5)):
        assert lib.sp_op_traits(d) == TRAITS
    assert not TRAITS & (_hip.SP_TRAIT_FUSED_LATENT | _hip.SP_TRAIT_DPS_WORKSPACE)
    unknown = make()
    unknown.kind = KIND + 1
    assert lib.sp_op_traits(unknown) == 0 and lib.sp_rsq_partials(unknown) == EINVAL
    # the descriptor another kind's suite probes "its number + 1" with is Hadamard-shaped (C = 1,
    # radius 0, non-null keep_bits and word_rank, m = 16, n = 64); each rule it breaks rejects it alone
    had = make(c=1, cy=0, h=8, w=8, m=16, keep=PTR, rank=PTR)
    assert lib.sp_op_traits(had) == 0 and lib.sp_rsq_partials(had) == EINVAL
    for alone in (make(c=1, cy=1, keep=PTR, rank=PTR), make(c=1, cy=1, m=16)):  # the NULL rule; m = Cy H W
        assert lib.sp_op_traits(alone) == 0 and lib.sp_rsq_partials(alone) == EINVAL
    assert lib.sp_op_traits(make(c=1, cy=1)) == TRAITS


def test_descriptor_rules_by_violation(lib):
    bad = [make(c=0, cy=0), make(c=9, cy=1), make(cy=0), make(c=3, cy=4), make(factor=1), make(taps=None),
           make(keep=PTR), make(rank=PTR), make(n=3 * 64 + 1), make(m=65), make(cy=2, m=64), make(h=0),
           make(w=0), make(h=-1, w=-8)]
    c = _hip.SpDpsCoefs()
    pc = _hip.SpProxCoefs(1.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    dc = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 0.85, 1.0, 0.5)
    ac = _hip.SpAdamWCoefs()
    for d in bad:
        what = (d.channels, d.height, d.width, d.radius, d.factor, d.n, d.m)
        assert lib.sp_rsq_partials(d) == EINVAL, what
        assert lib.sp_op_traits(d) == 0
        for size in (lib.sp_op_workspace, lib.sp_dps_workspace, lib.sp_prox_workspace, lib.sp_ddrm_workspace,
                     lib.sp_prox_prepare_size):
            assert size(d, 1) == EINVAL, what
        assert lib.sp_op_apply(d, PTR, PTR, 3, None) == EINVAL
        assert lib.sp_op_adjoint(d, PTR, PTR, 3, None) == EINVAL
        assert lib.sp_op_apply_ws(d, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, PTR, None) == EINVAL
        assert lib.sp_pgdm_prepare(d, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
        assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, PTR, None) == EINVAL
        assert lib.sp_dps_residual_sched(d, PTR, PTR, PTR, 3, 1, PTR, PTR, PTR, PTR, None) == EINVAL
        assert lib.sp_dps_update(d, PTR, PTR, PTR, PTR, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR, None) == EINVAL
        assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
        assert lib.sp_prox_prepare(d, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, 0.5, PTR, PTR, None) == EINVAL
        assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, pc, PTR, PTR, None) == EINVAL
        assert lib.sp_ddrm_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, dc, PTR, PTR, None) == EINVAL
        assert lib.sp_prox_cg_workspace(d, 3, 0) == EINVAL
        assert lib.sp_op_prox_cg_ws(d, PTR, PTR, 3, 1, 0.5, 4, 1e-6, PTR, None, PTR, None) == EINVAL
        assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EINVAL
        assert lib.sp_psld_cotangent(d, PTR, PTR, PTR, PTR, 0.1, 3, PTR, None) == EINVAL
        assert lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 3, 1, 1.0, ac, None, PTR, None) == EINVAL
    ok = [make(), make(8, 8), make(8, 1), make(1, 1, 1, 1), make(3, 2, 3, 5), make(5, 5, 1, 7), make(3, 1, 1024, 1024)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.channels, d.radius, d.height, d.width)


@pytest.mark.parametrize("c,cy,h,w", [(3, 1, 1, 1), (3, 2, 3, 5), (3, 1, 64, 36), (3, 3, 33, 35), (8, 5, 256, 256)])
def test_sizes_against_the_header(lib, c, cy, h, w):
    d = make(c, cy, h, w)
    groups = h * w // 4 if h * w % 4 == 0 else h * w
    assert lib.sp_rsq_partials(d) == -(-groups // 256) == cr.partials((c, cy, h, w))
    for size in (lib.sp_op_workspace, lib.sp_prox_workspace, lib.sp_prox_prepare_size, lib.sp_dps_workspace,
                 lib.sp_ddrm_workspace):
        assert size(d, 3) == 0 and size(d, 0) == EINVAL and size(d, -1) == EINVAL
    assert lib.sp_prox_cg_workspace(d, 3, 0) > 0  # conjugate gradients keep their own vectors


def test_return_code_of_every_entry_point(lib):
    d, c = make(), _hip.SpDpsCoefs(1.0, 0.5, 1.0, 0, 0, 0, 0, 0)
    pc = _hip.SpProxCoefs(1.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    dc = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 0.85, 1.0, 0.5)
    ac = _hip.SpAdamWCoefs()
    # null arguments answer before "unsupported"; the fused latent passes do not exist for the kind
    assert lib.sp_psld_pixel(d, None, PTR, 3, 1, PTR, PTR, PTR, None) == EINVAL
    assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_pixel_opt_step(d, None, PTR, PTR, PTR, 3, 1, 1.0, ac, None, PTR, None) == EINVAL
    assert lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 3, 1, 1.0, ac, None, PTR, None) == EUNSUPPORTED
    assert lib.sp_psld_cotangent(d, PTR, PTR, None, PTR, 0.1, 3, PTR, None) == EINVAL  # needs A^T A u
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, PTR, None) == EUNSUPPORTED  # linear: sp_op_adjoint
    # the maps
    assert lib.sp_op_apply(d, None, PTR, 3, None) == EINVAL
    assert lib.sp_op_apply(d, PTR, PTR, 0, None) == EINVAL
    assert lib.sp_op_adjoint(d, PTR, None, 3, None) == EINVAL
    assert lib.sp_op_adjoint(d, PTR, PTR, 65536, None) == EINVAL
    assert lib.sp_op_apply_ws(d, None, PTR, 3, None, None) == EINVAL  # forwards to sp_op_apply
    assert lib.sp_op_pinv_ws(d, None, PTR, 3, 0, None, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 2, None, None) == EINVAL  # transpose is 0 or 1
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 65536, 0, PTR, None) == EINVAL
    # pass 1 of DPS and PGDM
    assert lib.sp_dps_residual(d, PTR, PTR, None, 3, 1, c, PTR, PTR, None) == EINVAL
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 0, c, PTR, PTR, None) == EINVAL
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, None, PTR, PTR, None) == EINVAL
    assert lib.sp_dps_residual_sched(d, PTR, PTR, PTR, 3, 1, None, PTR, PTR, PTR, None) == EINVAL
    assert lib.sp_dps_update(d, PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR, None) == EINVAL  # reads v
    assert lib.sp_pgdm_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 3, PTR, None) == 0  # nothing to prepare, nothing launched
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, None, 3, 1, c, PTR, None, None) == EINVAL  # q is y
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, None, PTR, None, None) == EINVAL
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 0, 1, c, PTR, None, None) == EINVAL
    # the proximal entries: nothing to prepare, y read, no work
    assert lib.sp_prox_prepare(d, PTR, 3, None, None) == 0
    assert lib.sp_prox_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, None, 3, 1, 0.5, PTR, None, None) == EINVAL  # y == NULL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, 0.0, PTR, None, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, float("nan"), PTR, None, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, -1.0, PTR, None, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, pc, PTR, None, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, None, PTR, None, None) == EINVAL
    zero_rho = _hip.SpProxCoefs(1.0, 1.0, 0.0, 1.0, 0.0, 0.0)
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, zero_rho, PTR, None, None) == EINVAL
    # conjugate gradients serve the kind through apply / adjoint
    assert lib.sp_prox_cg_workspace(d, 3, 1) > 0
    assert lib.sp_op_prox_cg_ws(d, PTR, PTR, 3, 1, 0.5, 0, 1e-6, PTR, None, PTR, None) == EINVAL   # max_iter
    assert lib.sp_op_prox_cg_ws(d, PTR, PTR, 3, 1, 0.0, 4, 1e-6, PTR, None, PTR, None) == EINVAL   # rho
    assert lib.sp_diffpir_step_cg_ws(d, PTR, PTR, PTR, None, 0, 0, 0, 3, 1, pc, 8, 1e-6, PTR, None, None,
                                     None) == EINVAL                                              # work
    # DDRM: y read, neither q nor work
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, dc, PTR, None, None) == EINVAL
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 0, dc, PTR, None, None) == EINVAL
    bad = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 1.5, 1.0, 0.5)
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, bad, PTR, None, None) == EINVAL


def test_constructor_errors_by_name():
    eye = np.eye(3)
    rules = [
        (dict(x_shape=(8, 8), matrix=eye), "x_shape must be"),
        (dict(x_shape=(3, 0, 8), matrix=eye), "x_shape must be positive"),
        (dict(x_shape=(3, 8, 8), matrix=np.ones(3)), "matrix must be 2-D"),
        (dict(x_shape=(3, 8, 8), matrix=np.ones((1, 3, 1))), "matrix must be 2-D"),
        (dict(x_shape=(3, 8, 8), matrix=np.ones((1, 4))), "matrix must have C = 3 columns"),
        (dict(x_shape=(3, 8, 8), matrix=np.ones((4, 3))), r"matrix must have between 1 and C = 3 rows"),
        (dict(x_shape=(3, 8, 8), matrix=np.zeros((0, 3))), r"matrix must have between 1 and C = 3 rows"),
        (dict(x_shape=(3, 8, 8), matrix=np.array([[1.0, np.nan, 0.0]])), "matrix must be finite"),
        (dict(x_shape=(3, 8, 8), matrix=np.array([[1.0, np.inf, 0.0]])), "matrix must be finite"),
        (dict(x_shape=(3, 8, 8), matrix=np.zeros((2, 3))), "matrix must be non-zero"),
        (dict(x_shape=(3, 8, 8), matrix=eye, rtol=1.0), "rtol must be in"),
        (dict(x_shape=(3, 8, 8), matrix=eye, rtol=-1e-3), "rtol must be in"),
    ]
    for kwargs, text in rules:
        with pytest.raises(ValueError, match=text):
            ChannelMixOperator(**kwargs)
    with pytest.raises(ValueError, match="weights='luma' requires C = 3"):
        ChannelMixOperator.colorization((4, 8, 8), "luma")
    with pytest.raises(ValueError, match="weights must be"):
        ChannelMixOperator.colorization((3, 8, 8), "green")
    with pytest.raises(ValueError, match="weights must have C = 3 values"):
        ChannelMixOperator.colorization((3, 8, 8), [0.5, 0.5])
    ChannelMixOperator((1, 1, 1), [[2.0]])
    ChannelMixOperator.from_matrix((3, 5, 7), torch.eye(3)[:2])


def test_descriptor_and_interface(lib):
    shape = (3, 6, 10)
    op = ChannelMixOperator.colorization(shape, "luma")
    assert isinstance(op, SVDOperator) and op.pinv_grad_scale == 2.0 and op.hip_linear
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width, d.radius, d.factor) == (KIND, 3, 6, 10, 1, 0)
    assert d.n == 180 and d.m == 60 and d.taps == op.tables.data_ptr() and not d.keep_bits and not d.word_rank
    assert op.tables.dtype == torch.float32 and op.tables.numel() == 2 * 3 + 1 + 9 + 2
    assert lib.sp_rsq_partials(d) == 1 and lib.sp_op_traits(d) == TRAITS
    assert op.shape == (60, 180) and tuple(op.y_shape) == (1, 6, 10)
    assert torch.equal(op.matrix, torch.tensor([[0.299, 0.587, 0.114]]))
    mean = ChannelMixOperator.colorization((4, 2, 2))
    assert torch.equal(mean.matrix, torch.full((1, 4), 0.25)) and torch.equal(mean.pinv_matrix, torch.ones(4, 1))
    w = ChannelMixOperator.colorization(shape, [0.25, 0.5, 0.25])
    assert torch.equal(w.matrix, torch.tensor([[0.25, 0.5, 0.25]]))
    # the kept set: s > rtol * s_max
    two = ChannelMixOperator(shape, cr.from_spectrum(3, (0.8, 4e-4), 19), rtol=1e-2)
    assert two.keep.tolist() == [True, False] and two.pinv_multiplier[1] == 0 and two.singular_values_full[1] > 0
    s = two.get_singular_values()
    assert tuple(s.shape) == (2, 6, 10) and bool((s[1] == 0).all()) and bool((s[0] == two.singular_values_full[0]).all())
    from samplers_amd.samplers.ddrm import SUPPORTED, ddrm_descriptor
    from samplers_amd.samplers.diffpir import cg_descriptor, prox_descriptor
    assert "ChannelMixOperator" in SUPPORTED
    assert ddrm_descriptor(op).kind == prox_descriptor(op).kind == cg_descriptor(op).kind == KIND


@pytest.mark.parametrize("i", [1, 2, 4, 7, 9], ids=[cr.CASES[i][0] for i in (1, 2, 4, 7, 9)])
def test_host_maps_against_the_reference(i):
    name, (c, cy, _, _), _, rtol = cr.case(i)
    shape = (c, cy, 3, 5)
    op = ChannelMixOperator((c, 3, 5), cr.CASES[i][2], rtol=rtol)
    tab = dict(M=op.matrix.numpy(), N=op.pinv_matrix.numpy(), U=op.U.numpy(), V=op.V.numpy(),
               S=op.singular_values_full.numpy(), P=op.pinv_multiplier.numpy())
    ref = cr.svd_tables(cr.CASES[i][2], rtol)  # the tables themselves, up to the sign of a singular pair
    assert np.allclose(tab["M"], ref["M"], atol=1e-7) and np.allclose(tab["N"], ref["N"], atol=1e-6)
    assert np.allclose(tab["S"], ref["S"], atol=1e-7) and np.allclose(tab["P"], ref["P"], rtol=1e-6)
    assert np.array_equal(op.keep.numpy(), ref["keep"])
    mix = cr.Mix(shape, tab)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, c, 3, 5, generator=g, dtype=torch.float64)
    y = torch.randn(2, cy, 3, 5, generator=g, dtype=torch.float64)
    th = mix.V[:, :cy]
    pairs = [(op.apply(x), mix.apply(x)), (op.apply_transpose(y), mix.adjoint(y)),
             (op.apply_pseudo_inverse(y), mix.pinv(y)), (op.apply_pseudo_inverse_transpose(x), mix.pinv_t(x)),
             (op.apply_prox(x, y, 0.3), mix.prox(x, y, 0.3)),
             (op.apply_V_transpose(x), torch.einsum("kr,bkhw->brhw", th, x)),
             (op.apply_V(y), torch.einsum("rk,bkhw->brhw", th, y)),
             (op.apply_U(y), mix.mul("U", y)), (op.apply_U_transpose(y), mix.mul("U", y, True))]
    for got, want in pairs:
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert op.apply(x.float()).dtype == torch.float32 and tuple(op.apply(x[0]).shape) == (cy, 3, 5)
    z = op.apply_prox_cg(x, y, 0.3, iterations=64, tol=1e-9)
    assert float((z - mix.prox(x, y, 0.3)).abs().max()) <= 1e-5  # M against U S V^T in fp32 tables


# --- the samplers on host tensors -----------------------------------------------------------------------------
def _own(op, shape, dt=torch.float64):
    return cr.Mix(shape, dict(M=op.matrix.numpy(), N=op.pinv_matrix.numpy(), U=op.U.numpy(), V=op.V.numpy(),
                              S=op.singular_values_full.numpy(), P=op.pinv_multiplier.numpy()), dtype=dt)


def _host_problem(c=3):
    shape, sigma = (c, 8, 6), 0.1
    op = ChannelMixOperator.colorization(shape, "luma" if c == 3 else "mean")
    y = torch.randn(2, 1, 8, 6, generator=torch.Generator().manual_seed(4))
    return shape, (c, 1, 8, 6), sigma, op, y


@pytest.mark.parametrize("c", [3, 9])
@pytest.mark.parametrize("recon", [1, 2])
def test_host_ddrm_sampler_is_the_plain_loop(recon, c):
    """C = 9 has no descriptor and still runs: ddrm_step_svd through the host maps."""
    shape, full, sigma, op, y = _host_problem(c)
    assert (op.hip_descriptor() is None) == (c == 9)
    host_ddrm_check(op, _own(op, full), y, shape, sigma, recon)
    if c == 3:
        host_refusals(op, y, shape, sigma)


@pytest.mark.parametrize("recon", [1, 2])
def test_host_pgdm_sampler_is_the_plain_loop(recon):
    shape, full, sigma, op, y = _host_problem()
    host_pgdm_check(op, lambda dt: _own(op, full, dt), y, shape, sigma, recon)


@pytest.mark.parametrize("prox", ["cg", "closed_form", "auto"])
def test_host_diffpir_sampler_is_the_plain_loop(prox):
    shape, full, sigma, op, y = _host_problem()
    sampler = host_diffpir_check(op, lambda dt: _own(op, full, dt), y, shape, sigma, prox, tol=1e-6)
    assert sampler.last_step.cg == (prox == "cg")  # auto takes the closed form
    if prox == "cg":  # A A^T = |M|^2 I: the recurrence stops within two iterations
        assert int(sampler.last_step.iterations.max()) <= 2
