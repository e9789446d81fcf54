"""The Walsh–Hadamard kind's C API and Python surface on the host (no GPU): the constant, traits,
descriptor rules by violation, sizes against the header, the return code of every entry point, the
constructor's errors by name, the host maps against tests/hadamard_ref.py, and PGDMSampler,
DiffPIRSampler (closed form and conjugate gradients) and DDRMSampler on host tensors against the
plain loops (DPS has no host form for any operator: its step needs a device)."""

import ctypes

import numpy as np
import pytest
import torch

import hadamard_ref as hr
from kind_harness import host_ddrm_check, host_diffpir_check, host_pgdm_check, host_refusals
from samplers_amd import _hip
from samplers_amd.operators import HadamardOperator, SVDOperator

KIND, EINVAL, EUNSUPPORTED = 12, -1, -3
_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def make(c=1, h=8, w=8, mp=16, n=None, m=None, taps=PTR, keep=PTR, rank=PTR, radius=0, factor=0):
    d = _hip.SpOp()
    d.kind, d.channels, d.height, d.width, d.radius, d.factor = KIND, c, h, w, radius, factor
    d.n = c * h * w if n is None else n
    d.m = c * mp if m is None else m
    d.taps, d.keep_bits, d.word_rank = taps, keep, rank
    return d


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def test_version_constant_and_traits(lib):
    assert _hip.SP_OP_HADAMARD == KIND and lib.sp_version() >= 114
    t = _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_PINV
    assert lib.sp_op_traits(make()) == t and lib.sp_op_traits(make(taps=None)) == t
    assert not t & (_hip.SP_TRAIT_LINEAR | _hip.SP_TRAIT_FUSED_LATENT | _hip.SP_TRAIT_NEEDS_ATA_U)
    unknown = make()
    unknown.kind = KIND + 1
    assert lib.sp_op_traits(unknown) == 0 and lib.sp_rsq_partials(unknown) == EINVAL


def test_descriptor_rules_by_violation(lib):
    bad = [make(h=4, w=8, mp=4),                 # k = 5
           make(h=2048, w=1024, mp=4),           # k = 21
           make(h=8, w=12, mp=4),                # not a power of two
           make(h=0, w=64), make(w=0, h=64), make(c=0), make(n=65), make(c=3, m=47),   # m % C != 0
           make(mp=0), make(mp=65), make(keep=None), make(rank=None), make(radius=1), make(factor=1)]
    c = _hip.SpDpsCoefs()
    pc = _hip.SpProxCoefs(1.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    dc = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 0.85, 1.0, 0.5)
    for d in bad:
        what = (d.channels, d.height, d.width, d.radius, d.factor, d.n, d.m)
        assert lib.sp_rsq_partials(d) == EINVAL, what
        assert lib.sp_op_traits(d) == 0
        for size in (lib.sp_op_workspace, lib.sp_dps_workspace, lib.sp_prox_workspace, lib.sp_ddrm_workspace,
                     lib.sp_prox_prepare_size):
            assert size(d, 1) == EINVAL, what
        assert lib.sp_op_apply_ws(d, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, PTR, None) == EINVAL
        assert lib.sp_pgdm_prepare(d, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, PTR, None) == EINVAL
        assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
        assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, 0.5, PTR, PTR, None) == EINVAL
        assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, pc, PTR, PTR, None) == EINVAL
        assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, dc, PTR, PTR, None) == EINVAL
        assert lib.sp_prox_cg_workspace(d, 3, 0) == EINVAL
    ok = [make(), make(taps=None), make(h=1, w=64, mp=64), make(h=64, w=1, mp=1), make(h=1024, w=1024, mp=7),
          make(c=3, h=8, w=16, mp=32), make(h=2, w=32, mp=64), make(h=4, w=1 << 18, mp=5)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.height, d.width, d.m)


@pytest.mark.parametrize("c,h,w,tiles", [(1, 8, 8, 1), (3, 8, 16, 1), (1, 64, 64, 1), (2, 64, 128, 2),
                                         (3, 128, 128, 4), (3, 256, 256, 16), (1, 512, 512, 64), (1, 1024, 1024, 128)])
def test_sizes_against_the_header(lib, c, h, w, tiles):
    d = make(c, h, w, mp=h * w // 4)
    n = c * h * w
    assert lib.sp_rsq_partials(d) == c * tiles  # one per plane, or per tile of the high stage
    for size in (lib.sp_op_workspace, lib.sp_prox_workspace, lib.sp_prox_prepare_size, lib.sp_dps_workspace,
                 lib.sp_ddrm_workspace):
        assert size(d, 3) == 3 * n and size(d, 0) == EINVAL and size(d, -1) == EINVAL
    assert n >= d.m  # a row of q (n floats) holds a row of y
    assert lib.sp_prox_cg_workspace(d, 3, 0) > lib.sp_op_workspace(d, 3)


def test_return_code_of_every_entry_point(lib):
    d, c = make(), _hip.SpDpsCoefs(1.0, 0.5, 1.0, 0, 0, 0, 0, 0)
    pc = _hip.SpProxCoefs(1.0, 1.0, 0.5, 1.0, 0.0, 0.0)
    dc = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 0.85, 1.0, 0.5)
    # the maps run through the workspace forms only; no latent passes
    assert lib.sp_op_apply(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_op_adjoint(d, PTR, PTR, 3, None) == EUNSUPPORTED
    assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None) == EUNSUPPORTED
    assert lib.sp_op_apply_ws(d, PTR, PTR, 3, None, None) == EINVAL          # work == NULL
    assert lib.sp_op_apply_ws(d, None, PTR, 3, PTR, None) == EINVAL
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, None, None) == EINVAL
    assert lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 0, PTR, None) == EINVAL
    assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None, None) == EINVAL
    assert lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 0, c, PTR, PTR, PTR, None) == EINVAL
    assert lib.sp_dps_residual_sched_ws(d, PTR, PTR, PTR, 3, 1, None, PTR, PTR, PTR, PTR, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, None, None) == EINVAL
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 2, PTR, None) == EINVAL         # transpose is 0 or 1
    assert lib.sp_op_pinv_ws(d, PTR, PTR, 65536, 0, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_pgdm_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, None, 3, 1, c, PTR, PTR, None) == EINVAL
    assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, None, None) == EINVAL
    assert lib.sp_dps_update(d, PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR, None) == EINVAL
    # the proximal entries: nothing to prepare (the launches read y itself), work required
    assert lib.sp_prox_prepare(d, PTR, 3, None, None) == 0
    assert lib.sp_prox_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, None, 3, 1, 0.5, PTR, PTR, None) == EINVAL   # y == NULL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, 0.5, PTR, None, None) == EINVAL   # work == NULL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, 0.0, PTR, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, PTR, None, 3, 1, float("nan"), PTR, PTR, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, pc, PTR, PTR, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, pc, PTR, None, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, PTR, None, None, 0, 0, 0, 3, 1, None, PTR, PTR, None) == EINVAL
    # conjugate gradients serve the kind through apply_ws / vjp_ws
    assert lib.sp_prox_cg_workspace(d, 3, 1) > 0
    assert lib.sp_op_prox_cg_ws(d, PTR, PTR, 3, 1, 0.5, 0, 1e-6, PTR, None, PTR, None) == EINVAL   # max_iter
    assert lib.sp_diffpir_step_cg_ws(d, PTR, PTR, PTR, None, 0, 0, 0, 3, 1, pc, 8, 1e-6, PTR, None, None,
                                     None) == EINVAL                                              # work
    # DDRM: q and work required, y not read
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, dc, PTR, PTR, None) == EINVAL
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, dc, PTR, None, None) == EINVAL
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 0, dc, PTR, PTR, None) == EINVAL
    bad = _hip.SpDdrmCoefs(1.0, 0.5, 1.0, 0.5, 0.05, 1.5, 1.0, 0.5)
    assert lib.sp_ddrm_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, bad, PTR, PTR, None) == EINVAL


def test_constructor_errors_by_name():
    ones = torch.ones(64)
    rules = [
        (dict(x_shape=(8, 8)), "x_shape must be"),
        (dict(x_shape=(0, 8, 8)), "x_shape must be positive"),
        (dict(x_shape=(1, 8, 12)), "power of two"),
        (dict(x_shape=(1, 4, 8)), "out of range"),
        (dict(x_shape=(1, 2048, 1024)), "out of range"),
        (dict(x_shape=(1, 8, 8), ratio=0.0), "ratio must be in"),
        (dict(x_shape=(1, 8, 8), kept=torch.zeros(64, dtype=torch.bool)), "kept set is empty"),
        (dict(x_shape=(1, 8, 8), kept=torch.zeros(0, dtype=torch.int64)), "kept set is empty"),
        (dict(x_shape=(1, 8, 8), kept=torch.ones(63, dtype=torch.bool)), "wrong length"),
        (dict(x_shape=(1, 8, 8), kept=torch.tensor([3, 64])), "wrong length"),
        (dict(x_shape=(1, 8, 8), signs=ones[:63]), "wrong length"),
        (dict(x_shape=(1, 8, 8), signs=ones * 0.5), "signs must be ±1"),
        (dict(x_shape=(1, 8, 8), signs=ones * 0), "signs must be ±1"),
    ]
    for kwargs, text in rules:
        with pytest.raises(ValueError, match=text):
            HadamardOperator(**kwargs)
    HadamardOperator((1, 1, 64), kept=[5])            # one coefficient, H = 1
    HadamardOperator((2, 8, 8), ratio=1.0, signs=-ones)


def test_descriptor_and_interface(lib):
    shape = (2, 8, 16)
    op = HadamardOperator(shape, ratio=0.25, seed=3)
    assert isinstance(op, SVDOperator) and op.pinv_grad_scale == 2.0 and not op.hip_linear
    same = HadamardOperator(shape, ratio=0.25, seed=3)
    assert torch.equal(same.keep, op.keep) and torch.equal(same.signs, op.signs)
    assert not torch.equal(HadamardOperator(shape, ratio=0.25, seed=4).keep, op.keep)
    assert int(op.keep.sum()) == 32 and set(op.signs.tolist()) == {-1.0, 1.0}
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width, d.radius, d.factor) == (KIND, 2, 8, 16, 0, 0)
    assert d.n == 2 * 128 and d.m == 2 * 32 and d.taps == op.signs.data_ptr()
    assert d.keep_bits == op._keep_bits.data_ptr() and d.word_rank == op._word_rank.data_ptr()
    assert op._keep_bits.numel() == 2 and op._word_rank.tolist() == [0, int(op.keep[:64].sum())]
    assert lib.sp_rsq_partials(d) == 2 and lib.sp_op_traits(d) == 35
    plain = HadamardOperator(shape, kept=op.keep, signs=False)
    assert plain.signs is None and not plain.hip_descriptor().taps and HadamardOperator(shape, signs=None).signs is None
    assert op.shape == (64, 256) and tuple(op.y_shape) == (2, 32)
    s = op.get_singular_values()
    assert tuple(s.shape) == (2, 32) and bool((s == 1).all())
    by_index = HadamardOperator(shape, kept=torch.nonzero(op.keep).squeeze(1).flip(0), signs=op.signs)
    assert torch.equal(by_index.keep, op.keep)  # ascending order whatever the order given
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, *shape, generator=g, dtype=torch.float64)
    y = torch.randn(3, 2, 32, generator=g, dtype=torch.float64)
    S = hr.Had(shape, op.keep.numpy(), op.signs.numpy())
    for got, want in ((op.apply(x), S.apply(x)), (op.apply_transpose(y), S.adjoint(y)),
                      (op.apply_pseudo_inverse(y), S.pinv(y)), (op.apply_pseudo_inverse_transpose(x), S.pinv_t(x)),
                      (op.apply_prox(x, y, 0.3), S.prox(x, y, 0.3)), (op.apply_V_transpose(x), S.apply(x)),
                      (op.apply_V(y), S.adjoint(y)), (plain.apply(x), hr.Had(shape, op.keep.numpy()).apply(x))):
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert op.apply_U(y) is y and op.apply_U_transpose(y) is y
    assert op.apply(x.float()).dtype == torch.float32 and tuple(op.apply(x[0]).shape) == (2, 32)
    assert float((op.apply(op.apply_transpose(y)) - y).abs().max()) <= 1e-12  # A Aᵀ = I
    z, iters = op.apply_prox_cg(x, y, 0.3, iterations=64, tol=1e-6, return_iterations=True)
    assert float((z - S.prox(x, y, 0.3)).abs().max()) <= 1e-10 and 1 <= int(iters.min()) and int(iters.max()) <= 2
    from samplers_amd.samplers.ddrm import SUPPORTED, ddrm_descriptor
    from samplers_amd.samplers.diffpir import cg_descriptor, prox_descriptor
    assert "HadamardOperator" in SUPPORTED
    assert ddrm_descriptor(op).kind == prox_descriptor(op).kind == cg_descriptor(op).kind == KIND


# --- the samplers on host tensors -----------------------------------------------------------------------------
def _host_problem():
    shape, sigma = (1, 8, 16), 0.1
    op = HadamardOperator(shape, ratio=0.5, seed=5)
    y = torch.randn(2, 1, 64, generator=torch.Generator().manual_seed(4))
    return shape, sigma, op, (op.keep.numpy(), op.signs.numpy()), y


@pytest.mark.parametrize("recon", [1, 2])
def test_host_ddrm_sampler_is_the_plain_loop(recon):
    shape, sigma, op, (keep, sg), y = _host_problem()
    host_ddrm_check(op, hr.Had(shape, keep, sg), y, shape, sigma, recon)
    host_refusals(op, y, shape, sigma)


@pytest.mark.parametrize("recon", [1, 2])
def test_host_pgdm_sampler_is_the_plain_loop(recon):
    shape, sigma, op, (keep, sg), y = _host_problem()
    host_pgdm_check(op, lambda dt: hr.Had(shape, keep, sg, dtype=dt), y, shape, sigma, recon)


@pytest.mark.parametrize("prox", ["cg", "closed_form", "auto"])
def test_host_diffpir_sampler_is_the_plain_loop(prox):
    shape, sigma, op, (keep, sg), y = _host_problem()
    sampler = host_diffpir_check(op, lambda dt: hr.Had(shape, keep, sg, dtype=dt), y, shape, sigma, prox, tol=1e-6)
    if prox == "cg":  # A Aᵀ = I: the recurrence stops within two iterations, on the closed form's point
        assert int(sampler.last_step.iterations.max()) <= 2
