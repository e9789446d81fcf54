"""The separable-SVD kind's C API and Python surface on the host (no GPU): the constants, traits,
descriptor rules by violation, workspace and prepare sizes against the header's formulas, the return
code of every entry point, the constructor's errors by name, the host maps, and DDRMSampler, PGDMSampler and
DiffPIRSampler (conjugate gradients and the closed form) on host tensors against the plain loops."""

import ctypes

import numpy as np
import pytest
import torch

import svd_sep_ref as sr
from kind_harness import host_ddrm_check, host_diffpir_check, host_pgdm_check, host_refusals
from samplers_amd import _hip
from samplers_amd.operators import SeparableSVDOperator, SVDOperator

KIND, EINVAL, EUNSUPPORTED = 11, -1, -3
_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def make(c=1, h=8, w=8, hy=8, wy=8, n=None, m=None, taps=PTR, keep=None, rank=None):
    d = _hip.SpOp()
    d.kind, d.channels, d.height, d.width, d.radius, d.factor = KIND, c, h, w, hy, wy
    d.n = c * h * w if n is None else n
    d.m = c * hy * wy if m is None else m
    d.taps, d.keep_bits, d.word_rank = taps, keep, rank
    return d


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def test_version_constant_and_traits(lib):
    assert _hip.SP_OP_SVD_SEPARABLE == KIND and lib.sp_version() >= 113
    t = _hip.SP_TRAIT_UPDATE_READS_V | _hip.SP_TRAIT_DPS_WORKSPACE | _hip.SP_TRAIT_PINV
    assert lib.sp_op_traits(make()) == t
    assert not t & (_hip.SP_TRAIT_LINEAR | _hip.SP_TRAIT_FUSED_LATENT | _hip.SP_TRAIT_NEEDS_ATA_U)


def test_descriptor_rules_by_violation(lib):
    bad = [make(h=1, hy=1), make(w=1, wy=1), make(h=513, hy=8), make(w=513, wy=8), make(hy=9), make(wy=9),
           make(hy=0), make(wy=0), make(c=0), make(m=63), make(n=65), make(taps=None), make(keep=PTR),
           make(rank=PTR), make(hy=2, wy=2, m=16)]  # the last: m != C Hy Wy (test_sr_periodic_api.py's literal)
    c = _hip.SpDpsCoefs()
    for d in bad:
        what = (d.channels, d.height, d.width, d.radius, d.factor, d.n, d.m)
        assert lib.sp_rsq_partials(d) == EINVAL, what
        assert lib.sp_op_traits(d) == 0
        for size in (lib.sp_op_workspace, lib.sp_dps_workspace, lib.sp_prox_workspace, lib.sp_ddrm_workspace,
                     lib.sp_prox_prepare_size):
            assert size(d, 1) == EINVAL, what
        assert lib.sp_op_apply_ws(d, PTR, PTR, 3, PTR, None) == EINVAL
        assert lib.sp_op_pinv_ws(d, PTR, PTR, 3, 0, PTR, None) == EINVAL
        assert lib.sp_pgdm_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
    ok = [make(), make(h=2, w=2, hy=1, wy=1), make(h=512, w=512, hy=512, wy=512), make(c=3, h=33, w=35, hy=33, wy=35),
          make(h=24, w=16, hy=12, wy=4), make(h=129, w=130, hy=1, wy=130)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.height, d.width, d.radius, d.factor)


@pytest.mark.parametrize("c,h,w,hy,wy", [(1, 3, 5, 3, 5), (2, 32, 32, 8, 8), (1, 129, 130, 129, 130),
                                         (3, 256, 256, 256, 256), (1, 512, 512, 65, 64)])
def test_sizes_against_the_header(lib, c, h, w, hy, wy):
    d = make(c, h, w, hy, wy)
    n = c * h * w
    assert lib.sp_rsq_partials(d) == c * -(-hy // 64) * -(-wy // 64)  # one per (plane, 64 x 64 tile)
    for size, per in ((lib.sp_op_workspace, 2), (lib.sp_prox_workspace, 2), (lib.sp_prox_prepare_size, 2),
                      (lib.sp_dps_workspace, 3), (lib.sp_ddrm_workspace, 4)):
        assert size(d, 3) == per * 3 * n and size(d, 0) == EINVAL and size(d, -1) == EINVAL
    assert 2 * n >= 2 * d.m  # a row of q holds q and the prepare launches' intermediate
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
    # the proximal entries: the kind prepares, so q and work are required and y may be NULL
    assert lib.sp_prox_prepare(d, PTR, 3, None, None) == EINVAL
    assert lib.sp_prox_prepare(d, None, 3, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, None, 3, 1, 0.5, PTR, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, 0.5, PTR, None, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, 0.0, PTR, PTR, None) == EINVAL
    assert lib.sp_op_prox_ws(d, PTR, None, PTR, 3, 1, float("nan"), PTR, PTR, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, None, None, 0, 0, 0, 3, 1, pc, PTR, PTR, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, pc, PTR, None, None) == EINVAL
    assert lib.sp_diffpir_step_ws(d, PTR, PTR, None, PTR, None, 0, 0, 0, 3, 1, None, PTR, PTR, None) == EINVAL
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
    a8, a6 = np.eye(8), np.eye(6)
    rules = [
        (dict(x_shape=(8, 8), A_h=a8, A_w=a8), "x_shape must be"),
        (dict(x_shape=(1, 1, 8), A_h=np.eye(1), A_w=a8), r"H and W must be in \[2, 512\]"),
        (dict(x_shape=(1, 8, 513), A_h=a8, A_w=np.eye(513)), r"H and W must be in \[2, 512\]"),
        (dict(x_shape=(0, 8, 8), A_h=a8, A_w=a8), "C positive"),
        (dict(x_shape=(1, 8, 8), A_h=a6, A_w=a8), "A_h must be a 2-D matrix with 8 columns"),
        (dict(x_shape=(1, 8, 8), A_h=a8, A_w=np.ones(8)), "A_w must be a 2-D matrix with 8 columns"),
        (dict(x_shape=(1, 8, 8), A_h=np.ones((9, 8)), A_w=a8), "A_h must have between 1 and 8 rows"),
        (dict(x_shape=(1, 8, 8), A_h=np.ones((0, 8)), A_w=a8), "A_h must have between 1 and 8 rows"),
        (dict(x_shape=(1, 8, 8), A_h=np.full((8, 8), float("nan")), A_w=a8), "A_h must be finite"),
        (dict(x_shape=(1, 8, 8), A_h=a8, A_w=np.full((8, 8), float("inf"))), "A_w must be finite"),
        (dict(x_shape=(1, 8, 8), A_h=a8 * 0, A_w=a8), "non-zero"),
        (dict(x_shape=(1, 8, 8), A_h=a8, A_w=a8, rtol=0.0), "rtol must be in"),
        (dict(x_shape=(1, 8, 8), A_h=a8, A_w=a8, rtol=1.0), "rtol must be in"),
    ]
    for kwargs, text in rules:
        with pytest.raises(ValueError, match=text):
            SeparableSVDOperator(**kwargs)
    for call, text in ((lambda: SeparableSVDOperator.gaussian_blur((1, 8, 8), 8), "kernel_size must be odd"),
                       (lambda: SeparableSVDOperator.gaussian_blur((1, 8, 8), 9, -1.0), "sigma must be positive"),
                       (lambda: SeparableSVDOperator.gaussian_blur((1, 8, 8), 9), "longer than 2R"),
                       (lambda: SeparableSVDOperator.uniform_blur((1, 8, 8), 4), "kernel_size must be odd"),
                       (lambda: SeparableSVDOperator.from_taps((1, 8, 8), [1.0, 2.0], [1.0]), "must be odd"),
                       (lambda: SeparableSVDOperator.from_taps((1, 8, 8), [[1.0]], [1.0]), "taps must be 1-D"),
                       (lambda: SeparableSVDOperator.bicubic_sr((1, 8, 8), 3), "factor must be one of"),
                       (lambda: SeparableSVDOperator.filtered_sr((1, 12, 8), np.ones(8), 8), "must divide"),
                       (lambda: SeparableSVDOperator.filtered_sr((1, 8, 8), np.ones(5), 2), "K − s even")):
        with pytest.raises(ValueError, match=text):
            call()
    SeparableSVDOperator((1, 2, 2), np.ones((1, 2)), np.ones((1, 2)))   # a 1 x 1 observation
    SeparableSVDOperator.uniform_blur((1, 512, 9), 3)


def test_descriptor_and_interface(lib):
    op = SeparableSVDOperator.bicubic_sr((2, 24, 16), 4, rtol=0.7)
    assert isinstance(op, SVDOperator) and op.pinv_grad_scale == 2.0 and not op.hip_linear
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width, d.radius, d.factor) == (KIND, 2, 24, 16, 6, 4)
    assert d.n == 2 * 24 * 16 and d.m == 2 * 6 * 4 and d.taps == op.tables.data_ptr()
    assert not d.keep_bits and not d.word_rank and lib.sp_rsq_partials(d) == 2
    assert op.tables.dtype == torch.float32 and op.tables.numel() == 24 * 24 + 16 * 16 + 36 + 16 + 2 * 24
    assert op.shape == (48, 768) and tuple(op.y_shape) == (2, 6, 4)
    s, sk = op.singular_values_full, op.get_singular_values()
    assert tuple(s.shape) == (6, 4) and bool((s > 0).all()) and bool((sk[~op.keep] == 0).all())
    assert 0 < int(op.keep.sum()) < op.keep.numel() and torch.equal(sk[op.keep], s[op.keep])
    assert bool((s.reshape(-1)[:-1] >= 0).all()) and float(s[0, 0]) == float(s.max())
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 2, 24, 16, generator=g, dtype=torch.float64)
    y = torch.randn(3, 2, 6, 4, generator=g, dtype=torch.float64)
    t = sr.Tables.from_flat(op.tables, 24, 16, 6, 4)
    S = sr.Sep(t)
    for got, want in ((op.apply(x), S.apply(x)), (op.apply_transpose(y), S.adjoint(y)),
                      (op.apply_pseudo_inverse(y), S.pinv(y)), (op.apply_pseudo_inverse_transpose(x), S.pinv_t(x)),
                      (op.apply_prox(x, y, 0.3), S.prox(x, y, 0.3)), (op.apply_V_transpose(x), S.T(x)),
                      (op.apply_V(y), S.Tinv(y)), (op.apply_U_transpose(y), S.Ty(y)), (op.apply_U(y), S.Tyinv(y))):
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert op.apply(x.float()).dtype == torch.float32 and tuple(op.apply(x[0]).shape) == (2, 6, 4)
    z, iters = op.apply_prox_cg(x, y, 0.3, iterations=200, tol=1e-12, return_iterations=True)
    # the closed form takes the rounded fp32 tables as orthogonal; they are so to 1e-7, which is
    # how far the converged iteration on the same tables lies from it
    assert float((z - S.prox(x, y, 0.3)).abs().max()) <= 2e-6 and int(iters.min()) >= 1
    from samplers_amd.samplers.ddrm import SUPPORTED, ddrm_descriptor
    from samplers_amd.samplers.diffpir import cg_descriptor, prox_descriptor
    assert "SeparableSVDOperator" in SUPPORTED
    assert ddrm_descriptor(op).kind == prox_descriptor(op).kind == cg_descriptor(op).kind == KIND


def _host_problem():
    shape, sigma = (1, 12, 10), 0.1
    op = SeparableSVDOperator.from_taps(shape, sr._gauss(3, 0.8), sr._gauss(5, 1.2))
    t = sr.Tables.from_flat(op.tables, 12, 10, 12, 10)
    y = torch.randn(2, *shape, generator=torch.Generator().manual_seed(4))
    return shape, sigma, op, t, y


@pytest.mark.parametrize("recon", [1, 2])
def test_host_ddrm_sampler_is_the_plain_loop(recon):
    shape, sigma, op, t, y = _host_problem()
    assert 0.1 <= t.kept_share() <= 0.9
    host_ddrm_check(op, sr.Sep(t), y, shape, sigma, recon)
    host_refusals(op, y, shape, sigma)


@pytest.mark.parametrize("recon", [1, 2])
def test_host_pgdm_sampler_is_the_plain_loop(recon):
    shape, sigma, op, t, y = _host_problem()
    host_pgdm_check(op, lambda dt: sr.Sep(t, dtype=dt), y, shape, sigma, recon)


def _cg_sep(t, dt):
    """Sep whose data step is the plain CGLS recurrence (K = 16, tol 1e-4) on the dense matrix."""
    import prox_cg_ref as cg

    S, A = sr.Sep(t, dtype=dt), torch.from_numpy(sr.Dense(t).A)

    def prox(x0, yy, rho):
        z, _ = cg.cgls(A, x0.reshape(len(x0), -1), yy.reshape(len(x0), -1), rho, 16, 1e-4, dtype=dt)
        return z.reshape(x0.shape)

    S.prox = prox
    return S


@pytest.mark.parametrize("prox", ["cg", "closed_form"])
def test_host_diffpir_sampler_is_the_plain_loop(prox):
    shape, sigma, op, t, y = _host_problem()
    make_S = (lambda dt: _cg_sep(t, dt)) if prox == "cg" else (lambda dt: sr.Sep(t, dtype=dt))
    host_diffpir_check(op, make_S, y, shape, sigma, prox, tol=1e-4)
