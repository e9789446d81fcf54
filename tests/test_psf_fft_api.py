"""FFTPSFBlurOperator on the host, the fp64 helper tests/psf_fft_ops.py itself, the spectrum layout
and the library's SP_OP_PSF_FFT descriptor rules (no GPU: every library call here returns before a
launch)."""

import ctypes

import numpy as np
import pytest
import torch

import psf_fft_ops
import psf_ops
from samplers_amd import _hip
from samplers_amd import operators
from samplers_amd.operators import (FFTPSFBlurOperator, LinearOperator, PSFBlurOperator, padded_size,
                                    psf_spectrum)

PADDINGS = psf_fft_ops.PADDINGS
# shape, radius: the GPU suite's shapes up to the size the direct fp64 route does in a moment
CASES = [((1, 3, 3), 1), ((2, 7, 10), 3), ((1, 5, 9), 4), ((3, 16, 16), 8), ((1, 40, 72), 31),
         ((3, 64, 64), 16), ((1, 96, 160), 30)]
TOL = 2e-5

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def _close(got, ref):
    ref = ref.numpy()
    np.testing.assert_allclose(got.double().numpy(), ref, rtol=0, atol=TOL * np.abs(ref).max())


def _kernels(r):
    g = torch.Generator().manual_seed(100 + r)
    return psf_ops.random_sparse_kernel(r, seed=r), torch.randn(2 * r + 1, 2 * r + 1, generator=g)


def test_exported():
    for name in ("FFTPSFBlurOperator", "padded_size", "psf_spectrum"):
        assert name in operators.__all__
    assert issubclass(FFTPSFBlurOperator, LinearOperator)
    assert not issubclass(FFTPSFBlurOperator, PSFBlurOperator)
    assert FFTPSFBlurOperator.hip_linear is False
    assert _hip.SP_OP_PSF_FFT == 7


def test_padded_size_rule():
    """The smallest 2^k or 3 * 2^k in [8, 1024] that holds the extended axis."""
    valid = sorted({2 ** k for k in range(3, 11)} | {3 * 2 ** k for k in range(2, 9)})
    assert valid[0] == 8 and valid[-1] == 1024
    for n in list(range(1, 60)) + [96, 97, 128, 129, 316, 384, 385, 768, 769, 1022, 1024]:
        assert padded_size(n) == min(v for v in valid if v >= n), n
    for n, want in ((5, 8), (13, 16), (16, 16), (17, 24), (102, 128), (136, 192), (316, 384),
                    (768, 768), (1022, 1024)):
        assert padded_size(n) == want
    with pytest.raises(ValueError, match="1024"):
        padded_size(1025)


# --- the helper ---------------------------------------------------------------------------------

@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("shape,r", CASES)
def test_helper_fft_route_is_the_direct_route(shape, r, padding):
    g = torch.Generator().manual_seed(1)
    x, y = (torch.randn(2, *shape, generator=g, dtype=torch.float64) for _ in range(2))
    for h in _kernels(r):
        bound = 1e-10 * float(h.double().abs().sum())
        d = psf_fft_ops.apply64(x, h, padding)
        f = psf_fft_ops.apply64(x, h, padding, route="fft")
        assert float((d - f).abs().max()) <= bound * float(x.abs().max())
        da = psf_fft_ops.adjoint64(y, h, padding)
        fa = psf_fft_ops.adjoint64(y, h, padding, route="fft")
        assert float((da - fa).abs().max()) <= 3 * bound * float(y.abs().max())  # <= 3 fold terms


@pytest.mark.parametrize("shape,r", [((2, 7, 10), 3), ((3, 32, 40), 15), ((1, 61, 61), 30)])
def test_helper_reflect_is_the_psf_helper(shape, r):
    g = torch.Generator().manual_seed(2)
    x, y = (torch.randn(2, *shape, generator=g, dtype=torch.float64) for _ in range(2))
    h = psf_ops.random_sparse_kernel(r, seed=r)
    assert torch.equal(psf_fft_ops.blur(x, h, "reflect"), psf_ops.blur(x, h))
    assert torch.equal(psf_fft_ops.adjoint(y, h, "reflect"), psf_ops.adjoint(y, h))


@pytest.mark.parametrize("padding", PADDINGS)
def test_helper_delta_psf_shifts_by_the_index_rule(padding):
    shape, r = (2, 6, 9), 4
    x = torch.randn(3, *shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for dy, dx in ((0, 0), (-4, 4), (4, -4), (3, 0), (0, -2), (-1, -3), (4, 4)):
        h = torch.zeros(2 * r + 1, 2 * r + 1)
        h[r + dy, r + dx] = 1.0
        want = psf_fft_ops.shifted(x, dy, dx, padding)
        assert torch.equal(psf_fft_ops.blur(x, h, padding), want), (dy, dx)
        if padding == "reflect":
            assert torch.equal(want, psf_ops.shifted(x, dy, dx))
    # the rule itself, spelled out on one row: x~[i + d]
    row = torch.arange(5.0).reshape(1, 1, 5)
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, 2, "reflect")[0, 0].tolist() == [2, 3, 4, 3, 2]
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, 2, "circular")[0, 0].tolist() == [2, 3, 4, 0, 1]
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, 2, "zeros")[0, 0].tolist() == [2, 3, 4, 0, 0]
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, -2, "reflect")[0, 0].tolist() == [2, 1, 0, 1, 2]
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, -2, "circular")[0, 0].tolist() == [3, 4, 0, 1, 2]
    assert psf_fft_ops.shifted(row.expand(1, 5, 5), 0, -2, "zeros")[0, 0].tolist() == [0, 0, 0, 1, 2]


# --- the operator on host tensors ---------------------------------------------------------------

@pytest.mark.parametrize("padding", PADDINGS)
@pytest.mark.parametrize("shape,r", CASES[:6])
def test_host_maps_match_the_fp64_helper(shape, r, padding):
    for h in _kernels(r):
        op = FFTPSFBlurOperator(shape, h, padding=padding)
        assert op.x_shape == shape and op.y_shape == shape and op.radius == r
        assert op.padding == padding and op.kernel_size == 2 * r + 1
        assert op.kernel.dtype == torch.float32 and torch.equal(op.kernel, h)
        assert op.padded_shape == (padded_size(shape[1] + 2 * r), padded_size(shape[2] + 2 * r))
        g = torch.Generator().manual_seed(0)
        x, y = (torch.randn(2, *shape, generator=g) for _ in range(2))
        _close(op.apply(x), psf_fft_ops.apply64(x, h, padding))
        _close(op.apply_transpose(y), psf_fft_ops.adjoint64(y, h, padding))
        assert torch.equal(op(x), op.apply(x))
        two = op.apply(x.reshape(2, 1, *shape))  # leading batch dimensions are kept
        assert tuple(two.shape) == (2, 1, *shape) and torch.equal(two.reshape(x.shape), op.apply(x))
        # <A x, y> = <x, A^T y> in fp64
        x64, y64 = x.double(), y.double()
        lhs = float((op.apply(x64) * y64).sum())
        rhs = float((x64 * op.apply_transpose(y64)).sum())
        scale = float(op.apply(x64).norm() * y64.norm())
        assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_default_padding_is_reflect_and_equals_the_direct_operator():
    shape, r = (2, 17, 19), 8
    h = psf_ops.random_sparse_kernel(r, seed=r)
    op, direct = FFTPSFBlurOperator(shape, h), PSFBlurOperator(shape, h)
    assert op.padding == "reflect"
    x = torch.randn(2, *shape, generator=torch.Generator().manual_seed(5))
    assert torch.equal(op.apply(x), direct.apply(x))
    assert torch.equal(op.apply_transpose(x), direct.apply_transpose(x))


def test_rectangular_kernel_is_centred_in_a_square():
    g = torch.Generator().manual_seed(3)
    k = torch.randn(3, 7, generator=g)  # negative taps allowed, no normalisation imposed
    op = FFTPSFBlurOperator((2, 9, 11), k.numpy(), padding="circular")  # an array is accepted
    assert op.kernel_size == 7 and op.radius == 3
    sq = torch.zeros(7, 7)
    sq[2:5, :] = k
    assert torch.equal(op.kernel, sq)
    x, y = (torch.randn(2, 2, 9, 11, generator=g) for _ in range(2))
    _close(op.apply(x), psf_fft_ops.apply64(x, sq, "circular"))
    _close(op.apply_transpose(y), psf_fft_ops.adjoint64(y, sq, "circular"))
    tall = FFTPSFBlurOperator((1, 9, 11), k.T.contiguous(), padding="zeros")
    assert torch.equal(tall.kernel, sq.T)


def test_radius_beyond_the_direct_operators_cap():
    shape, r = (1, 40, 72), 31
    h = psf_ops.random_sparse_kernel(r, seed=1)
    with pytest.raises(ValueError):
        PSFBlurOperator(shape, h)
    op = FFTPSFBlurOperator(shape, h)
    assert op.radius == 31 and op.padded_shape == (128, 192)
    big = FFTPSFBlurOperator.gaussian((1, 128, 128), kernel_size=129, sigma=20.0, padding="zeros")
    assert big.radius == 64 and big.padded_shape == (256, 256)
    assert abs(float(big.kernel.double().sum()) - 1.0) < 1e-5
    small = FFTPSFBlurOperator.gaussian((3, 32, 32), 9, 1.5)
    assert torch.equal(small.kernel, PSFBlurOperator.gaussian((3, 32, 32), 9, 1.5).kernel)


def test_rejected_arguments():
    k3 = torch.ones(3, 3)
    with pytest.raises(ValueError, match="radius"):       # R >= min(H, W)
        FFTPSFBlurOperator((1, 4, 9), torch.ones(9, 9))
    FFTPSFBlurOperator((1, 5, 9), torch.ones(9, 9))       # R = min(H, W) - 1
    with pytest.raises(ValueError, match="1024"):         # H + 2R > 1024
        FFTPSFBlurOperator((1, 1023, 8), k3)
    with pytest.raises(ValueError, match="1024"):         # W + 2R > 1024
        FFTPSFBlurOperator((1, 64, 1000), torch.ones(27, 27))
    FFTPSFBlurOperator((1, 1022, 8), k3)                  # 1024 exactly
    for bad in (torch.ones(4, 4), torch.ones(3, 4), torch.ones(2, 3)):  # even sizes
        with pytest.raises(ValueError, match="odd"):
            FFTPSFBlurOperator((1, 16, 16), bad)
    with pytest.raises(ValueError):                       # a 1 x 1 kernel has R = 0
        FFTPSFBlurOperator((1, 16, 16), torch.ones(1, 1))
    for val in (float("nan"), float("inf")):
        k = k3.clone()
        k[1, 2] = val
        with pytest.raises(ValueError, match="finite"):
            FFTPSFBlurOperator((1, 16, 16), k)
    with pytest.raises(ValueError, match="padding"):
        FFTPSFBlurOperator((1, 16, 16), k3, padding="replicate")
    with pytest.raises(ValueError):
        FFTPSFBlurOperator((16, 16), k3)
    with pytest.raises(ValueError):
        FFTPSFBlurOperator((1, 16, 16), torch.ones(3, 3, 3))
    with pytest.raises(ValueError):
        FFTPSFBlurOperator.gaussian((1, 16, 16), 4, 1.0)
    with pytest.raises(ValueError):
        FFTPSFBlurOperator.gaussian((1, 16, 16), 5, 0.0)


def test_pgdm_rejects_the_operator():
    op = FFTPSFBlurOperator((1, 8, 8), torch.ones(3, 3))
    with pytest.raises(NotImplementedError):
        op.apply_pseudo_inverse(torch.zeros(1, 1, 8, 8))


# --- the spectrum -------------------------------------------------------------------------------

@pytest.mark.parametrize("r,Nh,Nw", [(1, 8, 8), (3, 16, 24), (4, 24, 16), (15, 96, 48)])
def test_psf_spectrum_layout(r, Nh, Nw):
    h = _kernels(r)[1]
    spec = psf_spectrum(h, Nh, Nw)
    assert spec.dtype == torch.float32 and tuple(spec.shape) == (Nw // 2 + 1, Nh, 2)
    assert spec.is_contiguous()
    full = np.zeros((Nh, Nw))
    full[: 2 * r + 1, : 2 * r + 1] = h.double().numpy()
    ref = np.fft.fft2(full)  # [kh][kw], unnormalised
    want = ref[:, : Nw // 2 + 1].T  # [kw][kh], kw <= Nw / 2
    got = spec[..., 0].double().numpy() + 1j * spec[..., 1].double().numpy()
    assert np.abs(got - want).max() <= 1e-6 * np.abs(ref).max()  # fp32 rounding of fp64 values
    # each value is the fp64 one rounded to fp32 (2^-24 relative), not an fp32 transform's
    assert (np.abs(got - want) <= 6e-8 * np.abs(want) + 1e-13 * np.abs(ref).max()).all()
    assert abs(got[0, 0] - float(h.double().sum())) <= 1e-6 * np.abs(ref).max()  # DC = sum of taps
    with pytest.raises(ValueError):
        psf_spectrum(h, 2 * r, Nw)


def test_operator_keeps_the_spectrum_as_a_buffer():
    h = _kernels(3)[0]
    op = FFTPSFBlurOperator((2, 7, 10), h, padding="zeros")
    assert "spectrum" in dict(op.named_buffers()) and "kernel" in dict(op.named_buffers())
    assert torch.equal(op.spectrum, psf_spectrum(h, 16, 16))
    d = op.hip_descriptor()
    assert (d.kind, d.channels, d.height, d.width, d.n, d.m) == (7, 2, 7, 10, 140, 140)
    assert (d.radius, d.factor, d.taps) == (3, 2, op.spectrum.data_ptr())
    assert not d.keep_bits and not d.word_rank


# --- the library without a GPU ------------------------------------------------------------------

def make(c=1, h=8, w=8, r=1, factor=0, taps=PTR, n=None, m=None, keep=None, rank=None):
    d = _hip.SpOp()
    d.kind = _hip.SP_OP_PSF_FFT
    d.channels, d.height, d.width = c, h, w
    d.n = c * h * w if n is None else n
    d.m = c * h * w if m is None else m
    d.radius, d.factor, d.taps, d.keep_bits, d.word_rank = r, factor, taps, keep, rank
    return d


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def _lines(N):
    """Lines of an N-point transform per workgroup (csrc/sp_fft.h: 32000 bytes of LDS, <= 16)."""
    NP = (N + N // 16) | 1
    return max(1, min(16, (32000 - 8 * N) // (16 * NP)))


@pytest.mark.parametrize("c,h,w,r", [(1, 8, 8, 1), (2, 7, 10, 3), (1, 40, 72, 31), (3, 64, 64, 16),
                                     (1, 256, 256, 30), (1, 512, 512, 255), (3, 3, 3, 1)])
def test_counts(lib, c, h, w, r):
    d = make(c, h, w, r)
    Nh, Nw = padded_size(h + 2 * r), padded_size(w + 2 * r)
    partials = c * -(-h // _lines(Nw))       # C * ceil(H / row lines)
    floats = 2 * 3 * c * (Nw // 2 + 1) * h   # 2 * batch * C * (Nw / 2 + 1) * H
    assert lib.sp_rsq_partials(d) == partials > 0
    assert lib.sp_dps_workspace(d, 3) == lib.sp_op_workspace(d, 3) == floats > 0
    assert lib.sp_dps_workspace(d, 0) == EINVAL and lib.sp_op_workspace(d, 0) == EINVAL


def test_traits(lib):
    bits = (_hip.SP_TRAIT_UPDATE_READS_V, _hip.SP_TRAIT_DPS_WORKSPACE, _hip.SP_TRAIT_FUSED_LATENT,
            _hip.SP_TRAIT_LINEAR, _hip.SP_TRAIT_NEEDS_ATA_U)
    for factor in (0, 1, 2):
        t = lib.sp_op_traits(make(factor=factor))
        assert tuple(int(bool(t & b)) for b in bits) == (1, 1, 0, 0, 0)
        assert t & ~sum(bits) == 0
    assert lib.sp_op_traits(make(factor=3)) == 0


def _entry_calls(lib, d, work=PTR):
    c, a = _hip.SpDpsCoefs(), _hip.SpAdamWCoefs()
    return {
        "sp_dps_residual": lambda: lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None),
        "sp_dps_residual_ws": lambda: lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR,
                                                            work, None),
        "sp_dps_residual_sched": lambda: lib.sp_dps_residual_sched(d, PTR, PTR, PTR, 3, 1, PTR, PTR,
                                                                  PTR, PTR, None),
        "sp_dps_residual_sched_ws": lambda: lib.sp_dps_residual_sched_ws(d, PTR, PTR, PTR, 3, 1, PTR,
                                                                        PTR, PTR, PTR, work, None),
        "sp_op_apply": lambda: lib.sp_op_apply(d, PTR, PTR, 3, None),
        "sp_op_adjoint": lambda: lib.sp_op_adjoint(d, PTR, PTR, 3, None),
        "sp_op_apply_ws": lambda: lib.sp_op_apply_ws(d, PTR, PTR, 3, work, None),
        "sp_op_vjp_ws": lambda: lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, work, None),
        "sp_psld_pixel": lambda: lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None),
        "sp_psld_cotangent": lambda: lib.sp_psld_cotangent(d, PTR, PTR, PTR, PTR, 0.1, 3, PTR, None),
        "sp_pixel_opt_step": lambda: lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 3, 1, 1.0, a,
                                                          None, PTR, None),
    }


def test_unsupported_entries(lib):
    calls = _entry_calls(lib, make())
    for name in ("sp_op_apply", "sp_op_adjoint", "sp_dps_residual", "sp_dps_residual_sched",
                 "sp_psld_pixel", "sp_psld_cotangent", "sp_pixel_opt_step"):
        assert calls[name]() == EUNSUPPORTED, name


def test_the_ws_forms_need_work(lib):
    calls = _entry_calls(lib, make(), work=None)
    for name in ("sp_dps_residual_ws", "sp_dps_residual_sched_ws", "sp_op_apply_ws", "sp_op_vjp_ws"):
        assert calls[name]() == EINVAL, name
    # without a work argument the entry does not serve the kind at all
    assert calls["sp_dps_residual"]() == EUNSUPPORTED
    assert calls["sp_dps_residual_sched"]() == EUNSUPPORTED
    # pass 2 is the identity-kind update over v: v is required
    c = _hip.SpDpsCoefs()
    assert lib.sp_dps_update(make(), PTR, PTR, PTR, None, PTR, PTR, None, 0, 0, 0, 3, 1, c, PTR,
                             None) == EINVAL


GEOMETRY_VIOLATIONS = {
    "factor 3": make(factor=3),
    "factor -1": make(factor=-1),
    "taps NULL": make(taps=None),
    "R = 0": make(r=0),
    "R = min(H, W)": make(1, 5, 9, 5),
    "R = min(H, W), wide": make(1, 9, 5, 5),
    "H + 2R = 1025": make(1, 1023, 8, 1),
    "W + 2R = 1025": make(1, 8, 1023, 1),
    "m != n": make(m=63),
    "n != C H W": make(n=65, m=65),
    "keep_bits set": make(keep=PTR),
    "word_rank set": make(rank=PTR),
    "no channels": make(0, 8, 8, 1, n=64, m=64),
}


@pytest.mark.parametrize("what", list(GEOMETRY_VIOLATIONS))
def test_rejected_descriptor_is_einval_everywhere(lib, what):
    d = GEOMETRY_VIOLATIONS[what]
    assert lib.sp_rsq_partials(d) == EINVAL
    assert lib.sp_dps_workspace(d, 3) == EINVAL and lib.sp_op_workspace(d, 3) == EINVAL
    assert lib.sp_op_traits(d) == 0
    for name, call in _entry_calls(lib, d).items():
        assert call() == EINVAL, name


def test_accepted_geometries(lib):
    for d in (make(1, 40, 72, 31), make(1, 5, 9, 4), make(1, 1022, 8, 1), make(1, 8, 1022, 1),
              make(1, 512, 512, 255), make(1, 512, 512, 256), make(1, 2, 2, 1), make(3, 3, 3, 1, 2)):
        assert lib.sp_rsq_partials(d) > 0, (d.height, d.width, d.radius)
