"""PSFBlurOperator / MotionBlurOperator on the host and the library's SP_OP_PSF descriptor rules
(no GPU).  The semantics are those of tests/psf_ops.py (fp64)."""

import numpy as np
import pytest
import torch

import psf_ops
from samplers_amd import _hip
from samplers_amd import operators
from samplers_amd.operators import (GaussianBlurOperator, LinearOperator, MotionBlurOperator,
                                    PSFBlurOperator, motion_blur_kernel)

# shape, radius
CASES = [((1, 3, 3), 1), ((2, 7, 10), 2), ((1, 8, 12), 3), ((3, 32, 32), 4), ((2, 17, 19), 8),
         ((3, 32, 40), 15), ((1, 61, 61), 30)]
TOL = 2e-5


def _close(got, ref):
    ref = ref.numpy()
    np.testing.assert_allclose(got.double().numpy(), ref, rtol=0, atol=TOL * np.abs(ref).max())


def test_exported():
    for name in ("PSFBlurOperator", "MotionBlurOperator", "motion_blur_kernel"):
        assert name in operators.__all__
    assert issubclass(PSFBlurOperator, LinearOperator)
    assert issubclass(MotionBlurOperator, PSFBlurOperator)


@pytest.mark.parametrize("shape,r", CASES)
def test_host_maps_match_the_fp64_helper(shape, r):
    h = psf_ops.random_sparse_kernel(r, seed=r)
    assert not torch.equal(h, h.T) and not torch.equal(h, h.flip(0, 1))  # asymmetric
    op = PSFBlurOperator(shape, h)
    assert op.x_shape == shape and op.y_shape == shape and op.radius == r
    assert op.kernel.dtype == torch.float32 and torch.equal(op.kernel, h)
    g = torch.Generator().manual_seed(0)
    x, y = (torch.randn(2, *shape, generator=g) for _ in range(2))
    _close(op.apply(x), psf_ops.apply64(x, h))
    _close(op.apply_transpose(y), psf_ops.adjoint64(y, h))
    assert torch.equal(op(x), op.apply(x))
    two = op.apply(x.reshape(2, 1, *shape))  # leading batch dimensions are kept
    assert tuple(two.shape) == (2, 1, *shape) and torch.equal(two.reshape(x.shape), op.apply(x))


def test_rectangular_kernel_is_centred_in_a_square():
    g = torch.Generator().manual_seed(3)
    k = torch.randn(3, 7, generator=g)  # negative taps allowed, no normalisation imposed
    op = PSFBlurOperator((2, 9, 11), k.numpy())  # an array is accepted as a tensor is
    assert op.kernel_size == 7 and op.radius == 3
    sq = torch.zeros(7, 7)
    sq[2:5, :] = k
    assert torch.equal(op.kernel, sq)
    x, y = (torch.randn(2, 2, 9, 11, generator=g) for _ in range(2))
    _close(op.apply(x), psf_ops.apply64(x, sq))
    _close(op.apply_transpose(y), psf_ops.adjoint64(y, sq))
    tall = PSFBlurOperator((1, 9, 11), k.T.contiguous())
    assert torch.equal(tall.kernel, sq.T)


@pytest.mark.parametrize("shape,r", CASES)
def test_helper_dot_product_identity_in_fp64(shape, r):
    """<A x, y> = <x, A^T y> on the helper; H = 2R + 1 folds both borders onto a pixel."""
    h = psf_ops.random_sparse_kernel(r, seed=10 + r)
    g = torch.Generator().manual_seed(1)
    x, y = (torch.randn(2, *shape, dtype=torch.float64, generator=g) for _ in range(2))
    lhs = (psf_ops.apply64(x, h) * y).sum()
    rhs = (x * psf_ops.adjoint64(y, h)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * max(1.0, abs(float(lhs)))


def test_helper_adjoint_is_the_issue_gather_formula():
    """The fold sets M_H / M_W written out, against the helper's autograd adjoint."""
    (c, hh, ww), r = (1, 7, 9), 3  # H = 2R + 1: folds from both borders on the rows
    h = psf_ops.random_sparse_kernel(r, seed=5).double()
    y = torch.randn(c, hh, ww, dtype=torch.float64, generator=torch.Generator().manual_seed(2))

    def m_set(j, n):
        s = [j]
        if 1 <= j <= r:
            s.append(-j)
        if n - 1 - r <= j <= n - 2:
            s.append(2 * (n - 1) - j)
        return s

    def r0(i, j):
        return float(y[0, i, j]) if 0 <= i < hh and 0 <= j < ww else 0.0

    ref = torch.zeros(hh, ww, dtype=torch.float64)
    for jy in range(hh):
        for jx in range(ww):
            ref[jy, jx] = sum(float(h[u, v]) * r0(py - (u - r), px - (v - r))
                              for py in m_set(jy, hh) for px in m_set(jx, ww)
                              for u in range(2 * r + 1) for v in range(2 * r + 1))
    torch.testing.assert_close(psf_ops.adjoint64(y, h)[0], ref, rtol=0, atol=1e-13)


def test_fft_route_of_the_helper_is_the_direct_route():
    shape, r = (2, 70, 66), 30
    h = psf_ops.random_sparse_kernel(r, seed=7)
    g = torch.Generator().manual_seed(4)
    x, y = (torch.randn(2, *shape, generator=g) for _ in range(2))
    for fn in (psf_ops.apply64, psf_ops.adjoint64):
        direct = fn(x if fn is psf_ops.apply64 else y, h)
        fft = fn(x if fn is psf_ops.apply64 else y, h, route="fft")
        assert float((fft - direct).abs().max()) <= 1e-12 * float(direct.abs().max())
    a_d, t_d = psf_ops.psf_ops(shape, h)
    a_f, t_f = psf_ops.psf_ops(shape, h, route="fft")
    xf = x.reshape(2, -1).double().numpy()
    np.testing.assert_allclose(a_f(xf), a_d(xf), rtol=0, atol=1e-12)
    np.testing.assert_allclose(t_f(xf), t_d(xf), rtol=0, atol=1e-12)


def test_delta_kernels_are_exact():
    shape, r = (2, 9, 11), 3
    x = torch.randn(2, *shape, generator=torch.Generator().manual_seed(5))
    centre = torch.zeros(7, 7)
    centre[r, r] = 1.0
    assert torch.equal(PSFBlurOperator(shape, centre).apply(x), x)
    for u, v in ((0, 6), (5, 1), (3, 0), (6, 6)):
        d = torch.zeros(7, 7)
        d[u, v] = 1.0  # correlation: y[i, j] = x~[i + u - R, j + v - R]
        assert torch.equal(PSFBlurOperator(shape, d).apply(x), psf_ops.shifted(x, u - r, v - r))


def test_gaussian_outer_product_matches_the_separable_operator():
    shape = (3, 32, 32)
    op, sep = PSFBlurOperator.gaussian(shape, 9, 3.0), GaussianBlurOperator(shape, 9, 3.0)
    assert op.radius == 4 and abs(float(op.kernel.sum()) - 1.0) < 1e-6
    g = torch.Generator().manual_seed(6)
    x, y = (torch.randn(2, *shape, generator=g) for _ in range(2))
    _close(op.apply(x), sep.apply(x).double())
    _close(op.apply_transpose(y), sep.apply_transpose(y).double())
    paper = PSFBlurOperator.gaussian((3, 64, 64), 61, 3.0)  # the DPS paper's 61 x 61, sigma 3
    assert paper.radius == 30 and tuple(paper.kernel.shape) == (61, 61)


@pytest.mark.parametrize("shape,kernel", [
    ((3, 32, 32), torch.ones(4, 5)),          # an even size
    ((3, 32, 32), torch.ones(5, 4)),
    ((3, 128, 128), torch.ones(63, 63)),      # above 61
    ((3, 32, 32), torch.ones(1, 1)),          # below 3
    ((3, 32, 32), torch.ones(5)),             # not 2-D
    ((3, 32, 32), torch.tensor([[1.0, 2, 3], [4, float("nan"), 6], [7, 8, 9]])),
    ((3, 32, 32), torch.tensor([[1.0, 2, 3], [4, float("inf"), 6], [7, 8, 9]])),
    ((3, 6, 32), torch.ones(7, 7)),           # H <= 2R
    ((3, 32, 6), torch.ones(3, 7)),           # W <= 2R of the squared kernel
    ((32, 32), torch.ones(3, 3)),             # x_shape not (C, H, W)
])
def test_bad_arguments_raise(shape, kernel):
    with pytest.raises(ValueError):
        PSFBlurOperator(shape, kernel)


def test_descriptor_fields():
    h = psf_ops.random_sparse_kernel(15, seed=1)
    op = PSFBlurOperator((3, 32, 40), h)
    d = op.hip_descriptor()
    assert _hip.SP_OP_PSF == 5
    assert (d.kind, d.channels, d.height, d.width) == (_hip.SP_OP_PSF, 3, 32, 40)
    assert d.n == d.m == 3 * 32 * 40 and d.radius == 15 and d.factor == 0
    assert d.taps == op.kernel.data_ptr() and not d.keep_bits and not d.word_rank
    op.kernel = op.kernel.clone()  # the pointer is read at call time (e.g. after .to(device))
    assert op.hip_descriptor().taps == op.kernel.data_ptr()


def test_library_accepts_only_valid_psf_descriptors():
    lib = _hip.load_library()
    assert lib.sp_version() > 102
    ops = [PSFBlurOperator(shape, psf_ops.random_sparse_kernel(r, seed=r)) for shape, r in CASES]
    for op in ops:
        assert lib.sp_rsq_partials(op.hip_descriptor()) > 0
    big = PSFBlurOperator((3, 256, 256), psf_ops.random_sparse_kernel(30, seed=0))
    assert lib.sp_rsq_partials(big.hip_descriptor()) == 3 * 8 * 4  # 32 x 64 tiles

    base = PSFBlurOperator((3, 32, 32), psf_ops.random_sparse_kernel(4, seed=0))

    def rejected(**fields):
        d = base.hip_descriptor()
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.sp_rsq_partials(d), lib.sp_dps_workspace(d, 2)

    assert rejected()[0] > 0
    assert rejected(radius=0) == (-1, -1)
    assert rejected(radius=31) == (-1, -1)
    assert rejected(taps=None) == (-1, -1)
    assert rejected(radius=16) == (-1, -1)                          # 32 <= 2R
    assert rejected(height=8, n=3 * 8 * 32, m=3 * 8 * 32) == (-1, -1)  # H <= 2R
    assert rejected(width=8, n=3 * 32 * 8, m=3 * 32 * 8) == (-1, -1)   # W <= 2R
    assert rejected(m=3 * 32 * 32 - 1) == (-1, -1)                  # m != n
    assert rejected(n=3 * 32 * 32 + 4, m=3 * 32 * 32 + 4) == (-1, -1)  # C * H * W != n


def test_dps_workspace_sizes():
    from samplers_amd.operators import (IdentityOperator, RandomInpaintingOperator,
                                        SuperResolutionOperator)

    lib = _hip.load_library()
    shape = (3, 32, 32)
    inpaint = RandomInpaintingOperator(shape, 0.5, seed=0)
    for op in (IdentityOperator(shape), inpaint, GaussianBlurOperator(shape, 9, 3.0),
               SuperResolutionOperator(shape, 4)):
        assert lib.sp_dps_workspace(op.hip_descriptor(), 7) == 0
    psf = PSFBlurOperator(shape, psf_ops.random_sparse_kernel(4, seed=0))
    d = psf.hip_descriptor()
    for batch in (1, 7, 64):
        assert lib.sp_dps_workspace(d, batch) == batch * d.m
    assert lib.sp_dps_workspace(d, 0) == -1


@pytest.mark.parametrize("size,intensity", [(61, 0.5), (61, 0.0), (31, 1.0), (9, 0.5), (3, 0.3)])
def test_motion_blur_kernel(size, intensity):
    k = motion_blur_kernel(size, intensity, seed=0)
    assert tuple(k.shape) == (size, size) and k.dtype == torch.float32
    assert bool((k >= 0).all()) and abs(float(k.sum()) - 1.0) <= 1e-6
    assert torch.equal(k, motion_blur_kernel(size, intensity, seed=0))
    assert not torch.equal(k, motion_blur_kernel(size, intensity, seed=1))
    # the path passes through the centre: its bilinear footprint puts mass on the centre tap
    assert float(k[size // 2, size // 2]) > 0
    if size == 61:  # a thin curve in the box: what the span sweep exploits
        assert int((k != 0).sum()) < 0.15 * size * size


def test_motion_blur_kernel_straight_at_zero_intensity():
    """intensity = 0: all mass on one line through the centre (weighted PCA: no spread across it)."""
    for seed in range(3):
        k = motion_blur_kernel(61, 0.0, seed=seed).double()
        i, j = torch.meshgrid(torch.arange(61.0, dtype=torch.float64) - 30,
                              torch.arange(61.0, dtype=torch.float64) - 30, indexing="ij")
        pts = torch.stack([i.flatten(), j.flatten()], 1)
        w = k.flatten()
        cov = (pts * w[:, None]).T @ pts  # second moments about the centre
        evals, evecs = torch.linalg.eigh(cov)
        assert evals[1] > 10.0           # long along the line
        across = (pts @ evecs[:, 0]).abs()[w > 0]
        # every tap with mass is a corner of a unit cell that holds a point of the line, so it
        # lies within the cell's diagonal of it
        assert float(across.max()) < 2.0 ** 0.5
    curved = motion_blur_kernel(61, 1.0, seed=0).double().flatten()
    assert curved.numel() == 61 * 61


def test_motion_blur_kernel_rejects_bad_arguments():
    for args in ((60, 0.5), (63, 0.5), (61, -0.1), (61, 1.5)):
        with pytest.raises(ValueError):
            motion_blur_kernel(*args)


def test_motion_blur_operator():
    op = MotionBlurOperator((3, 64, 64), kernel_size=61, intensity=0.5, seed=3)
    assert torch.equal(op.kernel, motion_blur_kernel(61, 0.5, 3)) and op.radius == 30
    assert op.hip_descriptor().kind == _hip.SP_OP_PSF
    small = MotionBlurOperator((1, 16, 16), kernel_size=7, seed=1)
    x = torch.randn(1, 1, 16, 16, generator=torch.Generator().manual_seed(0))
    _close(small.apply(x), psf_ops.apply64(x, small.kernel))


def test_no_pseudo_inverse_so_pgdm_raises():
    import stand_ins as si
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.pgdm import PGDMSampler

    op = PSFBlurOperator((3, 32, 32), psf_ops.random_sparse_kernel(4, seed=0))
    with pytest.raises(NotImplementedError):
        op.apply_pseudo_inverse(torch.zeros(1, 3, 32, 32))
    net = si.make_samplers_amd_net("linear", 3, 0.1)
    ip = InverseProblem(op, torch.zeros(1, 3, 32, 32), GaussianNoise(0.05))
    with pytest.raises(NotImplementedError, match="apply_pseudo_inverse"):
        PGDMSampler(net)(ip, num_sampling_steps=4)
