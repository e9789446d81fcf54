"""tests/sr_filter_ref.py against the operator's host form, torch's antialiased bicubic and
average pooling, and the exact cases: operands on which a correct fp32 evaluation in either
algorithm shape has no freedom (no GPU)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sr_filter_ref as sf
from samplers_amd.operators import (BicubicSuperResolutionOperator, FilteredSuperResolutionOperator,
                                    bicubic_taps)

SHAPES = [(2, 8, 4, 12), (2, 2, 6, 4), (2, 32, 16, 32), (4, 16, 8, 24), (4, 6, 12, 8), (8, 32, 16, 32),
          (8, 8, 8, 24)]  # (s, K, H, W)


@pytest.mark.parametrize("s,K,H,W", SHAPES)
def test_helper_matches_the_host_form(s, K, H, W):
    k = sf.random_taps(K)
    op = FilteredSuperResolutionOperator((2, H, W), k, factor=s)
    rng = np.random.default_rng(K + H)
    x = rng.standard_normal((3, 2, H, W))
    g = rng.standard_normal((3, 2, H // s, W // s))
    ax = op.apply(torch.from_numpy(x)).numpy()
    atg = op.apply_transpose(torch.from_numpy(g)).numpy()
    assert ax.shape == (3, 2, H // s, W // s) and atg.shape == x.shape
    assert np.abs(ax - sf.apply64(x, k, s)).max() <= 1e-12
    assert np.abs(atg - sf.adjoint64(g, k, s)).max() <= 1e-12


@pytest.mark.parametrize("s", [2, 4, 8])
def test_bicubic_matches_torch_on_the_interior(s):
    H, W = 10 * s, 12 * s
    x = torch.randn(2, 3, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(s))
    want = F.interpolate(x, scale_factor=1 / s, mode="bicubic", antialias=True)
    got = sf.apply64(x.numpy(), sf.bicubic_taps64(s).astype(np.float32), s)
    host = BicubicSuperResolutionOperator((3, H, W), factor=s).apply(x)
    inner = (slice(None), slice(None), slice(2, H // s - 2), slice(2, W // s - 2))
    assert np.abs(got[inner] - want.numpy()[inner]).max() <= 1e-12
    assert float((host[inner] - want[inner]).abs().max()) <= 1e-12
    # torch clips and renormalises the window at the border: those outputs differ
    assert np.abs(got[..., 0, :] - want.numpy()[..., 0, :]).max() > 1e-3


@pytest.mark.parametrize("s", [2, 4, 8])
def test_bicubic_taps_are_dyadic_and_sum_to_one(s):
    k64 = sf.bicubic_taps64(s)
    k = bicubic_taps(s)
    assert k.dtype == torch.float32 and k.numel() == 4 * s
    assert np.array_equal(k.double().numpy(), k64)  # exact in fp32
    assert k64.sum() == 1.0
    bits = {2: 8, 4: 12, 8: 16}[s]  # cubic(odd / 2s) / s is a multiple of 1 / (16 s^4)
    assert np.array_equal(k64 * 2 ** bits, np.round(k64 * 2 ** bits))
    assert np.array_equal(k64, k64[::-1]) and k64[0] < 0 < k64[2 * s]


@pytest.mark.parametrize("s,K,H,W", SHAPES)
def test_transpose_identity(s, K, H, W):
    k = sf.random_taps(K)
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((H, W)), rng.standard_normal((H // s, W // s))
    lhs, rhs = (sf.apply64(x, k, s) * y).sum(), (x * sf.adjoint64(y, k, s)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


@pytest.mark.parametrize("s", [2, 4, 8])
def test_box_taps_are_average_pooling(s):
    L = 6 * s
    A = sf.matrix_1d(np.full(s, 1.0 / s), L, s)
    pool = F.avg_pool1d(torch.eye(L, dtype=torch.float64).unsqueeze(1), s).squeeze(1).t().numpy()
    assert np.array_equal(A, pool)
    x = np.random.default_rng(s).integers(-3, 4, size=(2, L, L)).astype(np.float64)
    assert np.array_equal(sf.apply64(x, np.full(s, 1.0 / s), s),
                          F.avg_pool2d(torch.from_numpy(x), s).numpy())


# --- the exact cases ------------------------------------------------------------------------------
EXACT = sf.EXACT_SHAPES


def _exact_data(s, K, H, W):
    k, x, _, g, _ = sf.exact_data(s, K, H, W)
    return k, x, g


@pytest.mark.parametrize("s,K,H,W", EXACT)
def test_exact_cases_every_emulation_returns_the_fp64_result(s, K, H, W):
    k, x, g = _exact_data(s, K, H, W)
    assert np.array_equal(k * 8, np.round(k * 8)) and k[0] != 0 and k[-1] != 0
    assert not np.array_equal(k, k[::-1])
    ax, atg = sf.apply64(x, k, s), sf.adjoint64(g, k, s)
    assert np.array_equal(ax.astype(np.float32).astype(np.float64), ax)
    for order in ("hv", "vh"):
        assert np.array_equal(sf.emu_apply(x, k, s, order).astype(np.float64), ax), order
    for order in ("cols_inner", "rows_inner"):
        assert np.array_equal(sf.emu_adjoint(g, k, s, order).astype(np.float64), atg), order


@pytest.mark.parametrize("s,K,H,W", [c for c in EXACT if c[1] > c[0]])
def test_exact_cases_see_the_faults_in_the_fold_bands(s, K, H, W):
    k, x, g = _exact_data(s, K, H, W)
    P = (K - s) // 2
    ax, atg = sf.apply64(x, k, s), sf.adjoint64(g, k, s)
    rows = np.zeros(H, dtype=bool)
    rows[:P], rows[H - P:] = True, True  # the pixels with fold terms
    orow = np.array([s * o - P < 0 or s * o + K - 1 - P >= H for o in range(H // s)])  # outputs with them
    cols = np.zeros(W, dtype=bool)
    cols[:P], cols[W - P:] = True, True
    ocol = np.array([s * o - P < 0 or s * o + K - 1 - P >= W for o in range(W // s)])

    def differs(got, want, band):
        return bool((got.astype(np.float64) != want)[..., band, :].any())

    assert differs(sf.emu_adjoint(g, k, s, reverse=True), atg, rows)
    for drop, band_x, band_y in (("lo", rows & (np.arange(H) < P), orow & (np.arange(H // s) < H // s / 2)),
                                 ("hi", rows & (np.arange(H) >= H - P), orow)):
        assert differs(sf.emu_adjoint(g, k, s, drop=drop), atg, band_x), drop
        assert differs(sf.emu_apply(x, k, s, drop=drop), ax, band_y), drop
        # and nowhere else: a dropped fold changes the fold bands (of either axis) only
        assert not (sf.emu_adjoint(g, k, s, drop=drop) != atg)[..., ~rows, :][..., ~cols].any(), drop
        assert not (sf.emu_apply(x, k, s, drop=drop) != ax)[..., ~orow, :][..., ~ocol].any(), drop
    for shift in (-1, 1):
        if P + shift < 0 or P + shift > min(H, W):
            continue
        assert differs(sf.emu_apply(x, k, s, shift=shift), ax, orow), shift
        assert differs(sf.emu_adjoint(g, k, s, shift=shift), atg, rows), shift


def test_bicubic_tables_round_in_two_passes():
    """The x4 table carries 12 fraction bits per tap (x8: 16): an output's products need 24 and
    the vertical pass sums rounded horizontal results, so on integers the two orders of the
    emulation are not both the fp64 result: these tables are not exact cases."""
    s = 4
    k = sf.bicubic_taps64(s).astype(np.float32)
    x = np.random.default_rng(0).integers(-2000, 2001, size=(4, 64, 64)).astype(np.float64) * 1025.0
    ax = sf.apply64(x, k, s)
    hv, vh = sf.emu_apply(x, k, s, "hv").astype(np.float64), sf.emu_apply(x, k, s, "vh").astype(np.float64)
    assert (hv != ax).any() and (vh != ax).any() and (hv != vh).any()
    assert np.abs(hv - ax).max() <= 2 * 16 * 2.0 ** -24 * np.abs(ax).max() * 4
