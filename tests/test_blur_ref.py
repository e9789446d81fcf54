"""tests/blur_ref.py pinned on the CPU: the dense index-arithmetic matrices against oracle/blur.py
(F.pad + conv2d + autograd), the exact cases shown unroundable, the fp32 emulations of the two
algorithm shapes of csrc/sp_blur.hip returning the fp64 reference bit for bit, and the same
emulations broken on purpose failing in the fold bands (the cases have teeth)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import blur_ref as br
from oracle import blur as oblur
from samplers_amd.operators import GaussianBlurOperator

RADII = list(range(1, 9))


def all_cases(radius):
    return br.tile_cases(radius) + (br.REG_CASES + br.DMA_CASES if radius <= 4 else [])


EXACT = [(r, *c) for r in RADII for c in all_cases(r)]
EXACT_IDS = [f"R{r}-{'x'.join(map(str, s))}-b{b}-d{d}" for r, s, b, d in EXACT]


@functools.lru_cache(maxsize=None)
def exact_case(radius, shape, batch, ydiv):
    x, eps, y = br.exact_inputs(br.case_seed(radius, shape, batch), batch, ydiv, shape)  # the GPU file's
    ref = br.dps_pass64(x, eps, y, ydiv, *br.EXACT_COEFS, br.exact_taps(radius), shape)
    return x, eps, y, ref


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", ["gauss", "asym", "exact"])
def test_dense_reference_matches_the_oracle(radius, name):
    taps = br.taps_of(name, radius)
    g = np.random.default_rng(radius)
    for shape, _, _ in all_cases(radius):
        x = g.standard_normal((2, *shape))
        if name == "exact":
            x = np.round(4 * x).clip(-4, 4)
        xt = torch.from_numpy(x)
        fwd, adj = oblur.blur(xt, taps).numpy(), oblur.blur_adjoint(xt, taps).numpy()
        got_f, got_a = br.apply64(x, taps, shape), br.adjoint64(x, taps, shape)
        if name == "exact":  # eighths times small integers: both statements are exact
            assert np.array_equal(got_f, fwd) and np.array_equal(got_a, adj)
        np.testing.assert_allclose(got_f, fwd, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got_a, adj, rtol=0, atol=1e-12)


@pytest.mark.parametrize("radius", RADII)
def test_adjoint_matrix_is_the_transpose(radius):
    taps = br.asym_taps(radius).astype(np.float64)
    g = np.random.default_rng(radius)
    for n in (2 * radius + 1, 2 * radius + 2, 37):
        a = br.reflect_matrix(n, taps)
        np.testing.assert_allclose(a.sum(axis=1), taps.sum(), rtol=0, atol=1e-15)  # rows keep the tap mass
        s, x = g.standard_normal((1, n, n)), g.standard_normal((1, n, n))
        lhs = (br.apply64(x, taps, (1, n, n)) * s).sum()
        rhs = (x * br.adjoint64(s, taps, (1, n, n))).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
        assert np.array_equal(br.adjoint64(s, taps, (1, n, n))[0], a.T @ s[0] @ a)


def test_reflect_matrix_small_by_hand():
    a = br.reflect_matrix(3, [0.25, 0.5, 0.125])
    assert np.array_equal(a, [[0.5, 0.375, 0.0], [0.25, 0.5, 0.125], [0.0, 0.375, 0.5]])


@pytest.mark.parametrize("radius", RADII)
def test_exact_taps_shape(radius):
    t = br.exact_taps(radius)
    assert t[0] == 0.25 and t[radius] == 0.5 and t[-1] == 0.125
    assert not np.array_equal(t, t[::-1]) and np.array_equal(t * 8, np.round(t * 8))
    assert np.count_nonzero(t) == (3 if radius == 1 else 4)
    assert br.rounding_count(radius) == 6 * (2 * radius + 1) + 12


@pytest.mark.parametrize("radius,shape,batch,ydiv", EXACT, ids=EXACT_IDS)
def test_exact_cases_cannot_round(radius, shape, batch, ydiv):
    x, eps, y, ref = exact_case(radius, shape, batch, ydiv)
    for t in (x, eps, y):
        assert np.array_equal(t, np.round(t)) and np.abs(t).max() <= 4
    x0 = ref.x0
    assert np.array_equal(x0, np.round(x0))
    taps = br.exact_taps(radius)
    assert np.array_equal(ref.v * 4096, np.round(ref.v * 4096))  # four passes of eighths: 2^-12
    for t in (ref.r, br.apply64(x, taps, shape), br.adjoint64(x, taps, shape)):  # two passes: 2^-6
        assert np.array_equal(t * 64, np.round(t * 64))
    assert np.array_equal(ref.v.astype(np.float32).astype(np.float64), ref.v)
    # every partial sum is a multiple of 2^-12 below E_v: 24 bits
    assert ref.E_v.max() * 2 ** 12 < 2 ** 24
    assert (np.abs(ref.v) <= ref.E_v).all() and (np.abs(ref.r) <= ref.E_r).all()


@pytest.mark.parametrize("radius,shape,batch,ydiv", EXACT, ids=EXACT_IDS)
def test_fp32_emulations_are_bitwise_and_wrong_ones_are_caught(radius, shape, batch, ydiv):
    x, eps, y, ref = exact_case(radius, shape, batch, ydiv)
    taps = br.exact_taps(radius)
    want = ref.v.astype(np.float32)
    band = br.fold_band_mask(shape, radius)
    for form in br.FORMS:
        for reverse in (False, True):
            got = br.emulate_pass32(x, eps, y, ydiv, *br.EXACT_COEFS, taps, shape, form, reverse)
            assert np.array_equal(got, want), (form, reverse, br.describe_mismatch(got, want, shape, radius))
        for wrong in br.WRONG:
            got = br.emulate_pass32(x, eps, y, ydiv, *br.EXACT_COEFS, taps, shape, form, wrong=wrong)
            bad = (got != want).reshape(-1, *shape)
            assert (bad & band).any(), (form, wrong)


def test_emulation_on_random_data_is_within_the_bound():
    """The derived per-element bound holds for the emulation (two roundings per tap, the worst the
    count allows for) on randn data: the bound is not vacuous, nor is it tight to a factor."""
    radius, (shape, batch, ydiv) = 3, br.tile_cases(3)[1]
    taps = br.asym_taps(radius)
    x, eps, y = br.random_inputs(5, batch, ydiv, shape)
    ref = br.dps_pass64(x, eps, y, ydiv, *br.RANDOM_COEFS, taps, shape)
    for form in br.FORMS:
        got = br.emulate_pass32(x, eps, y, ydiv, *br.RANDOM_COEFS, taps, shape, form)
        ratio = np.abs(got - ref.v) / (br.rounding_count(radius) * br.U32 * ref.E_v)
        assert 1e-3 < ratio.max() <= 1.0


@pytest.mark.parametrize("radius", [1, 5, 8])
def test_operator_cpu_paths_match_the_dense_reference(radius):
    shape = br.tile_cases(radius)[1][0]
    op = GaussianBlurOperator(shape, 2 * radius + 1, 3.0)
    taps = op.taps.numpy()
    assert np.array_equal(taps, br.gaussian_taps(radius))
    x = torch.randn(2, *shape, generator=torch.Generator().manual_seed(radius))
    xn = x.numpy()
    # the host path is the same two 1-D passes in fp32, but its products and sums may round
    # separately: twice the kernels' counts
    for got, ref, env, count in (
            (op.apply(x), br.apply64(xn, taps, shape), br.apply64(np.abs(xn), taps, shape),
             2 * br.apply_count(radius)),
            (op.apply_transpose(x), br.adjoint64(xn, taps, shape), br.adjoint64(np.abs(xn), taps, shape),
             2 * br.adjoint_count(radius))):
        assert (np.abs(got.numpy() - ref) <= count * br.U32 * env).all()
