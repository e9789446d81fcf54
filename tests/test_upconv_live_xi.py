"""The zero structure the fused upsample conv's live-ξ tile rests on (csrc/sp_wino.hip,
"Live-ξ forms"), in float32 numpy, no GPU.

(1) For a nearest-2x-upsampled, zero-padded image every even-aligned 4x4 window has rows 1, 2
and columns 1, 2 equal, so V = B^T d B — in the kernel's operation order (``wino_in``) — has
exact zeros in row 2 and column 2: 7 of the 16 ξ.  (2) With those 7 entries of M zero, the
output transform in ``xi_epilogue``'s operation order equals the same sums with the zero terms
dropped (``np.array_equal``: -0 == +0, the one permitted difference)."""

import numpy as np
import pytest

DEAD = [(r, c) for r in range(4) for c in range(4) if r == 2 or c == 2]


def wino_in(d):
    """V = B^T d B for windows d[..., 4, 4]; columns first, then rows, one IEEE op per element."""
    d = d.astype(np.float32)
    t = np.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :],
                  d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]], axis=-2)
    v = np.stack([t[..., 0] - t[..., 2], t[..., 1] + t[..., 2],
                  t[..., 2] - t[..., 1], t[..., 1] - t[..., 3]], axis=-1)
    assert v.dtype == np.float32
    return v


def windows(src, offset=0):
    """All 4x4 windows of the upsampled, zero-padded image whose 2x2 output tile starts at
    (2i + offset, 2j + offset): window rows 2i + offset - 1 .. + 2 of the upsampled image."""
    up = np.repeat(np.repeat(src, 2, axis=0), 2, axis=1)
    pad = np.pad(up, 1 + offset)
    h, w = src.shape
    return np.stack([pad[2 * i + 2 * offset:2 * i + 2 * offset + 4, 2 * j + 2 * offset:2 * j + 2 * offset + 4]
                     for i in range(h) for j in range(w)]).astype(np.float32)


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (4, 1), (2, 2), (5, 7), (8, 16)])
def test_even_aligned_windows_of_an_upsampled_image_have_seven_zero_xi(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    for scale in (1.0, 1e-30, 1e30):  # ordinary, near-denormal and large magnitudes
        src = (rng.standard_normal(hw) * scale).astype(np.float32)
        d = windows(src)  # every tile: all four borders and the corners included
        assert d.shape == (hw[0] * hw[1], 4, 4)
        assert np.array_equal(d[:, 1, :], d[:, 2, :]) and np.array_equal(d[:, :, 1], d[:, :, 2])
        v = wino_in(d)
        for r, c in DEAD:
            assert np.all(v[:, r, c] == 0.0), (r, c)
            assert not np.any(np.signbit(v[:, r, c])), "x - x rounds to +0"
        live = np.abs(v[:, [0, 1, 3]][:, :, [0, 1, 3]])
        assert live.max() > 0


def test_odd_aligned_windows_do_not_have_the_zeros():
    """The alignment matters: the same transform of windows one pixel off is dense."""
    src = np.random.default_rng(3).standard_normal((5, 7)).astype(np.float32)
    v = wino_in(windows(src, offset=1)[: 4 * 6])
    assert np.abs(v[:, 2, :]).max() > 0 and np.abs(v[:, :, 2]).max() > 0


def out_full(m, bv):
    """Y = A^T M A + bias as xi_epilogue adds it: row sums of each ξ row, then the columns."""
    s0 = [m[:, r, 0] + m[:, r, 1] + m[:, r, 2] for r in range(4)]
    s1 = [m[:, r, 1] - m[:, r, 2] - m[:, r, 3] for r in range(4)]
    return np.stack([s0[0] + s0[1] + s0[2] + bv, s1[0] + s1[1] + s1[2] + bv,
                     s0[1] - s0[2] - s0[3] + bv, s1[1] - s1[2] - s1[3] + bv])


def out_live(m, bv):
    """The same sums with the terms of ξ row 2 and ξ column 2 dropped, the order kept."""
    s0 = {r: m[:, r, 0] + m[:, r, 1] for r in (0, 1, 3)}
    s1 = {r: m[:, r, 1] - m[:, r, 3] for r in (0, 1, 3)}
    return np.stack([s0[0] + s0[1] + bv, s1[0] + s1[1] + bv,
                     s0[1] - s0[3] + bv, s1[1] - s1[3] + bv])


@pytest.mark.parametrize("bias", ["random", "zero", "negzero"])
def test_output_transform_with_the_zero_terms_dropped_is_the_same_sum(bias):
    rng = np.random.default_rng(11)
    n = 20000
    m = rng.standard_normal((n, 4, 4)).astype(np.float32) * np.float32(3.0)
    # exact cancellations and signed zeros among the live entries too
    m[: n // 8, 0, 1] = -m[: n // 8, 0, 0]
    m[n // 8: n // 4, 1, 1] = m[n // 8: n // 4, 1, 3]
    m[n // 4: n // 4 + 64] = 0.0
    m[n // 4 + 64: n // 4 + 128] = -0.0
    for r, c in DEAD:
        m[:, r, c] = 0.0  # what the accumulators of the dead ξ hold: +0
    bv = {"random": rng.standard_normal(n).astype(np.float32),
          "zero": np.zeros(n, np.float32), "negzero": np.full(n, -0.0, np.float32)}[bias]
    full, live = out_full(m, bv), out_live(m, bv)
    assert full.dtype == live.dtype == np.float32
    assert np.array_equal(full, live)
    if bias == "random":  # bitwise too wherever the result is not a zero
        nz = full != 0
        assert np.array_equal(full[nz].view(np.uint32), live[nz].view(np.uint32))
