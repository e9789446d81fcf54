"""The bf16 3x3 convolution judged per output, and the other bf16 layers away from the SD widths.

tests/test_bf16_gpu.py bounds one relative-L2 number per tensor; at 3e-3 over a million outputs a
handful of completely wrong ones pass, and halo, tile-tail and last-channel-block mistakes produce
exactly those.  Here every output is held to what one bf16 rounding of an fp32 sum of 9 cin terms
can give, against fp64 on the same bf16 operands:

    |y - y64| <= 2^-8 |y64| + 9 cin 2^-23 (|x| * |w| + |bias| + |res|)

(the input VJP likewise with cout terms), at shapes with h != w (``conv_tc`` admits any w % 32 == 0,
h % 16 == 0; several row blocks and column strips, more samples than one), at the small levels
whose tiles hold several samples, with a residual and with output channels that do not fill the
last block.  One test feeds unit impulses at the corners, edges and tile seams of an otherwise zero
input: every output is then one weight, a sum of a few, or exactly zero, so anything a halo cell
held shows.

GroupNorm (a group straddling the two concatenated parts, 12 channels per group, hw = 1 and 35; its
returned statistics per group on the value cases of tests/gn_ref.py),
LayerNorm (c = 8 and 2048, 0 / 1 / 37 rows), GEGLU (f = 8, 0 / 7 rows) and the 2x2 pool (c = 8,
2 x 6) at bf16, against fp64 at the bounds of tests/test_bf16_gpu.py.
"""

from __future__ import annotations

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U = 2.0 ** -8  # one bf16 rounding (8 significant bits)


def _rel(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _conv_case(cuda, shape, with_res, seed):
    """(y, dx) of the bf16 tile and (reference, envelope) pairs in fp64 for both."""
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import Conv3x3

    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(seed)
    conv = Conv3x3(cin, cout).requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5))
        conv.bias.copy_(torch.randn(cout, generator=g))
    conv = conv.to(BF)
    x = torch.randn(n, cin, h, w, generator=g).to(BF)
    dy = torch.randn(n, cout, h, w, generator=g).to(BF)
    res = torch.randn(n, cout, h, w, generator=g).to(BF) if with_res else None
    dev = copy.deepcopy(conv).to(cuda)
    xr = x.to(cuda).requires_grad_(True)
    assert bf16.conv_supported(dev, xr)
    with torch.enable_grad():
        y = bf16.conv3x3(dev, xr, res=None if res is None else res.to(cuda))
    (dx,) = torch.autograd.grad(y, xr, dy.to(cuda))
    assert y.dtype == BF and dx.dtype == BF and y.shape == dy.shape and dx.shape == x.shape
    wd, bd, xd, dyd = conv.weight.double(), conv.bias.double(), x.double(), dy.double()
    y64 = F.conv2d(xd, wd, bd, padding=1)
    env = F.conv2d(xd.abs(), wd.abs(), bd.abs(), padding=1)
    if res is not None:
        y64, env = y64 + res.double(), env + res.double().abs()
    dx64 = torch.nn.grad.conv2d_input(x.shape, wd, dyd, padding=1)
    denv = torch.nn.grad.conv2d_input(x.shape, wd.abs(), dyd.abs(), padding=1)
    return (y.double().cpu(), y64, env, 9 * cin), (dx.double().cpu(), dx64, denv, 9 * cout)


def _elementwise(got, want, env, terms) -> float:
    """The worst |got - want| as a fraction of the bound (<= 1 passes)."""
    assert torch.isfinite(got).all()
    return float(((got - want).abs() / (U * want.abs() + terms * 2.0 ** -23 * env)).max())


def _judge_conv(cuda, parity_record, shape, with_res):
    fwd, vjp = _conv_case(cuda, shape, with_res, seed=sum(shape))
    r_y, r_dx = _elementwise(*fwd), _elementwise(*vjp)
    e_y, e_dx = _rel(fwd[0], fwd[1]), _rel(vjp[0], vjp[1])
    parity_record("conv_bf16_elementwise", r_y, 1.0, shape=list(shape), res=with_res, rel_l2=e_y)
    parity_record("conv_bf16_vjp_elementwise", r_dx, 1.0, shape=list(shape), res=with_res, rel_l2=e_dx)
    print(f"conv {shape}: elementwise {r_y:.3f} / vjp {r_dx:.3f} of the bound; rel L2 {e_y:.2e} / {e_dx:.2e}")
    assert r_y <= 1.0 and r_dx <= 1.0, (r_y, r_dx)
    assert e_y < 3e-3 and e_dx < 5e-3, (e_y, e_dx)


@pytest.mark.parametrize("shape", [(2, 32, 64, 16, 32), (1, 48, 80, 48, 32), (3, 16, 16, 16, 64), (1, 64, 3, 32, 96)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
def test_conv3x3_bf16_rectangular_elementwise(cuda, parity_record, shape, with_res):
    _judge_conv(cuda, parity_record, shape, with_res)


SMALL = [(3, 64, 128, 16, 16), (5, 32, 64, 8, 8), (2, 64, 64, 4, 4), (2, 16, 64, 32, 32)]
RAGGED_COUT = {(3, 64, 128, 16, 16): 72, (5, 32, 64, 8, 8): 20, (2, 64, 64, 4, 4): 3, (2, 16, 64, 32, 32): 44}


@pytest.mark.parametrize("shape", SMALL + [(s[0], s[1], RAGGED_COUT[s], s[3], s[4]) for s in SMALL],
                         ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_bf16_small_levels_elementwise(cuda, parity_record, shape):
    """The 16 / 8 / 4 levels (several samples per tile, the last tile partly past the batch) and a
    32-wide one, with a residual; then with output channels that end inside a block of 16."""
    _judge_conv(cuda, parity_record, shape, True)


@pytest.mark.parametrize("shape", [(2, 32, 64, 32, 64), (1, 16, 16, 16, 96), (3, 16, 32, 16, 16), (5, 16, 16, 8, 8),
                                   (3, 32, 16, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_bf16_impulses_see_zero_halos(cuda, shape):
    """Unit impulses at the four corners, the middle of each edge and on both sides of every tile seam
    (rows 15 | 16, columns 31 | 32) of each sample, each in a channel of its own, into a zero input,
    bias 0: y[:, co, i, j] is w[co, ci, 1 + pi - i, 1 + pj - j] summed over the impulses within one
    pixel — a single weight, a sum of a few, or exactly 0 — and the kernel must store its bf16
    rounding.  A halo cell that kept an earlier stage's pixel, a neighbouring sample's row or a
    wrapped column adds a weight that does not belong."""
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import Conv3x3

    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(h * w + cin)
    conv = Conv3x3(cin, cout).requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g))
        conv.bias.zero_()
    conv = conv.to(BF)
    rows = sorted({0, h // 2, h - 1} | {r for r in (15, 16) if r < h})
    cols = sorted({0, w // 2, w - 1} | {c for c in (31, 32, 63, 64) if c < w})
    x = torch.zeros(n, cin, h, w)
    k = 0
    for i in rows:
        for j in cols:
            if i in (0, h - 1) or j in (0, w - 1) or i in (15, 16) or j in (31, 32, 63, 64):
                for s in range(n):
                    x[s, (k + 5 * s) % cin, i, j] = 1.0
                k += 1
    assert k >= 8
    y = bf16.conv3x3(conv.to(cuda), x.to(BF).to(cuda)).double().cpu()
    y64 = F.conv2d(x.double(), conv.weight.double().cpu(), None, padding=1)
    assert torch.isfinite(y).all()
    zero = y64 == 0
    assert (~zero).any() and (zero.any() or h <= 4)  # (at 4 x 4 every pixel is next to an impulse)
    assert (y[zero] == 0).all(), f"{int((y[zero] != 0).sum())} outputs that no impulse reaches are not 0"
    assert ((y - y64).abs() <= U * y64.abs()).all()


def _gn_case(cuda, parity_record, c1, c2, groups, h, w, act, bias, value=None, judge="all"):
    """``value``: a value case of tests/gn_ref.py for x and chan_bias, rounded to bf16 (the reference
    is fp64 on the rounded operands); the statistics ``bf16._gn_fwd_raw`` returns are then held per
    group to gn_ref's statistics bound (they are fp32 partial sums finalized in fp64).  ``judge``:
    "all", or "stats" / "rel_l2" for one of the two sets of assertions."""
    import gn_ref
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import GroupNormAct

    torch.manual_seed(c1 + 7 * c2 + h * w)
    n, c = 3, c1 + c2
    norm = GroupNormAct(groups, c, eps=1e-5, act=act)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(c))
        norm.bias.copy_(0.1 * torch.randn(c))
    norm = norm.to(device=cuda, dtype=BF).requires_grad_(False)
    x1 = (torch.randn(n, c1, h, w) * 2 + 3).to(BF)
    x2 = None if not c2 else (torch.randn(n, c2, h, w) - 1).to(BF)
    cb = (torch.randn(n, c) * 0.5).to(BF) if bias else None
    dz = torch.randn(n, c, h, w).to(BF)
    if value is not None:
        t = gn_ref.make_case(value, (n, c, h, w, groups))
        x1, cb = t.x[:, :c1].to(BF), t.cb.to(BF)
        x2 = None if not c2 else t.x[:, c1:].to(BF)
    x1g = x1.to(cuda).requires_grad_(True)
    x2g = None if x2 is None else x2.to(cuda).requires_grad_(True)
    assert bf16.group_norm_supported(norm, x1g, c2)
    with torch.enable_grad():
        z = bf16.group_norm(norm, x1g, x2g, None if cb is None else cb.to(cuda))
    grads = torch.autograd.grad(z, [t for t in (x1g, x2g) if t is not None], dz.to(cuda))
    xs = [x1.double().requires_grad_(True)] + ([] if x2 is None else [x2.double().requires_grad_(True)])
    with torch.enable_grad():
        xf = torch.cat(xs, 1)
        if cb is not None:
            xf = xf + cb.double()[:, :, None, None]
        ref = F.group_norm(xf, groups, norm.weight.double().cpu(), norm.bias.double().cpu(), 1e-5)
        if act:
            ref = F.silu(ref)
    rg = torch.autograd.grad(ref, xs, dz.double())
    assert torch.isfinite(z.float()).all() and all(torch.isfinite(t.float()).all() for t in grads)
    e = _rel(z, ref)
    ev = max(_rel(a, b) for a, b in zip(grads, rg))
    tag = {} if value is None else {"case": gn_ref.CASES[value]}
    parity_record("gn_bf16_rel_l2", e, 3e-3, c=[c1, c2], groups=groups, hw=h * w, **tag)
    parity_record("gn_bf16_vjp_rel_l2", ev, 5e-3, c=[c1, c2], groups=groups, hw=h * w, **tag)
    print(f"GroupNorm {c1}+{c2} / {groups}, hw {h * w}, case {value}: {e:.2e}, vjp {ev:.2e}")
    e_r = e_m = 0.0
    if value is not None:
        _, stats = bf16._gn_fwd_raw(norm, bf16.nhwc(x1g.detach()), None if x2g is None else bf16.nhwc(x2g.detach()),
                                    None if cb is None else cb.to(cuda).float().contiguous())
        sref = gn_ref.gn_fp64((x1, x2), groups, None, None, 1e-5, False, cb)
        e_r, e_m = gn_ref.rstd_error(stats[1], sref), gn_ref.mean_excess(stats[0], sref)
        parity_record("gn_bf16_rstd_rel", e_r, gn_ref.STAT_TOL, c=[c1, c2], groups=groups, hw=h * w, **tag)
        parity_record("gn_bf16_mean_of_bound", e_m, 1.0, c=[c1, c2], groups=groups, hw=h * w, **tag)
        print(f"    statistics: rstd {e_r:.2e} (bound {gn_ref.STAT_TOL:.0e}), mean {e_m:.3f} of its bound")
    if judge != "stats":
        assert e < 3e-3 and ev < 5e-3, (e, ev)
    if judge != "rel_l2":
        assert e_r <= gn_ref.STAT_TOL and e_m <= 1.0, (e_r, e_m)


@pytest.mark.parametrize("c1,c2,groups,h,w,act,bias", [(40, 56, 8, 12, 20, True, True),
                                                       (40, 56, 8, 12, 20, False, False),
                                                       (64, 0, 32, 1, 1, True, False), (64, 0, 32, 5, 7, True, True),
                                                       (24, 40, 32, 5, 7, False, False)])
def test_groupnorm_bf16_odd_groups_and_sizes(cuda, parity_record, c1, c2, groups, h, w, act, bias):
    """12 channels per group with group 3 (channels 36 .. 47) half in each part; one pixel (a group is
    two numbers); 35 pixels (no multiple of any chunk)."""
    _gn_case(cuda, parity_record, c1, c2, groups, h, w, act, bias)


GN_VALUE_SHAPES = [(64, 0, 32, 32, 32), (40, 56, 8, 12, 20), (1280, 1280, 32, 2, 2), (64, 0, 32, 5, 7)]


@pytest.mark.parametrize("value", [1, 2, 4, 6, 7, 10], ids=lambda v: f"case{v}")
@pytest.mark.parametrize("c1,c2,groups,h,w", GN_VALUE_SHAPES)
def test_groupnorm_bf16_statistics_on_value_cases(cuda, parity_record, c1, c2, groups, h, w, value):
    """The per-group statistics at an elementwise bound on the value cases that put the sample's
    first pixel, the first image row, one channel or the first channel's bias far from the group
    mean, or the mean far from zero (the stats pass shifts each channel's sums; 2560 channels take
    its column-block loop)."""
    _gn_case(cuda, parity_record, c1, c2, groups, h, w, True, True, value=value, judge="stats")


# Case 7 rounded to bf16 is x = 1000 everywhere, the spread all in chan_bias (1e-3): the fp32 mean
# the kernel returns (and any fp32 affine built on it) is 2^-24 * 1e3 * rstd = 0.02 of a y of 0.3
# off.  torch's fp32 CPU GroupNorm on the same operands is 6.1e-2 .. 9.0e-2 in relative L2; the
# kernel measured 5.3e-2 .. 8.0e-2 forward and 1.0e-2 .. 1.2e-2 in the VJP on an MI355X.  The
# statistics bound above has a term for the mean's representability, these two bounds have none.
_CASE7 = pytest.param(7, id="case7", marks=pytest.mark.xfail(
    strict=True, reason="fp32 mean of 1000 over a spread of 1e-3: forward 5.3e-2 .. 8.0e-2 (bound 3e-3), "
                        "VJP 1.0e-2 .. 1.2e-2 (bound 5e-3); torch fp32 CPU: 6.1e-2 .. 9.0e-2"))


@pytest.mark.parametrize("value", [1, 2, 4, 6, _CASE7, 10], ids=lambda v: f"case{v}")
@pytest.mark.parametrize("c1,c2,groups,h,w", GN_VALUE_SHAPES)
def test_groupnorm_bf16_forward_and_vjp_on_value_cases(cuda, parity_record, c1, c2, groups, h, w, value):
    """The forward and the input VJP on the same value cases at the relative-L2 bounds of
    tests/test_bf16_gpu.py."""
    _gn_case(cuda, parity_record, c1, c2, groups, h, w, True, True, value=value, judge="rel_l2")


@pytest.mark.parametrize("c", [8, 2048])
@pytest.mark.parametrize("rows", [0, 1, 37])
def test_layernorm_bf16_narrow_wide_and_few_rows(cuda, parity_record, c, rows):
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import LayerNorm

    gen = torch.Generator().manual_seed(c + rows)
    mod = LayerNorm(c)
    with torch.no_grad():
        mod.weight.copy_(1 + 0.1 * torch.randn(c, generator=gen))
        mod.bias.copy_(0.1 * torch.randn(c, generator=gen))
    mod.requires_grad_(False)
    x = (torch.randn(rows, c, generator=gen) * 3 + 1).to(BF)
    dy = torch.randn(rows, c, generator=gen).to(BF)
    gm = copy.deepcopy(mod).to(cuda, BF)
    xg = x.to(cuda).requires_grad_(True)
    assert bf16.layer_norm_supported(gm, xg)
    with torch.enable_grad():
        y = bf16.layer_norm(xg, gm)
    (dx,) = torch.autograd.grad(y, xg, dy.to(cuda))
    assert y.shape == x.shape and dx.shape == x.shape and y.dtype == BF and dx.dtype == BF
    if rows == 0:
        return
    xf = x.double().requires_grad_(True)
    with torch.enable_grad():
        ref = F.layer_norm(xf, (c,), mod.weight.double(), mod.bias.double(), mod.eps)
    (rx,) = torch.autograd.grad(ref, xf, dy.double())
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
    e1, e2 = _rel(y, ref), _rel(dx, rx)
    parity_record("layernorm_bf16_rel_l2", e1, 5e-3, c=c, rows=rows)
    parity_record("layernorm_bf16_vjp_rel_l2", e2, 1e-2, c=c, rows=rows)
    print(f"LayerNorm c {c} rows {rows}: {e1:.2e}, vjp {e2:.2e}")
    assert e1 < 5e-3 and e2 < 1e-2, (e1, e2)


@pytest.mark.parametrize("rows", [0, 7])
def test_geglu_bf16_one_vector_per_row(cuda, parity_record, rows):
    from samplers_amd.networks import bf16

    f = 8
    gen = torch.Generator().manual_seed(rows)
    h = torch.randn(rows, 2 * f, generator=gen).to(BF)
    dy = torch.randn(rows, f, generator=gen).to(BF)
    hg = h.to(cuda).requires_grad_(True)
    assert bf16.geglu_supported(hg)
    with torch.enable_grad():
        y = bf16.geglu(hg)
    (dh,) = torch.autograd.grad(y, hg, dy.to(cuda))
    assert y.shape == (rows, f) and dh.shape == h.shape and y.dtype == BF and dh.dtype == BF
    if rows == 0:
        return
    hf = h.double().requires_grad_(True)
    with torch.enable_grad():
        a, gate = hf.chunk(2, dim=-1)
        ref = a * F.gelu(gate)
    (rh,) = torch.autograd.grad(ref, hf, dy.double())
    e1, e2 = _rel(y, ref), _rel(dh, rh)
    parity_record("geglu_bf16_rel_l2", e1, 4e-3, f=f, rows=rows)
    parity_record("geglu_bf16_vjp_rel_l2", e2, 4e-3, f=f, rows=rows)
    assert e1 < 4e-3 and e2 < 4e-3, (e1, e2)


def test_pool2x2_bf16_one_vector_per_pixel(cuda):
    """sp_pool2x2_bf16 at c = 8 (one 8-channel vector per pixel), 2 x 6 -> 1 x 3: the 2 x 2 block
    sums in fp32, rounded once."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    n, c, h, w = 3, 8, 2, 6
    gen = torch.Generator().manual_seed(6)
    dz = torch.randn(n, h, w, c, generator=gen).to(BF)  # NHWC
    dzg = dz.to(cuda)
    dx = torch.full((n * (h // 2) * (w // 2) + 1, c), float("nan"), device=cuda, dtype=BF)  # + a guard row
    _hip.check(lib.sp_pool2x2_bf16(dzg.data_ptr(), n, c, h, w, dx.data_ptr(), None), "sp_pool2x2_bf16")
    torch.cuda.synchronize()
    assert torch.isnan(dx[-1]).all() and not torch.isnan(dx[:-1]).any()
    ref = dz.double().reshape(n, h // 2, 2, w // 2, 2, c).sum((2, 4))
    got = dx[:-1].double().cpu().reshape(ref.shape)
    # four bf16 addends summed in fp32 (three roundings of 2^-24 of the partial sums), one bf16 rounding
    env = dz.double().abs().reshape(n, h // 2, 2, w // 2, 2, c).sum((2, 4))
    assert ((got - ref).abs() <= U * ref.abs() + 3 * 2.0 ** -24 * env).all()
