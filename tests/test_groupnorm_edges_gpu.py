"""The fp32 GroupNorm kernels (csrc/sp_groupnorm.hip) at the inputs and shapes where a shifted-sum
variance and a chunked team kernel go wrong, against tests/gn_ref.py (fp64 closed form).

tests/test_groupnorm_gpu.py feeds ``randn * 2 + 0.7`` and bounds one relative-L2 number per tensor;
the returned statistics are never looked at.  Here ``layers.gn_forward`` / ``gn_backward`` are
called directly, so ``mean`` / ``rstd`` are judged per group, the forward per element and the
input VJP per group (bounds: gn_ref.FWD_TOL, STAT_TOL, VJP_TOL and what goes with them), on the
value cases of gn_ref (a group's first element / vector / row, its last element, one channel or
the first channel's bias far from the mean; a large mean over a small spread; a spread below eps;
a constant group), at group sizes on the chunk edges, on the scalar kernels with two chunks, at
128 and 129 channels per group, past 256 chunks per group in either direction, and on two-part
inputs whose groups straddle the parts.  Every case runs with the single-pass kernels disabled
and enabled, with and without SiLU, and a test of its own asserts from the profiler's kernel
names that each shape took the path it is there for.
"""

from __future__ import annotations

import pytest
import torch

import gn_ref

pytestmark = pytest.mark.gpu

SP_EINVAL = -1


def _kernel_names(fn) -> set[str]:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type.name == "CUDA"}


def _layer(t: gn_ref.GnCase, c: int, act: bool, cuda):
    from samplers_amd.networks.layers import GroupNormAct

    layer = GroupNormAct(t.groups, c, eps=t.eps, act=act)
    with torch.no_grad():
        layer.weight.copy_(t.gamma)
        layer.bias.copy_(t.beta)
    return layer.to(cuda).requires_grad_(False)


def _device_inputs(t: gn_ref.GnCase, c1: int, cuda):
    """(x1, x2, cb, dz, add1, add2) on the device; one part: x2, add1, add2 are None."""
    if not c1:
        return t.x.to(cuda), None, t.cb.to(cuda), t.dz.to(cuda), None, None
    return (t.x[:, :c1].contiguous().to(cuda), t.x[:, c1:].contiguous().to(cuda), t.cb.to(cuda), t.dz.to(cuda),
            t.add[:, :c1].contiguous().to(cuda), t.add[:, c1:].contiguous().to(cuda))


def _run(layer, dev):
    from samplers_amd.networks.layers import gn_backward, gn_forward

    x1, x2, cb, dz, a1, a2 = dev
    z, st = gn_forward(layer, x1, x2, cb)
    d1, d2 = gn_backward(layer, dz, x1, x2, cb, st, add1=a1, add2=a2)
    torch.cuda.synchronize()
    return z, st, (d1 if d2 is None else torch.cat([d1, d2], 1))


def _cases():
    for entry in gn_ref.SHAPES:
        for case in entry[2]:
            yield pytest.param(entry, case, id=f"{gn_ref.shape_id(entry)}-{gn_ref.CASES[case]}")


@pytest.mark.parametrize("entry,case", list(_cases()))
def test_statistics_forward_and_vjp_per_group(cuda, parity_record, entry, case):
    """mean / rstd per group, z per element and dx per group against fp64, two-pass and
    single-pass, with and without SiLU (the two shapes above 2^20 elements: one of the two per
    case, both over the cases).  Every figure is printed and recorded before anything is asserted."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    shape, c1, _ = entry
    n, c, h, w, groups = shape
    t = gn_ref.make_case(case, shape)
    dev = _device_inputs(t, c1, cuda)
    acts = (case % 2 == 1,) if c * h * w > 1 << 20 else (True, False)
    bad = []
    prev = lib.sp_groupnorm_single_pass(-1)
    try:
        for act in acts:
            ref = gn_ref.reference(case, shape, act, 0, bool(c1))
            yard = gn_ref.yardstick_vjp_error(case, shape, act, 0, bool(c1))
            vbound, relaxed = gn_ref.vjp_bound(yard, ref, case)
            layer = _layer(t, c, act, cuda)
            for single in (0, 1):
                lib.sp_groupnorm_single_pass(single)
                z, st, dx = _run(layer, dev)
                e_r, e_m = gn_ref.rstd_error(st[1], ref), gn_ref.mean_excess(st[0], ref)
                e_z, e_zp = gn_ref.forward_excess(z, ref, t.gamma, groups), gn_ref.forward_error(z, ref)
                e_v = gn_ref.vjp_error(dx, ref, groups)
                tag = dict(shape=gn_ref.shape_id(entry), case=gn_ref.CASES[case], act=act, single_pass=single)
                parity_record("gn_rstd_rel", e_r, gn_ref.STAT_TOL, **tag)
                parity_record("gn_mean_of_bound", e_m, 1.0, **tag)
                parity_record("gn_fwd_of_bound", e_z, 1.0, fwd_err=e_zp, **tag)
                parity_record("gn_vjp_per_group", e_v, vbound, yardstick=yard, relaxed=relaxed, **tag)
                print(f"{gn_ref.shape_id(entry)} case {case} act {act} single {single}: rstd {e_r:.2e} "
                      f"mean {e_m:.3f} fwd {e_z:.3f} ({e_zp:.2e}) vjp {e_v:.2e} / {vbound:.1e} (yardstick {yard:.2e})")
                if not (e_r <= gn_ref.STAT_TOL and e_m <= 1.0 and e_z <= 1.0 and e_v <= vbound):
                    bad.append((act, single, e_r, e_m, e_z, e_v, vbound))
    finally:
        lib.sp_groupnorm_single_pass(prev)
    assert not bad, bad


def _is(name: str, kernel: str, v: int | None = None) -> bool:
    """``name`` (demangled or mangled) is kernel template ``kernel`` (with first argument v)."""
    if v is None:
        return kernel + "<" in name or f"{len(kernel)}{kernel}I" in name
    return f"{kernel}<{v}" in name or f"{len(kernel)}{kernel}ILi{v}E" in name


@pytest.mark.parametrize("entry", gn_ref.SHAPES, ids=gn_ref.shape_id)
def test_each_shape_takes_its_path(cuda, entry):
    """The kernels each shape launches, from the profiler: with the single-pass kernels enabled
    the forward / backward named in gn_ref.PATHS (a shape that silently fell back would pass the
    comparison for the wrong reason), with them disabled the two-pass pairs, float4 or scalar."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    shape, c1, _ = entry
    v, fwd_single, bwd_single = gn_ref.expected_paths(entry)
    t = gn_ref.make_case(1, shape)
    dev = _device_inputs(t, c1, cuda)
    layer = _layer(t, shape[1], True, cuda)
    _run(layer, dev)  # allocations and the team region outside the profile
    prev = lib.sp_groupnorm_single_pass(-1)
    try:
        for single in (0, 1):
            lib.sp_groupnorm_single_pass(single)
            names = {nm for nm in _kernel_names(lambda: _run(layer, dev)) if "k_gn_" in nm}

            def ran(kernel, vv=None):
                return any(_is(nm, kernel, vv) for nm in names)

            fs, bs = bool(single and fwd_single), bool(single and bwd_single)
            assert ran("k_gn_fwd_pipe") == fs, names
            assert ran("k_gn_bwd_pipe") == bs, names
            assert (ran("k_gn_stats", v) and ran("k_gn_apply", v)) == (not fs), names
            assert (ran("k_gn_bwd_stats", v) and ran("k_gn_bwd_apply", v)) == (not bs), names
            other = 1 if v == 4 else 4
            assert not any(ran(k, other) for k in ("k_gn_stats", "k_gn_apply", "k_gn_bwd_stats", "k_gn_bwd_apply")), names
            if fs:
                assert not ran("k_gn_stats") and not ran("k_gn_apply"), names
            if bs:
                assert not ran("k_gn_bwd_stats") and not ran("k_gn_bwd_apply"), names
    finally:
        lib.sp_groupnorm_single_pass(prev)


def test_too_many_groups_is_rejected_without_a_launch(cuda):
    """n * groups = 65536 (the grid's y extent) is SP_EINVAL from both directions, one- and
    two-part, and nothing is launched: the outputs keep their fill."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    n, c, hw, groups = 32768, 2, 4, 2
    assert n * groups == 65536
    x = torch.randn(n, c, 2, 2, device=cuda)
    x1, x2 = x[:, :1].contiguous(), x[:, 1:].contiguous()
    z = torch.full_like(x, 7.0)
    dx, dx2 = torch.full_like(x, 7.0), torch.full_like(x2, 7.0)
    stats = torch.full((2, n * groups), 7.0, device=cuda)
    work = torch.zeros(max(int(lib.sp_groupnorm_workspace(n, c, hw, groups)), 1), device=cuda)
    p, s = _hip.ptr, _hip.stream_of(x)
    sp = p(stats)

    def calls():
        rcs = []
        for xa, xb, c1 in ((x, None, c), (x1, x2, 1)):
            rcs.append(lib.sp_groupnorm_silu_fwd2(p(xa), p(xb), c1, None, None, None, n, c, hw, groups, 1e-6, 1,
                                                  p(z), sp, sp + 4 * n * groups, p(work), None, 0, s))
            rcs.append(lib.sp_groupnorm_silu_bwd2(p(z), p(xa), p(xb), c1, None, None, None, sp, sp + 4 * n * groups,
                                                  n, c, hw, groups, 1, p(dx), p(dx2) if xb is not None else None,
                                                  None, None, None, p(work), None, 0, s))
        return rcs

    rcs = []
    names = _kernel_names(lambda: rcs.extend(calls()))
    assert rcs == [SP_EINVAL] * 4
    assert not {nm for nm in names if "k_gn_" in nm or "sp::" in nm}, names
    assert all(bool((v == 7.0).all()) for v in (z, dx, dx2, stats)) and int(work.count_nonzero()) == 0
    # one group fewer is served
    n -= 1
    rc = lib.sp_groupnorm_silu_fwd2(p(x), None, c, None, None, None, n, c, hw, groups, 1e-6, 1, p(z), sp,
                                    sp + 4 * n * groups, p(work), None, 0, s)
    torch.cuda.synchronize()
    assert rc == 0 and bool((z[:n] != 7.0).any()) and bool((z[n:] == 7.0).all())
