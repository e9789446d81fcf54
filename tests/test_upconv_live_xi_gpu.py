"""The fused upsample conv's forward on its 9 live ξ (csrc/sp_wino.hip, "Live-ξ forms";
sp_wino3x3_fwd_up): equal (``torch.equal``) to the 16-GEMM tile on the materialised upsample,
finite, and within the Winograd tile's usual bound of fp64 conv2d(interpolate(x)); cin != cout,
one and several tiles per workgroup, with and without a bias; the executed-FLOP record; and
the debug build's check of the duplicated window rows / columns the skip rests on."""

from __future__ import annotations

import functools
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from samplers_amd import _hip

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

SHAPES = [  # n, cin, cout, source h, w
    (1, 64, 64, 4, 16),      # one workgroup tile per image, touching all four borders
    (2, 64, 128, 8, 16),     # two channel-block workgroups, two tile rows
    (1, 128, 64, 4, 32),     # two tile columns, 64 k-steps
    (9, 128, 128, 32, 32),   # 288 tiles on 256 CUs: some workgroups walk two tiles
]


def _check(got, ref, slack=1):
    """test_conv_gpu.py::_check (slack 5: the Winograd tile's F(2,3) rounding)."""
    ref = ref.double()
    rel = ((got.double().cpu() - ref).norm() / ref.norm()).item()
    mx = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert rel < 2e-6 * slack and mx < 1e-5 * slack, (rel, mx)


@functools.lru_cache(maxsize=None)
def _operands(shape):
    """x, weight, bias and the fp64 reference without the bias (computed once per shape)."""
    n, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(sum(shape) + 3)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), wt.double(), None, padding=1)
    return x, wt, b, ref


def _run_pair(lib, cuda, shape, with_bias):
    from samplers_amd.networks.layers import upsample_nearest2x

    n, cin, cout, h, w = shape
    H, W = 2 * h, 2 * w
    assert lib.sp_wino3x3_up_supported(cin, cout, H, W)
    x, wt, b, _ = _operands(shape)
    st = torch.cuda.current_stream().cuda_stream
    xg, wg, bg = x.to(cuda), wt.to(cuda), b.to(cuda)
    bp = _hip.ptr(bg) if with_bias else None
    up = torch.empty(cin * cout * 16, device=cuda)
    assert lib.sp_wino3x3_pack(_hip.ptr(wg), cout, cin, 0, _hip.ptr(up), st) == 0
    y = torch.full((n, cout, H, W), float("nan"), device=cuda)
    assert lib.sp_wino3x3_fwd_up(_hip.ptr(xg), _hip.ptr(up), bp, n, cin, cout, H, W, _hip.ptr(y), st) == 0
    xu = upsample_nearest2x(xg).contiguous()
    yr = torch.full_like(y, float("nan"))
    assert lib.sp_wino3x3_fwd(_hip.ptr(xu), _hip.ptr(up), bp, n, cin, cout, H, W, _hip.ptr(yr), st) == 0
    torch.cuda.synchronize()
    return xg, up, bg, y, yr


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES)
def test_live_xi_forward_equals_the_full_tile_on_the_upsampled_image(cuda, shape, with_bias):
    lib = _hip.load_library()
    _, _, _, y, yr = _run_pair(lib, cuda, shape, with_bias)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(yr).all())
    assert torch.equal(y, yr)
    _, _, b, ref = _operands(shape)
    _check(y, ref + b.double().view(1, -1, 1, 1) if with_bias else ref, 5)


def test_live_xi_forward_repeats_bitwise_on_the_same_buffers(cuda):
    """Two tiles per workgroup: the second run finds the buffers and LDS as the first left them."""
    lib = _hip.load_library()
    shape = SHAPES[-1]
    n, cin, cout, h, w = shape
    xg, up, bg, y, _ = _run_pair(lib, cuda, shape, True)
    first = y.clone()
    st = torch.cuda.current_stream().cuda_stream
    assert lib.sp_wino3x3_fwd_up(_hip.ptr(xg), _hip.ptr(up), _hip.ptr(bg), n, cin, cout, 2 * h, 2 * w,
                                 _hip.ptr(y), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, first)


def test_live_xi_forward_records_the_flops_it_executes(cuda):
    from samplers_amd.samplers.dps import KernelTimer

    lib = _hip.load_library()
    n, cin, cout, h, w = SHAPES[1]
    H, W = 2 * h, 2 * w
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(n, cin, h, w, device=cuda)
    xu = torch.randn(n, cin, H, W, device=cuda)
    up = torch.empty(cin * cout * 16, device=cuda)
    wt = torch.randn(cout, cin, 3, 3, device=cuda)
    assert lib.sp_wino3x3_pack(_hip.ptr(wt), cout, cin, 0, _hip.ptr(up), st) == 0
    y = torch.empty(n, cout, H, W, device=cuda)
    timer = KernelTimer()
    try:
        assert lib.sp_wino3x3_fwd_up(_hip.ptr(x), _hip.ptr(up), None, n, cin, cout, H, W, _hip.ptr(y), st) == 0
        s = timer.summary()
        assert s["wino3x3_fwd"]["count"] == 1
        assert s["wino3x3_fwd"]["flops"] == 4.5 * n * cin * cout * H * W  # 9 GEMMs
        assert lib.sp_wino3x3_fwd(_hip.ptr(xu), _hip.ptr(up), None, n, cin, cout, H, W, _hip.ptr(y), st) == 0
        s = timer.summary()
        assert s["wino3x3_fwd"]["count"] == 1
        assert s["wino3x3_fwd"]["flops"] == 8.0 * n * cin * cout * H * W  # 16 GEMMs
    finally:
        timer.close()


CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
from samplers_amd.networks.layers import upsample_nearest2x
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
n, cin, cout, h, w = 1, 64, 64, 4, 16
g = torch.Generator().manual_seed(5)
x = torch.randn(n, cin, h, w, generator=g).to(dev)
wt = (torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5).to(dev)
b = (torch.randn(cout, generator=g) * 0.1).to(dev)
up = torch.empty(cin * cout * 16, device=dev)
_hip.check(lib.sp_wino3x3_pack(_hip.ptr(wt), cout, cin, 0, _hip.ptr(up), st), "pack")
y = torch.empty(n, cout, 2 * h, 2 * w, device=dev)
yr = torch.empty_like(y)
_hip.check(lib.sp_wino3x3_fwd_up(_hip.ptr(x), _hip.ptr(up), _hip.ptr(b), n, cin, cout, 2 * h, 2 * w,
                                 _hip.ptr(y), st), "fwd_up")
xu = upsample_nearest2x(x).contiguous()
_hip.check(lib.sp_wino3x3_fwd(_hip.ptr(xu), _hip.ptr(up), _hip.ptr(b), n, cin, cout, 2 * h, 2 * w,
                              _hip.ptr(yr), st), "fwd")
nv, site = _hip.debug_violations()
print("violations", nv, site, flush=True)
assert nv == 0, (nv, site)
assert torch.equal(y, yr)
print("live xi debug: clean", flush=True)
"""


def test_live_xi_debug_build_checks_the_duplicated_rows_and_columns(cuda):
    """The debug library's SP_DCHECK in the UP == 1 k-step (window rows 1, 2 and columns 1, 2
    bit-equal) runs on the one-tile shape and does not fire; a process holds one library, so a
    child loads the debug one."""
    if not _hip.DEBUG_LIB_PATH.exists():
        pytest.fail(f"{_hip.DEBUG_LIB_PATH} missing: run `make` (builds the debug library too)")
    env = dict(os.environ, SAMPLERS_HIP_LIB=str(_hip.DEBUG_LIB_PATH))
    out = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], env=env, capture_output=True,
                         text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "live xi debug: clean" in out.stdout
