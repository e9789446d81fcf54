"""The fp32 3x3 convolution tiles (csrc/sp_wino.hip, sp_conv.hip, sp_conv_s2.hip, sp_conv_thin.hip) held
to bit-exact integer cases, and per output on real-valued data.

tests/test_conv_gpu.py bounds one relative-L2 number per tensor on randn data, with 25-40x slack on the
Winograd tile: a few wrong outputs among 10^5 (a halo cell at a tile seam, a neighbour image's row in
the 8 x 8 mosaic, the last output-channel block, a k-step skipped or doubled at a ring wrap) pass it.
Here the operands are small integers (tests/exact_cases.py; tests/test_exact_cases.py shows on the CPU
that the fp64 reference is an fp32 number and that no order of summation can round), so a correct
kernel returns the reference bit for bit: ``torch.equal``, every output judged.  Every case calls the
raw entry points, writes into a NaN-filled output inside a buffer whose guard bands (at least one
image; four at 8 x 8, where a workgroup's mosaic reaches past the batch) hold a fixed bit pattern, and
asserts equality, no NaN left, bands untouched.

Channel counts follow the kernels' rules: the input VJP of a layer contracts over its cout and needs
the output-channel multiple on its cin, so a shape (n, K, C, h, w) runs the forward of a K -> C layer
and the input VJP of a C -> K layer (``swapped``): both contract over K and produce C channels.

The second half judges the same kernels per output on randn, 30 + randn and channels scaled by 2^+-12:
rho = |y - y64| / (2^-24 E), E the algorithm's envelope (Winograd: the algebra on absolute values),
against the fp32 emulation of the same algorithm on the same operands: max rho <= 4 x the emulation's
(accumulation order within a k-step, fma contraction, the max over up to 10^5 outputs) and relative
L2 <= 2 x the emulation's; the direct tiles also rho <= 9 K + 2 (their fmaf chain's length).
Measured on an MI355X (worst case per family, GPU / emulation): see README "Exact cases".
"""

from __future__ import annotations

import pytest
import torch

import exact_cases as ec
from samplers_amd import _hip

pytestmark = pytest.mark.gpu

ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)  # noqa: E731


class Runner:
    """The raw entry points on a case's operands; every output through a Guarded buffer."""

    def __init__(self, cuda):
        self.lib = _hip.load_library()
        self.cuda = cuda
        self.st = torch.cuda.current_stream().cuda_stream

    def dev(self, t):
        return None if t is None else t.to(self.cuda).contiguous()

    def out(self, shape):
        n, c, h, w = shape
        return ec.Guarded(shape, (4 if h * w <= 64 else 1) * c * h * w, self.cuda)

    def call(self, name, *args):
        _hip.check(getattr(self.lib, name)(*args), name)

    def done(self, *bufs):
        torch.cuda.synchronize()
        outs = [b.check() for b in bufs]
        return outs[0] if len(outs) == 1 else outs

    def packed(self, family, w, vjp):
        """w [cout][cin][3][3] packed for ``family``'s forward (vjp 0) or input VJP (vjp 1)."""
        cout, cin = w.shape[:2]
        wg = self.dev(w)
        if family == "thin":
            return wg
        pk = torch.empty(cin * cout * (16 if family == "wino" else 9), device=self.cuda)
        name = {"wino": "sp_wino3x3_pack", "direct": "sp_conv3x3_pack", "s2": "sp_conv3x3_s2_pack"}[family]
        self.call(name, wg.data_ptr(), cout, cin, vjp, pk.data_ptr(), self.st)
        return pk

    def workspace(self, nbytes, plane):
        return ec.Guarded((max(nbytes // 4, 1),), plane, self.cuda)

    # family: wino (entry fwd / fwd_res / fwd_ws / fwd_up), direct, s2 (entry fwd / fwd_ws), thin
    def forward(self, family, shape, x, w, bias=None, res=None, entry="fwd", ws_bytes=0):
        n, cin, cout, h, wd = shape
        lib, st, p = self.lib, self.st, _hip.ptr
        xg, pk, bg, rg = self.dev(x), self.packed(family, w, 0), self.dev(bias), self.dev(res)
        y = self.out((n, cout, h // 2, wd // 2) if family == "s2" else (n, cout, h, wd))
        ws = None
        if family == "wino" and entry == "fwd":
            assert res is None
            self.call("sp_wino3x3_fwd", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), st)
        elif family == "wino" and entry == "fwd_res":
            self.call("sp_wino3x3_fwd_res", p(xg), p(pk), p(bg), p(rg), n, cin, cout, h, wd, y.ptr(), st)
        elif family == "wino" and entry == "fwd_ws":
            ws = self.workspace(ws_bytes, h * wd)
            self.call("sp_wino3x3_fwd_ws", p(xg), p(pk), p(bg), p(rg), n, cin, cout, h, wd, y.ptr(), ws.ptr(),
                      ws_bytes, st)
        elif family == "wino" and entry == "fwd_up":
            assert res is None and lib.sp_wino3x3_up_supported(cin, cout, h, wd)
            self.call("sp_wino3x3_fwd_up", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), st)
        elif family == "direct":
            assert res is None and lib.sp_conv3x3_supported(cin, cout, h, wd)
            self.call("sp_conv3x3_fwd", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), st)
        elif family == "s2" and entry == "fwd":
            assert res is None and lib.sp_conv3x3_s2_supported(cin, cout, h, wd, 0)
            self.call("sp_conv3x3_s2_fwd", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), st)
        elif family == "s2" and entry == "fwd_ws":
            ws = self.workspace(ws_bytes, h * wd // 4)
            self.call("sp_conv3x3_s2_fwd_ws", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), ws.ptr(), ws_bytes, st)
        elif family == "thin":
            assert res is None and lib.sp_conv3x3_thin_supported(cin, cout, h, wd)
            self.call("sp_conv3x3_thin_fwd", p(xg), p(pk), p(bg), n, cin, cout, h, wd, y.ptr(), st)
        else:
            raise ValueError((family, entry))
        out = self.done(y)
        if ws is not None:
            ws.check(nan_ok=True)
        return out

    # entry: bwd / bwd_ws / bwd_pool (wino), bwd / bwd_acc / bwd_ws / bwd_ws_acc (s2; base = dx before)
    def vjp(self, family, shape, dy, w, entry="bwd", ws_bytes=0, base=None):
        n, cin, cout, h, wd = shape
        st, p = self.st, _hip.ptr
        dyg, pk = self.dev(dy), self.packed(family, w, 1)
        dx = self.out((n, cin, h // 2, wd // 2) if entry == "bwd_pool" else (n, cin, h, wd))
        if base is not None:
            dx.t.copy_(base)
        ws = None
        acc = 1 if entry.endswith("acc") else 0
        if family == "wino" and entry == "bwd":
            self.call("sp_wino3x3_bwd_input", p(dyg), p(pk), n, cin, cout, h, wd, dx.ptr(), st)
        elif family == "wino" and entry == "bwd_ws":
            ws = self.workspace(ws_bytes, h * wd)
            self.call("sp_wino3x3_bwd_input_ws", p(dyg), p(pk), n, cin, cout, h, wd, dx.ptr(), ws.ptr(), ws_bytes, st)
        elif family == "wino" and entry == "bwd_pool":
            self.call("sp_wino3x3_bwd_input_pool", p(dyg), p(pk), n, cin, cout, h, wd, dx.ptr(), st)
        elif family == "direct":
            self.call("sp_conv3x3_bwd_input", p(dyg), p(pk), n, cin, cout, h, wd, dx.ptr(), st)
        elif family == "s2" and entry in ("bwd", "bwd_acc"):
            assert self.lib.sp_conv3x3_s2_supported(cin, cout, h, wd, 1)
            self.call("sp_conv3x3_s2_bwd_input", p(dyg), p(pk), n, cin, cout, h, wd, acc, dx.ptr(), st)
        elif family == "s2" and entry in ("bwd_ws", "bwd_ws_acc"):
            ws = self.workspace(ws_bytes, h * wd)
            self.call("sp_conv3x3_s2_bwd_input_ws", p(dyg), p(pk), n, cin, cout, h, wd, acc, dx.ptr(), ws.ptr(),
                      ws_bytes, st)
        elif family == "thin":
            self.call("sp_conv3x3_thin_bwd_input", p(dyg), p(pk), n, cin, cout, h, wd, dx.ptr(), st)
        else:
            raise ValueError((family, entry))
        out = self.done(dx)
        if ws is not None:
            ws.check(nan_ok=True)
        return out


@pytest.fixture(scope="module")
def run(cuda):
    return Runner(cuda)


def _no_res(c):
    return c.y64 - c.res.double()


def _wino_unsplit(run, shape, impulse=False):
    """Forward without and with residual of the K -> C layer, input VJP of the C -> K layer."""
    n, cin, cout, h, w = shape
    assert run.lib.sp_wino3x3_supported(cin, cout, h, w)
    make = ec.impulse_conv_case if impulse else ec.int_conv_case
    c, cv = make(shape), make(ec.swapped(shape))
    ec.assert_bitwise(run.forward("wino", shape, c.x, c.w, c.bias), _no_res(c), f"sp_wino3x3_fwd {shape}")
    ec.assert_bitwise(run.forward("wino", shape, c.x, c.w, c.bias, c.res, "fwd_res"), c.y64,
                      f"sp_wino3x3_fwd_res {shape}")
    ec.assert_bitwise(run.vjp("wino", cv.shape, cv.dy, cv.w), cv.dx64, f"sp_wino3x3_bwd_input {cv.shape}")


@pytest.mark.parametrize("shape", ec.WINO_W32, ids=ids)
def test_wino_w32_geometry_is_exact(run, shape):
    """W % 32 == 0, unsplit (no workspace): cin % 8 == 0 and cin >= 16, so wino3x3() launches
    k_wino3x3_xi<RES, 16> (RES = false for sp_wino3x3_fwd and _bwd_input, true for _fwd_res).  cin 16:
    the xi ring's first and last blocks only, 24: one middle block, 40: three; cout 64 / 128: one and
    two output-channel blocks; 8 / 24 / 16 rows: one to three workgroup rows, 32 / 64 / 96 columns."""
    _wino_unsplit(run, shape)


@pytest.mark.parametrize("shape", ec.WINO_W16, ids=ids)
def test_wino_w16_geometry_is_exact(run, shape):
    """W == 16, unsplit: the narrow branch with cin % 8 == 0, cin >= 16: k_wino3x3_xi<RES, 8>
    (4 x 8 tiles per wave, 16 x 16 outputs per workgroup); 16 and 48 rows: one and three workgroups
    per image."""
    _wino_unsplit(run, shape)


@pytest.mark.parametrize("shape", ec.WINO_MOSAIC, ids=ids)
def test_wino_mosaic_is_exact_for_every_batch_remainder(run, shape):
    """8 x 8 images, unsplit: k_wino3x3_r<RES, 8, true> (MOSAIC: four images per workgroup).  Batches
    1, 2, 3, 4, 5, 7: every count of images a workgroup's mosaic can hold, the last one partly past
    the batch: the guard bands (four images) show a store for an image that does not exist."""
    _wino_unsplit(run, shape)


@pytest.mark.parametrize("kind,shape", ec.IMPULSE, ids=ids)
def test_impulses_see_zero_halos(run, kind, shape):
    """Unit impulses at the corners, edge midpoints and both sides of every workgroup / wave seam into a
    zero input, bias 0: each output is one weight, a sum of a few, or exactly 0 (more than half are), so
    a halo cell holding a neighbour tile's, a neighbour image's (the mosaic) or a wrapped pixel shows.
    Each shape on the kernel its family's test names: the Winograd tiles where sp_wino3x3_supported
    (k_wino3x3_xi<false, 16> / <false, 8>, k_wino3x3_r<false, 8, true>), k_conv3x3 (cin 132), the thin
    kernel (cin 3), k_conv3x3_s2 (impulses in the last row and column, next to the zero pad), and the
    fused upsample (k_wino3x3_xi<false, 16, 1>)."""
    n, cin, cout, h, w = shape
    c = ec.impulse_conv_case(shape, kind=kind)
    if kind == "s2":
        fam, entry = "s2", "fwd"
    elif kind == "up":
        fam, entry = "wino", "fwd_up"
    else:
        fam = "wino" if run.lib.sp_wino3x3_supported(cin, cout, h, w) else \
            "direct" if run.lib.sp_conv3x3_supported(cin, cout, h, w) else "thin"
        entry = "fwd"
    ec.assert_bitwise(run.forward(fam, shape, c.x, c.w, c.bias, None, entry), c.y64, f"{fam} {entry} {shape}")
    if kind == "s1" and fam == "wino":
        cv = ec.impulse_conv_case(ec.swapped(shape))
        ec.assert_bitwise(run.vjp("wino", cv.shape, cv.dy, cv.w), cv.dx64, f"wino vjp {cv.shape}")


def _parts(lib, shape):
    n, cin, cout, h, w = shape
    nb = int(lib.sp_wino3x3_workspace(n, cin, cout, h, w))
    assert nb % (4 * n * cout * h * w) == 0
    return nb // (4 * n * cout * h * w), nb


def test_wino_split_cases_reach_every_part_count(run):
    """wino_ksplit doubles the parts while every part keeps two rings of k-steps: one tile (n = 1,
    cout = 64) gets 2 parts at cin 32, 4 at 64 and 96, 8 at 128, 16 at 256, 32 (SP_WINO_SPLITK) from 512."""
    assert {_parts(run.lib, s)[0] for s in ec.WINO_SPLIT} == {2, 4, 8, 16, 32}
    assert _parts(run.lib, (1, 1024, 64, 8, 32))[0] == 32


@pytest.mark.parametrize("shape", ec.WINO_SPLIT, ids=ids)
def test_wino_split_k_is_exact(run, shape):
    """sp_wino3x3_fwd_ws / _bwd_input_ws with the workspace sp_wino3x3_workspace asks for: ksplit > 1, so
    k_wino3x3_r<false, 8, true, true> (8 x 8), <false, 8, false, true> (16 x 16) or <false, 16, false, true>
    (8 x 32) store the parts and k_wino_split_reduce adds them with the bias and the residual.  The
    workspace is NaN-filled (an unwritten part would reach the output) between guard bands.  A workspace
    one float short runs unsplit (k_wino3x3_xi / the mosaic tile) and is exact as well."""
    parts, nb = _parts(run.lib, shape)
    assert parts >= 2
    c, cv = ec.int_conv_case(shape), ec.int_conv_case(ec.swapped(shape))
    for nbytes, what in ((nb, f"{parts} parts"), (nb - 4, "short workspace, unsplit")):
        ec.assert_bitwise(run.forward("wino", shape, c.x, c.w, c.bias, c.res, "fwd_ws", nbytes), c.y64,
                          f"sp_wino3x3_fwd_ws {shape} {what}")
        ec.assert_bitwise(run.vjp("wino", cv.shape, cv.dy, cv.w, "bwd_ws", nbytes), cv.dx64,
                          f"sp_wino3x3_bwd_input_ws {cv.shape} {what}")


@pytest.mark.parametrize("shape", ec.WINO_UP, ids=ids)
def test_wino_fused_upsample_and_pool_are_exact(run, shape):
    """sp_wino3x3_fwd_up: k_wino3x3_xi<false, 16, 1> (the 9 live GEMMs on the half-resolution source);
    sp_wino3x3_bwd_input_pool: k_wino3x3_xi<false, 16, 2> (the 2 x 2 block sum in the epilogue).  The
    smallest sp_wino3x3_up_supported shapes (both channel counts % 64, 32-column geometry), against
    conv2d(interpolate(x)) and its VJP."""
    c = ec.int_conv_case(shape, kind="up")
    ec.assert_bitwise(run.forward("wino", shape, c.x, c.w, c.bias, None, "fwd_up"), c.y64, f"sp_wino3x3_fwd_up {shape}")
    ec.assert_bitwise(run.vjp("wino", shape, c.dy, c.w, "bwd_pool"), c.dx64, f"sp_wino3x3_bwd_input_pool {shape}")


@pytest.mark.parametrize("shape", ec.DIRECT, ids=ids)
def test_direct_tile_is_exact(run, shape):
    """sp_conv3x3_fwd / _bwd_input: k_conv3x3 (cin % 4, cout % 128, h % 8, w % 32); cin 4 and 12: one and
    three channel chunks, 132: not a multiple of 8 or 16; the VJP as the forward of the swapped layer."""
    c, cv = ec.int_conv_case(shape), ec.int_conv_case(ec.swapped(shape))
    ec.assert_bitwise(run.forward("direct", shape, c.x, c.w, c.bias), _no_res(c), f"sp_conv3x3_fwd {shape}")
    ec.assert_bitwise(run.vjp("direct", cv.shape, cv.dy, cv.w), cv.dx64, f"sp_conv3x3_bwd_input {cv.shape}")


@pytest.mark.parametrize("shape", ec.S2_FWD, ids=ids)
def test_stride2_forward_is_exact(run, shape):
    """sp_conv3x3_s2_fwd: k_conv3x3_s2, against conv2d(pad(x, (0, 1, 0, 1)), stride 2); and the _ws form
    where sp_conv3x3_s2_workspace > 0 (cin 32 at one workgroup: two parts + k_s2_split_reduce)."""
    n, cin, cout, h, w = shape
    c = ec.int_conv_case(shape, kind="s2")
    ec.assert_bitwise(run.forward("s2", shape, c.x, c.w, c.bias), c.y64, f"sp_conv3x3_s2_fwd {shape}")
    nb = int(run.lib.sp_conv3x3_s2_workspace(n, cin, cout, h, w, 0))
    assert (nb > 0) == (cin == 32)
    if nb:
        ec.assert_bitwise(run.forward("s2", shape, c.x, c.w, c.bias, None, "fwd_ws", nb), c.y64,
                          f"sp_conv3x3_s2_fwd_ws {shape}")


@pytest.mark.parametrize("shape", ec.S2_VJP, ids=ids)
def test_stride2_input_vjp_is_exact(run, shape):
    """sp_conv3x3_s2_bwd_input: k_conv3x3_s2_bwd, accumulate 0 and 1 (dx = base + conv^T dy, base integer),
    and the _ws forms where the workspace query is positive."""
    n, cin, cout, h, w = shape
    c = ec.int_conv_case(shape, kind="s2")
    base = torch.randint(-4, 5, c.x.shape, generator=ec.gen(sum(shape))).float()
    ec.assert_bitwise(run.vjp("s2", shape, c.dy, c.w), c.dx64, f"sp_conv3x3_s2_bwd_input {shape}")
    ec.assert_bitwise(run.vjp("s2", shape, c.dy, c.w, "bwd_acc", base=base), c.dx64 + base.double(),
                      f"sp_conv3x3_s2_bwd_input accumulate {shape}")
    nb = int(run.lib.sp_conv3x3_s2_workspace(n, cin, cout, h, w, 1))
    if nb:
        ec.assert_bitwise(run.vjp("s2", shape, c.dy, c.w, "bwd_ws", nb), c.dx64, f"sp_conv3x3_s2_bwd_input_ws {shape}")
        ec.assert_bitwise(run.vjp("s2", shape, c.dy, c.w, "bwd_ws_acc", nb, base=base), c.dx64 + base.double(),
                          f"sp_conv3x3_s2_bwd_input_ws accumulate {shape}")


@pytest.mark.parametrize("shape", ec.THIN, ids=ids)
def test_thin_kernel_is_exact(run, shape):
    """sp_conv3x3_thin_fwd / _bwd_input (VALU, raw weights): one pixel row of four, ragged tiles
    (h % 8, w % 64 != 0), 200 channels on either side."""
    c = ec.int_conv_case(shape)
    ec.assert_bitwise(run.forward("thin", shape, c.x, c.w, c.bias), _no_res(c), f"sp_conv3x3_thin_fwd {shape}")
    ec.assert_bitwise(run.vjp("thin", shape, c.dy, c.w), c.dx64, f"sp_conv3x3_thin_bwd_input {shape}")


# --- the Python dispatch (packing cache, workspace sizing) hands the same bits through ------------


def _module(c, stride, padding, cuda):
    from samplers_amd.networks.layers import Conv3x3

    cout, cin = c.w.shape[:2]
    m = Conv3x3(cin, cout) if stride == 1 else torch.nn.Conv2d(cin, cout, 3, stride=2, padding=padding)
    with torch.no_grad():
        m.weight.copy_(c.w)
        m.bias.copy_(c.bias)
    return m.to(cuda).requires_grad_(False)


def test_module_conv3x3_is_exact(cuda):
    """conv3x3_forward (bias + residual) / conv3x3_input_vjp at 64 -> 64, 16 x 16, one image: the Winograd
    tile with the workspace _wino_workspace sizes (4 parts)."""
    from samplers_amd.networks.layers import conv3x3_forward, conv3x3_input_vjp

    c = ec.int_conv_case((1, 64, 64, 16, 16))
    m = _module(c, 1, 1, cuda)
    ec.assert_bitwise(conv3x3_forward(m, c.x.to(cuda), res=c.res.to(cuda)), c.y64, "conv3x3_forward")
    ec.assert_bitwise(conv3x3_input_vjp(m, c.dy.to(cuda), c.x.shape), c.dx64, "conv3x3_input_vjp")


def test_module_downsample_conv_is_exact(cuda):
    """downsample_conv at 128 -> 128, 16 x 64: the stride-2 tiles both ways (downsample_s2_supported)."""
    from samplers_amd.networks.layers import downsample_conv, downsample_s2_supported

    c = ec.int_conv_case((1, 128, 128, 16, 64), kind="s2")
    m = _module(c, 2, 0, cuda)
    x = c.x.to(cuda).requires_grad_()
    assert downsample_s2_supported(m, x)
    y = downsample_conv(m, x)
    (dx,) = torch.autograd.grad(y, x, c.dy.to(cuda))
    ec.assert_bitwise(y, c.y64, "downsample_conv")
    ec.assert_bitwise(dx, c.dx64, "downsample_conv VJP")


@pytest.mark.parametrize("padding", [1, 0])
def test_module_conv3x3_stride2_is_exact(cuda, padding):
    """conv3x3_stride2 at 64 -> 64, 16 x 16 (no stride-2 tile: the Winograd tile at full resolution read
    at the even (padding 1) or odd (padding 0) positions; the VJP scatters dy there)."""
    import torch.nn.functional as F

    from samplers_amd.networks.layers import conv3x3_stride2, strided_full_supported

    c = ec.int_conv_case((1, 64, 64, 16, 16), seed=padding)
    m = _module(c, 2, padding, cuda)
    x = c.x.to(cuda).requires_grad_()
    assert strided_full_supported(m, x)
    y = conv3x3_stride2(m, x, padding)
    dy = c.dy[:, :, ::2, ::2].contiguous()
    (dx,) = torch.autograd.grad(y, x, dy.to(cuda))
    xd = c.x.double().requires_grad_()
    ref = F.conv2d(xd if padding else F.pad(xd, (0, 1, 0, 1)), c.w.double(), c.bias.double(), stride=2, padding=padding)
    (gref,) = torch.autograd.grad(ref, xd, dy.double())
    ec.assert_bitwise(y, ref.detach(), f"conv3x3_stride2 padding {padding}")
    ec.assert_bitwise(dx, gref, f"conv3x3_stride2 VJP padding {padding}")


# --- metamorphic checks on real-valued data: no tolerance ------------------------------------

FAMILY_SHAPES = [  # family, entry, shape: one per kernel the dispatch reaches
    ("wino", "fwd", (3, 16, 64, 8, 32)), ("wino", "fwd", (3, 16, 64, 16, 16)), ("wino", "fwd", (5, 24, 128, 8, 8)),
    ("wino", "fwd_ws", (1, 128, 64, 8, 32)), ("wino", "fwd_up", (1, 64, 64, 32, 32)),
    ("direct", "fwd", (2, 4, 128, 8, 32)), ("s2", "fwd", (1, 4, 128, 16, 64)), ("thin", "fwd", (2, 3, 5, 9, 68)),
]


def _kind(family, entry):
    return "s2" if family == "s2" else "up" if entry == "fwd_up" else "s1"


@pytest.mark.parametrize("family,entry,shape", FAMILY_SHAPES, ids=ids)
def test_power_of_two_scaling_is_bitwise(run, family, entry, shape):
    """x times 2^7 and w times 2^-3 (bias and residual zero) scales every product, partial sum and
    transform by 2^4 without a rounding changing: every output is 2^4 times the unscaled one, bit for
    bit, on randn data."""
    c = ec.real_conv_case(shape, "randn", kind=_kind(family, entry))
    nb = _parts(run.lib, shape)[1] if entry == "fwd_ws" else 0
    y0 = run.forward(family, shape, c.x, c.w, None, None, entry, nb)
    y1 = run.forward(family, shape, c.x * 2.0 ** 7, c.w * 2.0 ** -3, None, None, entry, nb)
    assert torch.equal(y1, y0 * 16.0)


@pytest.mark.parametrize("family,entry,shape", [f for f in FAMILY_SHAPES if f[2][0] > 1] +
                         [("wino", "fwd", (7, 16, 64, 8, 8))], ids=ids)
def test_batch_permutation_is_bitwise(run, family, entry, shape):
    """The unsplit launches treat images alike: permuting the batch permutes the outputs bit for bit
    (in the mosaic an image changes its place in a workgroup's 2 x 2 arrangement and its neighbours)."""
    c = ec.real_conv_case(shape, "randn", seed=1, kind=_kind(family, entry))
    perm = torch.randperm(shape[0], generator=ec.gen(shape[0]))
    if shape[0] > 1 and torch.equal(perm, torch.arange(shape[0])):
        perm = perm.flip(0)
    y0 = run.forward(family, shape, c.x, c.w, c.bias, None, entry)
    y1 = run.forward(family, shape, c.x[perm].contiguous(), c.w, c.bias, None, entry)
    assert torch.equal(y1, y0[perm])


# --- per-output bound on real-valued data against the algorithm's own fp32 emulation ------------

RHO_CASES = [  # family, forward entry, VJP entry, shape
    ("wino", "fwd_res", "bwd", (3, 16, 64, 8, 32)), ("wino", "fwd_res", "bwd", (2, 24, 128, 48, 16)),
    ("wino", "fwd_res", "bwd", (5, 24, 128, 8, 8)), ("wino", "fwd_ws", "bwd_ws", (1, 128, 64, 8, 32)),
    ("wino", "fwd_up", "bwd_pool", (1, 64, 64, 32, 32)),
    ("direct", "fwd", "bwd", (1, 12, 256, 16, 64)), ("s2", "fwd", None, (2, 12, 256, 32, 64)),
    ("s2", None, "bwd", (1, 128, 4, 4, 64)), ("thin", "fwd", "bwd", (2, 3, 5, 9, 68)),
]


@pytest.mark.parametrize("field", ec.FIELDS)
@pytest.mark.parametrize("family,fentry,ventry,shape", RHO_CASES, ids=ids)
def test_every_output_within_the_emulations_error(run, parity_record, family, fentry, ventry, shape, field):
    """max rho(GPU) <= 4 max rho(emulation) and relative L2 <= 2 x the emulation's, forward (with bias; with
    residual where the entry takes one) and input VJP; direct, stride-2 and thin kernels also
    rho <= 9 K + 2, the length of their fmaf chain (K the contraction's channels)."""
    kind = _kind(family, fentry or "")
    algo = ec.emu_wino if family == "wino" else ec.emu_direct
    split = (fentry or ventry).endswith("ws")
    swap = family in ("wino", "direct") and kind == "s1"
    n, cin, cout, h, w = shape
    jobs = []
    if fentry:
        c = ec.real_conv_case(shape, field, kind=kind)
        with_res = fentry in ("fwd_res", "fwd_ws")
        if not with_res:
            c.y64, c.res = c.y64 - c.res.double(), torch.zeros_like(c.res)
        got = run.forward(family, shape, c.x, c.w, c.bias, c.res if with_res else None, fentry,
                          _parts(run.lib, shape)[1] if split else 0)
        jobs.append(("fwd", got, c.y64, ec.emu_forward(c, algo), ec.emu_forward(c, algo, dtype=torch.float64, absolute=True), cin))
    if ventry:
        c = ec.real_conv_case(ec.swapped(shape) if swap else shape, field, seed=1, kind=kind)
        got = run.vjp(family, c.shape, c.dy, c.w, ventry, _parts(run.lib, shape)[1] if split else 0)
        jobs.append(("vjp", got, c.dx64, ec.emu_vjp(c, algo), ec.emu_vjp(c, algo, dtype=torch.float64, absolute=True),
                     c.shape[2]))
    for what, got, y64, emu, env, k in jobs:
        got = got.cpu()
        r_gpu, r_emu = ec.rho(got, y64, env), ec.rho(emu, y64, env)
        l_gpu, l_emu = ec.rel_l2(got, y64), ec.rel_l2(emu, y64)
        parity_record(f"conv_{family}_{what}_rho", r_gpu, 4 * r_emu, shape=list(shape), field=field, emulation=r_emu)
        parity_record(f"conv_{family}_{what}_rel_l2", l_gpu, 2 * l_emu, shape=list(shape), field=field, emulation=l_emu)
        print(f"{family} {what} {shape} {field}: rho {r_gpu:.3f} (emulation {r_emu:.3f}), "
              f"rel L2 {l_gpu:.2e} (emulation {l_emu:.2e})")
        assert r_gpu <= 4 * r_emu, (what, r_gpu, r_emu)
        assert l_gpu <= 2 * l_emu, (what, l_gpu, l_emu)
        if family != "wino":
            assert r_gpu <= 9 * k + 2, (what, r_gpu, k)
