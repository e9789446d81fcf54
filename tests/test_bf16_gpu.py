"""The priors at the reference's reduced precision (bf16) on this project's kernels
(``csrc/sp_bf16_*.hip`` through ``networks/bf16.py``).

The reference runs its priors in whatever ``torch_dtype`` it is given; its PSLD driver uses SD 1.5
in bf16 (``/root/reference/scripts/run_psld.py:14-20``, ``stable_diffusion.py:90-101``).  What is
pinned here, and at what tolerance (relative L2 unless said otherwise):

* each kernel against fp32 arithmetic on the same bf16-rounded operands: the kernels compute in
  fp32 and round once per output, so the bound is the bf16 rounding of the output (unit
  roundoff 2^-9; RMS of the relative rounding ~1.1e-3): conv / GroupNorm forward 3e-3, input VJPs
  5e-3, attention (P rounded to bf16 for the P V product as well) 1e-2;
* whole priors (SD 1.5 ε-UNet, VAE decode / encode, the ddpm-celebahq-256 UNet): bf16 on the GPU
  against the same bf16 modules on the CPU (torch's own bf16 layers: oneDNN convolutions, ATen
  GroupNorm / softmax), and both against the fp32 module: the GPU's bf16 error relative to fp32
  may be at most 1.5x the CPU bf16 error (+1e-3) — the device path is as close to the fp32
  network as torch's own bf16 run is (measured: 0.8x); the direct GPU-bf16 / CPU-bf16 distance is
  about the two independent bf16 errors combined (1e-2 .. 4.5e-2 over ~60 layers and their VJPs),
  bounded at 1e-1;
* a PSLD solve through the bf16 SD 1.5 priors against ``oracle/latent_loops.py`` driving the same
  bf16 modules on the CPU behind the same fp32 boundary (the sample, guidance and DDIM updates
  in fp32, the networks in bf16): bound ``PSLD_BF16_TOL``; the device kernels are asserted by name
  (no MIOpen convolution runs).
"""

from __future__ import annotations

import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stand_ins as si

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PSLD_BF16_TOL = 3e-2


def _rel(a, b) -> float:
    return si.relative_error(a.float().cpu(), b.float().cpu())


def _kernel_names(fn) -> set[str]:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type.name == "CUDA"}


def _no_miopen_conv(names: set[str]) -> None:
    """No MIOpen / torch convolution kernel ran (this project's sp:: kernels — the conv tile and its
    split-K reduce — are the only convolution code allowed)."""
    bad = {n for n in names if ("conv" in n.lower() or "miopen" in n.lower() or "igemm" in n.lower())
           and not n.startswith("sp::") and "void sp::" not in n}
    assert not bad, f"convolutions outside this project's kernels: {sorted(bad)[:5]}"


# ---- kernels ------------------------------------------------------------------------------------

CONV_SHAPES = [
    (2, 16, 64, 32, 32), (1, 320, 320, 64, 64), (3, 64, 128, 16, 16), (5, 32, 64, 8, 8),
    (2, 64, 64, 4, 4), (1, 4, 320, 32, 32), (2, 128, 3, 64, 64), (2, 320, 4, 32, 32), (1, 640, 1280, 8, 8),
]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_bf16_fwd_vjp_matches_fp32(cuda, shape, parity_record):
    from samplers_amd.networks.layers import Conv3x3

    n, cin, cout, h, w = shape
    torch.manual_seed(1)
    conv = Conv3x3(cin, cout).to(BF).requires_grad_(False)
    x = torch.randn(n, cin, h, w).to(BF)
    dy = torch.randn(n, cout, h, w).to(BF)
    g = copy.deepcopy(conv).to(cuda)
    xr = x.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        y = g(xr)
    (dx,) = torch.autograd.grad(y, xr, dy.to(cuda))
    assert y.dtype == BF and y.is_contiguous(memory_format=torch.channels_last)
    wf, bfv = conv.weight.float(), conv.bias.float()
    ref = F.conv2d(x.float(), wf, bfv, padding=1)
    ref_dx = torch.nn.grad.conv2d_input(x.shape, wf, dy.float(), padding=1)
    e, ed = _rel(y, ref), _rel(dx, ref_dx)
    parity_record("conv_bf16_rel_l2", e, 3e-3, shape=list(shape))
    parity_record("conv_bf16_vjp_rel_l2", ed, 5e-3, shape=list(shape))
    assert e < 3e-3 and ed < 5e-3, (e, ed)


def test_conv3x3_bf16_split_k_equals_unsplit_within_rounding(cuda):
    """The 8x8 / 16x16 levels split K (sp_conv3x3_bf16_workspace > 0): the fixed-order reduce is
    repeatable and agrees with the unsplit launch to the bf16 rounding of the output."""
    from samplers_amd import _hip
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import Conv3x3

    lib = _hip.load_library()
    torch.manual_seed(11)
    n, c, h = 32, 1280, 8
    assert lib.sp_conv3x3_bf16_workspace(n, c, c, h, h) > 0
    conv = Conv3x3(c, c).to(device=cuda, dtype=BF).requires_grad_(False)
    x = torch.randn(n, c, h, h, device=cuda).to(BF).contiguous(memory_format=torch.channels_last)
    res = torch.randn(n, c, h, h, device=cuda).to(BF).contiguous(memory_format=torch.channels_last)
    y1 = bf16.conv3x3(conv, x, res=res)
    y2 = bf16.conv3x3(conv, x, res=res)
    assert torch.equal(y1, y2)
    pk = bf16.conv_pack(conv, False)
    y0 = torch.empty_like(y1)
    b = conv.bias.float().contiguous()
    _hip.check(lib.sp_conv3x3_bf16(x.data_ptr(), pk.data_ptr(), b.data_ptr(), res.data_ptr(), n, c, c, h, h,
                                   y0.data_ptr(), _hip.stream_of(x)), "unsplit")
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), padding=1) + res.float()
    assert _rel(y1, ref) < 3e-3 and _rel(y0, ref) < 3e-3 and _rel(y1, y0) < 3e-3


def test_conv3x3_bf16_residual_and_repeatable(cuda):
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import Conv3x3

    torch.manual_seed(2)
    conv = Conv3x3(64, 128).to(device=cuda, dtype=BF).requires_grad_(False)
    x = torch.randn(2, 64, 32, 32, device=cuda).to(BF)
    res = torch.randn(2, 128, 32, 32, device=cuda).to(BF)
    y1 = bf16.conv3x3(conv, x, res=res)
    y2 = bf16.conv3x3(conv, x, res=res)
    assert torch.equal(y1, y2)  # fixed summation order
    ref = F.conv2d(x.float(), conv.weight.float(), conv.bias.float(), padding=1) + res.float()
    assert _rel(y1, ref) < 3e-3


@pytest.mark.parametrize("n,c,co,h", [(2, 320, 320, 32), (1, 128, 128, 64), (3, 64, 64, 8), (1, 1280, 1280, 4)])
def test_upsample_conv_bf16_fwd_vjp(cuda, n, c, co, h):
    """conv(upsample_nearest2x(x)) fused (sp_conv3x3_bf16_up) and its VJP (full-resolution input VJP
    + sp_pool2x2_bf16) against fp32 torch on the same bf16 operands."""
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import Conv3x3

    torch.manual_seed(9)
    conv = Conv3x3(c, co).to(BF).requires_grad_(False)
    x = torch.randn(n, c, h, h).to(BF)
    dy = torch.randn(n, co, 2 * h, 2 * h).to(BF)
    g = copy.deepcopy(conv).to(cuda)
    xr = x.to(cuda).requires_grad_(True)
    assert bf16.upsample_conv_supported(g, xr)
    with torch.enable_grad():
        y = bf16.upsample_conv3x3(g, xr)
    (dx,) = torch.autograd.grad(y, xr, dy.to(cuda))
    xf = x.float().requires_grad_(True)
    with torch.enable_grad():
        ref = F.conv2d(F.interpolate(xf, scale_factor=2.0, mode="nearest"), conv.weight.float(),
                       conv.bias.float(), padding=1)
    (rdx,) = torch.autograd.grad(ref, xf, dy.float())
    assert _rel(y, ref) < 3e-3 and _rel(dx, rdx) < 5e-3, (_rel(y, ref), _rel(dx, rdx))


@pytest.mark.parametrize("c1,c2,hw,act,bias", [(320, 0, 64, True, True), (640, 640, 16, True, False),
                                               (128, 0, 128, False, False), (1280, 1280, 8, True, True),
                                               (512, 0, 32, True, False)])
def test_groupnorm_bf16_fwd_vjp_matches_fp32(cuda, c1, c2, hw, act, bias, parity_record):
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import GroupNormAct

    torch.manual_seed(3)
    n, c = 3, c1 + c2
    norm = GroupNormAct(32, c, eps=1e-5, act=act)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(c))
        norm.bias.copy_(0.1 * torch.randn(c))
    norm = norm.to(device=cuda, dtype=BF).requires_grad_(False)
    x1 = (torch.randn(n, c1, hw, hw) * 2 + 3).to(BF)   # a mean far from 0: the shifted sums
    x2 = None if not c2 else (torch.randn(n, c2, hw, hw) - 1).to(BF)
    cb = (torch.randn(n, c) * 0.5).to(BF) if bias else None
    dz = torch.randn(n, c, hw, hw).to(BF)

    x1g = x1.to(cuda).requires_grad_(True)
    x2g = None if x2 is None else x2.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        z = bf16.group_norm(norm, x1g, x2g, None if cb is None else cb.to(cuda))
    grads = torch.autograd.grad(z, [t for t in (x1g, x2g) if t is not None], dz.to(cuda))

    xs = [x1.float().requires_grad_(True)] + ([] if x2 is None else [x2.float().requires_grad_(True)])
    with torch.enable_grad():
        xf = torch.cat(xs, 1)
        if cb is not None:
            xf = xf + cb.float()[:, :, None, None]
        ref = F.group_norm(xf, 32, norm.weight.float().cpu(), norm.bias.float().cpu(), 1e-5)
        if act:
            ref = F.silu(ref)
    rg = torch.autograd.grad(ref, xs, dz.float())
    e = _rel(z, ref)
    ev = max(_rel(a, b) for a, b in zip(grads, rg))
    parity_record("gn_bf16_rel_l2", e, 3e-3, c=[c1, c2], hw=hw)
    parity_record("gn_bf16_vjp_rel_l2", ev, 5e-3, c=[c1, c2], hw=hw)
    assert e < 3e-3 and ev < 5e-3, (e, ev)


def _attn_ref(q, k, v):
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    return torch.softmax(s, -1) @ v


@pytest.mark.parametrize("n,heads,d", [(4096, 8, 40), (1024, 8, 80), (256, 8, 160), (64, 8, 160), (448, 4, 64),
                                      (96, 8, 40)])
def test_attention_bf16_self_fwd_vjp(cuda, n, heads, d, parity_record):
    from samplers_amd.networks import bf16

    torch.manual_seed(4)
    b, c = 2, heads * d
    from samplers_amd import _hip

    if not (bf16.attention_supported(b, heads, n, n, d) and bf16.vjp_supported(b, heads, n, n, d)):
        pytest.skip("shape not served by the fused kernels")
    bf16_vjp = bool(_hip.load_library().sp_attention_bf16_bwd_supported(b, heads, n, n, d))
    qkv = torch.randn(b, n, 3 * c).to(BF)
    do = torch.randn(b, n, c).to(BF)
    g = qkv.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        o = bf16.self_attention(g, heads)
    (dg,) = torch.autograd.grad(o, g, do.to(cuda))
    qf = qkv.float().requires_grad_(True)
    with torch.enable_grad():
        q, k, v = (t.reshape(b, n, heads, d).transpose(1, 2) for t in qf.split(c, -1))
        ref = _attn_ref(q, k, v).transpose(1, 2).reshape(b, n, c)
    (rg,) = torch.autograd.grad(ref, qf, do.float())
    e, ev = _rel(o, ref), _rel(dg, rg)
    parity_record("attn_bf16_rel_l2", e, 1e-2, n=n, d=d)
    parity_record("attn_bf16_vjp_rel_l2", ev, 1e-2, n=n, d=d, bf16_vjp=bf16_vjp)
    assert e < 1e-2 and ev < 1e-2, (e, ev)


def test_attention_bf16_cross_77_context(cuda):
    from samplers_amd.networks import bf16

    torch.manual_seed(5)
    b, n, m, heads, d = 2, 1024, 77, 8, 80
    c = heads * d
    q = torch.randn(b, n, c).to(BF)
    k = torch.randn(1, m, c).to(BF)
    v = torch.randn(1, m, c).to(BF)
    do = torch.randn(b, n, c).to(BF)
    qg = q.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        o = bf16.cross_attention(qg, k.to(cuda), v.to(cuda), heads)
    (dq,) = torch.autograd.grad(o, qg, do.to(cuda))
    qf = q.float().requires_grad_(True)
    with torch.enable_grad():
        sp = lambda t, bb: t.reshape(bb, -1, heads, d).transpose(1, 2)  # noqa: E731
        ref = _attn_ref(sp(qf, b), sp(k.float(), 1), sp(v.float(), 1)).transpose(1, 2).reshape(b, n, c)
    (rq,) = torch.autograd.grad(ref, qf, do.float())
    assert _rel(o, ref) < 1e-2 and _rel(dq, rq) < 1e-2


def test_geglu_bf16_fwd_vjp(cuda, parity_record):
    """sp_geglu_bf16_fwd / _bwd vs the fp32 torch GEGLU of the same bf16 inputs (one rounding of
    the result each way), and the kernel runs instead of torch's gelu / cat."""
    from samplers_amd.networks.layers import geglu

    gen = torch.Generator().manual_seed(31)
    h = torch.randn(2, 77, 2 * 1280, generator=gen).to(BF)
    dy = torch.randn(2, 77, 1280, generator=gen).to(BF)
    hg = h.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        y = geglu(hg)
    (dh,) = torch.autograd.grad(y, hg, dy.to(cuda))
    hf = h.float().requires_grad_(True)
    with torch.enable_grad():
        a, g = hf.chunk(2, dim=-1)
        ref = a * torch.nn.functional.gelu(g)
    (rh,) = torch.autograd.grad(ref, hf, dy.float())
    e1, e2 = _rel(y, ref), _rel(dh, rh)
    parity_record("geglu_bf16_rel_l2", e1, 4e-3)
    parity_record("geglu_bf16_vjp_rel_l2", e2, 4e-3)
    assert y.dtype == BF and dh.dtype == BF and e1 < 4e-3 and e2 < 4e-3, (e1, e2)
    names = _kernel_names(lambda: geglu(h.to(cuda)))
    assert any("k_geglu_bf16_fwd" in s for s in names) and not any("Gelu" in s for s in names)


@pytest.mark.parametrize("c", [320, 640, 1280])
def test_layernorm_bf16_fwd_vjp(cuda, c, parity_record):
    """sp_layernorm_bf16_fwd / _bwd vs torch's fp32 LayerNorm of the same bf16 inputs."""
    from samplers_amd.networks.layers import LayerNorm, layer_norm

    gen = torch.Generator().manual_seed(c)
    mod = LayerNorm(c)
    with torch.no_grad():
        mod.weight.copy_(1 + 0.1 * torch.randn(c, generator=gen))
        mod.bias.copy_(0.1 * torch.randn(c, generator=gen))
    mod.requires_grad_(False)
    x = (torch.randn(2, 300, c, generator=gen) * 3 + 1).to(BF)
    dy = torch.randn(2, 300, c, generator=gen).to(BF)
    gm = copy.deepcopy(mod).to(cuda, BF)
    xg = x.to(cuda).requires_grad_(True)
    with torch.enable_grad():
        y = layer_norm(xg, gm)
    (dx,) = torch.autograd.grad(y, xg, dy.to(cuda))
    xf = x.float().requires_grad_(True)
    with torch.enable_grad():
        ref = torch.nn.functional.layer_norm(xf, (c,), mod.weight, mod.bias, mod.eps)
    (rx,) = torch.autograd.grad(ref, xf, dy.float())
    e1, e2 = _rel(y, ref), _rel(dx, rx)
    parity_record("layernorm_bf16_rel_l2", e1, 5e-3, c=c)
    parity_record("layernorm_bf16_vjp_rel_l2", e2, 1e-2, c=c)
    assert e1 < 5e-3 and e2 < 1e-2, (e1, e2)
    names = _kernel_names(lambda: layer_norm(x.to(cuda), gm))
    assert any("k_layernorm_bf16_fwd" in s for s in names) and not any("layer_norm" in s for s in names)


def test_transformer_block_bf16_residual_handoff(cuda, parity_record):
    """A BasicTransformerBlock at bf16: x + f(norm(x)) three times with the residual gradients added
    inside the LayerNorm VJP kernels (no autograd add kernels), against the block in fp32 on the CPU."""
    from samplers_amd.networks.unet2d_condition import BasicTransformerBlock

    torch.manual_seed(0)
    blk = BasicTransformerBlock(320, 8, 768).requires_grad_(False)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 256, 320, generator=gen)
    ctx = torch.randn(1, 77, 768, generator=gen)
    cot = torch.randn(2, 256, 320, generator=gen)
    gpu = copy.deepcopy(blk).to(cuda, BF)

    def run(m, v, cx):
        vr = v.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            out = m(vr, cx)
        (g,) = torch.autograd.grad(out, vr, cot.to(device=out.device, dtype=out.dtype))
        return out.float().cpu(), g.float().cpu()

    og, gg = run(gpu, x.to(cuda, BF), ctx.to(cuda, BF))
    orf, grf = run(blk, x, ctx)
    e1, e2 = _rel(og, orf), _rel(gg, grf)
    parity_record("transformer_block_bf16_rel_l2", e1, 2e-2)
    parity_record("transformer_block_bf16_vjp_rel_l2", e2, 3e-2)
    assert e1 < 2e-2 and e2 < 3e-2, (e1, e2)

    def fwd_bwd():
        vr = x.to(cuda, BF).requires_grad_(True)
        with torch.enable_grad():
            out = gpu(vr, ctx.to(cuda, BF))
        torch.autograd.grad(out, vr, cot.to(cuda, BF))

    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fwd_bwd()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    assert any("k_layernorm_bf16_bwd" in s for s in names)
    # the three residual adds of the forward (y += res after each residual linear); none in the VJP
    assert sum("CUDAFunctor_add" in s for s in names) <= 3, [s for s in names if "add" in s.lower()]


def _blocked(t):
    """(n, c, h, w) -> flat [n][c / 16][h][w][16] (the conv tile's channel-blocked input layout)."""
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n, h, w, c // 16, 16).permute(0, 3, 1, 2, 4).contiguous().reshape(-1)


@pytest.mark.parametrize("shape", [(2, 64, 128, 32, 64), (1, 320, 320, 64, 64), (3, 32, 64, 16, 32)])
def test_conv3x3_bf16_blocked_input_bitwise(cuda, shape):
    """sp_conv3x3_bf16_ex with the channel-blocked input equals the NHWC call bit for bit (same
    data, same summation order), split-K included."""
    from samplers_amd.networks import bf16

    n, ci, co, h, w = shape
    gen = torch.Generator().manual_seed(ci + co)
    conv = torch.nn.Conv2d(ci, co, 3, padding=1).to(BF).requires_grad_(False).to(cuda)
    x = torch.randn(n, ci, h, w, generator=gen).to(BF).to(cuda).contiguous(memory_format=torch.channels_last)
    pk, b = bf16.conv_pack(conv, False), bf16._bias_f32(conv, conv.bias)
    assert bf16.blocked_ok(ci, co, h, w)
    y0 = bf16._conv_launch(x, pk, b, None, co)
    y1 = bf16._conv_launch(_blocked(x), pk, b, None, co, shape=(n, ci, h, w))
    assert torch.equal(y0, y1)


def test_groupnorm_bf16_blocked_outputs_bitwise(cuda):
    """GroupNorm forward / VJP writing the channel-blocked layout equal the NHWC results bit for bit."""
    from samplers_amd.networks import bf16
    from samplers_amd.networks.layers import GroupNormAct

    gen = torch.Generator().manual_seed(3)
    norm = GroupNormAct(32, 128, eps=1e-6, act=True).to(cuda, BF).requires_grad_(False)
    x = torch.randn(2, 128, 32, 32, generator=gen).to(BF).to(cuda).contiguous(memory_format=torch.channels_last)
    dz = torch.randn(2, 128, 32, 32, generator=gen).to(BF).to(cuda).contiguous(memory_format=torch.channels_last)
    z0, st = bf16._gn_fwd_raw(norm, x, None, None)
    z1, _ = bf16._gn_fwd_raw(norm, x, None, None, blocked=True)
    assert torch.equal(_blocked(z0), z1)
    d0, _ = bf16._gn_bwd_raw(norm, dz, x, None, None, st)
    d1, _ = bf16._gn_bwd_raw(norm, dz, x, None, None, st, blocked=True)
    assert torch.equal(_blocked(d0), d1)


def test_resnet_block_bf16_blocked_equals_nhwc(cuda, monkeypatch):
    """The fused bf16 ResnetBlock with channel-blocked GroupNorm -> conv hand-offs equals the NHWC
    hand-offs bit for bit, forward and input VJP (skip input and 1x1 shortcut included)."""
    from samplers_amd.networks.unet2d import ResnetBlock2D

    torch.manual_seed(1)
    blk = ResnetBlock2D(128 + 64, 128, 64, 32, 1e-5).to(cuda, BF).requires_grad_(False)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, 128, 32, 64, generator=gen).to(BF).to(cuda)
    skip = torch.randn(2, 64, 32, 64, generator=gen).to(BF).to(cuda)
    temb = torch.randn(2, 64, generator=gen).to(BF).to(cuda)
    cot = torch.randn(2, 128, 32, 64, generator=gen).to(BF).to(cuda)

    def run():
        xr, sr = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
        with torch.enable_grad():
            out = blk(xr, temb, skip=sr)
        gx, gs = torch.autograd.grad(out, (xr, sr), cot)
        return out, gx, gs

    a = run()
    monkeypatch.setenv("SAMPLERS_AMD_BF16_BLOCKED", "0")
    b = run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("n,c1,c2,cout,h,w", [(2, 128, 64, 128, 32, 64), (1, 256, 256, 256, 32, 64),
                                              (3, 96, 0, 64, 16, 32)])
def test_resnet_block_bf16_shortcut_in_conv2(cuda, monkeypatch, parity_record, n, c1, c2, cout, h, w):
    """conv2 + the 1x1 shortcut as one contraction (sp_conv3x3_bf16_sc; the (1, 256 + 256, 32x64)
    case takes the split-K path with parts spanning both kinds of stage) against the shortcut GEMMs +
    residual epilogue (SAMPLERS_AMD_BF16_SC=0) and the block in fp32 on the CPU; the VJP is shared."""
    from samplers_amd.networks.unet2d import ResnetBlock2D

    torch.manual_seed(3)
    ref = ResnetBlock2D(c1 + c2, cout, 64, 32, 1e-5).requires_grad_(False)
    blk = copy.deepcopy(ref).to(cuda, BF)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, c1, h, w, generator=gen)
    skip = torch.randn(n, c2, h, w, generator=gen) if c2 else None
    temb = torch.randn(n, 64, generator=gen)

    def gpu_out():
        return blk(x.to(cuda, BF), temb.to(cuda, BF), skip=None if skip is None else skip.to(cuda, BF)).float().cpu()

    names = _kernel_names(gpu_out)
    assert any("k_conv3x3_bf16<32, false, true, true," in s or "k_conv3x3_bf16<32, false, false, true," in s
               for s in names), sorted(s for s in names if "conv" in s)
    a = gpu_out()
    monkeypatch.setenv("SAMPLERS_AMD_BF16_SC", "0")
    b = gpu_out()
    r = ref(x, temb, skip=skip)
    e_ab, e_a, e_b = _rel(a, b), _rel(a, r), _rel(b, r)
    parity_record("resnet_bf16_sc_vs_gemm_shortcut", e_ab, 1e-2, shape=[n, c1, c2, cout, h, w])
    parity_record("resnet_bf16_sc_vs_fp32", e_a, 1.2 * e_b + 1e-3, shape=[n, c1, c2, cout, h, w], gemm_vs_fp32=e_b)
    assert e_ab < 1e-2 and e_a <= 1.2 * e_b + 1e-3, (e_ab, e_a, e_b)


@pytest.mark.parametrize("n,c1,c2,cout,h,w,blocked", [(2, 128, 64, 128, 32, 64, "1"), (2, 128, 0, 128, 32, 32, "0"),
                                                      (1, 64, 64, 64, 64, 64, "1")])
def test_resnet_block_bf16_groupnorm_sums_from_conv_epilogue(cuda, monkeypatch, parity_record, n, c1, c2, cout, h, w,
                                                             blocked):
    """The block's VJP with both GroupNorm VJPs' sums taken in the preceding conv VJP's epilogue
    (sp_conv3x3_bf16_gnvjp, opt-in: per-tile partials, no sums pass) against the conv VJP + two-pass
    GroupNorm VJP (SAMPLERS_AMD_BF16_GNVJP=0) — the same terms summed in another fixed order — and
    the block in fp32 on the CPU."""
    from samplers_amd.networks.unet2d import ResnetBlock2D

    monkeypatch.setenv("SAMPLERS_AMD_BF16_BLOCKED", blocked)
    monkeypatch.setenv("SAMPLERS_AMD_BF16_GNVJP", "1")  # off by default (slower, see bf16.gnvjp_ok)
    torch.manual_seed(5)
    ref = ResnetBlock2D(c1 + c2, cout, 64, 32, 1e-5).requires_grad_(False)
    blk = copy.deepcopy(ref).to(cuda, BF)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(n, c1, h, w, generator=gen)
    skip = torch.randn(n, c2, h, w, generator=gen) if c2 else None
    temb = torch.randn(n, 64, generator=gen)
    cot = torch.randn(n, cout, h, w, generator=gen)

    def run(mod, dev, dt):
        xr = x.to(dev, dt).requires_grad_(True)
        sr = None if skip is None else skip.to(dev, dt).requires_grad_(True)
        with torch.enable_grad():
            out = mod(xr, temb.to(dev, dt), skip=sr)
        gs = torch.autograd.grad(out, (xr,) if sr is None else (xr, sr), cot.to(dev, dt))
        return torch.cat([g.float().cpu().reshape(-1) for g in gs])

    def gpu_vjp():
        return run(blk, cuda, BF)

    names = _kernel_names(gpu_vjp)
    assert any("k_conv3x3_bf16<32, false" in s and "false, true, false>" in s for s in names)  # GS, not SC / FS
    assert not any("k_gnb_stats<1" in s for s in names), "the GroupNorm VJP sums pass still ran"
    a = gpu_vjp()
    monkeypatch.setenv("SAMPLERS_AMD_BF16_GNVJP", "0")
    b = gpu_vjp()
    r = run(ref, "cpu", torch.float32)
    e_ab, e_a, e_b = _rel(a, b), _rel(a, r), _rel(b, r)
    tag = [n, c1, c2, cout, h, w, blocked]
    parity_record("resnet_bf16_gn_sums_epilogue_vs_two_pass_vjp", e_ab, 5e-3, shape=tag)
    parity_record("resnet_bf16_gn_sums_epilogue_vjp_vs_fp32", e_a, 1.2 * e_b + 1e-3, shape=tag, two_pass_vs_fp32=e_b)
    assert e_ab < 5e-3 and e_a <= 1.2 * e_b + 1e-3, (e_ab, e_a, e_b)


@pytest.mark.parametrize("n,c1,c2,cout,h,w,blocked", [(2, 128, 64, 128, 32, 64, "1"), (2, 128, 0, 128, 32, 32, "0"),
                                                      (1, 64, 64, 256, 64, 64, "1")])
def test_resnet_block_bf16_groupnorm_moments_from_conv_epilogue(cuda, monkeypatch, parity_record, n, c1, c2, cout, h,
                                                                w, blocked):
    """GN2's moments taken in conv1's epilogue (sp_conv3x3_bf16_gn, opt-in: per-tile moments shifted by the
    tile's first pixel, combined in fp64) against conv1 + the two-pass GroupNorm
    (SAMPLERS_AMD_BF16_GNFWD=0) and the block in fp32 on the CPU, forward and input VJP."""
    from samplers_amd.networks.unet2d import ResnetBlock2D

    monkeypatch.setenv("SAMPLERS_AMD_BF16_BLOCKED", blocked)
    monkeypatch.setenv("SAMPLERS_AMD_BF16_GNFWD", "1")  # off by default (slower, see bf16.gnfwd_ok)
    torch.manual_seed(7)
    ref = ResnetBlock2D(c1 + c2, cout, 64, 32, 1e-5).requires_grad_(False)
    blk = copy.deepcopy(ref).to(cuda, BF)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(n, c1, h, w, generator=gen) + 0.5  # a mean offset: the moments' shift matters
    skip = torch.randn(n, c2, h, w, generator=gen) if c2 else None
    temb = torch.randn(n, 64, generator=gen)
    cot = torch.randn(n, cout, h, w, generator=gen)

    def run(mod, dev, dt):
        xr = x.to(dev, dt).requires_grad_(True)
        sr = None if skip is None else skip.to(dev, dt).requires_grad_(True)
        with torch.enable_grad():
            out = mod(xr, temb.to(dev, dt), skip=sr)
        gs = torch.autograd.grad(out, (xr,) if sr is None else (xr, sr), cot.to(dev, dt))
        return out.float().cpu(), torch.cat([g.float().cpu().reshape(-1) for g in gs])

    names = _kernel_names(lambda: run(blk, cuda, BF))
    assert any("k_conv3x3_bf16<32, false" in s and "false, false, true>" in s for s in names)  # FS
    oa, ga = run(blk, cuda, BF)
    monkeypatch.setenv("SAMPLERS_AMD_BF16_GNFWD", "0")
    ob, gb = run(blk, cuda, BF)
    orf, grf = run(ref, "cpu", torch.float32)
    tag = [n, c1, c2, cout, h, w, blocked]
    for what, a, b, r in (("out", oa, ob, orf), ("vjp", ga, gb, grf)):
        e_ab, e_a, e_b = _rel(a, b), _rel(a, r), _rel(b, r)
        parity_record(f"resnet_bf16_gn_moments_epilogue_vs_two_pass_{what}", e_ab, 5e-3, shape=tag)
        parity_record(f"resnet_bf16_gn_moments_epilogue_{what}_vs_fp32", e_a, 1.2 * e_b + 1e-3, shape=tag,
                      two_pass_vs_fp32=e_b)
        assert e_ab < 5e-3 and e_a <= 1.2 * e_b + 1e-3, (what, e_ab, e_a, e_b)


# ---- whole priors -----------------------------------------------------------------------------

def _fwd_vjp(fn, x, cot):
    xr = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        out = fn(xr)
    (g,) = torch.autograd.grad(out, xr, grad_outputs=cot.to(device=out.device, dtype=out.dtype))
    return out.detach().float().cpu(), g.detach().float().cpu()


def _triple(name, fn_gpu, fn_cpu_bf, fn_cpu_32, x, cot, parity_record, direct_tol):
    """GPU bf16 vs CPU bf16 (direct), and both vs CPU fp32 (GPU error <= 1.5 x CPU error + 1e-3)."""
    g = _fwd_vjp(fn_gpu, x.to("cuda:0", BF), cot.to(BF))
    c = _fwd_vjp(fn_cpu_bf, x.to(BF), cot.to(BF))
    r = _fwd_vjp(fn_cpu_32, x.float(), cot.float())
    for tag, a, bb, rr in zip(("out", "vjp"), g, c, r):
        direct = _rel(a, bb)
        eg, ec = _rel(a, rr), _rel(bb, rr)
        parity_record(f"{tag}_gpu_bf16_vs_cpu_bf16", direct, direct_tol, module=name)
        parity_record(f"{tag}_gpu_bf16_vs_fp32", eg, 1.5 * ec + 1e-3, module=name, cpu_bf16_vs_fp32=ec)
        print(f"{name} {tag}: gpu-bf16 vs cpu-bf16 {direct:.3e}; vs fp32: gpu {eg:.3e}, cpu {ec:.3e}")
        assert direct < direct_tol, f"{name} {tag}: {direct:.3e}"
        assert eg <= 1.5 * ec + 1e-3, f"{name} {tag}: gpu {eg:.3e} vs cpu {ec:.3e}"


def test_sd15_unet_bf16_fwd_vjp(cuda, parity_record):
    from samplers_amd.networks.unet2d_condition import build_unet_condition, null_context

    cpu32 = build_unet_condition(seed=0)
    cpubf = copy.deepcopy(cpu32).to(BF)
    gpu = copy.deepcopy(cpubf).to(cuda)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, 4, 32, 32, generator=gen)
    cot = torch.randn(2, 4, 32, 32, generator=gen)
    ctx = null_context()
    _triple("sd15_unet", lambda v: gpu(v, 501, ctx.to(cuda, BF)), lambda v: cpubf(v, 501, ctx.to(BF)),
            lambda v: cpu32(v, 501, ctx), x, cot, parity_record, 1e-1)
    names = _kernel_names(lambda: gpu(x.to(cuda, BF), 501, ctx.to(cuda, BF)))
    assert any("k_conv3x3_bf16" in s for s in names) and any("k_gnb_apply" in s for s in names)
    assert any("k_attnb_fwd" in s for s in names)
    _no_miopen_conv(names)


def test_vae_bf16_decode_encode(cuda, parity_record):
    from samplers_amd.networks.vae import build_vae

    cpu32 = build_vae(seed=1)
    cpubf = copy.deepcopy(cpu32).to(BF)
    gpu = copy.deepcopy(cpubf).to(cuda)
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(1, 4, 32, 32, generator=gen)
    cz = torch.randn(1, 3, 256, 256, generator=gen)
    _triple("vae_decode", gpu.decode, cpubf.decode, cpu32.decode, z, cz, parity_record, 1e-1)
    x = torch.rand(1, 3, 256, 256, generator=gen) * 2 - 1
    cx = torch.randn(1, 4, 32, 32, generator=gen)
    _triple("vae_encode", gpu.encode_mean, cpubf.encode_mean, cpu32.encode_mean, x, cx, parity_record, 1e-1)
    names = _kernel_names(lambda: gpu.decode(z.to(cuda, BF)))
    assert any("k_conv3x3_bf16" in s for s in names)
    _no_miopen_conv(names)


def test_celebahq_unet_bf16_fwd_vjp(cuda, parity_record):
    from samplers_amd.networks.unet2d import build_unet

    cpu32 = build_unet(seed=0)
    cpubf = copy.deepcopy(cpu32).to(BF)
    gpu = copy.deepcopy(cpubf).to(cuda)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(1, 3, 256, 256, generator=gen)
    cot = torch.randn(1, 3, 256, 256, generator=gen)
    _triple("celebahq_unet", lambda v: gpu(v, 500), lambda v: cpubf(v, 500), lambda v: cpu32(v, 500), x, cot,
            parity_record, 1e-1)


def test_celebahq_unet_bf16_skip_grad_handoff(cuda, monkeypatch, parity_record):
    """The bf16 UNet's skip-tensor gradients handed from the up-block to the down-path ResnetBlock's
    GroupNorm VJP kernel (layers.SkipGrad) equal autograd's accumulation adds within one bf16
    rounding of the summed gradient, with fewer full-size add kernels in the step."""
    from torch.profiler import ProfilerActivity, profile

    from samplers_amd.networks.unet2d import build_unet

    gpu = build_unet(seed=0).to(cuda, BF).requires_grad_(False)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 256, 256, generator=gen).to(cuda, BF)
    cot = torch.randn(2, 3, 256, 256, generator=gen).to(cuda, BF)

    def run():
        xr = x.clone().requires_grad_(True)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            with torch.enable_grad():
                out = gpu(xr, 500)
            (g,) = torch.autograd.grad(out, xr, cot)
            torch.cuda.synchronize()
        adds = sum("CUDAFunctor_add" in e.name for e in prof.events() if e.device_type.name == "CUDA")
        return out.float().cpu(), g.float().cpu(), adds

    run()  # weight packs / folded biases built and cached (their construction launches adds too)
    oa, ga, adds_box = run()
    monkeypatch.setenv("SAMPLERS_AMD_SKIPGRAD", "0")
    ob, gb, adds_autograd = run()
    assert torch.equal(oa, ob)
    e = _rel(ga, gb)
    parity_record("celebahq_unet_bf16_skipgrad_vs_autograd_vjp", e, 1e-2)
    assert e < 1e-2, e
    assert adds_box + 10 <= adds_autograd, (adds_box, adds_autograd)


def test_psld_bf16_sd15_matches_oracle(cuda, parity_record):
    """PSLDSampler with LatentDiffusionNetwork.from_config(torch_dtype=bf16): 3 guided iterations +
    the final decode at 3x256², B = 2, centre inpainting, vs oracle/latent_loops.py with the same
    bf16 modules on the CPU behind the same fp32 boundary (networks in bf16, the loop in fp32)."""
    from oracle.latent_loops import psld_reference
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.networks.latent import LatentDiffusionNetwork, StableDiffusionCondition
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.operators import CenterInpaintingOperator
    from samplers_amd.samplers.psld import PSLDSampler

    b, shape, steps = 2, (3, 256, 256), 4
    lshape = (4, 32, 32)
    gen = torch.Generator().manual_seed(21)
    op = CenterInpaintingOperator(shape, 0.5)
    kept = op._kept_indices.cpu()
    n = int(np.prod(shape))

    def apply(v):
        return v.reshape(v.shape[0], -1)[:, kept]

    def adjoint(v):
        out = torch.zeros(v.shape[0], n, dtype=v.dtype)
        out = out.index_put((torch.arange(v.shape[0])[:, None], kept[None, :]), v)
        return out.reshape(v.shape[0], *shape)

    x_true = si.fixture_x_true(b, shape, 22)
    y = apply(x_true) + 0.05 * torch.randn(b, kept.numel(), generator=gen)
    z0 = torch.randn(b, *lshape, generator=gen)
    xi = {i: torch.randn(b, *lshape, generator=gen) for i in range(16)}

    cpu = LatentDiffusionNetwork.from_config(seed=0, torch_dtype=BF)
    assert cpu.dtype == BF
    gpu = copy.deepcopy(cpu).to(cuda)
    fn = lambda k, i, s: (z0 if k == "init" else xi[i]).to(cuda)  # noqa: E731
    problem = InverseProblem(op.to(cuda), y.to(cuda), GaussianNoise(0.05).to(cuda))
    cond = StableDiffusionCondition(prompt=[""] * b)  # as run_psld.py:39; CFG of equal rows collapses
    names = _kernel_names(lambda: PSLDSampler(gpu)(problem, num_sampling_steps=steps, noise_fn=fn, condition=cond))
    out = PSLDSampler(gpu)(problem, num_sampling_steps=steps, noise_fn=fn, condition=cond)
    assert out.dtype == BF and torch.isfinite(out.float()).all()
    for k in ("k_conv3x3_bf16", "k_gnb_apply", "k_gnb_bwd_apply", "k_attnb_fwd", "k_psld_pixel"):
        assert any(k in s for s in names), k
    _no_miopen_conv(names)

    cpu.set_sampling_parameters(steps, batch_size=b)
    cpu.set_condition(cond)
    f32 = lambda t: t.to(torch.float32)  # noqa: E731
    ref = psld_reference(lambda v, t: f32(cpu(v.to(BF), t)), cpu.alphas_cumprod.float(), cpu.timesteps_host,
                         apply, adjoint, lambda v: f32(cpu.decode(v.to(BF), differentiable=True)),
                         lambda v: f32(cpu.encode(v.to(BF), differentiable=True)), y, z0, lambda i: xi[i])
    err = _rel(out, ref.reshape(out.shape))
    print(f"PSLD bf16 SD1.5: 3 guided steps + decode, rel L2 vs the bf16 oracle {err:.3e}")
    parity_record("x0_rel_l2", err, PSLD_BF16_TOL, sampler="PSLD", dtype="bf16", guided_steps=3, batch=b,
                  image=list(shape))
    assert err < PSLD_BF16_TOL, err
