"""The fp32 attention kernels on peaked rows (tests/attn_ref.py): the exact fp32 forward and VJP
(csrc/sp_attention.hip: the maximum moves with every block, and the bare hardware exp2 sees
arguments far below -126 on ``down`` / ``spike``) and the split-bf16 forward (csrc/sp_attention6.hip:
the lazily moved reference point; tests/test_attn_ref.py shows it moves for every query on ``up`` /
``saw``), at every head dim and at one and several row blocks.

Scores of size S put eps S under any fp32 result, so the bound is not a constant: each error
against fp64 may be at most twice that of plain float32 torch on the CPU on the same inputs, + 1e-6
(relative L2 for O and the VJPs, absolute for lse) — and below the project's 1e-5 wherever that
bound is.  The ramps climb at most three levels of 12 log2 units to keep S small.  The split-bf16
forward is also held to 1.25 x the exact kernel's error, as on ``randn`` inputs
(tests/test_attention_gpu.py).
"""

from __future__ import annotations

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu

B, HEADS = 2, 2
NAN = float("nan")


def _inputs(n, m, d, schedule, kv_batch=None):
    q, k, v, do = ar.peaked_qkv(B, HEADS, n, m, d, schedule, ar.case_seed(n, m, d, schedule), torch.float32,
                                kv_batch=kv_batch, max_level=ar.FP32_MAX_LEVEL)
    scale = ar.f32_scale(d)
    ref = ar.attention_fp64(q, k, v, do, scale)
    f32 = ar.attention_f32_torch(q, k, v, do, scale)
    yard = {name: ar.rel_l2(f32[name], ref[name]) for name in ("o", "dq", "dk", "dv")}
    yard["lse"] = float((f32["lse"].double() - ref["lse"]).abs().max())
    return (q, k, v, do), scale, ref, yard


class _Judge:
    """Collects every figure, records it, and fails at the end with all that missed."""

    def __init__(self, record, ref, yard, **tag):
        self.record, self.ref, self.yard, self.tag, self.missed, self.err = record, ref, yard, tag, [], {}

    def __call__(self, kernel, name, got):
        want = self.ref[name]
        got = got.detach().cpu().double().reshape(want.shape)
        assert not torch.isnan(got).any(), f"{kernel} {name}: NaN (rows left unwritten)"
        e = float((got - want).abs().max()) if name == "lse" else ar.rel_l2(got, want)
        bound = 2 * self.yard[name] + 1e-6
        self.err[kernel, name] = e
        self.record(f"attn_peaked_{name}", e, bound, kernel=kernel, float32_torch=self.yard[name], **self.tag)
        print(f"{kernel:12s} {name:3s} {e:.3e}  float32 torch {self.yard[name]:.3e}  bound {bound:.3e}")
        if e > bound or (name != "lse" and bound < 1e-5 and not e < 1e-5):
            self.missed.append((kernel, name, e, bound))

    def no_worse(self, split, exact):
        """The split-bf16 forward against the exact kernel, as tests/test_attention_gpu.py."""
        for name, slack in (("o", 1e-8), ("lse", 1e-6)):
            e6, e32 = self.err[split, name], self.err[exact, name]
            if e6 > 1.25 * e32 + slack:
                self.missed.append((split, name, e6, f"1.25 x {exact} {e32}"))

    def done(self):
        assert not self.missed, self.missed


def _heads_first(t):
    """[b][heads][n][d] -> contiguous [b heads][n][d]."""
    return t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()


@pytest.mark.parametrize("schedule", ar.FP32_SCHEDULES)
@pytest.mark.parametrize("d,n", ar.FP32_SHAPES, ids=lambda v: str(v))
def test_fp32_attention_on_peaked_rows(cuda, parity_record, d, n, schedule):
    from samplers_amd import _hip

    lib = _hip.load_library()
    (q, k, v, do), scale, ref, yard = _inputs(n, n, d, schedule)
    bh, c = B * HEADS, HEADS * d
    assert lib.sp_attention_supported(bh, n, n, d) and lib.sp_attention_mh_supported(B, HEADS, n, n, d)
    split = bool(lib.sp_attention6_supported(B, HEADS, n, d))
    assert split == (d in (40, 80))
    judge = _Judge(parity_record, ref, yard, d=d, n=n, schedule=schedule)
    qc, kc, vc, dc = (_heads_first(t).to(cuda) for t in (q, k, v, do))
    x = torch.cat([ar.merge_heads(t) for t in (q, k, v)], -1).contiguous().to(cuda)  # [b][n][3 heads d]
    base = x.data_ptr()
    prev = lib.sp_attention_bf16x6(-1)
    try:
        for mode in ((0, 1) if split else (0,)):
            lib.sp_attention_bf16x6(mode)
            kern = "split-bf16" if mode else "fp32"
            # [bh][n][d] operands, forward and (exact kernel) VJP; the VJP after the split forward is
            # test_fp32_vjp_after_the_split_forward_on_peaked_rows
            out = torch.full((bh, n, d), NAN, device=cuda)
            lse = torch.full((bh, n), NAN, device=cuda)
            _hip.check(lib.sp_attention_fwd(_hip.ptr(qc), _hip.ptr(kc), _hip.ptr(vc), bh, n, d, scale, _hip.ptr(out),
                                            _hip.ptr(lse), None), "sp_attention_fwd")
            torch.cuda.synchronize()
            judge(kern, "o", out)
            judge(kern, "lse", lse)
            if schedule != "spike" and not mode:
                delta = torch.full((bh, n), NAN, device=cuda)
                dq, dk, dv = (torch.full((bh, n, d), NAN, device=cuda) for _ in range(3))
                _hip.check(lib.sp_attention_bwd(_hip.ptr(qc), _hip.ptr(kc), _hip.ptr(vc), _hip.ptr(out), _hip.ptr(dc),
                                                _hip.ptr(lse), bh, n, d, scale, _hip.ptr(delta), _hip.ptr(dq),
                                                _hip.ptr(dk), _hip.ptr(dv), None), "sp_attention_bwd")
                torch.cuda.synchronize()
                for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
                    judge(kern, name, got)
            # the fused projection's strided layout
            out2 = torch.full((B, n, c), NAN, device=cuda)
            lse2 = torch.full((bh, n), NAN, device=cuda)
            _hip.check(lib.sp_attention_fwd_mh(base, base + 4 * c, base + 8 * c, B, HEADS, n, n, d, 3 * c, 3 * c, B, c,
                                               scale, _hip.ptr(out2), _hip.ptr(lse2), None), "sp_attention_fwd_mh")
            torch.cuda.synchronize()
            judge(kern + "-mh", "o", ar.split_heads(out2.cpu(), HEADS))
            judge(kern + "-mh", "lse", lse2)
            if split:  # the split kernel's own entry points, whatever the switch says
                nb = lib.sp_attention6_workspace(B, HEADS, n, d)
                ws = torch.full((nb,), 255, dtype=torch.uint8, device=cuda)  # NaN patterns until written
                o_ws, o_mh = (torch.full((B, n, c), NAN, device=cuda) for _ in range(2))
                l_ws, l_mh = (torch.full((bh, n), NAN, device=cuda) for _ in range(2))
                _hip.check(lib.sp_attention6_fwd_ws(base, base + 4 * c, base + 8 * c, B, HEADS, n, d, 3 * c, c, scale,
                                                    _hip.ptr(o_ws), _hip.ptr(l_ws), _hip.ptr(ws), nb, None),
                           "sp_attention6_fwd_ws")
                _hip.check(lib.sp_attention6_fwd_mh(base, base + 4 * c, base + 8 * c, B, HEADS, n, d, 3 * c, c, scale,
                                                    _hip.ptr(o_mh), _hip.ptr(l_mh), None), "sp_attention6_fwd_mh")
                torch.cuda.synchronize()
                assert torch.equal(o_ws, o_mh) and torch.equal(l_ws, l_mh)  # the same terms in the same order
                judge(f"attn6-ws/{mode}", "o", ar.split_heads(o_ws.cpu(), HEADS))
                judge(f"attn6-ws/{mode}", "lse", l_ws)
                if mode:
                    assert torch.equal(o_ws, out2) and torch.equal(l_ws, lse2)  # what fwd_mh routed to
    finally:
        lib.sp_attention_bf16x6(prev)
    if split:
        judge.no_worse("split-bf16", "fp32")
        judge.no_worse("split-bf16-mh", "fp32-mh")
        judge.no_worse("attn6-ws/0", "fp32-mh")
    judge.done()


@pytest.mark.parametrize("schedule", ["up", "saw", "down"])
@pytest.mark.parametrize("d,n", [s for s in ar.FP32_SHAPES if s[0] != 160], ids=lambda v: str(v))
def test_fp32_vjp_after_the_split_forward_on_peaked_rows(cuda, parity_record, d, n, schedule):
    """What a self-attention at head dim 40 / 80 runs by default: the split-bf16 forward, then the fp32
    VJP kernels from that forward's O and lse, held to the same bound (2 x float32 torch + 1e-6).

    This test found a defect.  With delta = rowsum(dO o O) taken from the split forward's O, dq was
    1.3e-5 .. 1.7e-5 against bounds of 8.3e-6 .. 9.1e-6 (up to 2.07 x) in 11 of the 12 cases and dk
    1.02 x once, while from the exact fp32 forward the same kernels were inside (dq <= 0.71 x):
    k_attn_dq rebuilds P from its own fp32 scores, whose rounding differs from the split forward's,
    so delta no longer equalled sum_j P_ij dP_ij, the rows of dS stopped summing to 0, and the
    residue was multiplied by the P-weighted mean of k — large on these inputs (k[..., 0] up to 12),
    next to nothing on ``randn`` rows.  k_attn_dq<D, true> now measures that residue, removes it
    from dq and hands the consistent delta to k_attn_dkv: dq <= 0.85 x, dk <= 0.89 x, dv <= 0.86 x."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    (q, k, v, do), scale, ref, yard = _inputs(n, n, d, schedule)
    bh = B * HEADS
    assert lib.sp_attention6_supported(bh, 1, n, d)
    judge = _Judge(parity_record, ref, yard, d=d, n=n, schedule=schedule)
    qc, kc, vc, dc = (_heads_first(t).to(cuda) for t in (q, k, v, do))
    out = torch.full((bh, n, d), NAN, device=cuda)
    lse, delta = (torch.full((bh, n), NAN, device=cuda) for _ in range(2))
    dq, dk, dv = (torch.full((bh, n, d), NAN, device=cuda) for _ in range(3))
    prev = lib.sp_attention_bf16x6(1)
    try:
        _hip.check(lib.sp_attention_fwd(_hip.ptr(qc), _hip.ptr(kc), _hip.ptr(vc), bh, n, d, scale, _hip.ptr(out),
                                        _hip.ptr(lse), None), "sp_attention_fwd")
        _hip.check(lib.sp_attention_bwd(_hip.ptr(qc), _hip.ptr(kc), _hip.ptr(vc), _hip.ptr(out), _hip.ptr(dc),
                                        _hip.ptr(lse), bh, n, d, scale, _hip.ptr(delta), _hip.ptr(dq), _hip.ptr(dk),
                                        _hip.ptr(dv), None), "sp_attention_bwd")
        torch.cuda.synchronize()
    finally:
        lib.sp_attention_bf16x6(prev)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        judge("split-bf16", name, got)
    judge.done()


@pytest.mark.parametrize("schedule", ar.FP32_SCHEDULES)
@pytest.mark.parametrize("d", [40, 80, 160])
def test_fp32_cross_attention_77_on_peaked_rows(cuda, parity_record, d, schedule):
    """sp_attention_fwd_mh with the 77-token context shared by the batch: a last stage of 13 keys."""
    from samplers_amd import _hip

    lib = _hip.load_library()
    n, m, c, bh = (64 if d == 160 else 128), ar.FP32_CROSS_M, HEADS * d, B * HEADS
    (q, k, v, do), scale, ref, yard = _inputs(n, m, d, schedule, kv_batch=1)
    assert lib.sp_attention_mh_supported(B, HEADS, n, m, d)
    judge = _Judge(parity_record, ref, yard, d=d, n=n, m=m, schedule=schedule)
    xq, xk, xv = (ar.merge_heads(t).contiguous().to(cuda) for t in (q, k, v))
    out = torch.full((B, n, c), NAN, device=cuda)
    lse = torch.full((bh, n), NAN, device=cuda)
    _hip.check(lib.sp_attention_fwd_mh(_hip.ptr(xq), _hip.ptr(xk), _hip.ptr(xv), B, HEADS, n, m, d, c, c, 1, c, scale,
                                       _hip.ptr(out), _hip.ptr(lse), None), "sp_attention_fwd_mh")
    torch.cuda.synchronize()
    judge("fp32-cross", "o", ar.split_heads(out.cpu(), HEADS))
    judge("fp32-cross", "lse", lse)
    judge.done()
