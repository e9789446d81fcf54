"""Peaked attention inputs and fp64 references shared by the attention edge tests.

Trained attention rows are peaked; ``randn`` rows are not, and on them the fused kernels' lazily
moved softmax reference point (``mn = bm > mx + 8 ? bm : mx`` per 32-key block, log2 units) never
moves after the first block.  ``peaked_qkv`` puts a ramp on one coordinate so that it does,
``lazy_moves`` counts on the fp64 scores how often, and ``attention_fp64`` /
``attention_bf16_emulated`` are the references (exact, and with the bf16 kernels' documented
roundings) the GPU tests compare against.  Everything here runs on the CPU.

Tensors are [b][heads][n][d] (q, dO) and [bk][heads][m][d] (k, v) with bk = b, or 1 for one
context shared by the batch.
"""

from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
BLOCK = 32          # keys per softmax block of k_attnb_fwd / k_attn6_fwd
LAZY = 8.0          # AB_LAZY = A6_LAZY, log2 units
# One level of the ramp in log2 units of score.  The other d - 1 coordinates add N(0, log2(e)^2)
# to every score, so the running maximum after a block sits 2 .. 4 units above the block's level and
# the next block's maximum is as uncertain: a step of 12 clears the threshold of 8 by 4 units
# (about 4 sigma of the difference of two 32-key block maxima) for every query, not only on average.
STEP_LOG2 = 12.0
SPIKE_LOG2 = 64.0   # the spike key's score above the level of the rest (>= 40 after the noise)
SAW = (0, 1, 1, 2, 0, 2, 3, 3)
SCHEDULES = ("randn", "up", "down", "saw", "spike")


def levels(schedule: str, m: int, max_level: int | None = None) -> list[int]:
    """The ramp level of every 32-key block.  ``up`` climbs one level per block (spread over the
    blocks when ``max_level`` caps it), ``down`` is its reverse, ``saw`` repeats 0 1 1 2 0 2 3 3
    (each period starting where the last ended).  A last block of fewer than 32 keys climbs two
    levels in ``up`` / ``saw``: its maximum is over few keys, down to one, and must still clear the
    running maximum of 32 by the threshold."""
    nblk = -(-m // BLOCK)
    if schedule in ("randn", "spike") or nblk == 1:
        return [0] * nblk
    if schedule in ("up", "down"):
        top = nblk - 1 if max_level is None else min(max_level, nblk - 1)
        lv = [i * (top + 1) // nblk for i in range(nblk)]
    elif schedule == "saw":
        lv = [SAW[i % len(SAW)] + 3 * (i // len(SAW)) for i in range(nblk)]
        if max_level is not None:
            lv = [min(x, max_level) for x in lv]
    else:
        raise ValueError(schedule)
    if m % BLOCK and max_level is None:
        lv[-1] = max(lv[:-1]) + 2
    return lv[::-1] if schedule == "down" else lv


def peaked_qkv(b: int, heads: int, n: int, m: int, d: int, schedule: str, seed: int, dtype=torch.float64,
               kv_batch: int | None = None, max_level: int | None = None):
    """``randn`` q, k, v, dO rounded to ``dtype``; coordinate 0 carries the ramp: q[..., 0] = A and
    k[j, 0] = B level[j // 32] with A B scale log2(e) = STEP_LOG2 and A = B max(level), so neither
    operand is larger than it has to be (the VJP's rounding error grows with max |k|).  ``spike``:
    k[..., 0] = 0 but for one key in a middle block, SPIKE_LOG2 above."""
    if schedule not in SCHEDULES:
        raise ValueError(schedule)
    bk = b if kv_batch is None else kv_batch
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, heads, n, d, generator=g, dtype=torch.float64)
    k = torch.randn(bk, heads, m, d, generator=g, dtype=torch.float64)
    v = torch.randn(bk, heads, m, d, generator=g, dtype=torch.float64)
    do = torch.randn(b, heads, n, d, generator=g, dtype=torch.float64)
    unit = math.sqrt(d) / LOG2E  # A B for one log2 unit of score at scale = d^-1/2
    if schedule == "spike":
        a = math.sqrt(SPIKE_LOG2 * unit)
        q[..., 0] = a
        k[..., 0] = 0.0
        k[:, :, spike_key(m), 0] = a
    elif schedule != "randn":
        lv = levels(schedule, m, max_level)
        top = max(lv)
        if top > 0:
            bb = math.sqrt(STEP_LOG2 * unit / top)
            q[..., 0] = bb * top
            k[..., 0] = bb * torch.tensor(lv, dtype=torch.float64).repeat_interleave(BLOCK)[:m]
    return tuple(t.to(dtype) for t in (q, k, v, do))


def spike_key(m: int) -> int:
    """The spike's key: the sixth of a middle block (or the last key of a shorter row)."""
    return min((-(-m // BLOCK) // 2) * BLOCK + 5, m - 1)


def scores_log2(q, k, scale: float):
    """fp64 scores in the kernels' log2 units, [b][heads][n][m]."""
    return (q.double() @ k.double().transpose(-1, -2)) * (scale * LOG2E)


def lazy_moves(s_log2, block: int = BLOCK, lazy: float = LAZY):
    """Per query, how many blocks after the first moved the reference point under the kernels' rule
    (a move is a rescale of live accumulators by 0 < corr < 1)."""
    m = s_log2.shape[-1]
    mx = s_log2[..., :block].amax(-1)
    moves = torch.zeros_like(mx, dtype=torch.int64)
    for j in range(block, m, block):
        bm = s_log2[..., j:j + block].amax(-1)
        mv = bm > mx + lazy
        moves += mv
        mx = torch.where(mv, bm, mx)
    return moves


def attention_fp64(q, k, v, do, scale: float) -> dict:
    """softmax(q k^T scale) v and its VJP at dO in fp64 by the closed forms (no autograd), with the
    envelopes the elementwise bounds use: ``env_o`` = P |v| (what one relative rounding of every
    weight can move O by) and ``env_s`` = max_j sum_d |q_id k_jd| scale (the size of the terms an
    fp32 score sum rounds).  dk / dv are summed over the batch when k, v are shared."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = p @ v
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    dq = (ds @ k) * scale
    dk = (ds.transpose(-1, -2) @ q) * scale
    dv = p.transpose(-1, -2) @ do
    if k.shape[0] != q.shape[0]:
        dk, dv = dk.sum(0, keepdim=True), dv.sum(0, keepdim=True)
    env_s = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) * scale
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "env_o": p @ v.abs(), "env_s": env_s}


def bf16r(t):
    """Round to bf16 (nearest even), back in fp64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def attention_bf16_emulated(q, k, v, do, scale: float) -> dict:
    """The same in fp64 with the bf16 kernels' roundings and no others: P rounded for P V (the row
    sum is of the unrounded weights), O stored in bf16 and delta = rowsum(dO o O) taken from the
    stored O, P (for dv) and dS (for dq, dk) rounded as MFMA operands, every output rounded."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = (q @ k.transpose(-1, -2)) * scale
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    tot = e.sum(-1, keepdim=True)
    o = bf16r((bf16r(e) @ v) / tot)
    lse = (mx + torch.log(tot))[..., 0]
    p = e / tot
    dp = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    ds = bf16r(p * (dp - delta))
    dq = bf16r((ds @ k) * scale)
    dk = (ds.transpose(-1, -2) @ q) * scale
    dv = bf16r(p).transpose(-1, -2) @ do
    if k.shape[0] != q.shape[0]:
        dk, dv = dk.sum(0, keepdim=True), dv.sum(0, keepdim=True)
    return {"o": o, "lse": lse, "dq": dq, "dk": bf16r(dk), "dv": bf16r(dv)}


def attention_f32_torch(q, k, v, do, scale: float) -> dict:
    """Plain float32 torch on the CPU (matmul, softmax, autograd): what fp32 arithmetic gives on
    these inputs without any of this project's code; the yardstick of the fp32 kernels' bounds."""
    q, k, v = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    with torch.enable_grad():
        s = (q @ k.transpose(-1, -2)) * scale
        o = torch.softmax(s, -1) @ v
        dq, dk, dv = torch.autograd.grad(o, (q, k, v), do.float().expand_as(o))
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), -1), "dq": dq, "dk": dk, "dv": dv}


def rel_l2(a, b) -> float:
    a, b = a.double(), b.double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


def merge_heads(t):
    """[b][heads][n][d] -> token rows [b][n][heads d]."""
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d)


def split_heads(t, heads: int):
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).transpose(1, 2)


# ---- the cases of the GPU tests (tests/test_attn_ref.py checks every one on the CPU) ---------------

BF16_DIMS = (40, 64, 80, 160)
BF16_SELF = (1, 33, 100, 200)
BF16_CROSS = ((130, 77), (33, 1), (64, 65), (40, 129))
BF16_SPIKE = ((200, 200), (130, 77))


def bf16_schedules(n: int, m: int) -> list[str]:
    out = ["randn"]
    if m > BLOCK:
        out += ["up", "down", "saw"]
    if (n, m) in BF16_SPIKE:
        out.append("spike")
    return out


def bf16_cases() -> list[tuple[int, int, int, str]]:
    """(n, m, d, schedule) of tests/test_attention_bf16_edges_gpu.py."""
    shapes = [(n, n) for n in BF16_SELF] + list(BF16_CROSS)
    return [(n, m, d, s) for d in BF16_DIMS for n, m in shapes for s in bf16_schedules(n, m)]


FP32_SHAPES = ((40, 128), (40, 256), (80, 128), (80, 256), (160, 64), (160, 128))  # (d, n)
FP32_SCHEDULES = ("up", "saw", "down", "spike")
FP32_MAX_LEVEL = 3   # at most three climbs: ramped scores of size S put eps S under any fp32 result
FP32_CROSS_M = 77


# The bf16 forward's lse bound is LSE_CONST (1 + max_j sum_d |q_id k_jd| scale) per query.  The
# bf16 products are exact in fp32, so the error is that of an fp32 sum of d terms and of the fp32
# softmax; 2^-20 was the first guess, but plain float32 torch on these inputs reaches 1.16 x 2^-20
# (1 + ...) (spike at (200, 200), d = 160; 0.79 on the ramps), so the constant is 4 x that, 4.64,
# rounded up to 5 because float32 matmul sums differ a little between CPUs.  A rescale wrong by
# 2^-9 moves lse by 2e-3, 6 times the bound at the largest scores here (envelope 70) and more below.
LSE_CONST = 5 * 2.0 ** -20


def f32_scale(d: int) -> float:
    """d^-1/2 as the float32 the kernels are handed (the references use the same number)."""
    return float(torch.tensor(d ** -0.5, dtype=torch.float32))


def vjp_degenerate(m: int, schedule: str) -> bool:
    """A last block of one key that moves every query's reference point holds a weight of 1 - 2^-20
    or so: dS = P (dP - delta) is then the difference of two nearly equal numbers in every row, and
    delta = rowsum(dO o O) is taken from the bf16 O, so dq and dk are rounding noise relative to
    their (tiny) norm — for the emulation (relative L2 about 0.9) as for any kernel with these
    roundings.  The forward, lse and dv stay well conditioned."""
    return m > BLOCK and m % BLOCK == 1 and schedule in ("up", "saw")


def case_seed(n: int, m: int, d: int, schedule: str) -> int:
    return 1000 * n + 7 * m + d + 100003 * SCHEDULES.index(schedule)
