"""The bf16 attention kernels (``k_attnb_fwd`` / ``_dq`` / ``_dkv`` of csrc/sp_bf16_attention.hip) where the
SD-shaped ``randn`` tests never take them: peaked rows, on which the lazily moved softmax reference
point moves and live accumulators are rescaled (tests/attn_ref.py; tests/test_attn_ref.py shows on the
CPU that every ``up`` / ``saw`` case here moves it for every query), and ragged shapes — n, m that
are no multiple of 32, fewer than 32 keys, a last stage of one key — where the clamped row loads,
the -inf key masks, the absent queries of the dk / dv pass and the early return before the stores
do their work.  Through the C ABI, batch 2 x 2 heads, self-attention on the fused [b][n][3 heads d]
projection layout, cross-attention with the context per sample and shared.

Against fp64 on the bf16-rounded operands (``attn_ref.attention_fp64``), with every output buffer
pre-filled with NaN and one guard row behind it, and 64 rows of NaN behind every input (what an
unclamped row load past the last sample would read):

* O elementwise within 2^-8 (|O| + P |v|) (the two bf16 roundings, of the weights and of the
  output) and relative L2 1e-2;
* lse, which the VJP rebuilds P from, per query within LSE_CONST (1 + max_j sum_d |q k| scale)
  (attn_ref.LSE_CONST: 4 x what float32 torch shows);
* dk, dv relative L2 1e-2; dq max(1e-2, 2 x the error of the fp64 emulation of the kernels'
  roundings on the same inputs): delta comes from the bf16 O, which costs dq more the larger
  |k| is.  Where a one-key last block carries the whole row (``attn_ref.vjp_degenerate``) dk is
  bounded like dq: dq and dk are rounding noise there for any kernel with these roundings.
"""

from __future__ import annotations

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
B, HEADS = 2, 2
NAN = float("nan")


def _cases():
    out = []
    for n, m, d, s in ar.bf16_cases():
        for shared in ((0,) if n == m else (0, 1)):
            out.append(pytest.param(n, m, d, s, shared, id=f"n{n}-m{m}-d{d}-{s}" + ("-shared" if shared else "")))
    return out


def _guarded(rows: int, width: int, dev, dtype=BF):
    """A NaN-filled [rows + 1][width] buffer: the kernels own the first ``rows``, the last is a guard."""
    return torch.full((rows + 1, width), NAN, device=dev, dtype=dtype)


def _rows_then_nan(t, dev):
    """Token rows [b][n][w] as a device buffer followed by a stage (64 rows) of NaN: a row load
    that is not clamped to the last real row brings NaN into an MFMA, where a weight of 0 does
    not remove it."""
    rows = t.reshape(-1, t.shape[-1])
    return torch.cat([rows, torch.full((64, rows.shape[1]), NAN, dtype=rows.dtype)]).contiguous().to(dev)


def _written(buf, what):
    body, guard = buf[:-1], buf[-1]
    assert not torch.isnan(body).any(), f"{what}: rows left unwritten (NaN)"
    assert torch.isnan(guard).all(), f"{what}: written past the end"
    return body.detach().cpu().double()


@pytest.mark.parametrize("n,m,d,schedule,shared", _cases())
def test_attention_bf16_peaked_and_ragged(cuda, parity_record, n, m, d, schedule, shared):
    from samplers_amd import _hip

    lib = _hip.load_library()
    assert lib.sp_attention_bf16_supported(B, HEADS, n, m, d)
    self_attn = n == m
    c = HEADS * d
    scale = ar.f32_scale(d)
    q, k, v, do = ar.peaked_qkv(B, HEADS, n, m, d, schedule, ar.case_seed(n, m, d, schedule), BF,
                                kv_batch=1 if shared else None)
    ref = ar.attention_fp64(q, k, v, do, scale)
    emu = ar.attention_bf16_emulated(q, k, v, do, scale)
    tag = dict(n=n, m=m, d=d, schedule=schedule, kv_shared=shared)
    if schedule in ("up", "saw"):
        mv = ar.lazy_moves(ar.scores_log2(q, k, scale))
        assert int(mv.min()) >= 1  # the rescale of live accumulators runs for every query
        parity_record("attn_bf16_lazy_moves_min", int(mv.min()), None, max=int(mv.max()), **tag)

    stream = None
    if self_attn:  # q, k, v the thirds of one fused projection
        x = _rows_then_nan(torch.cat([ar.merge_heads(t) for t in (q, k, v)], -1), cuda)
        qp, kp, vp, rsq, rskv = x.data_ptr(), x.data_ptr() + 2 * c, x.data_ptr() + 4 * c, 3 * c, 3 * c
    else:
        xq, xk, xv = (_rows_then_nan(ar.merge_heads(t), cuda) for t in (q, k, v))
        qp, kp, vp, rsq, rskv = xq.data_ptr(), xk.data_ptr(), xv.data_ptr(), c, c
    dout = _rows_then_nan(ar.merge_heads(do), cuda)
    out = _guarded(B * n, c, cuda)
    lse = _guarded(B * HEADS, n, cuda, torch.float32)
    _hip.check(lib.sp_attention_bf16_fwd(qp, kp, vp, B, HEADS, n, m, d, rsq, rskv, shared, c, scale, out.data_ptr(),
                                         lse.data_ptr(), stream), "sp_attention_bf16_fwd")
    torch.cuda.synchronize()
    o = ar.split_heads(_written(out, "out").reshape(B, n, c), HEADS)
    ls = _written(lse, "lse").reshape(B, HEADS, n)

    ratio = float(((o - ref["o"]).abs() / (2.0 ** -8 * (ref["o"].abs() + ref["env_o"]))).max())
    e_o = ar.rel_l2(o, ref["o"])
    lratio = float(((ls - ref["lse"]).abs() / (ar.LSE_CONST * (1 + ref["env_s"]))).max())
    parity_record("attn_bf16_edge_o_elementwise", ratio, 1.0, **tag)
    parity_record("attn_bf16_edge_o_rel_l2", e_o, 1e-2, **tag)
    parity_record("attn_bf16_edge_lse", lratio, 1.0, abs=float((ls - ref["lse"]).abs().max()), **tag)
    print(f"O elementwise {ratio:.3f} of the bound, rel L2 {e_o:.2e}; lse {lratio:.3f} of the bound")
    assert ratio <= 1.0, ratio
    assert e_o < 1e-2, e_o
    assert lratio <= 1.0, lratio

    if schedule == "spike" or not lib.sp_attention_bf16_bwd_supported(B, HEADS, n, m, d):
        return
    delta = _guarded(B * HEADS, n, cuda, torch.float32)
    if self_attn:
        g = _guarded(B * n, 3 * c, cuda)
        dqp, dkp, dvp, rd = g.data_ptr(), g.data_ptr() + 2 * c, g.data_ptr() + 4 * c, 3 * c
    else:
        g = _guarded(B * n, c, cuda)
        dqp, dkp, dvp, rd = g.data_ptr(), None, None, c
    _hip.check(lib.sp_attention_bf16_bwd(qp, kp, vp, out.data_ptr(), dout.data_ptr(), lse.data_ptr(), B, HEADS, n, m,
                                         d, rsq, rskv, shared, c, rd, rd, scale, delta.data_ptr(), dqp, dkp, dvp,
                                         stream), "sp_attention_bf16_bwd")
    torch.cuda.synchronize()
    grads = _written(g, "dq / dk / dv").reshape(B, n, -1)
    _written(delta, "delta")
    dq = ar.split_heads(grads[..., :c], HEADS)
    e_emu = ar.rel_l2(emu["dq"], ref["dq"])
    e_dq = ar.rel_l2(dq, ref["dq"])
    bound = max(1e-2, 2 * e_emu)
    parity_record("attn_bf16_edge_dq_emulation_rel_l2", e_emu, None, **tag)
    parity_record("attn_bf16_edge_dq_rel_l2", e_dq, bound, **tag)
    print(f"dq rel L2 {e_dq:.2e} (emulation {e_emu:.2e}, bound {bound:.2e})")
    assert e_dq <= bound, (e_dq, e_emu)
    if not self_attn:
        return
    dk = ar.split_heads(grads[..., c:2 * c], HEADS)
    dv = ar.split_heads(grads[..., 2 * c:], HEADS)
    e_dk, e_dv = ar.rel_l2(dk, ref["dk"]), ar.rel_l2(dv, ref["dv"])
    bound_dk = 1e-2
    if ar.vjp_degenerate(m, schedule):
        bound_dk = max(1e-2, 2 * ar.rel_l2(emu["dk"], ref["dk"]))
    parity_record("attn_bf16_edge_dk_rel_l2", e_dk, bound_dk, **tag)
    parity_record("attn_bf16_edge_dv_rel_l2", e_dv, 1e-2, **tag)
    print(f"dk rel L2 {e_dk:.2e} (bound {bound_dk:.2e}), dv {e_dv:.2e}")
    assert e_dk <= bound_dk and e_dv <= 1e-2, (e_dk, e_dv)
