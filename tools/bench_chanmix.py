"""The fused passes of the channel-mixing kind (SP_OP_CHANNEL_MIX, csrc/sp_chanmix.hip) after the
network call, timed in one process at B = 64, 3 x 256 x 256 on
`ChannelMixOperator.colorization("mean")`: DPS pass 1, PGDM pass 1, the DiffPIR step and the DDRM
step, each against the same result composed from the operator's own device maps, sp_predict_x0,
sp_randn and torch elementwise operations.

The method is tools/bench_hadamard.py's: all entries interleaved group by group, each group of
`--inner` back-to-back passes bracketed by device events after a warm-up; the figures are the
median and the quartiles over `--repeats` groups, successive passes rotating over `--sets` buffer
sets; noise is drawn in the kernels (Philox).
  dps       sp_dps_residual | x0, r = y - A x0, A^T (gs r) and the squared norm in torch
  pgdm      sp_pgdm_residual_ws (q = y) | x0, -2 A^+ (y - A x0) through the maps
  diffpir   sp_diffpir_step_ws | sp_predict_x0, sp_op_prox_ws, sp_randn and the update in torch
  ddrm      sp_ddrm_step_ws | x0, xi, w and the base in torch, A^+ (f_y y + A w) through the maps
            (one singular value, so one class; sig_y = 0: f_th = 0, f_y = 1, f_xi = sig')
Context lines: `inpaint_ddrm` and `inpaint_diffpir`, SP_OP_INPAINT's one-launch steps with one third
of the pixels kept (m = n / 3, as here) on the same x, eps and out buffers.
`bars`: fused median <= composed median on the four passes; and for the DiffPIR and DDRM steps the
time per algorithmic byte no worse than the inpainting launch's median x (1 + its relative
interquartile range).  `hbm`: the algorithmic bytes of each fused pass (x, eps and y read, the
result written; the tables stay in cache and are not counted) over its median, as a share of the
8 TB/s HBM specification.

    python tools/bench_chanmix.py [--out profiles/bench_chanmix.json]
prints one JSON line and writes it to --out."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from samplers_amd import _hip  # noqa: E402
from samplers_amd.operators import ChannelMixOperator, RandomInpaintingOperator  # noqa: E402

HBM_SPEC_BYTES = 8e12


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--weights", default="mean")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_chanmix.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_chanmix.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    a_t = 0.31
    k_t = (1 - a_t**2) ** 0.5
    cf = dict(a=f32(a_t), k=f32(k_t), a_prev=f32(0.45), sig_prev=f32(0.89 / 0.45), sig_y=0.0, eta=f32(0.85),
              eta_b=1.0, c1=f32((1 - 0.85**2) ** 0.5))
    ddrm_c = _hip.SpDdrmCoefs(*(cf[f] for f, _ in _hip.SpDdrmCoefs._fields_))
    px = dict(a=cf["a"], k=cf["k"], rho=0.05, a_prev=cf["a_prev"], c_eps=0.75, c_xi=0.49)
    prox_c = _hip.SpProxCoefs(*(px[f] for f, _ in _hip.SpProxCoefs._fields_))
    gs = 400.0
    dps_c = _hip.SpDpsCoefs(cf["a"], cf["k"], gs, 0.9, 0.2, 0.1, 0.05, 1e-9)
    pgdm_c = _hip.SpDpsCoefs(cf["a"], cf["k"], -2.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    op = ChannelMixOperator.colorization(shape, a.weights).to(dev)
    inp = RandomInpaintingOperator(shape, fraction=2.0 / 3.0, seed=1).to(dev)
    d, di = op.hip_descriptor(), inp.hip_descriptor()
    m, m_in = int(d.m), int(di.m)
    P = int(lib.sp_rsq_partials(d))
    for size in (lib.sp_dps_workspace, lib.sp_op_workspace, lib.sp_prox_workspace, lib.sp_ddrm_workspace):
        assert int(size(d, b)) == 0  # every pass is one launch without a workspace
    # sig_y = 0, eta_b = 1: the observed component takes y (f_th = 0, f_y = 1, f_xi = sig'), the rest the prior
    ce, es, sp = cf["c1"] * cf["sig_prev"], cf["eta"] * cf["sig_prev"], cf["sig_prev"]
    sets = []
    for _ in range(a.sets):
        x, eps = (torch.randn(b, *shape, device=dev) for _ in range(2))
        truth = torch.randn(b, *shape, device=dev)
        sets.append(dict(x=x, eps=eps, y=op.apply(truth).contiguous(), y_in=inp.apply(truth).contiguous(),
                         out=torch.empty_like(x), t0=torch.empty_like(x), xi=torch.empty_like(x),
                         z=torch.empty_like(x), part=torch.empty(b * P, device=dev)))
    turn = [0]

    def next_set():
        s = sets[turn[0] % a.sets]
        turn[0] += 1
        return s

    def x0_of(s):
        _hip.check(lib.sp_predict_x0(s["x"].data_ptr(), s["eps"].data_ptr(), b * n, cf["a"], cf["k"],
                                     s["t0"].data_ptr(), stream), "sp_predict_x0")
        return s["t0"]

    def randn(s):
        _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
        return s["xi"]

    def dps_fused():
        s = next_set()
        _hip.check(lib.sp_dps_residual(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), b, 1, dps_c,
                                       s["out"].data_ptr(), s["part"].data_ptr(), stream), "sp_dps_residual")
        return s["out"]

    def dps_composed():
        s = next_set()
        r = s["y"] - op.apply(x0_of(s))
        s["rsq"] = (r * r).reshape(b, -1).sum(1)
        return op.apply_transpose(gs * r)

    def pgdm_fused():
        s = next_set()
        _hip.check(lib.sp_pgdm_residual_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), b, 1,
                                           pgdm_c, s["out"].data_ptr(), None, stream), "sp_pgdm_residual_ws")
        return s["out"]

    def pgdm_composed():
        s = next_set()
        return -2.0 * op.apply_pseudo_inverse(s["y"] - op.apply(x0_of(s)))

    def diffpir_fused():
        s = next_set()
        _hip.check(lib.sp_diffpir_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), None,
                                          None, seed, step, 0, b, 1, prox_c, s["out"].data_ptr(), None, stream),
                   "sp_diffpir_step_ws")
        return s["out"]

    def diffpir_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        _hip.check(lib.sp_op_prox_ws(d, x0.data_ptr(), s["y"].data_ptr(), None, b, 1, px["rho"],
                                     s["z"].data_ptr(), None, stream), "sp_op_prox_ws")
        z = s["z"]
        return px["a_prev"] * z + (px["c_eps"] * ((s["x"] - px["a"] * z) / px["k"]) + px["c_xi"] * xi)

    def ddrm_fused():
        s = next_set()
        _hip.check(lib.sp_ddrm_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), None, None,
                                       seed, step, 0, b, 1, ddrm_c, s["out"].data_ptr(), None, stream),
                   "sp_ddrm_step_ws")
        return s["out"]

    def ddrm_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        w = -x0 - ce * s["eps"] + (sp - es) * xi  # (f_th - 1) x0 - c1 sig' eps + (f_xi - eta sig') xi
        tail = op.apply_pseudo_inverse(s["y"] + op.apply(w))
        return cf["a_prev"] * ((x0 + (ce * s["eps"] + es * xi)) + tail)

    def inpaint_ddrm():
        s = next_set()
        _hip.check(lib.sp_ddrm_step_ws(di, s["x"].data_ptr(), s["eps"].data_ptr(), s["y_in"].data_ptr(), None,
                                       None, seed, step, 0, b, 1, ddrm_c, s["out"].data_ptr(), None, stream),
                   "sp_ddrm_step_ws (inpaint)")
        return s["out"]

    def inpaint_diffpir():
        s = next_set()
        _hip.check(lib.sp_diffpir_step_ws(di, s["x"].data_ptr(), s["eps"].data_ptr(), s["y_in"].data_ptr(), None,
                                          None, seed, step, 0, b, 1, prox_c, s["out"].data_ptr(), None, stream),
                   "sp_diffpir_step_ws (inpaint)")
        return s["out"]

    names = ("dps", "pgdm", "diffpir", "ddrm")
    entries = {"dps_fused": dps_fused, "dps_composed": dps_composed, "pgdm_fused": pgdm_fused,
               "pgdm_composed": pgdm_composed, "diffpir_fused": diffpir_fused,
               "diffpir_composed": diffpir_composed, "ddrm_fused": ddrm_fused, "ddrm_composed": ddrm_composed,
               "inpaint_ddrm": inpaint_ddrm, "inpaint_diffpir": inpaint_diffpir}

    # the entries of one pass compute the same thing (checked once, on one buffer set)
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    agree = {}
    for name in names:
        ref = first(f"{name}_fused")
        agree[f"{name}_composed"] = float((first(f"{name}_composed") - ref).abs().max() / ref.abs().max())

    for _ in range(a.warmup):
        for run in entries.values():
            for _ in range(a.inner):
                run()
    torch.cuda.synchronize()
    times = {k: [] for k in entries}
    for _ in range(a.repeats):
        for key, run in entries.items():  # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) * 1e-3 / a.inner)

    N, M, MI = 4.0 * b * n, 4.0 * b * m, 4.0 * b * m_in
    # x, eps and y in, the result out (DPS and PGDM: v); xi is drawn in the kernels
    algorithmic = {"dps_fused": 3 * N + M, "pgdm_fused": 3 * N + M, "diffpir_fused": 3 * N + M,
                   "ddrm_fused": 3 * N + M, "inpaint_ddrm": 3 * N + MI, "inpaint_diffpir": 3 * N + MI}

    row = {"bench": "chanmix", "batch": b, "shape": list(shape), "weights": a.weights,
           "y_shape": list(op.y_shape), "inpaint_kept_share": round(m_in / n, 4), "ddrm_coefficients": cf,
           "prox_coefficients": px, "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "hbm_spec_bytes_per_s": HBM_SPEC_BYTES, "bytes_note": "algorithmic bytes: x, eps, y read, the result written",
           "max_diff_over_max_vs_fused": agree}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
        if key in algorithmic:
            row[key]["algorithmic_bytes"] = algorithmic[key]
            row[key]["ps_per_byte"] = round(t / algorithmic[key] * 1e12, 4)
            row[key]["tb_per_s"] = round(algorithmic[key] / t * 1e-12, 2)
            row[key]["fraction_of_hbm_spec"] = round(algorithmic[key] / t / HBM_SPEC_BYTES, 3)
    row["ratios"] = {f"{k}_composed_over_fused": round(row[f"{k}_composed"]["us"] / row[f"{k}_fused"]["us"], 3)
                     for k in names}
    row["bars"] = {f"{k}_fused_le_composed": row[f"{k}_fused"]["us"] <= row[f"{k}_composed"]["us"] for k in names}
    for k in ("diffpir", "ddrm"):  # per byte against the inpainting launch, the margin its own spread
        ref = row[f"inpaint_{k}"]
        iqr = (ref["us_q3"] - ref["us_q1"]) / ref["us"]
        limit = ref["ps_per_byte"] * (1.0 + iqr)
        row["ratios"][f"{k}_ps_per_byte_over_inpaint"] = round(row[f"{k}_fused"]["ps_per_byte"] / ref["ps_per_byte"], 3)
        row["bars"][f"{k}_per_byte_le_inpaint"] = {"ps_per_byte": row[f"{k}_fused"]["ps_per_byte"],
                                                   "limit": round(limit, 4), "inpaint_relative_iqr": round(iqr, 4),
                                                   "met": row[f"{k}_fused"]["ps_per_byte"] <= limit}

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
