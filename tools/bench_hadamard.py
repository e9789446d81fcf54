"""The fused passes of the Walsh-Hadamard compressed-sensing kind (SP_OP_HADAMARD,
csrc/sp_hadamard.hip) after the network call, timed in one process at B = 64, 3 x 256 x 256 on
`HadamardOperator(ratio=0.25)`: DPS pass 1, the DiffPIR step and the DDRM step, each against the
same result composed from the operator's own device maps, sp_predict_x0, sp_randn and torch
elementwise operations.

The method is tools/bench_svd_sep.py's: all entries interleaved group by group, each group of
`--inner` back-to-back passes bracketed by device events after a warm-up; the figures are the
median and the quartiles over `--repeats` groups, successive passes rotating over `--sets` buffer
sets; noise is drawn in the kernels (Philox).  q (y copied) is prepared once outside the timed
region, as the samplers do.
  dps       sp_dps_residual_ws | x0, r = y - A x0, A^T (gs r) and the squared norm in torch
  diffpir   sp_diffpir_step_ws | sp_predict_x0, sp_op_prox_ws, sp_randn and the update in torch
  ddrm      sp_ddrm_step_ws | x0, xi, w and the base in torch, A^T (f_y y + A w) through the maps
            (sig_y = 0: f_th = 0, f_y = 1, f_xi = sig' on the kept set)
Context lines: `inpaint_ddrm` and `inpaint_diffpir`, SP_OP_INPAINT's one-launch steps at the same
kept share on the same x, eps and out buffers.
`bars`: fused median <= composed median on the three passes.  `hbm`: the algorithmic bytes of each
fused pass, the workspace round trips included (three launches: the low stage reads its sources and
writes work, the high stage reads and writes work and reads y, the last stage reads work and its
sources again and writes the result; the sign vector, keep_bits and word_rank stay in cache and are
not counted), over its median, as a share of the 8 TB/s HBM specification.

    python tools/bench_hadamard.py [--out profiles/bench_hadamard.json]
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
from samplers_amd.operators import HadamardOperator, RandomInpaintingOperator  # noqa: E402

HBM_SPEC_BYTES = 8e12


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_hadamard.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_hadamard.py times kernels on the GPU; no device found")
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
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    op = HadamardOperator(shape, ratio=a.ratio, seed=0).to(dev)
    inp = RandomInpaintingOperator(shape, fraction=1.0 - a.ratio, seed=1).to(dev)
    d, di = op.hip_descriptor(), inp.hip_descriptor()
    m = int(d.m)
    P = int(lib.sp_rsq_partials(d))
    # sig_y = 0, eta_b = 1: the kept set takes y (f_th = 0, f_y = 1, f_xi = sig'), the rest the prior
    ce, es, sp = cf["c1"] * cf["sig_prev"], cf["eta"] * cf["sig_prev"], cf["sig_prev"]
    work_floats = max(int(lib.sp_ddrm_workspace(d, b)), int(lib.sp_dps_workspace(d, b)),
                      int(lib.sp_prox_workspace(d, b)))
    sets = []
    for _ in range(a.sets):
        x, eps = (torch.randn(b, *shape, device=dev) for _ in range(2))
        truth = torch.randn(b, *shape, device=dev)
        y = op.apply(truth).contiguous()
        s = dict(x=x, eps=eps, y=y, y_in=inp.apply(truth).contiguous(), out=torch.empty_like(x),
                 t0=torch.empty_like(x), xi=torch.empty_like(x), z=torch.empty_like(x),
                 work=torch.empty(work_floats, device=dev), part=torch.empty(b * P, device=dev),
                 q=torch.empty(int(lib.sp_op_workspace(d, b)), device=dev))
        _hip.check(lib.sp_pgdm_prepare(d, y.data_ptr(), b, s["q"].data_ptr(), stream), "sp_pgdm_prepare")
        sets.append(s)
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
        _hip.check(lib.sp_dps_residual_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), b, 1,
                                          dps_c, s["out"].data_ptr(), s["part"].data_ptr(), s["work"].data_ptr(),
                                          stream), "sp_dps_residual_ws")
        return s["out"]

    def dps_composed():
        s = next_set()
        r = s["y"] - op.apply(x0_of(s))
        s["rsq"] = (r * r).reshape(b, -1).sum(1)
        return op.apply_transpose(gs * r)

    def diffpir_fused():
        s = next_set()
        _hip.check(lib.sp_diffpir_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), None,
                                          None, seed, step, 0, b, 1, prox_c, s["out"].data_ptr(),
                                          s["work"].data_ptr(), stream), "sp_diffpir_step_ws")
        return s["out"]

    def diffpir_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        _hip.check(lib.sp_op_prox_ws(d, x0.data_ptr(), s["y"].data_ptr(), None, b, 1, px["rho"],
                                     s["z"].data_ptr(), s["work"].data_ptr(), stream), "sp_op_prox_ws")
        z = s["z"]
        return px["a_prev"] * z + (px["c_eps"] * ((s["x"] - px["a"] * z) / px["k"]) + px["c_xi"] * xi)

    def ddrm_fused():
        s = next_set()
        _hip.check(lib.sp_ddrm_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), None, s["q"].data_ptr(), None,
                                       seed, step, 0, b, 1, ddrm_c, s["out"].data_ptr(), s["work"].data_ptr(),
                                       stream), "sp_ddrm_step_ws")
        return s["out"]

    def ddrm_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        w = -x0 - ce * s["eps"] + (sp - es) * xi  # (f_th - 1) x0 - c1 sig' eps + (f_xi - eta sig') xi
        tail = op.apply_transpose(s["y"] + op.apply(w))
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

    entries = {"dps_fused": dps_fused, "dps_composed": dps_composed, "diffpir_fused": diffpir_fused,
               "diffpir_composed": diffpir_composed, "ddrm_fused": ddrm_fused, "ddrm_composed": ddrm_composed,
               "inpaint_ddrm": inpaint_ddrm, "inpaint_diffpir": inpaint_diffpir}

    # the entries of one pass compute the same thing (checked once, on one buffer set)
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    names = ("dps", "diffpir", "ddrm")
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

    N, M = 4.0 * b * n, 4.0 * b * m
    # low stage: sources in, work out; high stage: work in and out, y in; last stage: work and the
    # sources in, the result out (DPS: v alone).  xi is drawn in the kernels.
    algorithmic = {"dps_fused": (2 + 1) * N + (2 * N + M) + (1 + 1) * N,
                   "diffpir_fused": (2 + 1) * N + (2 * N + M) + (3 + 1) * N,
                   "ddrm_fused": (2 + 1) * N + (2 * N + M) + (3 + 1) * N,
                   "inpaint_ddrm": 3 * N + M, "inpaint_diffpir": 3 * N + M}

    row = {"bench": "hadamard", "batch": b, "shape": list(shape), "ratio": a.ratio,
           "kept_share": round(float(op.keep.float().mean()), 4), "ddrm_coefficients": cf, "prox_coefficients": px,
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "hbm_spec_bytes_per_s": HBM_SPEC_BYTES,
           "bytes_note": "algorithmic bytes, workspace round trips included", "max_diff_over_max_vs_fused": agree}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
        if key in algorithmic:
            row[key]["algorithmic_bytes"] = algorithmic[key]
            row[key]["tb_per_s"] = round(algorithmic[key] / t * 1e-12, 2)
            row[key]["fraction_of_hbm_spec"] = round(algorithmic[key] / t / HBM_SPEC_BYTES, 3)
    row["ratios"] = {f"{k}_composed_over_fused": round(row[f"{k}_composed"]["us"] / row[f"{k}_fused"]["us"], 3)
                     for k in names}
    row["ratios"]["ddrm_fused_over_inpaint_ddrm"] = round(row["ddrm_fused"]["us"] / row["inpaint_ddrm"]["us"], 3)
    row["ratios"]["diffpir_fused_over_inpaint_diffpir"] = round(row["diffpir_fused"]["us"]
                                                                / row["inpaint_diffpir"]["us"], 3)
    row["bars"] = {f"{k}_fused_le_composed": row[f"{k}_fused"]["us"] <= row[f"{k}_composed"]["us"] for k in names}

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
