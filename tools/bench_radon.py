"""DPS pass 1 for the parallel-beam projector (sp_dps_residual_ws on an SP_OP_RADON descriptor:
the two launches of csrc/sp_radon.hip) against the same v = A^T(grad_scale (y - A x0)) composed
with torch on the GPU, timed in one process: B = 64, 1 x 256 x 256, 23 and 180 angles over a half
turn, the default detector (365 bins).

Entries (interleaved group by group, each group of `--inner` back-to-back passes bracketed by
device events after a warm-up; the figures are the median and the quartiles over `--repeats`
groups, successive passes rotating over `--sets` buffer sets):
  hip_A{23,180}           the fused pass: project (x0 formed while staging, work = grad_scale r,
                          |r|^2 partials), backproject
  torch_sparse_A{23,180}  torch.sparse.mm with A and A^T as CSR matrices built from the same table
                          (operators.radon.radon_matrix, fp32), handed x0 already formed and every
                          operand already transposed to (elements, batch), which favours it
No threshold is set: the ratio is reported as measured.  The pass's algorithmic bytes are x, eps
and y in, v out, and work out and in; `fraction_of_8TBps` is those bytes over the pass's time over
8 TB/s.  Per-launch times come from the library's dispatch-packet events (sp_timing_enable),
collected in separate passes after the timed groups.
    python tools/bench_radon.py [--out profiles/bench_radon.json]
prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from samplers_amd import _hip  # noqa: E402
from samplers_amd.operators import RadonOperator  # noqa: E402

LAUNCHES = ("project", "backproject")
HBM_BYTES_PER_S = 8e12


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--angles", type=int, nargs="+", default=[23, 180])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_radon.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_radon.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    S, b = a.size, a.batch
    shape = (1, S, S)
    n = S * S
    a_t, gs = 0.31, 400.0
    coefs = _hip.SpDpsCoefs(a_t, (1 - a_t**2) ** 0.5, gs, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream

    entries, meta, sets_of = {}, {}, {}
    turn = [0]

    def add(nA):
        op = RadonOperator(shape, num_angles=nA).to(dev)
        desc = op.hip_descriptor()
        m = int(desc.m)
        A, At = (mat.to_sparse_csr() for mat in op._matrices(torch.float32, dev))
        sets = []
        for _ in range(a.sets):
            x, eps = (torch.randn(b, n, device=dev) for _ in range(2))
            y = torch.randn(b, m, device=dev)
            x0t = ((x - coefs.k * eps) / coefs.a).t().contiguous()
            sets.append(dict(x=x, eps=eps, y=y, v=torch.empty(b, n, device=dev),
                             work=torch.empty(int(lib.sp_dps_workspace(desc, b)), device=dev),
                             x0t=x0t, yt=y.t().contiguous()))
        sets_of[nA] = sets
        part = torch.empty(b, int(lib.sp_rsq_partials(desc)), device=dev)

        def next_set():
            s = sets[turn[0] % a.sets]
            turn[0] += 1
            return s

        def run_hip():
            s = next_set()
            _hip.check(lib.sp_dps_residual_ws(desc, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), b, 1, coefs, s["v"].data_ptr(),
                                              part.data_ptr(), s["work"].data_ptr(), stream),
                       "sp_dps_residual_ws")
            return s["v"], part.sum(1)

        def run_torch():
            s = next_set()
            res = s["yt"] - torch.sparse.mm(A, s["x0t"])
            rsq = res.square().sum(0)
            return torch.sparse.mm(At, gs * res).t(), rsq

        entries[f"hip_A{nA}"] = run_hip
        entries[f"torch_sparse_A{nA}"] = run_torch
        bytes_ = 4 * b * (2 * n + m + n + 2 * m)
        meta[nA] = {"detector": op.detector_size, "m": m, "nnz": int(A._nnz()),
                    "partials_per_sample": int(part.shape[1]), "algorithmic_bytes": bytes_,
                    "keep": (op, A, At, part)}

    for nA in a.angles:
        add(nA)

    # both entries of an angle count compute the same thing (checked once, on one buffer set)
    agree = {}
    for nA in a.angles:
        turn[0] = 0
        v_new, rsq_new = entries[f"hip_A{nA}"]()
        v_new, rsq_new = v_new.clone(), rsq_new.clone()
        turn[0] = 0
        v, rsq = entries[f"torch_sparse_A{nA}"]()
        agree[f"A{nA}"] = {"v_max_diff_over_max": float((v - v_new).abs().max() / v_new.abs().max()),
                           "rsq_max_rel_diff": float((rsq / rsq_new - 1).abs().max())}
    for _ in range(a.warmup):
        for run in entries.values():
            for _ in range(a.inner):
                run()
    torch.cuda.synchronize()
    times = {k: [] for k in entries}
    for _ in range(a.repeats):
        for name, run in entries.items():  # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3 / a.inner)

    # per-launch times of the fused pass: the two kind-1 records of each pass, in launch order
    per_launch = {}
    kinds, ms = (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)()
    for nA in a.angles:
        cols = [[] for _ in LAUNCHES]
        lib.sp_timing_enable(1)
        for _ in range(a.repeats):
            entries[f"hip_A{nA}"]()
            got = lib.sp_timing_collect(kinds, ms, 64)
            if got == len(LAUNCHES):
                for i in range(got):
                    cols[i].append(ms[i] * 1e3)
        lib.sp_timing_enable(0)
        per_launch[f"A{nA}"] = {l: round(statistics.median(c), 1) for l, c in zip(LAUNCHES, cols) if c}

    row = {"bench": "radon_dps_pass1", "batch": b, "shape": list(shape), "repeats": a.repeats,
           "inner": a.inner, "buffer_sets": a.sets, "device": torch.cuda.get_device_name(0),
           "sp_version": int(lib.sp_version()),
           "geometry": {f"A{k}": {kk: vv for kk, vv in v.items() if kk != "keep"} for k, v in meta.items()},
           "agreement_torch_vs_hip": agree, "per_launch_us": per_launch}
    for name in entries:
        t = statistics.median(times[name])
        q1, q3 = quartiles(times[name])
        row[name] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                     "us_min": round(min(times[name]) * 1e6, 1), "us_max": round(max(times[name]) * 1e6, 1)}
    for nA in a.angles:
        hip, other = row[f"hip_A{nA}"], row[f"torch_sparse_A{nA}"]
        hip["fraction_of_8TBps"] = round(meta[nA]["algorithmic_bytes"] / (hip["us"] * 1e-6) / HBM_BYTES_PER_S, 5)
        row[f"ratio_hip_over_torch_A{nA}"] = round(hip["us"] / other["us"], 4)
        row[f"hip_faster_A{nA}"] = bool(hip["us"] < other["us"])
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
