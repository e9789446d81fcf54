"""PGDM pass 1 and DPS pass 1 for the periodic blur (SP_OP_PSF_PERIODIC, csrc/sp_psf_fft.hip),
timed in one process: B = 64, 3 x 256 x 256, a dense R = 30 PSF by default.

Entries (all interleaved group by group, each group of `--inner` back-to-back passes bracketed by
device events after a warm-up; the figures are the median and the quartiles over `--repeats`
groups, successive passes rotating over `--sets` buffer sets):
  pgdm_fused       sp_pgdm_residual_ws: v = -2 (A^+ y - Pi x0), three launches, Q = P FFT2(y)
                   prepared once outside the timed region (as PGDMSampler does)
  pgdm_composed    the same v from sp_predict_x0, sp_op_apply_ws, a subtraction, sp_op_pinv_ws and
                   a scale (four 2-D transforms instead of two, plus three elementwise passes)
  pgdm_torch_fft   x0, rfft2, Q - keep * X, irfft2, the scale: the same v with torch.fft on the
                   device, handed the precomputed Q and keep
  dps_periodic     sp_dps_residual_ws on the new kind: five launches on 256 x 256 transforms
  dps_fft_circular sp_dps_residual_ws on FFTPSFBlurOperator(padding="circular"), the same map
                   through padded_size(256 + 60) = 384-point transforms
Per-launch times of the HIP entries come from the library's dispatch-packet events
(sp_timing_enable), collected in separate passes after the timed groups.
    python tools/bench_periodic.py [--out profiles/bench_periodic.json]
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
from samplers_amd.operators import FFTPSFBlurOperator, PeriodicBlurOperator  # noqa: E402


def dense_kernel(radius: int) -> torch.Tensor:
    k = 2 * radius + 1
    h = torch.rand(k, k, generator=torch.Generator().manual_seed(radius), dtype=torch.float64) + 0.05
    return (h / h.sum()).to(torch.float32)


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--radius", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_periodic.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_periodic.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    a_t = 0.31
    k_t = (1 - a_t**2) ** 0.5
    pgdm = _hip.SpDpsCoefs(a_t, k_t, -2.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    dps = _hip.SpDpsCoefs(a_t, k_t, 400.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream

    h = dense_kernel(a.radius)
    per = PeriodicBlurOperator(shape, h).to(dev)
    circ = FFTPSFBlurOperator(shape, h, padding="circular").to(dev)
    dper, dcirc = per.hip_descriptor(), circ.hip_descriptor()
    work_floats = max(int(lib.sp_dps_workspace(d, b)) for d in (dper, dcirc))
    q_floats = int(lib.sp_op_workspace(dper, b))
    keep_half = per.keep[:, : S // 2 + 1].to(torch.float32)  # rfft2's half spectrum

    sets = []
    for _ in range(a.sets):
        x, eps, y = (torch.randn(b, n, device=dev) for _ in range(3))
        s = dict(x=x, eps=eps, y=y, v=torch.empty(b, n, device=dev),
                 work=torch.empty(work_floats, device=dev), q=torch.empty(q_floats, device=dev),
                 t0=torch.empty(b, n, device=dev), t1=torch.empty(b, n, device=dev))
        _hip.check(lib.sp_pgdm_prepare(dper, y.data_ptr(), b, s["q"].data_ptr(), stream), "prepare")
        s["q_torch"] = torch.fft.rfft2(per.apply_pseudo_inverse(y.view(b, C, S, S)))  # P FFT2(y)
        sets.append(s)
    turn = [0]

    def next_set():
        s = sets[turn[0] % a.sets]
        turn[0] += 1
        return s

    def pgdm_fused():
        s = next_set()
        _hip.check(lib.sp_pgdm_residual_ws(dper, s["x"].data_ptr(), s["eps"].data_ptr(),
                                           s["q"].data_ptr(), b, 1, pgdm, s["v"].data_ptr(),
                                           s["work"].data_ptr(), stream), "sp_pgdm_residual_ws")
        return s["v"]

    def pgdm_composed():
        s = next_set()
        _hip.check(lib.sp_predict_x0(s["x"].data_ptr(), s["eps"].data_ptr(), b * n, a_t, k_t,
                                     s["t0"].data_ptr(), stream), "sp_predict_x0")
        _hip.check(lib.sp_op_apply_ws(dper, s["t0"].data_ptr(), s["t1"].data_ptr(), b,
                                      s["work"].data_ptr(), stream), "sp_op_apply_ws")
        torch.sub(s["y"], s["t1"], out=s["t0"])
        _hip.check(lib.sp_op_pinv_ws(dper, s["t0"].data_ptr(), s["t1"].data_ptr(), b, 0,
                                     s["work"].data_ptr(), stream), "sp_op_pinv_ws")
        torch.mul(s["t1"], -2.0, out=s["v"])
        return s["v"]

    def pgdm_torch_fft():
        s = next_set()
        x0 = ((s["x"] - k_t * s["eps"]) / a_t).view(b, C, S, S)
        z = s["q_torch"] - torch.fft.rfft2(x0) * keep_half
        return (-2.0 * torch.fft.irfft2(z, s=(S, S))).reshape(b, n)

    def dps_pass(desc):
        part = torch.empty(b, int(lib.sp_rsq_partials(desc)), device=dev)

        def run():
            s = next_set()
            _hip.check(lib.sp_dps_residual_ws(desc, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), b, 1, dps, s["v"].data_ptr(),
                                              part.data_ptr(), s["work"].data_ptr(), stream),
                       "sp_dps_residual_ws")
            return s["v"]

        return run

    entries = {"pgdm_fused": pgdm_fused, "pgdm_composed": pgdm_composed,
               "pgdm_torch_fft": pgdm_torch_fft, "dps_periodic": dps_pass(dper),
               "dps_fft_circular": dps_pass(dcirc)}

    # the entries of one group compute the same thing (checked once, on one buffer set)
    def first(name):
        turn[0] = 0
        return entries[name]().clone()

    v_new, agree = first("pgdm_fused"), {}
    for other in ("pgdm_composed", "pgdm_torch_fft"):
        agree[other] = float((first(other) - v_new).abs().max() / v_new.abs().max())
    agree["dps_fft_circular_vs_dps_periodic"] = float(
        (first("dps_fft_circular") - first("dps_periodic")).abs().max()
        / first("dps_periodic").abs().max())

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

    # per-launch times (kind-1 records, in launch order): the fused PGDM pass and both DPS passes
    launches = {"pgdm_fused": ("rows", "columns_pgdm", "rows_inv"),
                "dps_periodic": ("rows", "columns_A", "rows_inv_rows", "columns_AT", "rows_inv_AT"),
                "dps_fft_circular": ("rows", "columns_A", "rows_inv_rows", "columns_AT", "rows_inv_AT")}
    per_launch = {}
    kinds, ms = (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)()
    for name, names in launches.items():
        cols = [[] for _ in names]
        lib.sp_timing_enable(1)
        for _ in range(a.repeats):
            entries[name]()
            got = lib.sp_timing_collect(kinds, ms, 64)
            if got == len(names):
                for i in range(got):
                    cols[i].append(ms[i] * 1e3)
        lib.sp_timing_enable(0)
        per_launch[name] = {l: round(statistics.median(c), 1) for l, c in zip(names, cols) if c}

    row = {"bench": "periodic_pgdm_and_dps_pass1", "batch": b, "shape": list(shape),
           "radius": a.radius, "kept_share": round(float(per.keep.float().mean()), 4),
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "transform_sizes": {"periodic": [S, S], "fft_circular": list(circ.padded_shape)},
           "max_diff_over_max_vs_pgdm_fused": agree, "per_launch_us": per_launch}
    for name in entries:
        t = statistics.median(times[name])
        q1, q3 = quartiles(times[name])
        row[name] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                     "us_min": round(min(times[name]) * 1e6, 1),
                     "us_max": round(max(times[name]) * 1e6, 1)}
    row["ratios"] = {
        "pgdm_composed_over_fused": round(row["pgdm_composed"]["us"] / row["pgdm_fused"]["us"], 3),
        "pgdm_torch_fft_over_fused": round(row["pgdm_torch_fft"]["us"] / row["pgdm_fused"]["us"], 3),
        "dps_fft_circular_over_periodic": round(row["dps_fft_circular"]["us"]
                                                / row["dps_periodic"]["us"], 3)}
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
