"""DPS pass 1, the fused PGDM pass 1 and the DiffPIR step of the periodic blur-and-decimate
super-resolution kind (SP_OP_SR_PERIODIC, csrc/sp_psf_fft.hip), timed in one process: B = 64,
3 x 256 x 256, s = 4, bicubic (K = 16) and Gaussian (K = 16, sigma = 3).

Entries (all interleaved group by group, each group of `--inner` back-to-back passes bracketed by
device events after a warm-up; the figures are the median and the quartiles over `--repeats`
groups, successive passes rotating over `--sets` buffer sets), per tap set:
  dps_sr           sp_dps_residual_ws on the new kind: five launches, the middle one on the H / s
                   lattice rows alone
  pgdm_fused       sp_pgdm_residual_ws: v = -2 A^+ (y - A x0), the same five launches with P
  pgdm_composed    the same v from sp_predict_x0, sp_op_apply_ws, a subtraction, sp_op_pinv_ws, a scale
  pgdm_torch_fft   the same v with torch.fft on the device (rfft2, M, the lattice, zero insertion,
                   rfft2, P, irfft2)
  step_fused       sp_diffpir_step_ws: the DiffPIR sample with the caller's xi
  step_composed    sp_predict_x0, sp_op_prox_ws and the update in torch
  step_torch_fft   the same sample with torch.fft on the device
and once:
  dps_periodic     sp_dps_residual_ws of PeriodicBlurOperator (SP_OP_PSF_PERIODIC) on the same
                   image with a Gaussian 17 x 17 PSF: the unchanged kernel that does full-height
                   work in its middle launch.
Acceptance (recorded as "acceptance"): each dps_sr median is at most the dps_periodic median x
(1 + the relative interquartile range of the dps_periodic groups of this run).
    python tools/bench_sr_periodic.py [--out profiles/bench_sr_periodic.json]
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
from samplers_amd.operators import PeriodicBlurOperator, PeriodicSuperResolutionOperator  # noqa: E402


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_sr_periodic.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_sr_periodic.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b, s = 3, a.size, a.batch, a.factor
    shape = (C, S, S)
    n, m, L = C * S * S, C * (S // s) ** 2, S // s
    a_t = 0.31
    k_t = (1 - a_t**2) ** 0.5
    pgdm = _hip.SpDpsCoefs(a_t, k_t, -2.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    dps = _hip.SpDpsCoefs(a_t, k_t, 400.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    vals = dict(a=a_t, k=k_t, a_prev=0.9, c_eps=0.35, c_xi=0.25)
    rho = 0.37
    prox = _hip.SpProxCoefs(a_t, k_t, rho, vals["a_prev"], vals["c_eps"], vals["c_xi"])
    stream = torch.cuda.current_stream().cuda_stream

    ops = {"bicubic": PeriodicSuperResolutionOperator.bicubic(shape, s).to(dev),
           "gaussian": PeriodicSuperResolutionOperator.gaussian(shape, s, 16, 3.0).to(dev)}
    blur = PeriodicBlurOperator.gaussian(shape, 17, 3.0).to(dev)
    dblur = blur.hip_descriptor()
    descs = {k: op.hip_descriptor() for k, op in ops.items()}
    work_floats = int(lib.sp_dps_workspace(dblur, b))
    assert all(int(lib.sp_dps_workspace(d, b)) == work_floats for d in descs.values())
    half = {k: dict(M=op._half(0), P=op._half(1), lam=op.lambda_half) for k, op in ops.items()}

    sets = []
    for _ in range(a.sets):
        x, eps, xi, yb = (torch.randn(b, n, device=dev) for _ in range(4))
        y = torch.randn(b, m, device=dev)
        st = dict(x=x, eps=eps, xi=xi, y=y, yb=yb, v=torch.empty(b, n, device=dev),
                  work=torch.empty(work_floats, device=dev), q=torch.empty(work_floats, device=dev),
                  t0=torch.empty(b, n, device=dev), t1=torch.empty(b, m, device=dev),
                  t2=torch.empty(b, m, device=dev))
        # q holds y itself for this kind, whichever prepare wrote it and whatever the taps
        _hip.check(lib.sp_pgdm_prepare(descs["bicubic"], y.data_ptr(), b, st["q"].data_ptr(), stream),
                   "sp_pgdm_prepare")
        sets.append(st)
    turn = [0]

    def next_set():
        st = sets[turn[0] % a.sets]
        turn[0] += 1
        return st

    def up(t):
        out = torch.zeros(b, C, S, S, device=dev)
        out[..., ::s, ::s] = t.view(b, C, L, L)
        return out

    def torch_residual(name, st):
        """x0 and y - A x0 on the lattice with torch.fft."""
        x0 = ((st["x"] - k_t * st["eps"]) / a_t).view(b, C, S, S)
        ax = torch.fft.irfft2(torch.fft.rfft2(x0) * half[name]["M"], s=(S, S))[..., ::s, ::s]
        return x0, st["y"].view(b, C, L, L) - ax

    def make(name):
        d = descs[name]
        part = torch.empty(b, int(lib.sp_rsq_partials(d)), device=dev)

        def dps_sr():
            st = next_set()
            _hip.check(lib.sp_dps_residual_ws(d, st["x"].data_ptr(), st["eps"].data_ptr(),
                                              st["y"].data_ptr(), b, 1, dps, st["v"].data_ptr(),
                                              part.data_ptr(), st["work"].data_ptr(), stream),
                       "sp_dps_residual_ws")
            return st["v"]

        def pgdm_fused():
            st = next_set()
            _hip.check(lib.sp_pgdm_residual_ws(d, st["x"].data_ptr(), st["eps"].data_ptr(),
                                               st["q"].data_ptr(), b, 1, pgdm, st["v"].data_ptr(),
                                               st["work"].data_ptr(), stream), "sp_pgdm_residual_ws")
            return st["v"]

        def pgdm_composed():
            st = next_set()
            _hip.check(lib.sp_predict_x0(st["x"].data_ptr(), st["eps"].data_ptr(), b * n, a_t, k_t,
                                         st["t0"].data_ptr(), stream), "sp_predict_x0")
            _hip.check(lib.sp_op_apply_ws(d, st["t0"].data_ptr(), st["t1"].data_ptr(), b,
                                          st["work"].data_ptr(), stream), "sp_op_apply_ws")
            torch.sub(st["y"], st["t1"], out=st["t2"])
            _hip.check(lib.sp_op_pinv_ws(d, st["t2"].data_ptr(), st["t0"].data_ptr(), b, 0,
                                         st["work"].data_ptr(), stream), "sp_op_pinv_ws")
            torch.mul(st["t0"], -2.0, out=st["v"])
            return st["v"]

        def pgdm_torch_fft():
            st = next_set()
            _, r = torch_residual(name, st)
            z = torch.fft.rfft2(up(r)) * half[name]["P"]
            return (-2.0 * torch.fft.irfft2(z, s=(S, S))).reshape(b, n)

        def update(x, z, xi):
            return vals["a_prev"] * z + (vals["c_eps"] * ((x - a_t * z) / k_t) + vals["c_xi"] * xi)

        def step_fused():
            st = next_set()
            _hip.check(lib.sp_diffpir_step_ws(d, st["x"].data_ptr(), st["eps"].data_ptr(), None,
                                              st["q"].data_ptr(), st["xi"].data_ptr(), 0, 0, 0, b, 1,
                                              prox, st["v"].data_ptr(), st["work"].data_ptr(), stream),
                       "sp_diffpir_step_ws")
            return st["v"]

        def step_composed():
            st = next_set()
            _hip.check(lib.sp_predict_x0(st["x"].data_ptr(), st["eps"].data_ptr(), b * n, a_t, k_t,
                                         st["t0"].data_ptr(), stream), "sp_predict_x0")
            _hip.check(lib.sp_op_prox_ws(d, st["t0"].data_ptr(), None, st["q"].data_ptr(), b, 1, rho,
                                         st["v"].data_ptr(), st["work"].data_ptr(), stream),
                       "sp_op_prox_ws")
            return update(st["x"], st["v"], st["xi"])

        def step_torch_fft():
            st = next_set()
            x0, r = torch_residual(name, st)
            mult = half[name]["M"].conj() / (half[name]["lam"] + rho)
            z = x0 + torch.fft.irfft2(torch.fft.rfft2(up(r)) * mult, s=(S, S))
            return update(st["x"], z.reshape(b, n), st["xi"])

        return {"dps_sr": dps_sr, "pgdm_fused": pgdm_fused, "pgdm_composed": pgdm_composed,
                "pgdm_torch_fft": pgdm_torch_fft, "step_fused": step_fused,
                "step_composed": step_composed, "step_torch_fft": step_torch_fft}

    part_blur = torch.empty(b, int(lib.sp_rsq_partials(dblur)), device=dev)

    def dps_periodic():
        st = next_set()
        _hip.check(lib.sp_dps_residual_ws(dblur, st["x"].data_ptr(), st["eps"].data_ptr(),
                                          st["yb"].data_ptr(), b, 1, dps, st["v"].data_ptr(),
                                          part_blur.data_ptr(), st["work"].data_ptr(), stream),
                   "sp_dps_residual_ws")
        return st["v"]

    entries = {"dps_periodic": dps_periodic}
    for name in ops:
        for k, fn in make(name).items():
            entries[f"{name}.{k}"] = fn

    # the entries of one group compute the same thing (checked once, on one buffer set)
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    agree = {}
    for name in ops:
        for fam in ("pgdm", "step"):
            ref = first(f"{name}.{fam}_fused")
            for other in ("composed", "torch_fft"):
                got = first(f"{name}.{fam}_{other}")
                agree[f"{name}.{fam}_{other}"] = float((got - ref).abs().max() / ref.abs().max())

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

    row = {"bench": "sr_periodic_dps_pgdm_diffpir", "batch": b, "shape": list(shape), "factor": s,
           "taps": {"bicubic": 4 * s, "gaussian": [16, 3.0]}, "periodic_blur_psf": [17, 3.0],
           "kept": {k: [int(op.keep.sum()), op.keep.numel()] for k, op in ops.items()},
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "max_diff_over_max_vs_fused": agree}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
    base = row["dps_periodic"]
    rel_iqr = (base["us_q3"] - base["us_q1"]) / base["us"]
    bar = base["us"] * (1 + rel_iqr)
    row["acceptance"] = {"dps_periodic_us": base["us"], "relative_iqr": round(rel_iqr, 4),
                         "bar_us": round(bar, 1),
                         "met": {k: row[f"{k}.dps_sr"]["us"] <= bar for k in ops}}
    row["ratios"] = {}
    for name in ops:
        row["ratios"][f"{name}.dps_sr_over_dps_periodic"] = round(row[f"{name}.dps_sr"]["us"] / base["us"], 3)
        for fam in ("pgdm", "step"):
            for other in ("composed", "torch_fft"):
                row["ratios"][f"{name}.{fam}_{other}_over_fused"] = round(
                    row[f"{name}.{fam}_{other}"]["us"] / row[f"{name}.{fam}_fused"]["us"], 3)
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")
    if not all(row["acceptance"]["met"].values()):
        sys.exit("acceptance not met: a dps_sr median exceeds the periodic bar")


if __name__ == "__main__":
    main()
