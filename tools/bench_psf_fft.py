"""DPS pass 1 for the FFT-domain PSF blur (sp_dps_residual_ws on an SP_OP_PSF_FFT descriptor: the
five launches of csrc/sp_psf_fft.hip) against the direct SP_OP_PSF pass and a torch.fft chain that
produce the same v = A^T(grad_scale (y - A x0)) and |r|^2 on the device, timed in one process:
B = 64, 3 x 256 x 256 by default, reflect padding.

Entries (all interleaved group by group, each group of `--inner` back-to-back passes bracketed by
device events after a warm-up; the figures are the median and the quartiles over `--repeats`
groups, successive passes rotating over `--sets` buffer sets):
  fft_R{4,15,30}_dense   the new kind, a dense (all taps non-zero) PSF
  fft_R30_motion         the new kind, motion_blur_kernel(61, 0.5, 0) (its cost ignores sparsity)
  fft_R{64,127}_dense    the new kind alone, beyond the direct kernel's radius cap
  direct_R{4,8,12,15,20,30}_dense, direct_R30_motion
                         the SP_OP_PSF pass (csrc/sp_psf.hip), for the crossover radius
  torch_fft_R{4,15,30}   F.pad(reflect), rfft2, times the precomputed spectrum, irfft2, crop, and
                         its autograd adjoint, handed x0 already formed (which favours it)
The transform sizes of the new kind depend on R only through the padded size (256 + 2R -> 384 up
to R = 64, 512 at R = 127), so its time is flat in R where the direct kernel's grows with K^2.
Per-launch times of the new kind come from the library's dispatch-packet events
(sp_timing_enable), collected in separate passes after the timed groups so that the events do not
sit in the timed figures.
    python tools/bench_psf_fft.py [--out profiles/bench_psf_fft.json]
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
import torch.nn.functional as F  # noqa: E402

from samplers_amd import _hip  # noqa: E402
from samplers_amd.operators import FFTPSFBlurOperator, PSFBlurOperator, motion_blur_kernel  # noqa: E402

LAUNCHES = ("rows", "columns_A", "rows_inv_rows", "columns_AT", "rows_inv_AT")


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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_psf_fft.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_psf_fft.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    a_t, gs = 0.31, 400.0
    coefs = _hip.SpDpsCoefs(a_t, (1 - a_t**2) ** 0.5, gs, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream

    fft_radii, direct_radii, torch_radii = (4, 15, 30, 64, 127), (4, 8, 12, 15, 20, 30), (4, 15, 30)
    kernels = {r: dense_kernel(r) for r in sorted(set(fft_radii) | set(direct_radii))}
    motion = motion_blur_kernel(61, 0.5, 0)
    ops = {}
    for r in fft_radii:
        ops[f"fft_R{r}_dense"] = FFTPSFBlurOperator(shape, kernels[r]).to(dev)
    ops["fft_R30_motion"] = FFTPSFBlurOperator(shape, motion).to(dev)
    for r in direct_radii:
        ops[f"direct_R{r}_dense"] = PSFBlurOperator(shape, kernels[r]).to(dev)
    ops["direct_R30_motion"] = PSFBlurOperator(shape, motion).to(dev)
    descs = {k: op.hip_descriptor() for k, op in ops.items()}
    work_floats = max(int(lib.sp_dps_workspace(d, b)) for d in descs.values())

    sets = []
    for _ in range(a.sets):
        x, eps, y = (torch.randn(b, n, device=dev) for _ in range(3))
        v, work = torch.empty(b, n, device=dev), torch.empty(work_floats, device=dev)
        x0 = ((x - coefs.k * eps) / coefs.a).view(b, C, S, S)
        sets.append(dict(x=x, eps=eps, y=y, v=v, work=work, x0=x0))
    turn = [0]

    def next_set():
        s = sets[turn[0] % a.sets]
        turn[0] += 1
        return s

    entries = {}

    def add_hip(name):
        desc = descs[name]
        part = torch.empty(b, int(lib.sp_rsq_partials(desc)), device=dev)

        def run():
            s = next_set()
            _hip.check(lib.sp_dps_residual_ws(desc, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), b, 1, coefs, s["v"].data_ptr(),
                                              part.data_ptr(), s["work"].data_ptr(), stream),
                       "sp_dps_residual_ws")
            return s["v"], part.sum(1)

        entries[name] = run

    def add_torch_fft(name, h):
        r = h.shape[0] // 2
        size = (S + 2 * r, S + 2 * r)
        hf = torch.fft.rfft2(h.to(dev), s=size).conj()

        def run():
            s = next_set()
            x0 = s["x0"].detach().requires_grad_(True)
            p = F.pad(x0, (r, r, r, r), mode="reflect")
            z = torch.fft.irfft2(torch.fft.rfft2(p) * hf, s=size)[..., :S, :S]
            res = s["y"].view(b, C, S, S) - z
            rsq = res.detach().square().sum(dim=(1, 2, 3))
            (v,) = torch.autograd.grad(z, x0, grad_outputs=gs * res.detach())
            return v, rsq

        entries[name] = run

    for name in ops:
        add_hip(name)
    for r in torch_radii:
        add_torch_fft(f"torch_fft_R{r}", kernels[r])

    # the entries of one radius compute the same thing (checked once, on one buffer set)
    agree = {}
    for r in torch_radii:
        turn[0] = 0
        v_new, rsq_new = entries[f"fft_R{r}_dense"]()
        v_new, rsq_new = v_new.clone().view(b, C, S, S), rsq_new.clone()
        for other in (f"direct_R{r}_dense", f"torch_fft_R{r}"):
            turn[0] = 0
            v, rsq = entries[other]()
            agree[other] = {
                "v_max_diff_over_max": float((v.reshape(v_new.shape) - v_new).abs().max() / v_new.abs().max()),
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

    # per-launch times of the new kind: the five kind-1 records of each pass, in launch order
    per_launch = {}
    kinds, ms = (ctypes.c_int32 * 64)(), (ctypes.c_float * 64)()
    for name in (k for k in entries if k.startswith("fft_")):
        cols = [[] for _ in LAUNCHES]
        lib.sp_timing_enable(1)
        for _ in range(a.repeats):
            entries[name]()
            got = lib.sp_timing_collect(kinds, ms, 64)
            if got == len(LAUNCHES):
                for i in range(got):
                    cols[i].append(ms[i] * 1e3)
        lib.sp_timing_enable(0)
        per_launch[name] = {l: round(statistics.median(c), 1) for l, c in zip(LAUNCHES, cols) if c}

    row = {"bench": "psf_fft_dps_pass1", "batch": b, "shape": list(shape), "padding": "reflect",
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "padded_sizes": {k: list(op.padded_shape) for k, op in ops.items() if k.startswith("fft_")},
           "work_floats_per_sample": {k: int(lib.sp_dps_workspace(descs[k], 1)) for k in ops},
           "agreement_with_fft_dense": agree, "per_launch_us": per_launch}
    for name in entries:
        t = statistics.median(times[name])
        q1, q3 = quartiles(times[name])
        row[name] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                     "us_min": round(min(times[name]) * 1e6, 1),
                     "us_max": round(max(times[name]) * 1e6, 1)}
    new = row["fft_R30_dense"]
    verdict = {}
    for other in ("direct_R30_dense", "torch_fft_R30"):
        o = row[other]
        spread = max(new["us_q3"] - new["us_q1"], o["us_q3"] - o["us_q1"])
        verdict[other] = {"ratio_new_over_other": round(new["us"] / o["us"], 4),
                          "gap_us": round(o["us"] - new["us"], 1), "iqr_us": round(spread, 1),
                          "met": bool(o["us"] - new["us"] > spread)}
    row["requirement"] = "fft_R30_dense below direct_R30_dense and torch_fft_R30 by more than the IQR"
    row["requirement_met"] = verdict
    # first measured radius at which the new pass is the faster one (its time is flat up to R = 64)
    flat = statistics.median(row[f"fft_R{r}_dense"]["us"] for r in (4, 15, 30))
    faster = [r for r in direct_radii if row[f"direct_R{r}_dense"]["us"] > flat]
    row["crossover"] = {"fft_us_flat_R<=64": round(flat, 1),
                        "direct_us": {str(r): row[f"direct_R{r}_dense"]["us"] for r in direct_radii},
                        "first_measured_radius_fft_faster": faster[0] if faster else None}
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
