"""DPS pass 1 for Fourier phase retrieval (sp_dps_residual_ws: the three launches of
csrc/sp_phase.hip) against what a user has without the native kind — F.pad + torch.fft.fft2 + abs
and its autograd backward on the device — producing the same v = J(x0)^T(grad_scale (y - |z|)) and
|r|^2, timed in one process: B = 64, 3 x 256 x 256, pad 64 (384 x 384 planes) by default.

Entries (interleaved group by group, each group of `--inner` back-to-back passes bracketed by
device events after a warm-up; the figure is the median over `--repeats` groups):
  phase_hip     the HIP pass
  phase_torch   the torch chain, handed x0 already formed (the HIP pass forms it from x and eps
                while staging), which favours it
Successive passes rotate over `--sets` buffer sets.  Bytes are the HIP plan's compulsory traffic:
x, eps and v (n each), y (m), and the H x Nw complex intermediate written by the row launch, read
and rewritten by the column launch and read by the inverse row launch (4 x 2 C Nw H).
    python tools/bench_phase.py [--out profiles/bench_phase.json]
prints one JSON line and writes it to --out."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from samplers_amd import _hip  # noqa: E402
from samplers_amd.operators import PhaseRetrievalOperator  # noqa: E402

COPY_RATE = 6.29e12  # B / s: the project's measured float4 copy rate on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--pad", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_phase.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_phase.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, p, b = 3, a.size, a.pad, a.batch
    shape = (C, S, S)
    op = PhaseRetrievalOperator(shape, pad=p).to(dev)
    desc = op.hip_descriptor()
    n, m = int(desc.n), int(desc.m)
    N = S + 2 * p
    a_t, gs = 0.31, 400.0
    coefs = _hip.SpDpsCoefs(a_t, (1 - a_t**2) ** 0.5, gs, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream
    floats = int(lib.sp_dps_workspace(desc, b))
    P = int(lib.sp_rsq_partials(desc))
    part = torch.empty(b, P, device=dev)

    sets = []
    for _ in range(a.sets):
        x, eps = (torch.randn(b, n, device=dev) for _ in range(2))
        y = torch.rand(b, m, device=dev)
        v, work = torch.empty(b, n, device=dev), torch.empty(floats, device=dev)
        x0 = ((x - coefs.k * eps) / coefs.a).view(b, C, S, S)
        sets.append(dict(x=x, eps=eps, y=y, v=v, work=work, x0=x0))
    turn = [0]

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
        return s["v"], part

    def run_torch():
        s = next_set()
        x0 = s["x0"].detach().requires_grad_(True)
        mag = torch.fft.fft2(F.pad(x0, (p, p, p, p)), norm="ortho").abs()
        res = s["y"].view(b, C, N, N) - mag
        rsq = res.detach().square().sum(dim=(1, 2, 3))
        (v,) = torch.autograd.grad(mag, x0, grad_outputs=gs * res.detach())
        return v.reshape(b, n), rsq

    entries = {"phase_hip": run_hip, "phase_torch": run_torch}
    # the yardstick computes what the HIP pass computes (checked once, on one buffer set)
    turn[0] = 0
    v_hip, rsq_hip = run_hip()
    v_hip, rsq_hip = v_hip.clone(), rsq_hip.sum(1)
    turn[0] = 0
    v_t, rsq_t = run_torch()
    agree = {"v_max_diff_over_max": float((v_t - v_hip).abs().max() / v_hip.abs().max()),
             "rsq_max_rel_diff": float((rsq_t / rsq_hip - 1).abs().max())}
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
    bytes_moved = 4.0 * b * (3 * n + m + 4 * 2 * C * N * S)
    row = {"bench": "phase_dps_pass1", "batch": b, "shape": list(shape), "pad": p,
           "padded": [N, N], "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "partials_per_sample": P, "workspace_bytes": 4 * floats, "plan_bytes": bytes_moved,
           "copy_rate": COPY_RATE, "yardstick_agreement": agree}
    for name in entries:
        t = statistics.median(times[name])
        row[name] = {"us": round(t * 1e6, 1), "us_min": round(min(times[name]) * 1e6, 1),
                     "us_max": round(max(times[name]) * 1e6, 1)}
    t_hip = row["phase_hip"]["us"] * 1e-6
    row["phase_hip"]["launches"] = 3
    row["phase_hip"]["plan_TBps"] = round(bytes_moved / t_hip / 1e12, 3)
    row["phase_hip"]["copy_rate_fraction"] = round(bytes_moved / t_hip / COPY_RATE, 4)
    row["hip_over_torch"] = round(row["phase_hip"]["us"] / row["phase_torch"]["us"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
