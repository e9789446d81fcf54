"""DPS pass 1 (sp_dps_residual) for x s super-resolution against the identity-kind pass, timed in
one process on the same buffers' worth of traffic: B = 64, 3 x 256 x 256, s = 4 by default.

The two kinds alternate launch by launch groups (SR, identity, SR, ...), each group of `--inner`
back-to-back launches bracketed by device events, after a warm-up; the figure is the median over
`--repeats` groups of the per-launch time.  Successive launches rotate over `--sets` input /
output buffer sets, more bytes than the 256 MiB Infinity Cache holds, so the passes stream from
HBM as they do between the prior's forward and VJP.  Bytes are the algorithm's: x, eps read and
v written (3 x 4n) plus the observation (4n / s^2 for SR, 4n for identity) per sample.
    python tools/bench_sr.py [--batch 64] [--size 256] [--factor 4] [--out profiles/bench_sr.json]
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
from samplers_amd.operators import IdentityOperator, SuperResolutionOperator  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_sr.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_sr.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    shape, b, s = (3, a.size, a.size), a.batch, a.factor
    ops = {"sr": SuperResolutionOperator(shape, s).to(dev), "identity": IdentityOperator(shape)}
    descs = {k: op.hip_descriptor() for k, op in ops.items()}
    n = int(descs["sr"].n)
    coefs = _hip.SpDpsCoefs(0.31, (1 - 0.31**2) ** 0.5, 400.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    sets = []
    for _ in range(a.sets):
        x, eps, v = (torch.randn(b, n, device=dev) for _ in range(3))
        ys = {k: torch.randn(b, int(d.m), device=dev) for k, d in descs.items()}
        parts = {k: torch.empty(b, int(lib.sp_rsq_partials(d)), device=dev) for k, d in descs.items()}
        sets.append((x, eps, v, ys, parts))
    stream = torch.cuda.current_stream().cuda_stream
    turn = [0]

    def launch(kind):
        x, eps, v, ys, parts = sets[turn[0] % a.sets]
        turn[0] += 1
        _hip.check(lib.sp_dps_residual(descs[kind], x.data_ptr(), eps.data_ptr(),
                                       ys[kind].data_ptr(), b, 1, coefs, v.data_ptr(),
                                       parts[kind].data_ptr(), stream), "sp_dps_residual")

    for _ in range(a.warmup):
        for kind in descs:
            for _ in range(a.inner):
                launch(kind)
    torch.cuda.synchronize()
    times = {k: [] for k in descs}
    for _ in range(a.repeats):
        for kind in descs:  # interleaved: SR, identity, SR, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                launch(kind)
            e1.record()
            e1.synchronize()
            times[kind].append(e0.elapsed_time(e1) * 1e-3 / a.inner)
    nbytes = {"sr": (3.0 + 1.0 / (s * s)) * 4 * n * b, "identity": 16.0 * n * b}
    row = {"bench": "sr_dps_residual", "batch": b, "shape": list(shape), "factor": s,
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version())}
    for kind in descs:
        t = statistics.median(times[kind])
        row[kind] = {"us": round(t * 1e6, 2), "us_min": round(min(times[kind]) * 1e6, 2),
                     "us_max": round(max(times[kind]) * 1e6, 2), "bytes": int(nbytes[kind]),
                     "GBps": round(nbytes[kind] / t / 1e9, 1),
                     "hbm_fraction": round(nbytes[kind] / t / HBM_PEAK, 3)}
    row["sr_over_identity"] = round(row["sr"]["us"] / row["identity"]["us"], 3)
    row["bound"] = 1.10
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
