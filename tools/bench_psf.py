"""DPS pass 1 for the point-spread-function blur (sp_dps_residual_ws: the `residual` and `adjoint`
launches of csrc/sp_psf.hip) against yardsticks that produce the same v = A^T(grad_scale (y - A x0))
and |r|^2 on the device, timed in one process: B = 64, 3 x 256 x 256 by default.

Entries (all interleaved group by group, each group of `--inner` back-to-back passes bracketed
by device events after a warm-up; the figure is the median over `--repeats` groups):
  psf_R{4,15,30}_dense   the HIP pass, a dense (all taps non-zero) PSF
  psf_R30_motion         the HIP pass, motion_blur_kernel(61, 0.5, 0): work follows the support
  torch_R{4,15,30}       (a) F.pad(reflect) + F.conv2d(groups=C) and its autograd adjoint — what
                         GenericDPSStep costs today for such an operator
  fft_R{4,15,30}         (b) the same two maps through torch.fft (the PSF's spectrum precomputed)
  gauss_R4               (c) the separable GaussianBlurOperator pass (sp_dps_residual), 9 x 9
The yardsticks are handed x0 already formed (the HIP pass forms it from x and eps while staging),
which favours them.  Successive passes rotate over `--sets` buffer sets.  FLOPs are
2 * (taps swept) * n * B per direction: K^2 for a dense PSF and for (a) / (b), the taps between
the first and last non-zero column of every tap row for the motion PSF, 2 K for (c).
    python tools/bench_psf.py [--out profiles/bench_psf.json]
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
from samplers_amd.operators import GaussianBlurOperator, PSFBlurOperator, motion_blur_kernel  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12  # FLOP / s (MI355X, packed fp32 FMA)


def dense_kernel(radius: int) -> torch.Tensor:
    k = 2 * radius + 1
    h = torch.rand(k, k, generator=torch.Generator().manual_seed(radius), dtype=torch.float64) + 0.05
    return (h / h.sum()).to(torch.float32)


def taps_swept(h: torch.Tensor) -> int:
    """Taps between the first and last non-zero column of every tap row (all-zero rows: none)."""
    total = 0
    for row in h:
        nz = torch.nonzero(row).flatten()
        if nz.numel():
            total += int(nz[-1] - nz[0]) + 1
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--psf-only", action="store_true",
                    help="time the HIP entries alone (kernel work; no yardsticks, no ratios)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_psf.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("--repeats must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_psf.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    a_t, gs = 0.31, 400.0
    coefs = _hip.SpDpsCoefs(a_t, (1 - a_t**2) ** 0.5, gs, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream

    sets = []
    for _ in range(a.sets):
        x, eps, y = (torch.randn(b, n, device=dev) for _ in range(3))
        v, work = torch.empty(b, n, device=dev), torch.empty(b * n, device=dev)
        x0 = ((x - coefs.k * eps) / coefs.a).view(b, C, S, S)
        sets.append(dict(x=x, eps=eps, y=y, v=v, work=work, x0=x0))
    turn = [0]

    def next_set():
        s = sets[turn[0] % a.sets]
        turn[0] += 1
        return s

    entries, flops, launches = {}, {}, {}

    def add_psf(name, h):
        op = PSFBlurOperator(shape, h).to(dev)
        desc = op.hip_descriptor()
        part = torch.empty(b, int(lib.sp_rsq_partials(desc)), device=dev)
        assert int(lib.sp_dps_workspace(desc, b)) == b * n

        def run():
            s = next_set()
            _hip.check(lib.sp_dps_residual_ws(desc, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), b, 1, coefs, s["v"].data_ptr(),
                                              part.data_ptr(), s["work"].data_ptr(), stream),
                       "sp_dps_residual_ws")
            return s["v"], part

        run.keep = op
        entries[name], flops[name], launches[name] = run, 2.0 * taps_swept(h) * n * b, 2

    def add_torch(name, h):
        k = h.shape[0]
        r = k // 2
        wgt = h.to(dev).view(1, 1, k, k).repeat(C, 1, 1, 1).contiguous()

        def run():
            s = next_set()
            x0 = s["x0"].detach().requires_grad_(True)
            z = F.conv2d(F.pad(x0, (r, r, r, r), mode="reflect"), wgt, groups=C)
            res = s["y"].view(b, C, S, S) - z
            rsq = res.detach().square().sum(dim=(1, 2, 3))
            (v,) = torch.autograd.grad(z, x0, grad_outputs=gs * res.detach())
            return v, rsq

        entries[name], flops[name], launches[name] = run, 2.0 * k * k * n * b, None

    def add_fft(name, h):
        k = h.shape[0]
        r = k // 2
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

        entries[name], flops[name], launches[name] = run, 2.0 * k * k * n * b, None

    def add_gauss(name, ksize, sigma):
        op = GaussianBlurOperator(shape, ksize, sigma).to(dev)
        desc = op.hip_descriptor()
        part = torch.empty(b, int(lib.sp_rsq_partials(desc)), device=dev)

        def run():
            s = next_set()
            _hip.check(lib.sp_dps_residual(desc, s["x"].data_ptr(), s["eps"].data_ptr(),
                                           s["y"].data_ptr(), b, 1, coefs, s["v"].data_ptr(),
                                           part.data_ptr(), stream), "sp_dps_residual")
            return s["v"], part

        run.keep = op
        entries[name], flops[name], launches[name] = run, 2.0 * 2 * ksize * n * b, 1

    kernels = {r: dense_kernel(r) for r in (4, 15, 30)}
    motion = motion_blur_kernel(61, 0.5, 0)
    for r, h in kernels.items():
        add_psf(f"psf_R{r}_dense", h)
    add_psf("psf_R30_motion", motion)
    for r, h in ({} if a.psf_only else kernels).items():
        add_torch(f"torch_R{r}", h)
        add_fft(f"fft_R{r}", h)
    add_gauss("gauss_R4", 9, 3.0)

    # the yardsticks compute what the HIP pass computes (checked once, on one buffer set)
    agree = {}
    for r in ({} if a.psf_only else kernels):
        turn[0] = 0
        v_hip, part = entries[f"psf_R{r}_dense"]()
        v_hip, rsq_hip = v_hip.clone().view(b, C, S, S), part.sum(1)
        for kind in ("torch", "fft"):
            turn[0] = 0
            v, rsq = entries[f"{kind}_R{r}"]()
            agree[f"{kind}_R{r}"] = {
                "v_max_diff_over_max": float((v - v_hip).abs().max() / v_hip.abs().max()),
                "rsq_max_rel_diff": float((rsq / rsq_hip - 1).abs().max())}
    failed = {}
    for _ in range(a.warmup):
        for name, run in list(entries.items()):
            try:
                for _ in range(a.inner):
                    run()
            except RuntimeError as exc:  # a yardstick the backend cannot run: recorded, not timed
                failed[name] = str(exc).splitlines()[0][:200]
                del entries[name]
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
    row = {"bench": "psf_dps_pass1", "batch": b, "shape": list(shape), "repeats": a.repeats,
           "inner": a.inner, "buffer_sets": a.sets, "device": torch.cuda.get_device_name(0),
           "sp_version": int(lib.sp_version()), "fp32_vector_peak": FP32_VECTOR_PEAK,
           "motion_taps_swept": taps_swept(motion), "motion_taps_nonzero": int((motion != 0).sum()),
           "yardstick_agreement": agree, "failed": failed}
    for name in entries:
        t = statistics.median(times[name])
        fl = 2.0 * flops[name]  # both directions
        row[name] = {"us": round(t * 1e6, 1), "us_min": round(min(times[name]) * 1e6, 1),
                     "us_max": round(max(times[name]) * 1e6, 1), "launches": launches[name],
                     "us_per_launch": round(t * 1e6 / launches[name], 1) if launches[name] else None,
                     "flops": fl, "TFLOPs": round(fl / t / 1e12, 2),
                     "peak_fraction": round(fl / t / FP32_VECTOR_PEAK, 4)}
    for r in kernels:
        for kind in ("torch", "fft"):
            if f"{kind}_R{r}" in entries:
                row[f"psf_over_{kind}_R{r}"] = round(row[f"psf_R{r}_dense"]["us"] / row[f"{kind}_R{r}"]["us"], 4)
    if "gauss_R4" in entries:
        row["psf_over_gauss_R4"] = round(row["psf_R4_dense"]["us"] / row["gauss_R4"]["us"], 3)
    row["requirement"] = "psf_over_torch_R{4,15,30} < 1"
    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
