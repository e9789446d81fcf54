"""The DiffPIR step after the network call (sp_diffpir_step_ws: x0, the proximal data step, the
update) for the three operator families with a closed-form prox, timed in one process at B = 64,
3 x 256 x 256: inpaint 50 %, SR x4 and the periodic blur with a dense R = 30 PSF.

Entries per operator (all interleaved group by group, each group of `--inner` back-to-back passes
bracketed by device events after a warm-up; the figures are the median and the quartiles over
`--repeats` groups, successive passes rotating over `--sets` buffer sets):
  fused      sp_diffpir_step_ws with in-kernel Philox noise: one launch (inpaint, SR) or three
             (periodic: rows, columns with the prox multiplier, rows^-1 with the update epilogue;
             q = conj(M) FFT2(y) prepared once outside the timed region, as the sampler does)
  composed   the same x' from sp_predict_x0, sp_op_prox_ws, sp_randn and torch elementwise
             operations for eps_hat and the update
  torch_fft  (periodic only) x0, rfft2, (Q + rho X0) / (|M|^2 + rho), irfft2 and the update with
             torch.fft on the device, handed the precomputed Q and |M|^2
and the yardstick of the elementwise launch, timed in the same run on the inpainting operator:
  dps_update sp_dps_update re-deriving v (the DPS pass 2 of the headline workload).
Each entry carries its algorithmic HBM bytes (fp32; per launch for the fused periodic step) and
their rate as a fraction of the 8 TB/s HBM specification.  The new launches carry no
dispatch-packet timing kind, so the periodic step's three launches are timed together.

--network ddpm also times a whole DiffPIR step against a whole DPS step (network forward, and for
DPS its input VJP) on the headline configuration: the DDPM UNet, inpaint 50 %, the same batch.

    python tools/bench_diffpir.py [--out profiles/bench_diffpir.json]
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
from samplers_amd.operators import (PeriodicBlurOperator, RandomInpaintingOperator,  # noqa: E402
                                    SuperResolutionOperator)

HBM_BYTES_PER_S = 8.0e12


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
    ap.add_argument("--network", choices=("none", "ddpm"), default="none")
    ap.add_argument("--network-steps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_diffpir.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_diffpir.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    a_t, rho = 0.31, 0.05
    k_t = (1 - a_t**2) ** 0.5
    cf = dict(a=a_t, k=k_t, a_prev=0.45, c_eps=0.75, c_xi=0.49)
    coefs = _hip.SpProxCoefs(cf["a"], cf["k"], rho, cf["a_prev"], cf["c_eps"], cf["c_xi"])
    dps = _hip.SpDpsCoefs(a_t, k_t, 400.0, 0.97, 0.11, 0.05, 1.0, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    ops = {"inpaint": RandomInpaintingOperator(shape, 0.5, seed=1).to(dev),
           "sr4": SuperResolutionOperator(shape, 4).to(dev),
           "periodic": PeriodicBlurOperator(shape, dense_kernel(a.radius)).to(dev)}
    descs = {k: op.hip_descriptor() for k, op in ops.items()}
    hw = S // 2 + 1
    m2 = None

    sets = {name: [] for name in ops}
    for name, op in ops.items():
        d = descs[name]
        m = int(d.m)
        work_floats = int(lib.sp_prox_workspace(d, b))
        q_floats = int(lib.sp_prox_prepare_size(d, b))
        for _ in range(a.sets):
            x, eps, w = (torch.randn(b, n, device=dev) for _ in range(3))
            y = torch.randn(b, m, device=dev)
            s = dict(x=x, eps=eps, w=w, y=y, out=torch.empty(b, n, device=dev),
                     t0=torch.empty(b, n, device=dev), t1=torch.empty(b, n, device=dev),
                     xi=torch.empty(b, n, device=dev),
                     work=torch.empty(max(work_floats, 4), device=dev),
                     q=torch.empty(max(q_floats, 4), device=dev))
            _hip.check(lib.sp_prox_prepare(d, y.data_ptr(), b, s["q"].data_ptr(), stream),
                       "sp_prox_prepare")
            if name == "periodic":
                mh = torch.view_as_complex(op.spectra[0]).transpose(0, 1)  # (S, S / 2 + 1)
                m2 = (mh.abs() ** 2).contiguous()
                s["q_torch"] = mh.conj() * torch.fft.rfft2(y.view(b, C, S, S))
            sets[name].append(s)
    turn = [0]

    def next_set(name):
        s = sets[name][turn[0] % a.sets]
        turn[0] += 1
        return s

    def update(s, z):
        eh = (s["x"] - cf["a"] * z) / cf["k"]
        return cf["a_prev"] * z + (cf["c_eps"] * eh + cf["c_xi"] * s["xi"])

    def fused(name):
        d = descs[name]

        def run():
            s = next_set(name)
            _hip.check(lib.sp_diffpir_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), s["q"].data_ptr(), None, seed, step,
                                              0, b, 1, coefs, s["out"].data_ptr(),
                                              s["work"].data_ptr(), stream), "sp_diffpir_step_ws")
            return s["out"]

        return run

    def composed(name):
        d = descs[name]

        def run():
            s = next_set(name)
            _hip.check(lib.sp_predict_x0(s["x"].data_ptr(), s["eps"].data_ptr(), b * n, a_t, k_t,
                                         s["t0"].data_ptr(), stream), "sp_predict_x0")
            _hip.check(lib.sp_op_prox_ws(d, s["t0"].data_ptr(), s["y"].data_ptr(), s["q"].data_ptr(),
                                         b, 1, rho, s["t1"].data_ptr(), s["work"].data_ptr(), stream),
                       "sp_op_prox_ws")
            _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
            return update(s, s["t1"])

        return run

    def torch_fft():
        s = next_set("periodic")
        _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
        x0 = ((s["x"] - k_t * s["eps"]) / a_t).view(b, C, S, S)
        zs = (s["q_torch"] + rho * torch.fft.rfft2(x0)) / (m2 + rho)
        return update(s, torch.fft.irfft2(zs, s=(S, S)).reshape(b, n))

    def dps_update():
        s = next_set("inpaint")
        _hip.check(lib.sp_dps_update(descs["inpaint"], s["x"].data_ptr(), s["eps"].data_ptr(),
                                     s["y"].data_ptr(), None, s["w"].data_ptr(), None, None, seed,
                                     step, 0, b, 1, dps, s["out"].data_ptr(), stream), "sp_dps_update")
        return s["out"]

    entries = {"dps_update": dps_update}
    for name in ops:
        entries[f"{name}_fused"] = fused(name)
        entries[f"{name}_composed"] = composed(name)
    entries["periodic_torch_fft"] = torch_fft

    # the entries of one operator compute the same thing (checked once, on one buffer set)
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    agree = {}
    for name in ops:
        ref = first(f"{name}_fused")
        agree[f"{name}_composed"] = float((first(f"{name}_composed") - ref).abs().max() / ref.abs().max())
    ref = first("periodic_fused")
    agree["periodic_torch_fft"] = float((first("periodic_torch_fft") - ref).abs().max() / ref.abs().max())

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

    # algorithmic bytes per call (fp32): what the launch has to move once
    m_in, m_sr = int(descs["inpaint"].m), int(descs["sr4"].m)
    index = 12.0 * n / 64  # the keep words and their ranks, per sample
    inter = 8.0 * C * hw * S  # the complex half-spectrum intermediate of one sample
    nbytes = {
        "dps_update": b * (4.0 * (4 * n + m_in) + index),        # x, eps, w read; x' written; y
        "inpaint_fused": b * (4.0 * (3 * n + m_in) + index),     # x, eps read; x' written; y
        "sr4_fused": b * 4.0 * (3 * n + m_sr),
        "periodic_fused": {"rows": b * (8.0 * n + inter),        # x, eps -> intermediate
                           "columns_prox": b * 3 * inter + 8.0 * hw * S,  # intermediate r/w, q; M
                           "rows_inv_update": b * (inter + 8.0 * n)},     # intermediate, x -> x'
    }

    row = {"bench": "diffpir_step", "batch": b, "shape": list(shape), "radius": a.radius,
           "rho": rho, "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "hbm_spec_bytes_per_s": HBM_BYTES_PER_S, "max_diff_over_max_vs_fused": agree}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
        if key in nbytes:
            per = nbytes[key]
            total = sum(per.values()) if isinstance(per, dict) else per
            row[key]["algorithmic_bytes"] = total
            if isinstance(per, dict):
                row[key]["algorithmic_bytes_per_launch"] = per
            row[key]["fraction_of_hbm_spec"] = round(total / t / HBM_BYTES_PER_S, 3)
    row["ratios"] = {f"{name}_composed_over_fused":
                     round(row[f"{name}_composed"]["us"] / row[f"{name}_fused"]["us"], 3) for name in ops}
    row["ratios"]["periodic_torch_fft_over_fused"] = round(
        row["periodic_torch_fft"]["us"] / row["periodic_fused"]["us"], 3)
    row["ratios"]["inpaint_fused_hbm_fraction_over_dps_update"] = round(
        row["inpaint_fused"]["fraction_of_hbm_spec"] / row["dps_update"]["fraction_of_hbm_spec"], 3)

    if a.network == "ddpm":
        row["network_ddpm"] = whole_steps(b, shape, a.network_steps, dev)

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


def whole_steps(b, shape, steps, dev):
    """Milliseconds of a whole guided step (network included), DiffPIR against DPS, on the headline
    configuration: the DDPM UNet, inpaint 50 %, Philox noise; one warm-up step, then `steps`."""
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.networks.base import host_timesteps
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers import FusedDiffPIRStep, FusedDPSStep

    op = RandomInpaintingOperator(shape, 0.5, seed=1).to(dev)
    y = torch.randn(b, *op.y_shape, device=dev)
    prob = InverseProblem(op, y, GaussianNoise(0.05).to(dev))
    net = DDPMNetwork.from_config(seed=0, device=dev)
    net.set_sampling_parameters(1000, batch_size=b)
    ts = host_timesteps(net)
    out = {}
    for name, make in (("dps", lambda: FusedDPSStep(net, prob, y, 1)),
                       ("diffpir", lambda: FusedDiffPIRStep(net, prob, y, 1))):
        st = make()
        x = torch.randn(b, *shape, device=dev)
        extra = (ts[0],) if name == "dps" else ()
        i = len(ts) - 1
        st(x, i, ts[i], ts[i - 1], *extra, seed=1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(steps):
            i = len(ts) - 2 - j
            st(x, i, ts[i], ts[i - 1], *extra, seed=1)
        e1.record()
        e1.synchronize()
        out[f"{name}_step_ms"] = round(e0.elapsed_time(e1) / steps, 2)
    out["dps_over_diffpir"] = round(out["dps_step_ms"] / out["diffpir_step_ms"], 3)
    out["steps"] = steps
    net.clear_sampling_parameters()
    return out


if __name__ == "__main__":
    main()
