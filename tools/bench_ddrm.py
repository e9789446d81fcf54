"""The DDRM step after the network call (sp_ddrm_step_ws: x0 and the spectral update) for the three
operator families with a fused step, timed in one process at B = 64, 3 x 256 x 256: inpaint 50 %,
SR x4 and the periodic blur with a dense R = 30 PSF.

Entries per operator (all interleaved group by group, each group of `--inner` back-to-back passes
bracketed by device events after a warm-up; the figures are the median and the quartiles over
`--repeats` groups, successive passes rotating over `--sets` buffer sets):
  fused      sp_ddrm_step_ws with in-kernel Philox noise: one launch (inpaint, SR) or three
             (periodic: rows of x0, eps and xi; columns with the four per-frequency coefficients;
             rows^-1 times a_prev; q = P FFT2(y) prepared once outside the timed region, as the
             sampler does)
  composed   the same x' from sp_predict_x0, sp_randn, the operator's device maps (A^T y once
             outside the timed region; the projector A^T A / g, or A^+ A for the periodic kind) and
             torch elementwise operations
  torch_fft  (periodic only) x0, three rfft2, the per-frequency coefficients (precomputed), irfft2
             with torch.fft on the device
  diffpir    sp_diffpir_step_ws on the same operator and buffers: the yardstick of the launch
The periodic operator runs at sig_y = 0 (noiseless deblurring), where every kept frequency is in
one class and the projector composition is exact; the launches' work does not depend on the
scalars.  Each fused entry carries its algorithmic HBM bytes (fp32; per launch for the periodic
step) and their rate as a fraction of the 8 TB/s HBM specification.  `bars` states the pass / fail
of: fused <= composed (and <= torch_fft) for every operator; for inpaint and SR fused <= the
DiffPIR launch's median x (1 + its relative interquartile range).

--network ddpm also times a whole DDRM step against a whole DPS step (network forward, and for DPS
its input VJP) on the headline configuration: the DDPM UNet, inpaint 50 %, the same batch.

    python tools/bench_ddrm.py [--out profiles/bench_ddrm.json]
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


def class_coefficients(cf, s2, observed):
    """(f_th, f_eps, f_y, f_xi) per component in fp32 torch, the map of samplers_hip.h."""
    sp, sy, eta, eb, c1 = (torch.tensor(cf[k], dtype=torch.float32, device=s2.device)
                           for k in ("sig_prev", "sig_y", "eta", "eta_b", "c1"))
    one, zero = torch.ones_like(s2), torch.zeros_like(s2)
    observed = observed & (s2 > 0)
    big = observed & ((sp * sp) * s2 >= sy * sy)
    small = observed & ~big
    safe = torch.where(observed, s2, one)
    r = torch.where(small, (c1 * sp) * torch.sqrt(s2) / torch.where(small, sy * one, one), zero)
    f_th = torch.where(big, (1 - eb) * one, 1 - r)
    f_y = torch.where(big, eb * one, r)
    f_ep = torch.where(observed, zero, (c1 * sp) * one)
    f_xi = torch.where(big, torch.sqrt(torch.clamp(sp * sp - (eb * sy) ** 2 / safe, min=0)),
                       (eta * sp) * one)
    return f_th, f_ep, f_y, f_xi


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_ddrm.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_ddrm.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    C, S, b = 3, a.size, a.batch
    shape = (C, S, S)
    n = C * S * S
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
    a_t = 0.31
    k_t = (1 - a_t**2) ** 0.5
    base = dict(a=f32(a_t), k=f32(k_t), a_prev=f32(0.45), sig_prev=f32(0.89 / 0.45), eta=f32(0.85),
                eta_b=1.0, c1=f32((1 - 0.85**2) ** 0.5))
    cfs = {"inpaint": dict(base, sig_y=f32(0.05)), "sr4": dict(base, sig_y=f32(0.05)),
           "periodic": dict(base, sig_y=0.0)}
    order = [f for f, _ in _hip.SpDdrmCoefs._fields_]
    coefs = {k: _hip.SpDdrmCoefs(*(v[f] for f in order)) for k, v in cfs.items()}
    prox = _hip.SpProxCoefs(base["a"], base["k"], 0.05, base["a_prev"], 0.75, 0.49)
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    ops = {"inpaint": RandomInpaintingOperator(shape, 0.5, seed=1).to(dev),
           "sr4": SuperResolutionOperator(shape, 4).to(dev),
           "periodic": PeriodicBlurOperator(shape, dense_kernel(a.radius)).to(dev)}
    descs = {k: op.hip_descriptor() for k, op in ops.items()}
    gains = {"inpaint": 1.0, "sr4": 1.0 / 16, "periodic": None}
    hw = S // 2 + 1
    keep_px = (~ops["inpaint"].mask).reshape(1, n)
    mh = torch.view_as_complex(ops["periodic"].spectra[0]).transpose(0, 1)  # (S, S / 2 + 1)
    ph = torch.view_as_complex(ops["periodic"].spectra[1]).transpose(0, 1)
    s2h = (mh.real * mh.real + mh.imag * mh.imag).contiguous()
    fth_h, fep_h, fy_h, fxi_h = class_coefficients(cfs["periodic"], s2h, (ph.real != 0) | (ph.imag != 0))

    def x_rows(name, t):
        return t.reshape(b, *ops[name].x_shape)

    sets = {name: [] for name in ops}
    for name, op in ops.items():
        d = descs[name]
        m = int(d.m)
        work_floats = max(int(lib.sp_ddrm_workspace(d, b)), int(lib.sp_prox_workspace(d, b)))
        q_floats = int(lib.sp_prox_prepare_size(d, b))
        for _ in range(a.sets):
            x, eps = (torch.randn(b, n, device=dev) for _ in range(2))
            y = torch.randn(b, m, device=dev)
            s = dict(x=x, eps=eps, y=y, out=torch.empty(b, n, device=dev),
                     t0=torch.empty(b, n, device=dev), xi=torch.empty(b, n, device=dev),
                     work=torch.empty(max(work_floats, 4), device=dev),
                     q_prox=torch.empty(max(q_floats, 4), device=dev))
            _hip.check(lib.sp_prox_prepare(d, y.data_ptr(), b, s["q_prox"].data_ptr(), stream),
                       "sp_prox_prepare")
            yv = y.reshape(b, *op.y_shape)
            if name == "periodic":
                s["q"] = torch.empty(int(lib.sp_op_workspace(d, b)), device=dev)
                _hip.check(lib.sp_pgdm_prepare(d, y.data_ptr(), b, s["q"].data_ptr(), stream),
                           "sp_pgdm_prepare")
                s["y_up"] = op.apply_pseudo_inverse(yv).reshape(b, n)          # A^+ y
                s["y_spec"] = fy_h * (ph * torch.fft.rfft2(yv))               # f_y P Y
            else:
                s["q"] = None
                s["y_up"] = op.apply_transpose(yv).reshape(b, n) / gains[name]  # A^T y / g
            sets[name].append(s)
    turn = [0]

    def next_set(name):
        s = sets[name][turn[0] % a.sets]
        turn[0] += 1
        return s

    def fused(name):
        d = descs[name]

        def run():
            s = next_set(name)
            _hip.check(lib.sp_ddrm_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(),
                                           s["q"].data_ptr() if s["q"] is not None else None, None,
                                           seed, step, 0, b, 1, coefs[name], s["out"].data_ptr(),
                                           s["work"].data_ptr(), stream), "sp_ddrm_step_ws")
            return s["out"]

        return run

    def diffpir(name):
        d = descs[name]

        def run():
            s = next_set(name)
            _hip.check(lib.sp_diffpir_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(),
                                              s["y"].data_ptr(), s["q_prox"].data_ptr(), None, seed,
                                              step, 0, b, 1, prox, s["out"].data_ptr(),
                                              s["work"].data_ptr(), stream), "sp_diffpir_step_ws")
            return s["out"]

        return run

    def head(s):
        _hip.check(lib.sp_predict_x0(s["x"].data_ptr(), s["eps"].data_ptr(), b * n, base["a"], base["k"],
                                     s["t0"].data_ptr(), stream), "sp_predict_x0")
        _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
        return s["t0"], s["xi"]

    def composed(name):
        op, cf = ops[name], cfs[name]
        g = gains[name] if gains[name] is not None else 1.0
        one = torch.ones((), device=dev)
        f_th, _, f_y, f_xi = (float(t) for t in class_coefficients(cf, g * one, one > 0))
        ce, es = cf["c1"] * cf["sig_prev"], cf["eta"] * cf["sig_prev"]

        def run():
            s = next_set(name)
            x0, xi = head(s)
            if name == "inpaint":  # the projector is the keep mask itself
                obs = f_th * x0 + f_y * s["y_up"] + f_xi * xi
                return cf["a_prev"] * torch.where(keep_px, obs, x0 + ce * s["eps"] + es * xi)
            inner = x_rows(name, (f_th - 1) * x0 - ce * s["eps"] + (f_xi - es) * xi)
            if name == "periodic":
                tail = op.apply_pseudo_inverse(op.apply(inner))               # A^+ A
            else:
                tail = op.apply_transpose(op.apply(inner)) / g                # A^T A / g
            return cf["a_prev"] * ((x0 + ce * s["eps"] + es * xi) + tail.reshape(b, n) + f_y * s["y_up"])

        return run

    def torch_fft():
        s = next_set("periodic")
        x0, xi = head(s)
        r = lambda t: torch.fft.rfft2(t.view(b, C, S, S))  # noqa: E731
        spec = fth_h * r(x0) + fep_h * r(s["eps"]) + fxi_h * r(xi) + s["y_spec"]
        return cfs["periodic"]["a_prev"] * torch.fft.irfft2(spec, s=(S, S)).reshape(b, n)

    entries = {}
    for name in ops:
        entries[f"{name}_fused"] = fused(name)
        entries[f"{name}_composed"] = composed(name)
        entries[f"{name}_diffpir"] = diffpir(name)
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
        "inpaint_fused": b * (4.0 * (3 * n + m_in) + index),     # x, eps read; x' written; y
        "inpaint_diffpir": b * (4.0 * (3 * n + m_in) + index),
        "sr4_fused": b * 4.0 * (3 * n + m_sr),
        "sr4_diffpir": b * 4.0 * (3 * n + m_sr),
        "periodic_fused": {"rows": b * (8.0 * n + 3 * inter),    # x, eps -> three intermediates
                           "columns": b * 5 * inter + 16.0 * hw * S,  # three read, one written, q; M, P
                           "rows_inv": b * (inter + 4.0 * n)},   # intermediate -> x'
    }

    row = {"bench": "ddrm_step", "batch": b, "shape": list(shape), "radius": a.radius,
           "coefficients": cfs, "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
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
    for name in ops:
        row["ratios"][f"{name}_fused_over_diffpir"] = round(
            row[f"{name}_fused"]["us"] / row[f"{name}_diffpir"]["us"], 3)
    bars = {f"{name}_fused_le_composed": row[f"{name}_fused"]["us"] <= row[f"{name}_composed"]["us"]
            for name in ops}
    bars["periodic_fused_le_torch_fft"] = row["periodic_fused"]["us"] <= row["periodic_torch_fft"]["us"]
    for name in ("inpaint", "sr4"):
        dp = row[f"{name}_diffpir"]
        band = dp["us"] * (1 + (dp["us_q3"] - dp["us_q1"]) / dp["us"])
        row[f"{name}_diffpir"]["us_band"] = round(band, 1)
        bars[f"{name}_fused_le_diffpir_band"] = row[f"{name}_fused"]["us"] <= band
    row["bars"] = bars

    if a.network == "ddpm":
        row["network_ddpm"] = whole_steps(b, shape, a.network_steps, dev)

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


def whole_steps(b, shape, steps, dev):
    """Milliseconds of a whole guided step (network included), DDRM against DPS, on the headline
    configuration: the DDPM UNet, inpaint 50 %, Philox noise; one warm-up step, then `steps`."""
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.networks.base import host_timesteps
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers import FusedDDRMStep, FusedDPSStep

    op = RandomInpaintingOperator(shape, 0.5, seed=1).to(dev)
    y = torch.randn(b, *op.y_shape, device=dev)
    prob = InverseProblem(op, y, GaussianNoise(0.05).to(dev))
    net = DDPMNetwork.from_config(seed=0, device=dev)
    net.set_sampling_parameters(1000, batch_size=b)
    ts = host_timesteps(net)
    out = {}
    for name, make in (("dps", lambda: FusedDPSStep(net, prob, y, 1)),
                       ("ddrm", lambda: FusedDDRMStep(net, prob, y, 1))):
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
    out["dps_over_ddrm"] = round(out["dps_step_ms"] / out["ddrm_step_ms"], 3)
    out["steps"] = steps
    net.clear_sampling_parameters()
    return out


if __name__ == "__main__":
    main()
