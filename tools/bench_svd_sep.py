"""The fused passes of the separable-SVD kind (SP_OP_SVD_SEPARABLE, csrc/sp_svd_sep.hip) after the
network call, timed in one process at B = 64, 3 x 256 x 256 on `SeparableSVDOperator.gaussian_blur`
(9 x 9, sigma 3, reflect padding): the DDRM step, the DiffPIR closed-form step, PGDM pass 1 and DPS
pass 1, each against the same result composed from the operator's own device maps, sp_predict_x0,
sp_randn and torch elementwise operations.

The method is tools/bench_ddrm.py's: all entries interleaved group by group, each group of `--inner`
back-to-back passes bracketed by device events after a warm-up; the figures are the median and the
quartiles over `--repeats` groups, successive passes rotating over `--sets` buffer sets; noise is
drawn in the kernels (Philox).  q (the spectral observation) is prepared once outside the timed
region, as the samplers do.
  ddrm      sp_ddrm_step_ws | x0, xi, the projector form through A^+ A (sig_y = 0, where every kept
            component is in one class and the projector composition is exact) and A^+ y (once)
  diffpir   sp_diffpir_step_ws | sp_predict_x0, sp_op_prox_ws, sp_randn and the update in torch
  pgdm      sp_pgdm_residual_ws | x0, -2 (A^+ y - A^+ A x0) with A^+ y once
  dps       sp_dps_residual_ws | x0, r = y - A x0, A^T (gs r) and the squared norm in torch
Context lines: `matmul_chain`, the DDRM step's eight products as torch.matmul on the same tables
(x0 and xi from the library, the coefficient planes precomputed); `blur_cg_k8`,
sp_diffpir_step_cg_ws at K = 8 on GaussianBlurOperator; `blur_dps`, SP_OP_BLUR's DPS pass 1.
`bars`: fused median <= composed median on the four passes.  `mfma`: the executed flops of each
fused pass's product launches (2 M N K per plane with M, N rounded up to the 64 x 64 tile and K to
the k chunk of 16) over its median, as a share of the 157.3 TFLOP/s fp32 MFMA specification (the
time includes the launches' prologues and epilogues).

--network ddpm also times whole DDRM and DiffPIR steps (the DDPM UNet's forward included).

    python tools/bench_svd_sep.py [--out profiles/bench_svd_sep.json]
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
from samplers_amd.operators import GaussianBlurOperator, SeparableSVDOperator  # noqa: E402

MFMA_SPEC_FLOPS = 157.3e12


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def up(v, to):
    return -(-v // to) * to


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--network", choices=("none", "ddpm"), default="none")
    ap.add_argument("--network-steps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_svd_sep.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_svd_sep.py times kernels on the GPU; no device found")
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
    pgdm_c = _hip.SpDpsCoefs(cf["a"], cf["k"], -2.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    op = SeparableSVDOperator.gaussian_blur(shape, 9, 3.0).to(dev)
    blur = GaussianBlurOperator(shape, 9, 3.0).to(dev)
    d, db = op.hip_descriptor(), blur.hip_descriptor()
    P, Pb = int(lib.sp_rsq_partials(d)), int(lib.sp_rsq_partials(db))
    vh, vw, sfull, keep = op.V_h, op.V_w, op.singular_values_full, op.keep
    # the DDRM coefficient planes at sig_y = 0 (eta_b = 1): kept components take y, the rest the prior
    ce, es, sp = cf["c1"] * cf["sig_prev"], cf["eta"] * cf["sig_prev"], cf["sig_prev"]
    one = torch.ones_like(sfull)
    fth, fep, fxi, fy = (torch.where(keep, 0 * one, one), torch.where(keep, 0 * one, ce * one),
                         torch.where(keep, sp * one, es * one), torch.where(keep, one, 0 * one))
    work_floats = max(int(lib.sp_ddrm_workspace(d, b)), int(lib.sp_dps_workspace(d, b)),
                      int(lib.sp_prox_cg_workspace(db, b, 1)))
    sets = []
    for _ in range(a.sets):
        x, eps = (torch.randn(b, *shape, device=dev) for _ in range(2))
        y = op.apply(torch.randn(b, *shape, device=dev)).contiguous()
        s = dict(x=x, eps=eps, y=y, out=torch.empty_like(x), t0=torch.empty_like(x), xi=torch.empty_like(x),
                 z=torch.empty_like(x), work=torch.empty(work_floats, device=dev),
                 part=torch.empty(b * max(P, Pb), device=dev),
                 q=torch.empty(int(lib.sp_op_workspace(d, b)), device=dev),
                 q_prox=torch.empty(int(lib.sp_prox_prepare_size(d, b)), device=dev))
        _hip.check(lib.sp_pgdm_prepare(d, y.data_ptr(), b, s["q"].data_ptr(), stream), "sp_pgdm_prepare")
        _hip.check(lib.sp_prox_prepare(d, y.data_ptr(), b, s["q_prox"].data_ptr(), stream), "sp_prox_prepare")
        s["pinv_y"] = op.apply_pseudo_inverse(y)
        s["y_spec"] = fy * op.pinv_multiplier * (op.U_h.t() @ y @ op.U_w)
        sets.append(s)
    turn = [0]

    def next_set():
        s = sets[turn[0] % a.sets]
        turn[0] += 1
        return s

    def x0_of(s, c_a=cf["a"], c_k=cf["k"]):
        _hip.check(lib.sp_predict_x0(s["x"].data_ptr(), s["eps"].data_ptr(), b * n, c_a, c_k, s["t0"].data_ptr(),
                                     stream), "sp_predict_x0")
        return s["t0"]

    def randn(s):
        _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
        return s["xi"]

    def ddrm_fused():
        s = next_set()
        _hip.check(lib.sp_ddrm_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), None, s["q"].data_ptr(), None,
                                       seed, step, 0, b, 1, ddrm_c, s["out"].data_ptr(), s["work"].data_ptr(),
                                       stream), "sp_ddrm_step_ws")
        return s["out"]

    def ddrm_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        inner = -x0 - ce * s["eps"] + (sp - es) * xi  # (f_th - 1) x0 - c1 sig' eps + (f_xi - eta sig') xi
        tail = op.apply_pseudo_inverse(op.apply(inner))  # A^+ A
        return cf["a_prev"] * ((x0 + ce * s["eps"] + es * xi) + tail + s["pinv_y"])

    def matmul_chain():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        T = lambda t: vh.t() @ t @ vw  # noqa: E731
        spec = fth * T(x0) + fep * T(s["eps"]) + fxi * T(xi)
        spec[..., :sfull.shape[0], :sfull.shape[1]] += s["y_spec"]
        return cf["a_prev"] * (vh @ spec @ vw.t())

    def diffpir_fused():
        s = next_set()
        _hip.check(lib.sp_diffpir_step_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), None, s["q_prox"].data_ptr(),
                                          None, seed, step, 0, b, 1, prox_c, s["out"].data_ptr(),
                                          s["work"].data_ptr(), stream), "sp_diffpir_step_ws")
        return s["out"]

    def diffpir_composed():
        s = next_set()
        x0, xi = x0_of(s), randn(s)
        _hip.check(lib.sp_op_prox_ws(d, x0.data_ptr(), None, s["q_prox"].data_ptr(), b, 1, px["rho"],
                                     s["z"].data_ptr(), s["work"].data_ptr(), stream), "sp_op_prox_ws")
        z = s["z"]
        return px["a_prev"] * z + (px["c_eps"] * ((s["x"] - px["a"] * z) / px["k"]) + px["c_xi"] * xi)

    def pgdm_fused():
        s = next_set()
        _hip.check(lib.sp_pgdm_residual_ws(d, s["x"].data_ptr(), s["eps"].data_ptr(), s["q"].data_ptr(), b, 1,
                                           pgdm_c, s["out"].data_ptr(), s["work"].data_ptr(), stream),
                   "sp_pgdm_residual_ws")
        return s["out"]

    def pgdm_composed():
        s = next_set()
        return -2.0 * (s["pinv_y"] - op.apply_pseudo_inverse(op.apply(x0_of(s))))

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

    def blur_dps():
        s = next_set()
        _hip.check(lib.sp_dps_residual(db, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), b, 1, dps_c,
                                       s["out"].data_ptr(), s["part"].data_ptr(), stream), "sp_dps_residual")
        return s["out"]

    def blur_cg_k8():
        s = next_set()
        _hip.check(lib.sp_diffpir_step_cg_ws(db, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), None,
                                             seed, step, 0, b, 1, prox_c, 8, 1e-4, s["out"].data_ptr(), None,
                                             s["work"].data_ptr(), stream), "sp_diffpir_step_cg_ws")
        return s["out"]

    entries = {"ddrm_fused": ddrm_fused, "ddrm_composed": ddrm_composed, "diffpir_fused": diffpir_fused,
               "diffpir_composed": diffpir_composed, "pgdm_fused": pgdm_fused, "pgdm_composed": pgdm_composed,
               "dps_fused": dps_fused, "dps_composed": dps_composed, "matmul_chain": matmul_chain,
               "blur_cg_k8": blur_cg_k8, "blur_dps": blur_dps}

    # the entries of one pass compute the same thing (checked once, on one buffer set)
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    agree = {}
    for name in ("ddrm", "diffpir", "pgdm", "dps"):
        ref = first(f"{name}_fused")
        agree[f"{name}_composed"] = float((first(f"{name}_composed") - ref).abs().max() / ref.abs().max())
    ref = first("ddrm_fused")
    agree["matmul_chain"] = float((first("matmul_chain") - ref).abs().max() / ref.abs().max())
    ref = first("dps_fused")
    agree["blur_dps"] = float((first("blur_dps") - ref).abs().max() / ref.abs().max())

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

    hy, wy = op.y_shape[1], op.y_shape[2]
    planes = b * C
    prod = lambda m, nn, k: 2.0 * up(m, 64) * up(nn, 64) * up(k, 16) * planes  # noqa: E731
    full = prod(S, S, S)
    to_obs = prod(hy, S, S) + prod(hy, wy, S)
    from_obs = prod(S, wy, hy) + prod(S, S, wy)
    t_y = prod(hy, wy, hy) + prod(hy, wy, wy)
    flops = {"ddrm_fused": 8 * full, "diffpir_fused": 4 * full, "pgdm_fused": to_obs + from_obs,
             "dps_fused": t_y + to_obs + from_obs}

    row = {"bench": "svd_separable", "batch": b, "shape": list(shape), "operator": "gaussian_blur 9x9 sigma 3",
           "kept_share": round(float(keep.float().mean()), 4), "ddrm_coefficients": cf, "prox_coefficients": px,
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "mfma_spec_flops": MFMA_SPEC_FLOPS, "max_diff_over_max_vs_fused": agree}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
        if key in flops:
            row[key]["executed_flops"] = flops[key]
            row[key]["tflops"] = round(flops[key] / t * 1e-12, 2)
            row[key]["fraction_of_mfma_spec"] = round(flops[key] / t / MFMA_SPEC_FLOPS, 3)
    names = ("ddrm", "diffpir", "pgdm", "dps")
    row["ratios"] = {f"{k}_composed_over_fused": round(row[f"{k}_composed"]["us"] / row[f"{k}_fused"]["us"], 3)
                     for k in names}
    row["ratios"]["matmul_chain_over_ddrm_fused"] = round(row["matmul_chain"]["us"] / row["ddrm_fused"]["us"], 3)
    row["ratios"]["blur_cg_k8_over_diffpir_fused"] = round(row["blur_cg_k8"]["us"] / row["diffpir_fused"]["us"], 3)
    row["ratios"]["dps_fused_over_blur_dps"] = round(row["dps_fused"]["us"] / row["blur_dps"]["us"], 3)
    row["bars"] = {f"{k}_fused_le_composed": row[f"{k}_fused"]["us"] <= row[f"{k}_composed"]["us"] for k in names}

    if a.network == "ddpm":
        row["network_ddpm"] = whole_steps(b, shape, a.network_steps, dev)

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


def whole_steps(b, shape, steps, dev):
    """Milliseconds of a whole step (network included), DDRM and DiffPIR on the operator, the DDPM
    UNet, Philox noise; one warm-up step, then `steps`."""
    from samplers_amd.inverse_problem import InverseProblem
    from samplers_amd.networks.base import host_timesteps
    from samplers_amd.networks.ddpm import DDPMNetwork
    from samplers_amd.noise import GaussianNoise
    from samplers_amd.samplers.ddrm import FusedDDRMStep
    from samplers_amd.samplers.diffpir import FusedDiffPIRStep

    op = SeparableSVDOperator.gaussian_blur(shape, 9, 3.0).to(dev)
    y = torch.randn(b, *op.y_shape, device=dev)
    prob = InverseProblem(op, y, GaussianNoise(0.05).to(dev))
    net = DDPMNetwork.from_config(seed=0, device=dev)
    net.set_sampling_parameters(1000, batch_size=b)
    ts = host_timesteps(net)
    out = {}
    for name, make in (("ddrm", lambda: FusedDDRMStep(net, prob, y, 1)),
                       ("diffpir", lambda: FusedDiffPIRStep(net, prob, y, 1))):
        st = make()
        x = torch.randn(b, *shape, device=dev)
        i = len(ts) - 1
        st(x, i, ts[i], ts[i - 1], seed=1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(steps):
            i = len(ts) - 2 - j
            st(x, i, ts[i], ts[i - 1], seed=1)
        e1.record()
        e1.synchronize()
        out[f"{name}_step_ms"] = round(e0.elapsed_time(e1) / steps, 2)
    out["steps"] = steps
    net.clear_sampling_parameters()
    return out


if __name__ == "__main__":
    main()
