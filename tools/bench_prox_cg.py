"""The DiffPIR step with the conjugate-gradient data step (sp_diffpir_step_cg_ws, csrc/sp_cg.hip)
for three operators without a closed-form prox, timed in one process at B = 64: the 9 x 9 Gaussian
blur and a dense R = 4 PSF on 3 x 256 x 256, and the Radon transform with 23 angles on
1 x 256 x 256.  K = 8 iterations, rho = 1, tol = 0, so every iteration of every sample is live.

Entries per operator (all interleaved group by group, each group of `--inner` back-to-back passes
bracketed by device events after a warm-up; the figures are the median and the quartiles over
`--repeats` groups, successive passes rotating over `--sets` buffer sets):
  fused      sp_diffpir_step_cg_ws with in-kernel Philox noise: the head, (K + 1) x (A, A^T), four
             vector launches per iteration (three in the last), the tail
  composed   the same recurrence as a user writes it today: the operator's device apply /
             apply_transpose, torch elementwise operations and reductions with per-sample scalars
             kept as device tensors (torch.where for the stop, no host synchronisation), sp_randn
             and the update in torch
  maps       K x (sp_op_apply + sp_op_adjoint) alone into preallocated buffers: the floor no
             solver can beat
and from them: composed / fused, the share of the fused time outside its (K + 1) x (A + A^T), and
the rate of the vector launches on their algorithmic HBM bytes (fp32) as a fraction of the 8 TB/s
HBM specification, taking their time as fused - (K + 1) / K x maps.

    python tools/bench_prox_cg.py [--out profiles/bench_prox_cg.json]
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
from samplers_amd.operators import GaussianBlurOperator, PSFBlurOperator, RadonOperator  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def dense_kernel(radius: int) -> torch.Tensor:
    k = 2 * radius + 1
    h = torch.rand(k, k, generator=torch.Generator().manual_seed(radius), dtype=torch.float64) + 0.05
    return (h / h.sum()).to(torch.float32)


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return q[0], q[2]


def vector_bytes(n: int, m: int, iters: int) -> float:
    """Algorithmic bytes per sample of the vector launches of one sp_diffpir_step_cg_ws call."""
    head = 12.0 * n                      # x, eps read; x0 written
    start = 12.0 * m + 12.0 * n          # s = y - q; g read, d and p written
    per_iter = 16.0 * m + 32.0 * n       # qq 4m; yupd 12m; xupd 20n; pupd 12n
    tail = 16.0 * n                      # x0, d, x read; x' written
    return head + start + iters * per_iter - 12.0 * n + tail  # the last iteration has no pupd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_prox_cg.json"))
    a = ap.parse_args()
    if a.repeats < 20 or a.sets < 3:
        ap.error("--repeats must be at least 20 and --sets at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_prox_cg.py times kernels on the GPU; no device found")
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    S, b, K = a.size, a.batch, a.iterations
    a_t, rho, tol = 0.31, 1.0, 0.0
    k_t = (1 - a_t**2) ** 0.5
    cf = dict(a=a_t, k=k_t, a_prev=0.45, c_eps=0.75, c_xi=0.49)
    coefs = _hip.SpProxCoefs(cf["a"], cf["k"], rho, cf["a_prev"], cf["c_eps"], cf["c_xi"])
    stream = torch.cuda.current_stream().cuda_stream
    seed, step = 7, 3

    ops = {"blur9": GaussianBlurOperator((3, S, S), 9, 3.0).to(dev),
           "psf_r4": PSFBlurOperator((3, S, S), dense_kernel(4)).to(dev),
           "radon23": RadonOperator((1, S, S), num_angles=23).to(dev)}
    descs = {k: op.hip_descriptor() for k, op in ops.items()}

    sets = {name: [] for name in ops}
    for name, op in ops.items():
        d = descs[name]
        n, m = int(d.n), int(d.m)
        floats = int(lib.sp_prox_cg_workspace(d, b, 1))
        if floats < 0:
            sys.exit(f"sp_prox_cg_workspace rejected {name} ({floats})")
        for _ in range(a.sets):
            sets[name].append(dict(
                x=torch.randn(b, n, device=dev), eps=torch.randn(b, n, device=dev),
                y=torch.randn(b, m, device=dev), out=torch.empty(b, n, device=dev),
                xi=torch.empty(b, n, device=dev), ym=torch.empty(b, m, device=dev),
                xn=torch.empty(b, n, device=dev), iters=torch.zeros(b, dtype=torch.int32, device=dev),
                work=torch.empty(floats, device=dev)))
    turn = [0]

    def next_set(name):
        s = sets[name][turn[0] % a.sets]
        turn[0] += 1
        return s

    def fused(name):
        d = descs[name]

        def run():
            s = next_set(name)
            _hip.check(lib.sp_diffpir_step_cg_ws(
                d, s["x"].data_ptr(), s["eps"].data_ptr(), s["y"].data_ptr(), None, seed, step, 0, b,
                1, coefs, K, tol, s["out"].data_ptr(), s["iters"].data_ptr(), s["work"].data_ptr(),
                stream), "sp_diffpir_step_cg_ws")
            return s["out"]

        return run

    def composed(name):
        op = ops[name]
        n = int(descs[name].n)

        def sq(t):
            return (t * t).reshape(b, -1).sum(1).view(b, 1, 1, 1)

        @torch.no_grad()
        def run():
            s = next_set(name)
            x = s["x"].view(b, *op.x_shape)
            x0 = (x - k_t * s["eps"].view_as(x)) / a_t
            r = s["y"].view(b, *op.y_shape) - op.apply(x0)
            g = op.apply_transpose(r)
            d, p = torch.zeros_like(x0), g.clone()
            gamma = sq(g)
            gamma0 = gamma.clone()
            for _ in range(K):
                q = op.apply(p)
                delta = sq(q) + rho * sq(p)
                live = ((gamma > (tol * tol) * gamma0) & (delta > 0) & torch.isfinite(gamma)
                        & torch.isfinite(delta))
                alpha = gamma / delta
                d = torch.where(live, d + alpha * p, d)
                r = torch.where(live, r - alpha * q, r)
                g = torch.where(live, op.apply_transpose(r) - rho * d, g)
                gamma_new = sq(g)
                p = torch.where(live, g + (gamma_new / gamma) * p, p)
                gamma = torch.where(live, gamma_new, gamma)
            z = (x0 + d).reshape(b, n)
            _hip.check(lib.sp_randn(s["xi"].data_ptr(), b, n, seed, step, 0, stream), "sp_randn")
            eh = (s["x"] - cf["a"] * z) / cf["k"]
            return cf["a_prev"] * z + (cf["c_eps"] * eh + cf["c_xi"] * s["xi"])

        return run

    def maps(name):
        d = descs[name]

        def run():
            s = next_set(name)
            for _ in range(K):
                _hip.check(lib.sp_op_apply(d, s["x"].data_ptr(), s["ym"].data_ptr(), b, stream),
                           "sp_op_apply")
                _hip.check(lib.sp_op_adjoint(d, s["y"].data_ptr(), s["xn"].data_ptr(), b, stream),
                           "sp_op_adjoint")
            return s["xn"]

        return run

    entries = {}
    for name in ops:
        entries[f"{name}_fused"] = fused(name)
        entries[f"{name}_composed"] = composed(name)
        entries[f"{name}_maps"] = maps(name)

    # the two forms compute the same thing up to rounding, which K iterations of CG amplify
    def first(key):
        turn[0] = 0
        return entries[key]().clone()

    agree, live_iters = {}, {}
    for name in ops:
        ref = first(f"{name}_fused")
        live_iters[name] = sorted(set(sets[name][0]["iters"].tolist()))
        agree[name] = float((first(f"{name}_composed") - ref).abs().max() / ref.abs().max())

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

    row = {"bench": "diffpir_step_cg", "batch": b, "size": S, "iterations": K, "rho": rho, "tol": tol,
           "repeats": a.repeats, "inner": a.inner, "buffer_sets": a.sets,
           "device": torch.cuda.get_device_name(0), "sp_version": int(lib.sp_version()),
           "hbm_spec_bytes_per_s": HBM_BYTES_PER_S, "max_diff_over_max_composed_vs_fused": agree,
           "live_iterations": live_iters, "ratios": {}, "bar_fused_not_slower_than_composed": {}}
    for key in entries:
        t = statistics.median(times[key])
        q1, q3 = quartiles(times[key])
        row[key] = {"us": round(t * 1e6, 1), "us_q1": round(q1 * 1e6, 1), "us_q3": round(q3 * 1e6, 1),
                    "us_min": round(min(times[key]) * 1e6, 1), "us_max": round(max(times[key]) * 1e6, 1)}
    for name in ops:
        n, m = int(descs[name].n), int(descs[name].m)
        f, c, mp = (row[f"{name}_{k}"]["us"] for k in ("fused", "composed", "maps"))
        in_maps = mp * (K + 1) / K  # the call applies A and A^T once more, for the first residual
        outside = f - in_maps
        nbytes = b * vector_bytes(n, m, K)
        row[f"{name}_fused"].update({
            "shape": list(ops[name].x_shape), "n": n, "m": m,
            "vector_launches": 3 + 4 * K - 1, "map_calls": 2 * (K + 1),
            "us_outside_maps": round(outside, 1),
            "share_outside_maps": round(outside / f, 3),
            "vector_algorithmic_bytes": nbytes,
            "vector_fraction_of_hbm_spec": (round(nbytes / (outside * 1e-6) / HBM_BYTES_PER_S, 3)
                                            if outside > 0 else None)})
        row["ratios"][f"{name}_composed_over_fused"] = round(c / f, 3)
        row["ratios"][f"{name}_fused_over_maps_floor"] = round(f / in_maps, 3)
        row["bar_fused_not_slower_than_composed"][name] = bool(f <= c)

    line = json.dumps(row)
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
