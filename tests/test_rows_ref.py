"""tests/rows_ref.py on the CPU: the closed forms against fp64 torch + autograd, the fp32 emulation
of each row kernel's arithmetic inside every bound the HIP kernels are held to, at every width and
case tests/test_transformer_rows_gpu.py runs (with the emulation's margin to each bound printed:
``pytest -s``), and the tables reaching the kernel instantiations and grid-stride trips they are
there for."""

import math

import pytest
import torch
import torch.nn.functional as F

import gn_ref
import rows_ref as rr

ROWS = rr.ROWS


# ---- the references -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", rr.LN_ALL, ids=lambda c: rr.LN_CASES[c])
def test_layernorm_closed_form_matches_autograd(case):
    """``gn_fp64`` on 2-D rows (groups = 1) against fp64 ``F.layer_norm`` + autograd, at 1e-12 of
    each tensor's largest value."""
    c = 260
    t = rr.ln_case(case, ROWS, c)
    ref = rr.ln_fp64(t.x, t.gamma, t.beta, 1e-6, t.dz, t.add)
    x = t.x.double().requires_grad_(True)
    y = F.layer_norm(x, (c,), t.gamma.double(), t.beta.double(), 1e-6)
    (dx,) = torch.autograd.grad(y, x, t.dz.double())
    dx = dx + t.add.double()
    xd = t.x.double()
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    for got, want in ((ref.z, y.detach()), (ref.dx, dx), (ref.mean, mean), (ref.rstd, (var + 1e-6).rsqrt())):
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_layernorm_cases_are_what_they_say():
    c = 260
    assert (rr.ln_case(2, ROWS, c).x[:, 0] == 1000).all()
    assert (rr.ln_case(3, ROWS, c).x[:, :4] == 300).all()
    assert (rr.ln_case(4, ROWS, c).x[:, 0] == 100).all()
    assert (rr.ln_case(5, ROWS, c).x[:, -1] == 1000).all()
    assert float(rr.ln_case(6, ROWS, c).x[:, -1].mean()) > 45
    assert float(rr.ln_case(8, ROWS, c).x.std()) < 2e-4
    x9 = rr.ln_case(9, ROWS, c).x
    assert int((x9 != 2.75).sum()) == ROWS and (x9[:, c // 3] == 3.25).all()
    x30 = rr.ln_case(rr.MEAN_30, ROWS, c).x
    assert abs(float(x30.mean()) - 30) < 0.1 and abs(float(x30.std()) - 1) < 0.05
    assert 7 not in rr.LN_CASES and 10 not in rr.LN_CASES
    assert 3 not in rr.ln_cases_at(4) and 3 not in rr.ln_cases_at(8, bf16=True)
    # bf16 cases are bf16-representable, and the case lists are the issue's
    tb = rr.ln_case(2, ROWS, 520, True)
    assert all(torch.equal(v, rr.rb(v)) for v in (tb.x, tb.dz, tb.add))
    assert set(rr.ln_cases_at(260)) == set(rr.ln_cases_at(320)) == set(rr.LN_ALL)
    assert set(rr.ln_cases_at(1024)) == {1, 2, 5, rr.MEAN_30}


def test_geglu_reference_matches_autograd():
    """The erfc form against fp64 torch ``F.gelu`` + autograd: to 1e-12 in the units of the bounds
    everywhere, and to 1e-12 relative where torch's 1 + erf does not cancel (gate >= -1)."""
    h, dy = rr.geglu_case(9, 1280)
    ref = rr.geglu_fp64(h, dy)
    hd = h.double().requires_grad_(True)
    a, g = hd.chunk(2, -1)
    y = a * F.gelu(g)
    (dh,) = torch.autograd.grad(y, hd, dy.double())
    da, dg = dh.chunk(2, -1)
    a, g, d = a.detach(), g.detach(), dy.double()
    gm = g.abs().clamp_min(1.0)
    for got, want, scale in ((ref.y, y.detach(), a.abs() * gm), (ref.da, da, d.abs() * gm),
                             (ref.dgate, dg, (d * a).abs())):
        assert float(((got - want).abs() - 1e-12 * scale).max()) <= 0
    keep = (g >= -1) & (a != 0)
    assert float(((ref.y - y.detach()).abs() / y.detach().abs().clamp_min(1e-300))[keep].max()) <= 1e-12
    # the reference's own tail: relative to the asymptote phi(g) / |g| (1 - 1 / g^2 + 3 / g^4)
    gt = torch.tensor([-12.0, -10.0, -8.0], dtype=torch.float64)
    cdf = 0.5 * torch.special.erfc(-gt / math.sqrt(2.0))
    asym = torch.exp(-0.5 * gt * gt) / math.sqrt(2 * math.pi) / gt.abs() * (1 - gt ** -2 + 3 * gt ** -4 - 15 * gt ** -6)
    assert float((cdf / asym - 1).abs().max()) < 1e-3 * 8.0 ** -2


def test_gate_table_is_what_it_says():
    t = rr.GATE_TABLE.double()
    assert torch.isfinite(rr.GATE_TABLE).all()
    for v in (0.0, 1e-30, -1e-30, 38.0, -38.0, 1e4, -1e4):
        assert bool((rr.GATE_TABLE == torch.tensor(v, dtype=torch.float32)).any()), v
    assert int(((t.abs() > 0) & (t.abs() < 2.0 ** -126)).sum()) == 2      # +-1e-40, denormal
    assert int((t.abs() > 1e19).sum()) == 2
    assert int(((t >= -6.5) & (t <= -5.0)).sum()) >= 600
    ramp = t[-2049:]
    assert float(ramp[0]) == -12 and float(ramp[-1]) == 12 and float(ramp.diff().max()) <= 24 / 2048 + 1e-6
    assert rr.GATE_TABLE.numel() % 2 == 1
    h, dy = rr.geglu_case(9, 1280)
    a = h[:, :1280]
    assert int((a == 0).sum()) > 0 and int((a.abs() == 1e4).sum()) > 0
    assert int((dy == 0).sum()) > 0 and int((dy.abs() == 1e4).sum()) > 0
    assert 9 * 1280 >= rr.GATE_TABLE.numel()      # the (9, 1280) shape carries the whole table


@pytest.mark.parametrize("case", rr.SM_CASES)
def test_softmax_reference_matches_autograd(case):
    n = 260
    s = rr.softmax_case(case, ROWS, n)
    ref = rr.softmax_fp64(s)
    sd = s.double()
    assert float((ref.p - torch.softmax(sd, 1)).abs().max()) <= 1e-12
    lse = torch.logsumexp(sd, 1)
    assert float(((ref.lse - lse).abs() / lse.abs().clamp_min(1.0)).max()) <= 1e-12
    p32 = ref.p.float()
    for kind in rr.SM_DP:
        dp = rr.softmax_vjp_case(kind, ROWS, n)
        for scale in rr.SM_SCALES:
            sc = float(torch.tensor(scale, dtype=torch.float32))
            x = sd.clone().requires_grad_(True)
            # softmax of the scaled pre-scores x / sc, at the fp64 p itself
            (g,) = torch.autograd.grad(torch.softmax(x, 1), x, dp.double())
            want = sc * g
            got = rr.softmax_vjp_fp64(ref.p, dp, scale)
            assert float(((got - want).abs() / dp.double().abs().amax(1, keepdim=True)).max()) <= 1e-12
            # and the p the kernel is given is that p rounded once
            assert float((p32.double() - ref.p).abs().max()) <= 2.0 ** -24


def test_softmax_cases_are_what_they_say():
    n = 260
    m = rr.softmax_case("masked", ROWS, n)
    assert torch.isinf(m[:, 0:n - 1:3]).all() and torch.isfinite(m[:, n - 1]).all()
    assert int(torch.isinf(m).sum()) in (ROWS * len(range(0, n, 3)), ROWS * (len(range(0, n, 3)) - 1))
    m4 = rr.softmax_case("masked", ROWS, 4)
    assert torch.isinf(m4[:, 0]).all() and torch.isfinite(m4[:, 1:]).all()
    assert (rr.softmax_case("all_equal", ROWS, n) == 0.75).all()
    for name, i in (("peak_first", 0), ("peak_middle", n // 2), ("peak_last", n - 1)):
        s = rr.softmax_case(name, ROWS, n)
        assert (s.argmax(1) == i).all() and float(s[:, i].min()) > 70
    assert float(rr.softmax_case("randn_plus_3e4", ROWS, n).min()) > 29990
    assert float(rr.softmax_case("randn_x30_minus_1e4", ROWS, n).max()) < -9800
    assert float(rr.softmax_case("randn_x60", ROWS, n).std()) > 50
    assert set(rr.sm_cases_at(516)) == set(rr.SM_CASES) and set(rr.sm_cases_at(512)) == set(rr.SM_FEW)


# ---- the yardstick: the emulation is inside every bound ----------------------------------------
def _worst(acc: dict, figs: dict) -> None:
    for k, v in figs.items():
        acc[k] = max(acc.get(k, 0.0), v[0] / v[1])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_layernorm_emulation_is_inside_every_bound(bf16):
    widths = rr.LN_BF16_WIDTHS if bf16 else rr.LN_WIDTHS
    eps_once = rr.LN_BF16_EPS_ONCE if bf16 else rr.LN_EPS_ONCE
    worst, worst30, bad = {}, {}, []
    for c in widths:
        for case in rr.ln_cases_at(c, bf16):
            t = rr.ln_case(case, ROWS, c, bf16)
            for with_add in (False, True):
                for eps in (gn_ref.EPS,) + ((eps_once[1],) if c == eps_once[0] and case == 1 else ()):
                    ref = rr.ln_reference(case, ROWS, c, eps, with_add, bf16)
                    figs = rr.ln_figures(*rr.ln_emulate(t, eps, with_add, bf16), ref, t.gamma, bf16)
                    _worst(worst30 if case == rr.MEAN_30 else worst, figs)
                    if any(v > b for v, b in figs.values()):
                        bad.append((c, rr.LN_CASES[case], with_add, eps, figs))
    name = "bf16" if bf16 else "fp32"
    for tag, w in (("gn cases", worst), ("mean_30_std_1", worst30)):
        print(f"LayerNorm {name} emulation, {tag}: largest value / bound: "
              + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    assert not bad, bad


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_geglu_emulation_is_inside_every_bound(bf16):
    worst, bad = {}, []
    shapes = (rr.GEGLU_BF16_SHAPES if bf16 else rr.GEGLU_SHAPES) + (rr.GEGLU_TRIP,)
    for rows, f in shapes:
        h, dy = rr.geglu_case(rows, f, bf16)
        ref = rr.geglu_fp64(h, dy)
        y, dh = rr.geglu_emulate(h, dy, bf16)
        figs = rr.geglu_figures(y, dh, h, dy, ref, bf16)
        for k, (v, b, i) in figs.items():
            worst[k] = max(worst.get(k, 0.0), v)
            if v > b:
                bad.append((rows, f, k, v, b, i))
    print(f"GEGLU {'bf16 (value / bound)' if bf16 else 'fp32 (units of ULP, bound 12)'} emulation: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if not bf16:
        # torch's own fp32 F.gelu in the same units (on the last, largest shape)
        a, g = h.chunk(2, -1)
        yt = a * F.gelu(g)
        ft = rr.geglu_figures(yt, torch.cat([dy * F.gelu(g), torch.zeros_like(yt)], 1), h, dy,
                              ref._replace(dgate=torch.zeros_like(yt, dtype=torch.float64)))
        print(f"torch fp32 F.gelu: y {ft['geglu_y'][0]:.2f} da {ft['geglu_da'][0]:.2f}")
        assert ft["geglu_y"][0] <= rr.GEGLU_K
    assert not bad, bad


def test_softmax_emulation_is_inside_every_bound():
    worst, bad = {}, []
    for n in rr.SM_WIDTHS:
        for case in rr.sm_cases_at(n):
            s = rr.softmax_case(case, ROWS, n)
            ref = rr.softmax_fp64(s)
            p, lse = rr.softmax_emulate(s)
            figs = rr.softmax_figures(p, lse, ref, s)
            p32 = ref.p.float()
            for kind in rr.SM_DP:
                dp = rr.softmax_vjp_case(kind, ROWS, n)
                for scale in rr.SM_SCALES:
                    fv = rr.softmax_vjp_figures(rr.softmax_vjp_emulate(p32, dp, scale),
                                                rr.softmax_vjp_fp64(p32, dp, scale), p32, dp, scale)
                    figs["softmax_vjp"] = max(figs.get("softmax_vjp", (0, 0, 0)), fv["softmax_vjp"])
            for k, (v, b, i) in figs.items():
                worst[k] = max(worst.get(k, 0.0), v)
                if v > b:
                    bad.append((n, case, k, v, b, i))
    print("softmax emulation (units of ULP, bound 8): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("c", rr.CONV_C)
def test_conv_emulation_is_exact_on_integers_and_inside_the_bound(c):
    for n in rr.CONV_N:
        for hw in rr.CONV_HW:
            x, w, b = rr.conv_int_case(c, n, hw)
            assert float(x.abs().max()) <= 64 and float(w.abs().max()) <= 8 and float(b.abs().max()) <= 64
            assert c * 8 * 64 + 64 < 2 ** 24
            for bias in (b, None):
                assert torch.equal(rr.conv_emulate(x, w, bias).double(), rr.conv_exact(x, w, bias, False).double())
            assert torch.equal(rr.conv_emulate(x, w.t().contiguous(), None).double(),
                               rr.conv_exact(x, w, None, True).double())
    x, w, b = rr.conv_randn_case(c, 3, 1028)
    ref, bound = rr.conv_fp64(x, w, b)
    q = float(((rr.conv_emulate(x, w, b).double() - ref).abs() / bound).max())
    print(f"conv1x1 c={c} emulation: largest |err| / bound {q:.3f}")
    assert q <= 1.0


# ---- the tables reach what they claim ----------------------------------------------------------
def test_tables_cover_every_instantiation_and_trip():
    assert {rr.ln_nv(c) for c in rr.LN_WIDTHS} == set(range(1, 9))
    assert {rr.ln_bf16_nv(c) for c in rr.LN_BF16_WIDTHS} == {1, 2, 3, 4}
    assert {rr.sm_nv(n) for n in rr.SM_WIDTHS} == {1, 2, 4, 8, 16}
    assert all(c % 4 == 0 for c in rr.LN_WIDTHS) and all(c % 8 == 0 for c in rr.LN_BF16_WIDTHS)
    assert all(n % 4 == 0 and n <= 4096 for n in rr.SM_WIDTHS)
    # the widths on either side of a 64-vector boundary dispatch differently
    assert (rr.ln_nv(252), rr.ln_nv(256), rr.ln_nv(260)) == (1, 1, 2)
    assert (rr.ln_nv(1536), rr.ln_nv(1540), rr.ln_nv(2044), rr.ln_nv(2048)) == (6, 7, 8, 8)
    assert (rr.ln_bf16_nv(504), rr.ln_bf16_nv(512), rr.ln_bf16_nv(520)) == (1, 1, 2)
    assert (rr.ln_bf16_nv(1536), rr.ln_bf16_nv(1544), rr.ln_bf16_nv(2040)) == (3, 4, 4)
    assert [rr.sm_nv(n) for n in (256, 260, 512, 516, 1024, 1028, 2048, 2052)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert rr.ln_nv(1024) == 4 and rr.sm_nv(516) == 4
    # refused widths
    assert rr.ln_nv(2052) == 9 and 2056 // 8 > 4 * 64 and 4100 > 4096
    # second grid-stride trips
    rows, f = rr.GEGLU_TRIP
    one = rr.trip_elements(rr.GEGLU_GRID_CAP, rr.GEGLU_VEC)
    assert one == rr.trip_elements(rr.GEGLU_BF16_GRID_CAP, rr.GEGLU_BF16_VEC) == 8388608
    assert rows * f == 8396800 and one < rows * f < 2 * one and rows * f < 2 ** 31
    assert all(r * ff < one for r, ff in rr.GEGLU_SHAPES + rr.GEGLU_BF16_SHAPES)
    c, n, hw = rr.CONV_TRIP
    assert rr.trip_elements(rr.CONV_GRID_CAP, rr.CONV_VEC) < n * hw < 2 * rr.trip_elements(rr.CONV_GRID_CAP, rr.CONV_VEC)
    assert hw % 4 == 0 and all(nn * h < rr.trip_elements(rr.CONV_GRID_CAP, rr.CONV_VEC) for nn in rr.CONV_N for h in rr.CONV_HW)
    # rows = 9: two whole workgroups of 4 waves and one wave of a third
    assert ROWS == 2 * (rr.BLOCK // 64) + 1
