"""The transformer row kernels (csrc/sp_transformer.hip: LayerNorm, GEGLU, row softmax, the 4- /
8-channel 1x1 conv; csrc/sp_bf16_rows.hip: their bf16 LayerNorm and GEGLU) per row and per
element against tests/rows_ref.py (fp64 closed forms), at every width that is a template
instantiation or sits on a 64-vector boundary, on the value cases where a row kernel goes wrong
(an outlier in the first / last lane, a shifted mean, a spread below eps; peaked, offset and
masked scores; gates where 1 + erff() cancels and where expf underflows), and past the grid caps
of the grid-stride loops.

tests/test_transformer_gpu.py and tests/test_bf16_gpu.py feed ``randn`` and bound one relative-L2
figure per tensor.  Here the library entry points are called directly, so LayerNorm's saved
``mean`` / ``rstd`` and the softmax's ``lse`` are judged too; every output buffer is filled with
NaN and carries a 64-element NaN tail (afterwards the body must be finite and the tail still NaN);
rows = 9 is two whole workgroups plus one wave, and rows = 1 and 0 run as well; a row computed
alone must have the bits it has inside the batch, and a row permutation of GEGLU's input must
permute its output; a test of its own asserts from the profiler's kernel names that each width
ran the instantiation it is in the table for; and the refusals (SP_EINVAL) and the torch
fall-backs behind them are pinned.  Every figure goes to ``parity_record`` before anything is
asserted, and each test collects its misses and fails once at the end.

Largest figures measured on the MI355X over all widths and cases (the fp32 CPU emulation of
tests/rows_ref.py in brackets); ``parity_record`` holds every one:

  LayerNorm fp32   rstd 1.8e-7 of 5e-6 (2.1e-7), mean 0.39 of its bound (0.65), y 0.20 of its bound
                   (0.33), dx per row 7.1e-6 of 2e-5 (7.1e-6); the largest three on mean_30_std_1
  LayerNorm bf16   rstd 1.9e-7 of 5e-6 (1.9e-7), mean 0.11 (0.11), y 0.989 of its bound (0.989), dx per
                   row 3.77e-3 of 3.93e-3 (3.77e-3): the bf16 figures are one rounding, nearly attained
  GEGLU fp32       y 1.27, da 1.26, dgate 1.84 ULP units of 12 (1.27 / 1.26 / 1.78), all on the
                   second-trip shape; bf16 0.995 / 0.995 / 0.996 of the bound (the same)
  softmax          p 1.65, row sum 1.64, lse 0.56, VJP 1.57 ULP units of 8 (1.85 / 1.87 / 0.54 / 1.57)
  1x1 conv         integer cases exact; randn 0.27 of the bound (0.31)
  fall-backs       torch LayerNorm at c = 2052: y 0.011 of its bound, dx 1.9e-7; bf16 at 2056: 0.991
                   and 3.52e-3 of 3.93e-3; attention with 4100 keys 2.2e-7 of 6.7e-5; conv at hw = 6: 0.12
"""

from __future__ import annotations

import math

import pytest
import torch

import gn_ref
import rows_ref as rr
from kind_harness import run_debug_child

pytestmark = pytest.mark.gpu

SP_OK, SP_EINVAL = 0, -1
ROWS, TAIL = rr.ROWS, rr.TAIL
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")

def _lib():
    from samplers_amd import _hip

    return _hip.load_library()


def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _out(shape, cuda, dtype=F32):
    """(view, buffer): a NaN-filled output of ``shape`` with TAIL NaN elements behind it."""
    n = math.prod(shape)
    buf = torch.full((n + TAIL,), NAN, device=cuda, dtype=dtype)
    return buf[:n].view(shape), buf


def _inout(t: torch.Tensor, cuda, dtype=F32):
    """(view, buffer): ``t`` on the device for an in-place kernel, with the NaN tail behind it."""
    view, buf = _out(tuple(t.shape), cuda, dtype)
    view.copy_(t.to(dtype))
    return view, buf


def _guard_ok(*pairs) -> bool:
    """Every (view, buffer): the body finite, the tail still NaN."""
    for view, buf in pairs:
        n = view.numel()
        if buf.numel() != n + TAIL or not bool(torch.isfinite(buf[:n]).all()) or not bool(torch.isnan(buf[n:]).all()):
            return False
    return True


def _untouched(*pairs) -> bool:
    return all(bool(torch.isnan(buf).all()) for _, buf in pairs)


def _kernel_names(fn) -> set[str]:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type.name == "CUDA"}


def _is(name: str, kernel: str, v: int | None = None) -> bool:
    """``name`` (demangled or mangled) is kernel template ``kernel`` (with first argument v)."""
    if v is None:
        return kernel + "<" in name or f"{len(kernel)}{kernel}I" in name
    return f"{kernel}<{v}>" in name or f"{len(kernel)}{kernel}ILi{v}E" in name


class _Book:
    """Records every figure, prints it, and keeps the misses for one assert at the end."""

    def __init__(self, parity_record, **tag):
        self.rec, self.tag, self.bad = parity_record, tag, []

    def figures(self, figs: dict, shape=None, **tag) -> None:
        tag = {**self.tag, **tag}
        for metric, fig in figs.items():
            value, bound = fig[0], fig[1]
            extra = {}
            if len(fig) > 2 and isinstance(fig[2], tuple):      # a per-row figure names its row
                extra = {"worst_at": list(fig[2])}
            elif len(fig) > 2 and shape is not None:
                extra = {"worst_at": list(rr.flat_index(fig[2], shape))}
            self.rec(metric, value, bound, **tag, **extra)
            if not value <= bound:
                self.bad.append((metric, value, bound, tag, extra))
        print(" ".join(f"{k}={v}" for k, v in tag.items()) + ": "
              + ", ".join(f"{m} {f[0]:.3g}/{f[1]:.3g}" for m, f in figs.items()))

    def check(self, ok: bool, what: str, **tag) -> None:
        if not ok:
            self.bad.append((what, {**self.tag, **tag}))

    def done(self) -> None:
        assert not self.bad, self.bad


# =============================================================================================
# LayerNorm
# =============================================================================================
class _Ln:
    """sp_layernorm_* / sp_layernorm_bf16_* on guarded buffers."""

    def __init__(self, bf16: bool, cuda):
        lib = _lib()
        self.fwd_fn = lib.sp_layernorm_bf16_fwd if bf16 else lib.sp_layernorm_fwd
        self.bwd_fn = lib.sp_layernorm_bf16_bwd if bf16 else lib.sp_layernorm_bwd
        self.dt, self.cuda = (BF16 if bf16 else F32), cuda

    def dev(self, t):
        return t.to(self.cuda, self.dt).contiguous()

    def fwd(self, x, gamma, beta, eps):
        rows, c = x.shape
        y, mean, rstd = _out((rows, c), self.cuda, self.dt), _out((rows,), self.cuda), _out((rows,), self.cuda)
        rc = self.fwd_fn(_p(x), _p(gamma), _p(beta), rows, c, eps, _p(y[0]), _p(mean[0]), _p(rstd[0]), _st())
        return rc, y, mean, rstd

    def bwd(self, dz, x, gamma, mean, rstd, add):
        rows, c = x.shape
        dx = _out((rows, c), self.cuda, self.dt)
        rc = self.bwd_fn(_p(dz), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), rows, c, _p(dx[0]), _st())
        return rc, dx


def _layernorm_width(cuda, parity_record, c: int, bf16: bool) -> None:
    k = _Ln(bf16, cuda)
    name = "layernorm_bf16" if bf16 else "layernorm"
    book = _Book(parity_record, kernel=name, c=c, nv=rr.ln_bf16_nv(c) if bf16 else rr.ln_nv(c))
    eps_once = rr.LN_BF16_EPS_ONCE if bf16 else rr.LN_EPS_ONCE
    for case in rr.ln_cases_at(c, bf16):
        t = rr.ln_case(case, ROWS, c, bf16)
        x, dz, add = k.dev(t.x), k.dev(t.dz), k.dev(t.add)
        gamma, beta = t.gamma.to(cuda), t.beta.to(cuda)
        for eps in (gn_ref.EPS,) + ((eps_once[1],) if c == eps_once[0] and case == 1 else ()):
            rc, y, mean, rstd = k.fwd(x, gamma, beta, eps)
            book.check(rc == SP_OK and _guard_ok(y, mean, rstd), "forward rc / guards", case=case, eps=eps)
            for with_add in (False, True):
                rc, dx = k.bwd(dz, x, gamma, mean[0], rstd[0], add if with_add else None)
                book.check(rc == SP_OK and _guard_ok(dx), "vjp rc / guards", case=case, eps=eps, add=with_add)
                ref = rr.ln_reference(case, ROWS, c, eps, with_add, bf16)
                book.figures(rr.ln_figures(mean[0], rstd[0], y[0], dx[0], ref, t.gamma, bf16),
                             case=rr.LN_CASES[case], eps=eps, add=with_add)
                if eps != gn_ref.EPS:
                    continue
                # a row computed alone has the bits it has inside the batch
                for r in (0, 4, ROWS - 1):
                    rc1, y1, m1, s1 = k.fwd(x[r:r + 1], gamma, beta, eps)
                    rc2, d1 = k.bwd(dz[r:r + 1], x[r:r + 1], gamma, m1[0], s1[0], add[r:r + 1] if with_add else None)
                    same = (torch.equal(y1[0][0], y[0][r]) and torch.equal(m1[0][0], mean[0][r])
                            and torch.equal(s1[0][0], rstd[0][r]) and torch.equal(d1[0][0], dx[0][r]))
                    book.check(rc1 == SP_OK and rc2 == SP_OK and _guard_ok(y1, m1, s1, d1) and same,
                               "row alone != row in the batch", case=case, row=r, add=with_add)
    # rows = 0: served, nothing written
    x0 = torch.empty(0, c, device=cuda, dtype=k.dt)
    g1, b1 = torch.ones(c, device=cuda), torch.zeros(c, device=cuda)
    rc, y, mean, rstd = k.fwd(x0, g1, b1, 1e-6)
    rc2, dx = k.bwd(x0, x0, g1, mean[0], rstd[0], None)
    book.check(rc == SP_OK and rc2 == SP_OK and _untouched(y, mean, rstd, dx), "rows = 0")
    book.done()


@pytest.mark.parametrize("c", rr.LN_WIDTHS)
def test_layernorm_statistics_forward_and_vjp_per_row(cuda, parity_record, c):
    """sp_layernorm_fwd / _bwd: mean / rstd per row, y per element and dx per row against fp64
    (the gn_ref bounds), with and without the addend, rows = 9, 1 and 0."""
    _layernorm_width(cuda, parity_record, c, False)


@pytest.mark.parametrize("c", rr.LN_BF16_WIDTHS)
def test_layernorm_bf16_statistics_forward_and_vjp_per_row(cuda, parity_record, c):
    """sp_layernorm_bf16_fwd / _bwd against fp64 of the bf16-rounded inputs: the fp32 statistics at
    the fp32 bounds, y and dx at one bf16 rounding more."""
    _layernorm_width(cuda, parity_record, c, True)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_layernorm_through_the_layer(cuda, parity_record, bf16):
    """``layers.layer_norm`` (autograd function, the addend through the SkipGrad box) once, at the
    same bounds."""
    from samplers_amd.networks.layers import LayerNorm, SkipGrad, layer_norm

    c, case = (520, 2) if bf16 else (320, 2)
    dt = BF16 if bf16 else F32
    t = rr.ln_case(case, ROWS, c, bf16)
    gamma, beta = (rr.rb(t.gamma), rr.rb(t.beta)) if bf16 else (t.gamma, t.beta)
    ref = rr.ln_fp64(t.x, gamma, beta, 1e-6, t.dz, t.add)
    mod = LayerNorm(c, eps=1e-6)
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
    mod = mod.requires_grad_(False).to(cuda, dt)
    x = t.x.to(cuda, dt).requires_grad_(True)
    box = SkipGrad()

    def run():
        y = layer_norm(x, mod, box)
        box.grad = t.add.to(cuda, dt)
        (dx,) = torch.autograd.grad(y, x, t.dz.to(cuda, dt))
        return y.detach(), dx

    y, dx = run()
    assert box.enabled and box.grad is None
    names = _kernel_names(run)
    kern = "k_layernorm_bf16" if bf16 else "k_layernorm"
    assert any(_is(nm, kern + "_fwd", 2) for nm in names) and any(_is(nm, kern + "_bwd", 2) for nm in names), names
    figs = rr.ln_figures(ref.mean, ref.rstd, y, dx, ref, gamma, bf16)
    book = _Book(parity_record, kernel="layers.layer_norm", c=c, bf16=bf16)
    book.figures({m: figs[m] for m in ("fwd_of_bound", "vjp_per_row")}, case=rr.LN_CASES[case])
    book.done()


# =============================================================================================
# GEGLU
# =============================================================================================
def _geglu_run(cuda, h, dy, bf16: bool):
    lib = _lib()
    dt = BF16 if bf16 else F32
    fwd, bwd = (lib.sp_geglu_bf16_fwd, lib.sp_geglu_bf16_bwd) if bf16 else (lib.sp_geglu_fwd, lib.sp_geglu_bwd)
    rows, f = dy.shape
    y, dh = _out((rows, f), cuda, dt), _out((rows, 2 * f), cuda, dt)
    rc1 = fwd(_p(h), rows, f, _p(y[0]), _st())
    rc2 = bwd(_p(h), _p(dy), rows, f, _p(dh[0]), _st())
    return rc1, rc2, y, dh


def _geglu_shape(cuda, parity_record, rows: int, f: int, bf16: bool, trip: bool) -> None:
    dt = BF16 if bf16 else F32
    book = _Book(parity_record, kernel="geglu_bf16" if bf16 else "geglu", rows=rows, f=f, second_trip=trip)
    hc, dyc = rr.geglu_case(rows, f, bf16)
    ref = rr.geglu_fp64(hc, dyc)
    h, dy = hc.to(cuda, dt), dyc.to(cuda, dt)
    rc1, rc2, y, dh = _geglu_run(cuda, h, dy, bf16)
    book.check(rc1 == SP_OK and rc2 == SP_OK and _guard_ok(y, dh), "rc / guards")
    book.figures(rr.geglu_figures(y[0], dh[0], hc, dyc, ref, bf16), shape=(rows, f))
    if rows > 1:
        perm = torch.randperm(rows, generator=torch.Generator().manual_seed(rows)).to(cuda)
        _, _, yp, dhp = _geglu_run(cuda, h[perm].contiguous(), dy[perm].contiguous(), bf16)
        same = torch.equal(yp[0].view(torch.int16 if bf16 else torch.int32), y[0][perm].view(torch.int16 if bf16 else torch.int32))
        same = same and torch.equal(dhp[0].view(torch.int16 if bf16 else torch.int32),
                                    dh[0][perm].view(torch.int16 if bf16 else torch.int32))
        book.check(_guard_ok(yp, dhp) and same, "a row permutation of the input does not permute the output")
    book.done()


@pytest.mark.parametrize("rows,f", rr.GEGLU_SHAPES, ids=lambda v: str(v))
def test_geglu_per_element(cuda, parity_record, rows, f):
    """sp_geglu_fwd / _bwd on the gate table, per element against the erfc form in fp64."""
    _geglu_shape(cuda, parity_record, rows, f, False, False)


@pytest.mark.parametrize("rows,f", rr.GEGLU_BF16_SHAPES, ids=lambda v: str(v))
def test_geglu_bf16_per_element(cuda, parity_record, rows, f):
    _geglu_shape(cuda, parity_record, rows, f, True, False)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_geglu_second_grid_stride_trip(cuda, parity_record, bf16):
    """6560 x 1280 = 8,396,800 outputs: 2048 more than the capped grid covers in one trip (the SD
    UNet reaches this at 64x64 latents from batch 2).  Judged per element like the rest; the
    outputs were NaN before, so the elements of the second trip were written by it."""
    rows, f = rr.GEGLU_TRIP
    cap = rr.trip_elements(*((rr.GEGLU_BF16_GRID_CAP, rr.GEGLU_BF16_VEC) if bf16 else (rr.GEGLU_GRID_CAP, rr.GEGLU_VEC)))
    assert rows * f > cap
    _geglu_shape(cuda, parity_record, rows, f, bf16, True)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_geglu_through_the_layer_and_empty(cuda, parity_record, bf16):
    """``layers.geglu`` + autograd once at (9, 1280), and rows = 0 through the library."""
    from samplers_amd.networks.layers import geglu

    rows, f = 9, 1280
    dt = BF16 if bf16 else F32
    hc, dyc = rr.geglu_case(rows, f, bf16)
    ref = rr.geglu_fp64(hc, dyc)
    h = hc.to(cuda, dt).requires_grad_(True)
    out = {}

    def run():
        y = geglu(h)
        (out["dh"],) = torch.autograd.grad(y, h, dyc.to(cuda, dt))
        out["y"] = y.detach()

    names = _kernel_names(run)
    kern = "k_geglu_bf16" if bf16 else "k_geglu"
    assert any(kern + "_fwd" in nm for nm in names) and any(kern + "_bwd" in nm for nm in names), names
    book = _Book(parity_record, kernel="layers.geglu", rows=rows, f=f, bf16=bf16)
    book.figures(rr.geglu_figures(out["y"], out["dh"], hc, dyc, ref, bf16), shape=(rows, f))
    e = torch.empty(0, 2 * f, device=cuda, dtype=dt)
    rc1, rc2, y0, dh0 = _geglu_run(cuda, e, e[:, :f].contiguous(), bf16)
    book.check(rc1 == SP_OK and rc2 == SP_OK and _untouched(y0, dh0), "rows = 0")
    book.done()


# =============================================================================================
# Row softmax
# =============================================================================================
def _softmax(cuda, s: torch.Tensor, with_lse: bool):
    rows, n = s.shape
    p = _inout(s, cuda)
    lse = _out((rows,), cuda)
    rc = _lib().sp_softmax_rows(_p(p[0]), rows, n, _p(lse[0]) if with_lse else None, _st())
    return rc, p, lse


def _softmax_bwd(cuda, p: torch.Tensor, dp: torch.Tensor, scale: float):
    rows, n = dp.shape
    ds = _inout(dp, cuda)
    rc = _lib().sp_softmax_bwd_rows(_p(p), _p(ds[0]), rows, n, scale, _st())
    return rc, ds


@pytest.mark.parametrize("n", rr.SM_WIDTHS)
def test_softmax_rows_per_element(cuda, parity_record, n):
    """sp_softmax_rows with and without ``lse`` (the same bits either way), p per element, lse and
    the row sums per row, the -inf scores exactly 0; rows = 9, 1 (the same bits) and 0."""
    book = _Book(parity_record, kernel="softmax_rows", n=n, nv=rr.sm_nv(n))
    for case in rr.sm_cases_at(n):
        s = rr.softmax_case(case, ROWS, n)
        ref = rr.softmax_fp64(s)
        rc1, p, lse = _softmax(cuda, s, True)
        rc2, q, none = _softmax(cuda, s, False)
        book.check(rc1 == SP_OK and rc2 == SP_OK and _guard_ok(p, lse, q) and _untouched(none), "rc / guards", case=case)
        book.check(torch.equal(p[0].view(torch.int32), q[0].view(torch.int32)), "p differs with lse == NULL", case=case)
        book.figures(rr.softmax_figures(p[0], lse[0], ref, s), shape=(ROWS, n), case=case)
        for r in (0, 4, ROWS - 1):
            rc, p1, l1 = _softmax(cuda, s[r:r + 1], True)
            book.check(rc == SP_OK and _guard_ok(p1, l1) and torch.equal(p1[0][0], p[0][r])
                       and torch.equal(l1[0][0], lse[0][r]), "row alone != row in the batch", case=case, row=r)
    rc, p0, l0 = _softmax(cuda, torch.empty(0, n), True)
    book.check(rc == SP_OK and _untouched(l0) and bool(torch.isnan(p0[1]).all()), "rows = 0")
    book.done()


@pytest.mark.parametrize("n", rr.SM_WIDTHS)
def test_softmax_vjp_per_element(cuda, parity_record, n):
    """sp_softmax_bwd_rows on its own: p is the fp64 softmax rounded to fp32, dp randn and
    randn + 1e3, scale 0.5 and 512^-1/2."""
    book = _Book(parity_record, kernel="softmax_bwd_rows", n=n, nv=rr.sm_nv(n))
    for case in rr.sm_cases_at(n):
        p32 = rr.softmax_fp64(rr.softmax_case(case, ROWS, n)).p.float()
        p = p32.to(cuda)
        for kind in rr.SM_DP:
            dp = rr.softmax_vjp_case(kind, ROWS, n)
            for scale in rr.SM_SCALES:
                rc, ds = _softmax_bwd(cuda, p, dp, scale)
                book.check(rc == SP_OK and _guard_ok(ds), "rc / guards", case=case, dp=kind, scale=scale)
                book.figures(rr.softmax_vjp_figures(ds[0], rr.softmax_vjp_fp64(p32, dp, scale), p32, dp, scale),
                             shape=(ROWS, n), case=case, dp=kind, scale=round(scale, 4))
            for r in (0, 4, ROWS - 1):
                rc, d1 = _softmax_bwd(cuda, p[r:r + 1], dp[r:r + 1], rr.SM_SCALES[-1])
                book.check(rc == SP_OK and _guard_ok(d1) and torch.equal(d1[0][0], ds[0][r]),
                           "row alone != row in the batch", case=case, dp=kind, row=r)
    e = torch.empty(0, n, device=cuda)
    rc, d0 = _softmax_bwd(cuda, e, torch.empty(0, n), 0.5)
    book.check(rc == SP_OK and bool(torch.isnan(d0[1]).all()), "rows = 0")
    book.done()


# =============================================================================================
# 1x1 conv over 4 / 8 channels
# =============================================================================================
def _conv(cuda, x, w, b, trans: int):
    n, c, hw = x.shape
    y = _out((n, c, hw), cuda)
    rc = _lib().sp_conv1x1_small(_p(x), _p(w), _p(b), n, c, c, hw, trans, _p(y[0]), _st())
    return rc, y


@pytest.mark.parametrize("c", rr.CONV_C)
def test_conv1x1_small_exact_and_per_element(cuda, parity_record, c):
    """sp_conv1x1_small on integer operands (forward with and without bias, trans = 1): equal to
    the int64 einsum; one randn case against fp64 per element."""
    book = _Book(parity_record, kernel="conv1x1_small", c=c)
    for n in rr.CONV_N:
        for hw in rr.CONV_HW:
            xc, wc, bc = rr.conv_int_case(c, n, hw)
            x, w, b = xc.to(cuda), wc.to(cuda), bc.to(cuda)
            for bias, trans in ((b, 0), (None, 0), (None, 1)):
                rc, y = _conv(cuda, x, w, bias, trans)
                want = rr.conv_exact(xc, wc, None if bias is None else bc, bool(trans))
                wrong = int((y[0].cpu().double() != want.double()).sum())
                book.check(rc == SP_OK and _guard_ok(y), "rc / guards", n=n, hw=hw, trans=trans)
                book.figures({"conv1x1_int_wrong_elements": (wrong, 0)}, n=n, hw=hw, bias=bias is not None, trans=trans)
    n, hw = 3, 1028
    xc, wc, bc = rr.conv_randn_case(c, n, hw)
    for bias, trans in ((bc, 0), (None, 1)):
        rc, y = _conv(cuda, xc.to(cuda), wc.to(cuda), None if bias is None else bias.to(cuda), trans)
        ref, bound = rr.conv_fp64(xc, wc, bias, bool(trans))
        q = (y[0].cpu().double() - ref).abs() / bound
        i = int(q.argmax())
        book.check(rc == SP_OK and _guard_ok(y), "rc / guards", trans=trans)
        book.figures({"conv1x1_of_bound": (float(q.reshape(-1)[i]), 1.0, i)}, shape=(n, c, hw), n=n, hw=hw, trans=trans)
    rc, y0 = _conv(cuda, torch.empty(0, c, 8, device=cuda), wc.to(cuda), None, 0)
    book.check(rc == SP_OK and _untouched(y0), "n = 0")
    book.done()


def test_conv1x1_small_second_grid_stride_trip(cuda, parity_record):
    """c = 4, hw = 2^22 + 1024: 1,048,832 float4 pixels against 4096 x 256 threads, on the integer
    case (exact), forward with bias and trans = 1."""
    c, n, hw = rr.CONV_TRIP
    assert n * hw > rr.trip_elements(rr.CONV_GRID_CAP, rr.CONV_VEC)
    xc, wc, bc = rr.conv_int_case(c, n, hw)
    x, w, b = xc.to(cuda), wc.to(cuda), bc.to(cuda)
    bad = []
    for bias, trans in ((b, 0), (None, 1)):
        rc, y = _conv(cuda, x, w, bias, trans)
        want = rr.conv_exact(xc, wc, None if bias is None else bc, bool(trans)).float().to(cuda)
        wrong = int((y[0] != want).sum())
        parity_record("conv1x1_int_wrong_elements", wrong, 0, kernel="conv1x1_small", c=c, n=n, hw=hw, trans=trans,
                      second_trip=True)
        if not (rc == SP_OK and _guard_ok(y) and wrong == 0):
            bad.append((trans, rc, wrong))
    assert not bad, bad


# =============================================================================================
# Dispatch
# =============================================================================================
def test_each_width_runs_its_instantiation(cuda):
    """From the profiler's kernel names: every width launches the NV it is in the table for and no
    other, and over the tables every instantiation of the eight templated kernels runs."""
    seen = set()

    def only(names, kernel, nv):
        mine = {nm for nm in names if _is(nm, kernel)}
        assert mine and all(_is(nm, kernel, nv) for nm in mine), (kernel, nv, names)
        seen.add((kernel, nv))

    for bf16, widths, nvf in ((False, rr.LN_WIDTHS, rr.ln_nv), (True, rr.LN_BF16_WIDTHS, rr.ln_bf16_nv)):
        k = _Ln(bf16, cuda)
        for c in widths:
            x = torch.randn(ROWS, c, device=cuda).to(k.dt)
            g1, b1 = torch.ones(c, device=cuda), torch.zeros(c, device=cuda)

            def run():
                rc, y, mean, rstd = k.fwd(x, g1, b1, 1e-6)
                rc2, dx = k.bwd(x, x, g1, mean[0], rstd[0], None)
                assert rc == SP_OK and rc2 == SP_OK

            names = _kernel_names(run)
            kern = "k_layernorm_bf16" if bf16 else "k_layernorm"
            only(names, kern + "_fwd", nvf(c))
            only(names, kern + "_bwd", nvf(c))
    for n in rr.SM_WIDTHS:
        s = torch.randn(ROWS, n)

        def run():
            rc, p, _ = _softmax(cuda, s, False)
            rc2, _ = _softmax_bwd(cuda, p[0], s, 0.5)
            assert rc == SP_OK and rc2 == SP_OK

        names = _kernel_names(run)
        only(names, "k_softmax_rows", rr.sm_nv(n))
        only(names, "k_softmax_bwd_rows", rr.sm_nv(n))
    want = {(k, v) for k in ("k_layernorm_fwd", "k_layernorm_bwd") for v in range(1, 9)}
    want |= {(k, v) for k in ("k_layernorm_bf16_fwd", "k_layernorm_bf16_bwd") for v in range(1, 5)}
    want |= {(k, v) for k in ("k_softmax_rows", "k_softmax_bwd_rows") for v in (1, 2, 4, 8, 16)}
    assert seen == want, want ^ seen


# =============================================================================================
# Refusals and fall-backs
# =============================================================================================
def test_refusals_return_einval_and_write_nothing(cuda):
    lib = _lib()
    st = _st()
    rcs = {}
    outs = []

    def buf(n, dt=F32):
        o = _out((n,), cuda, dt)
        outs.append(o)
        return o[0]

    src = torch.randn(ROWS * 4100, device=cuda)
    srcb = src.to(BF16)
    w = torch.ones(4100, device=cuda)
    for c in (2052, 6):
        n = ROWS * c
        rcs[f"ln_fwd {c}"] = lib.sp_layernorm_fwd(_p(src), _p(w), _p(w), ROWS, c, 1e-6, _p(buf(n)), _p(buf(ROWS)), _p(buf(ROWS)), st)
        rcs[f"ln_bwd {c}"] = lib.sp_layernorm_bwd(_p(src), _p(src), _p(w), _p(w), _p(w), None, ROWS, c, _p(buf(n)), st)
        rcs[f"ln_bf16_fwd {c}"] = lib.sp_layernorm_bf16_fwd(_p(srcb), _p(w), _p(w), ROWS, c, 1e-6, _p(buf(n, BF16)),
                                                          _p(buf(ROWS)), _p(buf(ROWS)), st)
        rcs[f"ln_bf16_bwd {c}"] = lib.sp_layernorm_bf16_bwd(_p(srcb), _p(srcb), _p(w), _p(w), _p(w), None, ROWS, c,
                                                          _p(buf(n, BF16)), st)
        assert not lib.sp_layernorm_supported(ROWS, c) and not lib.sp_layernorm_bf16_supported(ROWS, c)
    keep = src.clone()
    for n in (4100, 6):
        rcs[f"softmax {n}"] = lib.sp_softmax_rows(_p(src), ROWS, n, _p(buf(ROWS)), st)
        rcs[f"softmax_bwd {n}"] = lib.sp_softmax_bwd_rows(_p(keep), _p(src), ROWS, n, 0.5, st)
        assert not lib.sp_softmax_rows_supported(ROWS, n)
    # aliased operands at a served width
    c = 320
    rcs["ln_fwd x == y"] = lib.sp_layernorm_fwd(_p(src), _p(w), _p(w), ROWS, c, 1e-6, _p(src), _p(buf(ROWS)), _p(buf(ROWS)), st)
    rcs["ln_bwd dx == x"] = lib.sp_layernorm_bwd(_p(w), _p(src), _p(w), _p(w), _p(w), None, ROWS, c, _p(src), st)
    rcs["softmax_bwd p == dp"] = lib.sp_softmax_bwd_rows(_p(src), _p(src), ROWS, c, 0.5, st)
    rcs["geglu_bwd dh == h"] = lib.sp_geglu_bwd(_p(src), _p(w), ROWS, c // 2, _p(src), st)
    rcs["conv trans + bias"] = lib.sp_conv1x1_small(_p(src), _p(w), _p(w), 1, 4, 4, 8, 1, _p(buf(32)), st)
    rcs["conv hw % 4"] = lib.sp_conv1x1_small(_p(src), _p(w), None, 1, 4, 4, 6, 0, _p(buf(24)), st)
    assert not lib.sp_conv1x1_small_supported(4, 4, 6) and lib.sp_conv1x1_small_supported(4, 4, 8)
    torch.cuda.synchronize()
    assert all(rc == SP_EINVAL for rc in rcs.values()), {k: v for k, v in rcs.items() if v != SP_EINVAL}
    assert _untouched(*outs) and torch.equal(src, keep)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_layer_norm_past_the_widest_kernel_falls_back_to_torch(cuda, parity_record, bf16):
    """c = 2052 (fp32) / 2056 (bf16) is one vector more than the widest instantiation holds:
    ``layers.layer_norm`` clears the box and torch computes it, at the same bounds."""
    from samplers_amd.networks.layers import LayerNorm, SkipGrad, layer_norm

    c = 2056 if bf16 else 2052
    dt = BF16 if bf16 else F32
    t = rr.ln_case(1, ROWS, c, bf16)
    gamma, beta = (rr.rb(t.gamma), rr.rb(t.beta)) if bf16 else (t.gamma, t.beta)
    ref = rr.ln_fp64(t.x, gamma, beta, 1e-6, t.dz, None)
    mod = LayerNorm(c, eps=1e-6)
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
    mod = mod.requires_grad_(False).to(cuda, dt)
    x = t.x.to(cuda, dt).requires_grad_(True)
    box = SkipGrad()
    out = {}

    def run():
        out["y"] = layer_norm(x, mod, box)

    names = _kernel_names(run)
    assert box.enabled is False
    assert not any("k_layernorm" in nm for nm in names), names
    (dx,) = torch.autograd.grad(out["y"], x, t.dz.to(cuda, dt))
    figs = rr.ln_figures(ref.mean, ref.rstd, out["y"].detach(), dx, ref, gamma, bf16)
    book = _Book(parity_record, kernel="layers.layer_norm (torch)", c=c, bf16=bf16)
    book.figures({m: figs[m] for m in ("fwd_of_bound", "vjp_per_row")}, case="randn")
    book.done()


def test_attention_with_4100_keys_falls_back_to_torch(cuda, parity_record):
    """``unet2d.attention`` past the softmax kernel's 4096 scores per row: torch's softmax, and
    the right answer.  Bound per element: a score carries (d / 2 + 1) ULP S at the most, S the
    largest sum_d |q||k| / sqrt(d) (a d-term dot product and the scaling), which moves the
    normalised weights by twice that in total; the softmax's own SOFTMAX_K ULP; and the 4100-term
    P V sum, sum p = 1, as a random walk of roundings, sqrt(4100) = 64 ULP / 2:
    |err| <= ULP max|v| ((d + 2) S + 8 + 32)."""
    from samplers_amd.networks.unet2d import attention

    n, d = 4100, 8
    gen = torch.Generator().manual_seed(41)
    q, k, v = (torch.randn(1, 1, n, d, generator=gen) for _ in range(3))
    qd, kd, vd = q.double(), k.double(), v.double()
    ref = torch.softmax(qd @ kd.transpose(-1, -2) / math.sqrt(d), -1) @ vd
    s_max = float((qd.abs() @ kd.abs().transpose(-1, -2)).max()) / math.sqrt(d)
    bound = rr.ULP * float(v.abs().max()) * ((d + 2) * s_max + rr.SOFTMAX_K + 32)
    names = _kernel_names(lambda: attention(q.to(cuda), k.to(cuda), v.to(cuda)))
    assert not any("k_softmax_rows" in nm for nm in names), names
    out = attention(q.to(cuda), k.to(cuda), v.to(cuda)).cpu().double()
    err = float((out - ref).abs().max())
    parity_record("attention_4100_keys_max_err", err, bound)
    print(f"attention 4100 keys: max err {err:.3g} / {bound:.3g}")
    assert out.shape == ref.shape and torch.isfinite(out).all() and err <= bound


@pytest.mark.parametrize("c", rr.CONV_C)
def test_conv1x1_small_at_hw_6_falls_back_to_torch(cuda, parity_record, c):
    from samplers_amd.networks.layers import conv1x1_small

    xc, wc, bc = rr.conv_randn_case(c, 3, 6)
    conv = torch.nn.Conv2d(c, c, 1)
    with torch.no_grad():
        conv.weight.copy_(wc.reshape(c, c, 1, 1))
        conv.bias.copy_(bc)
    conv = conv.requires_grad_(False).to(cuda)
    x = xc.reshape(3, c, 2, 3).to(cuda)
    names = _kernel_names(lambda: conv1x1_small(conv, x))
    assert not any("k_conv1x1_small" in nm for nm in names), names
    y = conv1x1_small(conv, x).reshape(3, c, 6).cpu().double()
    ref, bound = rr.conv_fp64(xc, wc, bc)
    q = float(((y - ref).abs() / bound).max())
    parity_record("conv1x1_hw6_torch_of_bound", q, 1.0, c=c)
    assert q <= 1.0, q


# =============================================================================================
# The debug library
# =============================================================================================
DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
rows = 9
_hip.debug_violations()  # clear
for bf16, widths in ((False, (252, 256, 260, 2044, 2048)), (True, (504, 512, 520, 2040, 2048))):
    dt = torch.bfloat16 if bf16 else torch.float32
    fwd = lib.sp_layernorm_bf16_fwd if bf16 else lib.sp_layernorm_fwd
    bwd = lib.sp_layernorm_bf16_bwd if bf16 else lib.sp_layernorm_bwd
    for c in widths:
        x, dy = (torch.randn(rows, c, device=dev).to(dt) for _ in range(2))
        w, b = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        stats = torch.empty(2, rows, device=dev)
        _hip.check(fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), rows, c, 1e-6, y.data_ptr(),
                       stats[0].data_ptr(), stats[1].data_ptr(), st), "layernorm fwd")
        _hip.check(bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                       None, rows, c, dx.data_ptr(), st), "layernorm bwd")
        nv, site = _hip.debug_violations()
        print("layernorm", "bf16" if bf16 else "fp32", c, "violations", nv, site, flush=True)
        assert nv == 0, (bf16, c, nv, site)
        assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all() and torch.isfinite(stats).all()
for n in (252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4092, 4096):
    s, dp = torch.randn(rows, n, device=dev) * 4, torch.randn(rows, n, device=dev)
    _hip.check(lib.sp_softmax_rows(s.data_ptr(), rows, n, None, st), "softmax")
    _hip.check(lib.sp_softmax_bwd_rows(s.data_ptr(), dp.data_ptr(), rows, n, 0.5, st), "softmax bwd")
    nv, site = _hip.debug_violations()
    print("softmax", n, "violations", nv, site, flush=True)
    assert nv == 0, (n, nv, site)
    assert torch.isfinite(s).all() and torch.isfinite(dp).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """The row kernels' SP_DCHECK width invariants (the row fits the instantiation's registers)
    under the bounds-checked library, in a fresh child process (a process holds one library), at
    the widths on either side of each 64-vector boundary."""
    run_debug_child(DEBUG_CHILD)
