"""The latent-sampler kernels (csrc/sp_latent.hip), the elementwise ReSample helpers and the
device-schedule forms of the two DPS passes (csrc/sp_dps.hip), entry point by entry point against
the fp64 semantics of tests/latent_ops.py, at the shapes where such kernels go wrong:

* the scalar (V = 1, n % 4 != 0) instantiations, with one tile and with several (the last tile
  ending inside the per-thread loop, inpaint ranks carried across tiles and 64-bit mask words);
* the second, partial trip of the grid-stride loops capped at 4096 / batch blocks (batch 400)
  and, at batch 1, past 4096 x 256 x V elements;
* the scalar fallback for pointers that are not 16-byte aligned (only where the host code checks
  alignment: sp_scaled_combine, sp_adamw_step(_until), sp_predict_x0);
* the Philox branch (xi = NULL) of the DDIM step and the stochastic resample;
* the stop rules' state (count > 1, prev_loss, the double compare, the sticky flag);
* the scheduled passes with a cursor that is not "next", for every operator kind;
* the documented aliasing (out == b, out == a, in place).

Bounds are the fused passes' standing ones (latent_ops.assert_close_scaled: 2e-5 x max|ref| per
element; assert_rsq: 2e-5 relative).  Outputs are prefilled with NaN; the number of partials is
read from sp_rsq_partials / sp_vec_partials."""

import functools
import math

import numpy as np
import pytest
import torch

import latent_ops as lo
import sr_ops
import stand_ins as si
from kind_harness import run_debug_child, stream as _stream
from oracle import blur as oblur
from oracle import closed_form, philox
from samplers_amd import _hip
from samplers_amd.operators import (GaussianBlurOperator, IdentityOperator, InpaintingOperator,
                                    SuperResolutionOperator, get_mask_random)
from samplers_amd.samplers.resample import adamw_coefficients
from samplers_amd.samplers.utils.bridge_kernels import eps_step_coefficients

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")

# (x shape, batch, y_div): the smallest shapes that reach each edge with two groups per thread
SHAPES = [
    ((3, 32, 32), 4, 1),   # V = 4, 48 full mask words, 2 tiles
    ((3, 40, 36), 6, 3),   # V = 4, 3 tiles, 224-element tail, half-used last word, shared y
    ((1, 19, 21), 2, 2),   # V = 1, one tile
    ((1, 37, 83), 3, 1),   # V = 1, n = 3071: 6 tiles, the last short by one, ranks across tiles
    ((1, 1, 3), 1, 1),     # explicit mask keeping elements 0 and 2: m = 2
]
MULTI_TILE = {(3, 32, 32), (3, 40, 36), (1, 37, 83)}
KINDS = ["identity", "inpaint", "mask", "inpaint_box", "mask_box"]
CASES = [(k, *s) for s in SHAPES for k in KINDS if not (s[0] == (1, 1, 3) and k.endswith("_box"))]
CASE_IDS = [f"{c[0]}-{'x'.join(map(str, c[1]))}-b{c[2]}-d{c[3]}" for c in CASES]
# batch 400: 12 blocks of work against a cap of 4096 // 400 = 10 -> a partial second trip
STRIDE = [((3, 64, 64), 400), ((1, 37, 83), 400)]
# batch 1: one element group past 4096 blocks x 256 threads x V
BIG_V1, BIG_V4 = 1_048_877, 4_195_504


def _call(name, *args):
    _hip.check(getattr(_hip.load_library(), name)(*args, _stream()), name)


def _p(t):
    return None if t is None else t.data_ptr()


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _nan_like(t):
    return torch.full_like(t, NAN)


def box_keep(n: int) -> np.ndarray:
    """Observed flags whose 64-bit words are each all-kept or all-dropped: the second quarter of
    the words and the last (possibly partial) word are dropped."""
    words = (n + 63) // 64
    w = np.arange(n) // 64
    return ~(((w >= words // 4) & (w < words // 2)) | (w == words - 1))


def make_operator(kind, shape):
    """(operator on the device, numpy fp64 apply, adjoint) for identity / inpaint / mask (random
    mask, "_box" whole-word mask; (1, 1, 3) keeps elements 0 and 2) / blur5 / blur9 / sr2."""
    n = math.prod(shape)
    if kind == "identity":
        return (IdentityOperator(shape), *closed_form.identity_ops())
    if kind.startswith("blur"):
        ks, sigma = (5, 1.5) if kind == "blur5" else (9, 3.0)
        return (GaussianBlurOperator(shape, ks, sigma).to(DEV),
                *oblur.blur_ops(shape, oblur.taps(ks, sigma)))
    if kind == "sr2":
        return (SuperResolutionOperator(shape, 2).to(DEV), *sr_ops.sr_ops(shape, 2))
    base, _, variant = kind.partition("_")
    if shape == (1, 1, 3):
        mask = torch.tensor([False, True, False]).reshape(shape)
    elif variant == "box":
        mask = ~torch.from_numpy(box_keep(n)).reshape(shape)
    else:
        mask = get_mask_random(shape, 0.5, seed=3)
    op = InpaintingOperator(shape, mask, flatten=(base == "inpaint")).to(DEV)
    keep = ~mask.flatten().numpy()
    if base == "inpaint":
        return (op, *closed_form.inpaint_ops(np.flatnonzero(keep), n))
    return (op, *closed_form.mask_ops(keep))


@functools.lru_cache(maxsize=None)
def pixel_case(kind, shape, batch, ydiv):
    """Inputs (fp32, host) and the fp64 PSLD pixel-pass reference of one case, computed once and
    shared by the tests of sp_psld_pixel, sp_psld_cotangent and sp_pixel_opt_step."""
    op, apply, adjoint = make_operator(kind, shape)
    desc = op.hip_descriptor()
    n, m = math.prod(shape), int(desc.m)
    if shape == (1, 1, 3) and kind != "identity":
        assert m == (2 if kind == "inpaint" else 3)
    x0, u = _randn(11, batch, n), _randn(12, batch, n)
    y = _randn(13, batch // ydiv, m)
    x_eff, atr, rsq = lo.psld_pixel64(x0, y, ydiv, apply, adjoint)
    P = int(_hip.load_library().sp_rsq_partials(desc))
    assert P >= 1
    if shape in MULTI_TILE:
        assert P > 1, (shape, P)
    return dict(op=op, desc=desc, apply=apply, adjoint=adjoint, n=n, m=m, P=P, x0=x0, u=u, y=y,
                x_eff=x_eff, atr=atr, rsq=rsq)


# --- sp_psld_pixel ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,batch,ydiv", CASES, ids=CASE_IDS)
def test_psld_pixel_matches_fp64(cuda, parity_record, kind, shape, batch, ydiv):
    c = pixel_case(kind, shape, batch, ydiv)
    x0d, yd = c["x0"].to(cuda), c["y"].to(cuda)
    x_eff, atr = _nan_like(x0d), _nan_like(x0d)
    part = torch.full((batch, c["P"]), NAN, device=cuda)
    _call("sp_psld_pixel", c["desc"], x0d.data_ptr(), yd.data_ptr(), batch, ydiv,
          x_eff.data_ptr(), atr.data_ptr(), part.data_ptr())
    e1 = lo.assert_close_scaled(x_eff, c["x_eff"])
    e2 = lo.assert_close_scaled(atr, c["atr"])
    e3 = lo.assert_rsq(part, c["rsq"])
    print(f"psld_pixel {kind} {shape}: x_eff {e1:.3g} atr {e2:.3g} rsq {e3:.3g} P={c['P']}")
    parity_record("psld_pixel_x_eff_max_err_over_max", e1, lo.ELEMENT_BOUND)
    parity_record("psld_pixel_atr_max_err_over_max", e2, lo.ELEMENT_BOUND)
    parity_record("psld_pixel_rsq_max_rel_err", e3, lo.RSQ_BOUND)


def test_blur_is_unsupported_by_the_fused_pixel_passes(cuda):
    """BLUR: sp_psld_pixel and sp_pixel_opt_step return SP_EUNSUPPORTED and write nothing."""
    shape, b = (1, 19, 21), 2
    op, _, _ = make_operator("blur5", shape)
    desc, lib = op.hip_descriptor(), _hip.load_library()
    n = math.prod(shape)
    x, y = torch.randn(b, n, device=cuda), torch.randn(b, n, device=cuda)
    o1, o2 = _nan_like(x), _nan_like(x)
    part = torch.full((b, int(lib.sp_rsq_partials(desc))), NAN, device=cuda)
    assert lib.sp_psld_pixel(desc, x.data_ptr(), y.data_ptr(), b, 1, o1.data_ptr(), o2.data_ptr(),
                             part.data_ptr(), _stream()) == -3
    keep = x.clone()
    assert lib.sp_pixel_opt_step(desc, x.data_ptr(), o1.data_ptr(), o2.data_ptr(), y.data_ptr(), b, 1,
                                 -0.1, adamw_coefficients(1, 1e-2), None, part.data_ptr(),
                                 _stream()) == -3
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and o1.isnan().all() and o2.isnan().all() and part.isnan().all()


# --- sp_psld_cotangent -------------------------------------------------------------------------
def _cotangent(cuda, desc, atr, u, ata_u, norm_sq, omega, batch):
    atrd, ud = atr.to(cuda), u.to(cuda)
    au = None if ata_u is None else ata_u.to(cuda)
    nd = torch.tensor([norm_sq], dtype=torch.float32, device=cuda)
    out = _nan_like(ud)
    _call("sp_psld_cotangent", desc, atrd.data_ptr(), ud.data_ptr(), _p(au), nd.data_ptr(), omega,
          batch, out.data_ptr())
    return out


@pytest.mark.parametrize("zero_norm", [False, True], ids=["norm", "zero-norm"])
@pytest.mark.parametrize("kind,shape,batch,ydiv", CASES, ids=CASE_IDS)
def test_psld_cotangent_matches_fp64(cuda, parity_record, kind, shape, batch, ydiv, zero_norm):
    c = pixel_case(kind, shape, batch, ydiv)
    atr = torch.from_numpy(c["atr"]).float()
    norm_sq = 0.0 if zero_norm else float(np.float32(c["rsq"].sum()))
    out = _cotangent(cuda, c["desc"], atr, c["u"], None, norm_sq, 0.1, batch)
    ref = lo.psld_cotangent64(atr, c["u"], norm_sq, 0.1, c["apply"], c["adjoint"])
    err = lo.assert_close_scaled(out, ref)
    if zero_norm:  # exactly (I - A^T A) u, finite
        u64 = c["u"].double().numpy()
        assert torch.isfinite(out).all()
        np.testing.assert_array_equal(out.cpu().double().numpy(),
                                      u64 - c["adjoint"](c["apply"](u64)))
    parity_record("psld_cotangent_max_err_over_max", err, lo.ELEMENT_BOUND)


@pytest.mark.parametrize("zero_norm", [False, True], ids=["norm", "zero-norm"])
@pytest.mark.parametrize("shape,batch", [((1, 19, 21), 2), ((1, 37, 83), 3)])
def test_psld_cotangent_blur_matches_fp64(cuda, parity_record, shape, batch, zero_norm):
    """BLUR (kernel 5, sigma 1.5): A^T A u computed in fp64 and passed as fp32."""
    op, apply, adjoint = make_operator("blur5", shape)
    n = math.prod(shape)
    atr, u = _randn(21, batch, n), _randn(22, batch, n)
    ata_u = torch.from_numpy(adjoint(apply(u.double().numpy()))).float()
    norm_sq = 0.0 if zero_norm else 37.5
    out = _cotangent(cuda, op.hip_descriptor(), atr, u, ata_u, norm_sq, 0.1, batch)
    err = lo.assert_close_scaled(out, lo.psld_cotangent64(atr, u, norm_sq, 0.1, apply, adjoint))
    assert torch.isfinite(out).all()
    parity_record("psld_cotangent_blur_max_err_over_max", err, lo.ELEMENT_BOUND)
    # ata_u is required for BLUR
    lib = _hip.load_library()
    assert lib.sp_psld_cotangent(op.hip_descriptor(), out.data_ptr(), out.data_ptr(), None,
                                 out.data_ptr(), 0.1, batch, out.data_ptr(), _stream()) == -1


@pytest.mark.parametrize("kind", ["identity", "mask"])
@pytest.mark.parametrize("shape,batch", STRIDE, ids=["v4-b400", "v1-b400"])
def test_psld_cotangent_second_stride_trip(cuda, parity_record, kind, shape, batch):
    op, apply, adjoint = make_operator(kind, shape)
    n = math.prod(shape)
    atr, u = _randn(31, batch, n), _randn(32, batch, n)
    out = _cotangent(cuda, op.hip_descriptor(), atr, u, None, 123.0, 0.1, batch)
    err = lo.assert_close_scaled(out, lo.psld_cotangent64(atr, u, 123.0, 0.1, apply, adjoint))
    parity_record("psld_cotangent_stride_max_err_over_max", err, lo.ELEMENT_BOUND)


# --- sp_pixel_opt_step -------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,batch,ydiv", CASES, ids=CASE_IDS)
def test_pixel_opt_step_matches_fp64(cuda, parity_record, kind, shape, batch, ydiv):
    """A set stop flag leaves everything untouched; step 1 from zero moments and step 3 from
    random moments (v >= 0) against pixel_opt64; the partials are the loss of x before the
    update."""
    c = pixel_case(kind, shape, batch, ydiv)
    desc, n, P = c["desc"], c["n"], c["P"]
    gs = float(np.float32(-2.0 / (batch * c["m"])))
    yd = c["y"].to(cuda)
    stop = torch.ones(1, dtype=torch.int32, device=cuda)
    errs = []
    for step, (m0, v0) in ((1, (torch.zeros(batch, n), torch.zeros(batch, n))),
                           (3, (0.1 * _randn(14, batch, n), 0.01 * _randn(15, batch, n).abs()))):
        coefs = adamw_coefficients(step, 1e-2)
        xd, md, vd = c["x0"].to(cuda), m0.to(cuda), v0.to(cuda)
        part = torch.full((batch, P), NAN, device=cuda)
        args = (desc, xd.data_ptr(), md.data_ptr(), vd.data_ptr(), yd.data_ptr(), batch, ydiv, gs,
                coefs)
        stop.fill_(1)
        _call("sp_pixel_opt_step", *args, stop.data_ptr(), part.data_ptr())
        assert torch.equal(xd.cpu(), c["x0"]) and torch.equal(md.cpu(), m0)
        assert torch.equal(vd.cpu(), v0) and part.isnan().all()
        stop.zero_()
        _call("sp_pixel_opt_step", *args, stop.data_ptr(), part.data_ptr())
        xr, mr, vr, rsq = lo.pixel_opt64(c["x0"], m0, v0, c["y"], ydiv, gs, coefs, c["apply"],
                                         c["adjoint"])
        errs.append((lo.assert_close_scaled(xd, xr), lo.assert_close_scaled(md, mr),
                     lo.assert_close_scaled(vd, vr), lo.assert_rsq(part, rsq)))
        np.testing.assert_allclose(rsq, c["rsq"], rtol=1e-12)  # the loss before the update
        # stop = NULL runs too, to the same bits
        x2, m2, v2 = c["x0"].to(cuda), m0.to(cuda), v0.to(cuda)
        _call("sp_pixel_opt_step", desc, x2.data_ptr(), m2.data_ptr(), v2.data_ptr(), yd.data_ptr(),
              batch, ydiv, gs, coefs, None, part.data_ptr())
        assert torch.equal(x2, xd) and torch.equal(m2, md) and torch.equal(v2, vd)
    worst = np.max(np.array(errs), axis=0)
    for name, e, bound in zip(("x", "exp_avg", "exp_avg_sq", "rsq"), worst,
                              (lo.ELEMENT_BOUND,) * 3 + (lo.RSQ_BOUND,)):
        parity_record(f"pixel_opt_{name}_max_err", e, bound)


# --- sp_ddim_eps_step / sp_stochastic_resample ---------------------------------------------------
EW = [(3, 256), (3, 1003), (3, 12288), (400, 12288), (400, 3071)]
EW_IDS = [f"b{b}-n{n}" for b, n in EW]
SEED, STEP, OFFSET = 0x1234_5678_9ABC, 17, 5


def _acp():
    return torch.cat([torch.ones(1), si.ddpm_alphas_cumprod()]).clip(1e-6, 1).numpy()


def _eps_coefs(eta):
    c = eps_step_coefficients(_acp(), 500, 480, eta)
    assert (c["sigma"] == 0.0) == (eta == 0.0)
    return _hip.SpEpsCoefs(c["sqrt_oma"], c["oma"], c["sqrt_a"], c["sqrt_a_prev"], c["sigma"],
                           c["dir"])


def _max_ulp_distance(a, b):
    """max over the elements of |a - b| in units of the fp32 spacing at max(|a|, |b|)."""
    big = torch.maximum(a.abs(), b.abs()).clamp_min(torch.finfo(torch.float32).tiny)
    _, exp = torch.frexp(big)  # big = mant x 2^exp, mant in [0.5, 1): spacing 2^(exp - 24)
    return float(((a - b).abs().double() / torch.exp2(exp.double() - 24)).max())


def _resample_scalars():
    """a_prev and sigma as samplers/resample.py forms them (fp32, sigma_scale = 40)."""
    f = np.float32
    acp = _acp()
    a_t, a_prev = f(acp[500]), f(acp[480])
    sigma = float(f(40.0) * (f(1) - a_prev) / (f(1) - a_t) * (f(1) - a_t / a_prev))
    return float(a_prev), sigma


def _ddim(x, e, b, n, coefs, xi, offset, outs=(True, True, True)):
    o = [torch.full((b, n), NAN, device=x.device) if want else None for want in outs]
    _call("sp_ddim_eps_step", x.data_ptr(), e.data_ptr(), b, n, coefs, _p(xi), SEED, STEP, offset,
          _p(o[0]), _p(o[1]), _p(o[2]))
    return o


def _philox(b, n, offset):
    z = torch.full((b, n), NAN, device=DEV)
    _call("sp_randn", z.data_ptr(), b, n, SEED, STEP, offset)
    return z


@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("b,n", EW, ids=EW_IDS)
def test_ddim_eps_step_matches_fp64(cuda, parity_record, b, n, eta):
    coefs = _eps_coefs(eta)
    x, e, xi = _randn(41, b, n), _randn(42, b, n), _randn(43, b, n)
    xd, ed, xid = x.to(cuda), e.to(cuda), xi.to(cuda)
    full = _ddim(xd, ed, b, n, coefs, xid, 0)
    refs = lo.ddim_eps64(x, e, coefs, xi)
    for name, got, ref in zip(("x_prev", "x0", "pseudo_x0"), full, refs):
        parity_record(f"ddim_eps_{name}_max_err_over_max", lo.assert_close_scaled(got, ref),
                      lo.ELEMENT_BOUND)
    # NULL outputs: the remaining ones are bit-identical to the all-outputs call
    for outs in ((True, False, False), (False, True, True), (False, False, True)):
        some = _ddim(xd, ed, b, n, coefs, xid, 0, outs)
        for want, got, ref in zip(outs, some, full):
            assert (got is None) == (not want)
            if want:
                assert torch.equal(got, ref)


@pytest.mark.parametrize("eta", [1.0, 0.0])
@pytest.mark.parametrize("b,n", EW, ids=EW_IDS)
def test_ddim_eps_step_philox_branch(cuda, b, n, eta):
    """xi = NULL draws the normals of sp_randn(seed, step, offset): bit-identical to passing
    them, and two half-batch calls with sample offsets reproduce the full call bit-for-bit.

    This test found x_prev differing between the two noise sources in the scalar kernels (35-46 %
    of the elements at n = 1003 and n = 3071, by up to 9.5e-7 absolute = one spacing of the larger
    product, 262144 ulp of a cancelling element): the compiler fused a different product of
    sqrt_a_prev x0 + dir eps + sigma xi in each instantiation.  The kernel now states its fmas."""
    coefs = _eps_coefs(eta)
    xd, ed = _randn(44, b, n).to(cuda), _randn(45, b, n).to(cuda)
    drawn = _ddim(xd, ed, b, n, coefs, None, OFFSET)
    given = _ddim(xd, ed, b, n, coefs, _philox(b, n, OFFSET), OFFSET)
    for name, d, g in zip(("x_prev", "x0", "pseudo_x0"), drawn, given):
        assert torch.isfinite(d).all()
        assert torch.equal(d, g), (f"{name}: {int((d != g).sum())} of {d.numel()} elements differ, "
                                   f"by up to {_max_ulp_distance(d, g)} ulp")
    h = b // 2
    zd = _philox(b, n, OFFSET)
    for b0, bn in ((0, h), (h, b - h)):
        part = _ddim(xd[b0:b0 + bn], ed[b0:b0 + bn], bn, n, coefs, None, OFFSET + b0)
        # injected noise: the bits do not depend on the batch (and so the grid) either
        inj = _ddim(xd[b0:b0 + bn], ed[b0:b0 + bn], bn, n, coefs, zd[b0:b0 + bn], 0)
        for d, g, i in zip(drawn, part, inj):
            assert torch.equal(d[b0:b0 + bn], g) and torch.equal(d[b0:b0 + bn], i)


def _resample(px0, xt, b, n, xi, offset):
    a_prev, sigma = _resample_scalars()
    out = torch.full((b, n), NAN, device=px0.device)
    _call("sp_stochastic_resample", px0.data_ptr(), xt.data_ptr(), b, n, a_prev, sigma, _p(xi),
          SEED, STEP, offset, out.data_ptr())
    return out


@pytest.mark.parametrize("b,n", EW, ids=EW_IDS)
def test_stochastic_resample_matches_fp64_and_philox_branch(cuda, parity_record, b, n):
    """Against fp64 with xi given; xi = NULL bit-identical to passing sp_randn's normals; half
    batches bit-identical to the full batch.  At batch 400, n = 3071 this found 47661 of 1228400
    elements differing by one spacing between the two noise sources: the injected-noise scalar
    kernel's loop was unrolled by two with the mean's products fused in the pair and unfused in
    the remainder, so an element's bits depended on the grid.  The kernel now states its fmas."""
    px0, xt, xi = _randn(51, b, n), _randn(52, b, n), _randn(53, b, n)
    pd, xd = px0.to(cuda), xt.to(cuda)
    a_prev, sigma = _resample_scalars()
    assert 0 < a_prev < 1 and sigma > 0
    err = lo.assert_close_scaled(_resample(pd, xd, b, n, xi.to(cuda), 0),
                                 lo.stochastic_resample64(px0, xt, a_prev, sigma, xi))
    parity_record("stochastic_resample_max_err_over_max", err, lo.ELEMENT_BOUND)
    drawn = _resample(pd, xd, b, n, None, OFFSET)
    given = _resample(pd, xd, b, n, _philox(b, n, OFFSET), OFFSET)
    assert torch.isfinite(drawn).all()
    assert torch.equal(drawn, given), (f"{int((drawn != given).sum())} of {drawn.numel()} elements "
                                       f"differ, by up to {_max_ulp_distance(drawn, given)} ulp")
    h = b // 2
    zd = _philox(b, n, OFFSET)
    for b0, bn in ((0, h), (h, b - h)):
        assert torch.equal(drawn[b0:b0 + bn],
                           _resample(pd[b0:b0 + bn], xd[b0:b0 + bn], bn, n, None, OFFSET + b0))
        # injected noise: the bits do not depend on the batch (and so the grid) either
        assert torch.equal(drawn[b0:b0 + bn],
                           _resample(pd[b0:b0 + bn], xd[b0:b0 + bn], bn, n, zd[b0:b0 + bn], 0))


# --- batch-1 elementwise kernels: counts, alignment, aliasing ------------------------------------
COUNTS = [1003, 4096, BIG_V1, BIG_V4]


def _view(host, misaligned):
    """A device copy of the flat fp32 tensor; misaligned: a view one float past a 16-byte
    boundary (the host code must route the call to the scalar kernel)."""
    if not misaligned:
        t = host.to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.full((host.numel() + 4,), NAN, device=DEV)
    t = buf[1:1 + host.numel()]
    t.copy_(host)
    assert t.data_ptr() % 16 == 4
    return t


# (count, which of the buffers are offset views): "all" needs count % 4 == 0 to be a test of
# the alignment check (count % 4 != 0 is scalar anyway)
LAYOUTS = [(c, "aligned") for c in COUNTS] + [(4096, "all-offset"), (4096, "one-offset")]
LAYOUT_IDS = [f"{c}-{w}" for c, w in LAYOUTS]


@pytest.mark.parametrize("count,layout", LAYOUTS, ids=LAYOUT_IDS)
def test_adamw_step_five_steps_match_fp64(cuda, parity_record, count, layout):
    """Five consecutive sp_adamw_step calls against adamw64; sp_adamw_step_until with a clear
    flag is the same step to the bit, with a set flag a no-op."""
    p0, g0 = _randn(61, count), _randn(62, count)
    m0, v0 = 0.1 * _randn(63, count), 0.01 * _randn(64, count).abs()
    off = {"aligned": (0, 0, 0, 0), "all-offset": (1, 1, 1, 1), "one-offset": (0, 1, 0, 0)}[layout]
    p, g, m, v = (_view(t, o) for t, o in zip((p0, g0, m0, v0), off))
    pr, mr, vr = p0.double().numpy(), m0.double().numpy(), v0.double().numpy()
    first = None
    for step in range(1, 6):
        c = adamw_coefficients(step, 5e-3)
        gk = torch.roll(g0, 17 * step)
        g.copy_(gk)
        _call("sp_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, c)
        pr, mr, vr = lo.adamw64(pr, gk, mr, vr, c)
        errs = (lo.assert_close_scaled(p, pr), lo.assert_close_scaled(m, mr),
                lo.assert_close_scaled(v, vr))
        if step == 1:
            first = (p.clone(), m.clone(), v.clone())
    for name, e in zip(("param", "exp_avg", "exp_avg_sq"), errs):
        parity_record(f"adamw_{name}_step5_max_err_over_max", e, lo.ELEMENT_BOUND)
    # _until: clear flag = the plain step, set flag = nothing
    flag = torch.zeros(1, dtype=torch.int32, device=cuda)
    p, g, m, v = (_view(t, o) for t, o in zip((p0, torch.roll(g0, 17), m0, v0), off))
    c1 = adamw_coefficients(1, 5e-3)
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), count, c1, flag.data_ptr())
    _call("sp_adamw_step_until", *args)
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), first))
    flag.fill_(1)
    _call("sp_adamw_step_until", *args)
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), first))


@pytest.mark.parametrize("norm", [None, 6.25, 0.0], ids=["no-norm", "norm", "zero-norm"])
@pytest.mark.parametrize("with_a", [False, True], ids=["a-null", "a"])
@pytest.mark.parametrize("count,layout", LAYOUTS, ids=LAYOUT_IDS)
def test_scaled_combine_matches_fp64_and_aliases(cuda, parity_record, count, layout, with_a, norm):
    a0, b0 = _randn(71, count), _randn(72, count)
    alpha, beta = 0.75, -1.5
    oa, ob, oo = {"aligned": (0, 0, 0), "all-offset": (1, 1, 1), "one-offset": (0, 0, 1)}[layout]
    nd = None if norm is None else torch.tensor([norm], dtype=torch.float32, device=cuda)

    def run(a, b, out):
        _call("sp_scaled_combine", _p(a), alpha, b.data_ptr(), beta, _p(nd), count, out.data_ptr())
        return out

    a = _view(a0, oa) if with_a else None
    b = _view(b0, ob)
    out = run(a, b, _view(torch.full((count,), NAN), oo))
    ref = lo.scaled_combine64(a0 if with_a else None, alpha, b0, beta, norm)
    err = lo.assert_close_scaled(out, ref)
    assert torch.isfinite(out).all()
    parity_record("scaled_combine_max_err_over_max", err, lo.ELEMENT_BOUND)
    if layout != "aligned":  # the scalar fallback computes the vector kernel's bits
        assert torch.equal(run(a0.to(cuda) if with_a else None, b0.to(cuda),
                               torch.full((count,), NAN, device=cuda)), out)
    # out aliasing b (PSLD's blur x_eff) and out aliasing a: bit-equal to the out-of-place result
    # (with one buffer offset the aliased call is the other instantiation; this found alpha a +
    # beta b fused differently in the two, fixed by an explicit fma in the kernel)
    b2 = _view(b0, ob)
    assert torch.equal(run(a, b2, b2), out)
    if with_a:
        a2 = _view(a0, oa)
        assert torch.equal(run(a2, b, a2), out)


@pytest.mark.parametrize("count,layout", LAYOUTS, ids=LAYOUT_IDS)
def test_predict_x0_matches_fp64_and_in_place(cuda, parity_record, count, layout):
    x0, e0 = _randn(81, count), _randn(82, count)
    ox, oe, oo = {"aligned": (0, 0, 0), "all-offset": (1, 1, 1), "one-offset": (0, 1, 0)}[layout]
    a, k = 0.25, 0.9
    x, e = _view(x0, ox), _view(e0, oe)
    out = _view(torch.full((count,), NAN), oo)
    _call("sp_predict_x0", x.data_ptr(), e.data_ptr(), count, a, k, out.data_ptr())
    err = lo.assert_close_scaled(out, lo.predict_x0_64(x0, e0, a, k))
    parity_record("predict_x0_max_err_over_max", err, lo.ELEMENT_BOUND)
    _call("sp_predict_x0", x.data_ptr(), e.data_ptr(), count, a, k, x.data_ptr())
    assert torch.equal(x, out)


# --- sp_sum_partials / sp_opt_check / sp_opt_check_plateau ------------------------------------------
SENTINEL = -7.0


@pytest.mark.parametrize("count", [1, 255, 256, 257, 5000])
def test_sum_partials_and_opt_check_loss(cuda, parity_record, count):
    vals = torch.rand(count, generator=torch.Generator().manual_seed(count)) + 0.1
    ref = float(vals.double().sum())
    vd = vals.to(cuda)
    out = torch.full((1,), NAN, device=cuda)
    _call("sp_sum_partials", vd.data_ptr(), count, out.data_ptr())
    e1 = abs(out.item() - ref) / ref
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    loss = torch.full((1,), NAN, device=cuda)
    total = 3.0 * count
    _call("sp_opt_check", vd.data_ptr(), count, total, 0.0, stop.data_ptr(), loss.data_ptr())
    e2 = abs(loss.item() - ref / total) / (ref / total)
    print(f"sum of {count}: {e1:.3g}, opt_check loss {e2:.3g}")
    parity_record("sum_partials_rel_err", e1, lo.RSQ_BOUND)
    parity_record("opt_check_loss_rel_err", e2, lo.RSQ_BOUND)
    assert e1 <= lo.RSQ_BOUND and e2 <= lo.RSQ_BOUND and stop.item() == 0
    model = lo.StopRule(total, 0.0)
    model.check(vals)
    assert abs(model.loss - loss.item()) <= lo.RSQ_BOUND * model.loss


def test_opt_check_compares_strictly_and_in_double_and_is_sticky(cuda):
    part = torch.full((12,), 0.25, device=cuda)  # sums to exactly 3.0 in any order
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    loss = torch.full((1,), SENTINEL, device=cuda)

    def check(threshold, p=part):
        _call("sp_opt_check", p.data_ptr(), p.numel(), 4.0, threshold, stop.data_ptr(),
              loss.data_ptr())
        return stop.item(), loss.item()

    assert check(0.75) == (0, 0.75)                              # 0.75 < 0.75 is false
    above = float(np.nextafter(np.float64(0.75), np.float64(1.0)))
    assert np.float32(above) == np.float32(0.75)                 # a float compare would not stop
    assert check(above) == (1, 0.75)
    loss.fill_(SENTINEL)
    assert check(100.0, torch.ones(12, device=cuda)) == (1, SENTINEL)  # skipped once stopped
    # loss_out may be NULL
    stop.zero_()
    _call("sp_opt_check", part.data_ptr(), 12, 4.0, 1.0, stop.data_ptr(), None)
    assert stop.item() == 1


def test_opt_check_plateau_state_machine(cuda):
    """plateau_from = 3, count = 300, losses 5, 4, 6, 3, 2, (2 again), 2.5, 1 against the host
    model: no stop on the rise at iteration 2 and prev_loss untouched below plateau_from;
    iteration 3 writes prev; a fall and an equal loss do not stop; the rise at iteration 5 stops
    and writes prev = 2.5; iteration 6 writes nothing."""
    count, total, thr, pf = 300, 300.0, 0.5, 3
    stop = torch.zeros(1, dtype=torch.int32, device=cuda)
    prev = torch.full((1,), SENTINEL, device=cuda)
    loss = torch.full((1,), SENTINEL, device=cuda)
    model = lo.StopRule(total, thr, plateau_from=pf)

    def check(itr, value):
        part = torch.full((count,), float(value), device=cuda)
        loss.fill_(SENTINEL)
        _call("sp_opt_check_plateau", part.data_ptr(), count, total, thr, itr, pf, prev.data_ptr(),
              stop.data_ptr(), loss.data_ptr())
        wrote = model.check(np.full(count, float(value)), itr)
        got = (stop.item(), prev.item(), loss.item())
        want = (model.stop, SENTINEL if model.prev is None else model.prev,
                model.loss if wrote else SENTINEL)
        assert got == want, (itr, value, got, want)
        return got

    assert check(0, 5) == (0, SENTINEL, 5.0)
    assert check(1, 4) == (0, SENTINEL, 4.0)
    assert check(2, 6) == (0, SENTINEL, 6.0)   # a rise below plateau_from
    assert check(3, 3) == (0, 3.0, 3.0)        # prev written, not compared
    assert check(4, 2) == (0, 2.0, 2.0)
    assert check(4, 2) == (0, 2.0, 2.0)        # equal loss: prev < loss is false
    assert check(5, 2.5) == (1, 2.5, 2.5)      # the rise stops, prev updated
    assert check(6, 1) == (1, 2.5, SENTINEL)   # sticky: nothing written
    # below the threshold stops before plateau_from as well, prev untouched
    stop.zero_()
    prev.fill_(SENTINEL)
    model = lo.StopRule(total, thr, plateau_from=pf)
    assert check(0, 0.25) == (1, SENTINEL, 0.25)


# --- scheduled DPS passes --------------------------------------------------------------------------
REC = [((0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9), 11, 900),
       ((0.5, 0.86, 100.0, 0.8, 0.3, 0.2, 0.07, 1e-9), 12, 600),
       ((0.7, 0.71, 50.0, 0.95, 0.1, 0.3, 0.03, 1e-9), 5_000_000_007, 1_234_567_890_123)]
OTHER = [((0.9, 0.4, 7.0, 0.1, 0.9, 0.6, 0.5, 1e-3), 99, 1), ((0.2, 0.98, 9.0, 0.5, 0.5, 0.5, 1.0, 0.0), 98, 2)]


def _sched(records):
    recs = (_hip.SpStepRec * len(records))()
    for r, (c, step, t) in zip(recs, records):
        r.c = _hip.SpDpsCoefs(*c)
        r.step, r.t = step, t
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(DEV), recs


SCHED = [(k, s) for k in ("identity", "inpaint", "mask", "blur9", "sr2")
         for s in ((3, 32, 32), (1, 8, 12) if k == "sr2" else (1, 19, 21))]


@pytest.mark.parametrize("kind,shape", SCHED, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in SCHED])
def test_scheduled_passes_read_the_cursor_record(cuda, kind, shape):
    """sp_dps_residual_sched / sp_dps_update_sched (Philox) with the cursor at record 2 of 3 are
    bit-identical (v, partials, x') to the by-value calls with record 2's coefficients and step;
    sp_sched_timestep writes record 2's t; the other records are unused (changing them changes
    nothing), while record 0's coefficients would give other values."""
    lib = _hip.load_library()
    op, _, _ = make_operator(kind, shape)
    desc = op.hip_descriptor()
    b, ydiv, n, m = 4, 2, math.prod(shape), int(desc.m)
    P = int(lib.sp_rsq_partials(desc))
    x, eps, w = (_randn(s, b, n).to(cuda) for s in (91, 92, 93))
    y = _randn(94, b // ydiv, m).to(cuda)
    need_v = kind in ("blur9", "sr2")
    seed, off = 77, 3

    def by_value(c, step):
        v, part, out = _nan_like(x), torch.full((b, P), NAN, device=cuda), _nan_like(x)
        _call("sp_dps_residual", desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, ydiv, c,
              v.data_ptr(), part.data_ptr())
        _call("sp_dps_update", desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(),
              v.data_ptr() if need_v else None, w.data_ptr(), part.data_ptr(), None, seed, step, off,
              b, ydiv, c, out.data_ptr())
        return v, part, out

    def scheduled(records):
        sched, _ = _sched(records)
        cursor = torch.zeros(1, dtype=torch.int32, device=cuda)
        _call("sp_sched_advance", cursor.data_ptr())
        _call("sp_sched_advance", cursor.data_ptr())
        assert cursor.item() == 2
        t = torch.full((1,), -1, dtype=torch.int64, device=cuda)
        _call("sp_sched_timestep", sched.data_ptr(), cursor.data_ptr(), t.data_ptr())
        assert t.item() == records[2][2]
        v, part, out = _nan_like(x), torch.full((b, P), NAN, device=cuda), _nan_like(x)
        _call("sp_dps_residual_sched", desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, ydiv,
              sched.data_ptr(), cursor.data_ptr(), v.data_ptr(), part.data_ptr())
        _call("sp_dps_update_sched", desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(),
              v.data_ptr() if need_v else None, w.data_ptr(), part.data_ptr(), seed, off, b, ydiv,
              sched.data_ptr(), cursor.data_ptr(), out.data_ptr())
        assert cursor.item() == 2  # the passes do not move it
        return v, part, out

    want = by_value(_hip.SpDpsCoefs(*REC[2][0]), REC[2][1])
    assert all(torch.isfinite(t).all() for t in want)
    for records in (REC, OTHER + REC[2:]):
        got = scheduled(records)
        for name, g, r in zip(("v", "partials", "x'"), got, want):
            assert torch.equal(g, r), (name, float((g - r).abs().max()))
    other = by_value(_hip.SpDpsCoefs(*REC[0][0]), REC[0][1])
    assert not torch.equal(other[0], want[0]) and not torch.equal(other[2], want[2])
    low = by_value(_hip.SpDpsCoefs(*REC[2][0]), REC[2][1] & 0xFFFFFFFF)  # the step is 64-bit
    assert not torch.equal(low[2], want[2])


# --- grid-stride loops of the DPS helpers ---------------------------------------------------------
@pytest.mark.parametrize("shape,batch", STRIDE, ids=["v4-b400", "v1-b400"])
def test_randn_second_stride_trip(cuda, parity_record, shape, batch):
    n = math.prod(shape)
    full = _philox(batch, n, OFFSET)
    assert torch.isfinite(full).all()
    worst = 0.0
    for row in (0, 199, 399):
        assert torch.equal(full[row:row + 1], _philox(1, n, OFFSET + row))
        ref = philox.normals(SEED, STEP, OFFSET + row, n)
        got = full[row].cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5)
        worst = max(worst, float(np.abs(got - ref).max()))
    parity_record("randn_stride_max_abs_err", worst, 2e-5)


@pytest.mark.parametrize("shape,batch", STRIDE, ids=["v4-b400", "v1-b400"])
def test_mask_apply_second_stride_trip_bit_exact(cuda, shape, batch):
    n = math.prod(shape)
    mask = get_mask_random(shape, 0.5, seed=3)
    op = InpaintingOperator(shape, mask, flatten=False).to(cuda)
    x = _randn(95, batch, n)
    xd, yd = x.to(cuda), torch.full((batch, n), NAN, device=cuda)
    _call("sp_op_apply", op.hip_descriptor(), xd.data_ptr(), yd.data_ptr(), batch)
    assert torch.equal(yd.cpu(), x.masked_fill(mask.flatten(), 0))
    back = torch.full((batch, n), NAN, device=cuda)
    _call("sp_op_adjoint", op.hip_descriptor(), xd.data_ptr(), back.data_ptr(), batch)
    assert torch.equal(back, yd)


# --- the bounds-checked library --------------------------------------------------------------------
DEBUG_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from samplers_amd import _hip
from samplers_amd.operators import InpaintingOperator, get_mask_random
from samplers_amd.samplers.resample import adamw_coefficients
lib = _hip.load_library()
assert lib.sp_debug_build() == 1, "not the debug library"
dev = torch.device("cuda:0")
st = torch.cuda.current_stream().cuda_stream
_hip.debug_violations()  # clear
shape, n = (1, 37, 83), 3071
mask = get_mask_random(shape, 0.5, seed=3)
eps_c = _hip.SpEpsCoefs(0.6, 0.36, 0.8, 0.82, 0.1, 0.55)
dps_c = _hip.SpDpsCoefs(0.3, 0.95, 400.0, 0.9, 0.2, 0.1, 0.05, 1e-9)
recs = (_hip.SpStepRec * 2)()
for r in recs:
    r.c, r.step, r.t = dps_c, 4, 9
sched = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
for b in (3, 400):
    for flatten in (True, False):
        op = InpaintingOperator(shape, mask, flatten=flatten).to(dev)
        desc = op.hip_descriptor()
        m, P = int(desc.m), int(lib.sp_rsq_partials(desc))
        x, eps, w, u = (torch.randn(b, n, device=dev) for _ in range(4))
        y = torch.randn(b, m, device=dev)
        o1, o2, o3 = (torch.empty(b, n, device=dev) for _ in range(3))
        part = torch.empty(b, P, device=dev)
        c = _hip.check
        c(lib.sp_psld_pixel(desc, x.data_ptr(), y.data_ptr(), b, 1, o1.data_ptr(), o2.data_ptr(),
                            part.data_ptr(), st), "sp_psld_pixel")
        norm = torch.empty(1, device=dev)
        c(lib.sp_sum_partials(part.data_ptr(), part.numel(), norm.data_ptr(), st), "sp_sum_partials")
        c(lib.sp_psld_cotangent(desc, o2.data_ptr(), u.data_ptr(), None, norm.data_ptr(), 0.1, b,
                                o3.data_ptr(), st), "sp_psld_cotangent")
        mm, vv = torch.zeros_like(x), torch.zeros_like(x)
        stop = torch.zeros(1, dtype=torch.int32, device=dev)
        xo = x.clone()
        c(lib.sp_pixel_opt_step(desc, xo.data_ptr(), mm.data_ptr(), vv.data_ptr(), y.data_ptr(), b, 1,
                                -2.0 / (b * m), adamw_coefficients(1, 1e-2), stop.data_ptr(),
                                part.data_ptr(), st), "sp_pixel_opt_step")
        loss, prev = torch.empty(1, device=dev), torch.zeros(1, device=dev)
        c(lib.sp_opt_check(part.data_ptr(), part.numel(), float(b * m), 1e-9, stop.data_ptr(),
                           loss.data_ptr(), st), "sp_opt_check")
        c(lib.sp_opt_check_plateau(part.data_ptr(), part.numel(), float(b * m), 1e-9, 5, 3,
                                   prev.data_ptr(), stop.data_ptr(), loss.data_ptr(), st),
          "sp_opt_check_plateau")
        c(lib.sp_ddim_eps_step(x.data_ptr(), eps.data_ptr(), b, n, eps_c, None, 7, 3, 0, o1.data_ptr(),
                               o2.data_ptr(), o3.data_ptr(), st), "sp_ddim_eps_step")
        c(lib.sp_stochastic_resample(x.data_ptr(), eps.data_ptr(), b, n, 0.9, 0.5, None, 7, 3, 0,
                                     o1.data_ptr(), st), "sp_stochastic_resample")
        c(lib.sp_adamw_step(xo.data_ptr(), w.data_ptr(), mm.data_ptr(), vv.data_ptr(), b * n,
                            adamw_coefficients(2, 1e-2), st), "sp_adamw_step")
        c(lib.sp_adamw_step_until(xo.data_ptr(), w.data_ptr(), mm.data_ptr(), vv.data_ptr(), b * n,
                                  adamw_coefficients(3, 1e-2), stop.data_ptr(), st), "sp_adamw_step_until")
        c(lib.sp_scaled_combine(x.data_ptr(), 1.0, w.data_ptr(), 0.5, norm.data_ptr(), b * n,
                                o1.data_ptr(), st), "sp_scaled_combine")
        c(lib.sp_predict_x0(x.data_ptr(), eps.data_ptr(), b * n, 0.3, 0.95, o1.data_ptr(), st),
          "sp_predict_x0")
        c(lib.sp_randn(o1.data_ptr(), b, n, 7, 3, 0, st), "sp_randn")
        ax = torch.empty(b, m, device=dev)
        c(lib.sp_op_apply(desc, x.data_ptr(), ax.data_ptr(), b, st), "sp_op_apply")
        c(lib.sp_op_adjoint(desc, ax.data_ptr(), o1.data_ptr(), b, st), "sp_op_adjoint")
        cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        c(lib.sp_sched_advance(cursor.data_ptr(), st), "sp_sched_advance")
        c(lib.sp_sched_timestep(sched.data_ptr(), cursor.data_ptr(), t.data_ptr(), st), "sp_sched_timestep")
        c(lib.sp_dps_residual_sched(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), b, 1,
                                    sched.data_ptr(), cursor.data_ptr(), o2.data_ptr(), part.data_ptr(),
                                    st), "sp_dps_residual_sched")
        c(lib.sp_dps_update_sched(desc, x.data_ptr(), eps.data_ptr(), y.data_ptr(), None, w.data_ptr(),
                                  part.data_ptr(), 7, 0, b, 1, sched.data_ptr(), cursor.data_ptr(),
                                  o3.data_ptr(), st), "sp_dps_update_sched")
        got = _hip.debug_violations()
        print("batch", b, "flatten", flatten, "violations", got, flush=True)
        assert got == (0, None), (b, flatten, got)
        assert t.item() == 9 and torch.isfinite(o3).all() and torch.isfinite(xo).all()
print("debug build: clean", flush=True)
"""


def test_debug_build_has_no_violations(cuda):
    """Every entry point of this module once under the bounds-checked library (SP_DCHECK index
    invariants), in a fresh child process (a process holds one library): the six-tile scalar
    shape (1, 37, 83) at batch 3 and at batch 400 (second stride trip), inpaint and mask."""
    run_debug_child(DEBUG_CHILD)
