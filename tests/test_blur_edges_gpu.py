"""The three Gaussian-blur kernels of csrc/sp_blur.hip at every radius, path and seam, against the
dense fp64 reference of tests/blur_ref.py.

* tile kernel ``k_blur<R, MODE>``, R = 1..8, apply / adjoint / fused DPS, on the minimal plane
  (2R+1)^2 (both fold bands on one row), on planes whose bottom and right fold bands cross the tile
  seams at row 32 and column 64 (W % 4 = 0..3 over R: float4 and scalar stores), on second tiles of
  one row and one column, and on three planes with a shared observation;
* register-streamed ``k_blur_dps_reg<R>`` (even H / 32) and LDS-DMA ``k_blur_dps_dma<R>`` (odd H / 32),
  R = 1..4: one, two, three and four segments, both sweep directions, one and two planes.

The partial counts assert which kernel a case reaches.  Every case runs three tap sets through the
raw entry points into NaN-filled, guard-banded outputs:

* exact (dyadic, asymmetric taps; integer inputs; a = k = 1/2, gs = 4): no fp32 evaluation can
  round (tests/test_blur_ref.py), so v, A x and A^T s equal the reference bit for bit;
* the operator's Gaussian taps and random asymmetric positive taps on randn data: per element,
  ``|v - v64| <= rounding_count(R) 2^-24 E_v`` (apply 2K, adjoint 4K), the derived bound of
  tests/blur_ref.py, and the partial sums to the project's 2e-5;
* near-consistent data (x = 30 + randn, y = A x0 + 1e-3 randn): the same per-element bound on v
  with the residual four orders below its operands, and rsq to the error its envelope allows.

Measured worst ratios per kernel, mode and radius go to the parity log; README "Blur edges".
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import blur_ref as br
import exact_cases as ec
from kind_harness import stream as _stream
from oracle import closed_form
from samplers_amd import _hip
from samplers_amd.operators import GaussianBlurOperator

pytestmark = pytest.mark.gpu

RSQ_RTOL = 2e-5  # the project's bound on the summed partials
TAPSETS = ("exact", "gauss", "asym")
UPD = (0.9, 0.2, 0.1, 0.05, 1e-9)  # c_ell, c_s, std, gamma, norm_eps

sid = lambda s: "x".join(map(str, s))  # noqa: E731
TILE = [(r, *c) for r in range(1, 9) for c in br.tile_cases(r)]
TILE_IDS = [f"R{r}-{sid(s)}-b{b}-d{d}" for r, s, b, d in TILE]
STREAM = [(kern, r, *c) for kern, cases in (("reg", br.REG_CASES), ("dma", br.DMA_CASES))
          for r in range(1, 5) for c in cases]
STREAM_IDS = [f"{k}-R{r}-{sid(s)}-b{b}-d{d}" for k, r, s, b, d in STREAM]
NEAR = ([("tile", r, br.tile_cases(r)[1][0]) for r in range(1, 9)]
        + [("reg", r, (1, 64, 256)) for r in range(1, 5)]
        + [("dma", r, (2, 96, 256)) for r in range(1, 5)])
NEAR_IDS = [f"{k}-R{r}-{sid(s)}" for k, r, s in NEAR]


def _call(name, *args):
    _hip.check(getattr(_hip.load_library(), name)(*args, _stream()), name)


def _dev(t, dev):
    return torch.from_numpy(np.array(t, dtype=np.float32)).to(dev)  # a copy: the cached inputs are read-only


def _coefs(a, k, gs):
    return _hip.SpDpsCoefs(a, k, gs, *UPD)


def coefs_of(tapname):
    return br.EXACT_COEFS if tapname == "exact" else br.RANDOM_COEFS


def make_op(shape, radius, tapname, dev):
    """The operator with ``tapname``'s taps on the device, and those taps (fp32, host)."""
    op = GaussianBlurOperator(shape, 2 * radius + 1, 3.0).to(dev)
    taps = br.taps_of(tapname, radius)
    if tapname == "gauss":
        assert np.array_equal(op.taps.cpu().numpy(), taps)  # the operator's own
    else:
        op.taps.copy_(torch.from_numpy(taps))
    return op, taps


def check_partials(desc, kernel, shape):
    """The partial count names the kernel the dispatch picks for this plane."""
    p = int(_hip.load_library().sp_rsq_partials(desc))
    if kernel == "tile":
        assert p == br.tile_partials(shape), (p, shape)
        assert not (shape[2] == 256 and shape[1] % 32 == 0)
    else:
        assert p == br.stream_partials(shape), (p, shape)
        assert (shape[1] // 32) % 2 == (0 if kernel == "reg" else 1)
    return p


@functools.lru_cache(maxsize=None)
def dps_case(radius, shape, batch, ydiv, tapname, data):
    """Host inputs and the fp64 pass of one case; computed once, shared, never modified."""
    taps = br.taps_of(tapname, radius)
    a, k, gs = coefs_of(tapname)
    seed = br.case_seed(radius, shape, batch)
    if data == "near":
        x, eps, y = br.near_consistent_inputs(seed, batch, ydiv, shape, taps, a, k)
    elif tapname == "exact":
        x, eps, y = br.exact_inputs(seed, batch, ydiv, shape)
    else:
        x, eps, y = br.random_inputs(seed, batch, ydiv, shape)
    ref = br.dps_pass64(x, eps, y, ydiv, a, k, gs, taps, shape)
    if tapname == "exact" and data == "plain":
        assert ref.E_v.max() * 2 ** 12 < 2 ** 24  # multiples of 2^-12 in 24 bits: nothing can round
    for t in (x, eps, y):
        t.setflags(write=False)
    return x, eps, y, ref


def run_residual(dev, desc, p, x, eps, y, batch, ydiv, coefs, sched=None, cursor=None):
    """sp_dps_residual (or its scheduled form) into guarded, NaN-filled v and partials."""
    n = x.shape[1]
    xd, ed, yd = (_dev(t, dev) for t in (x, eps, y))
    v = ec.Guarded((batch, n), n, dev)
    part = ec.Guarded((batch, p), 64, dev)
    if sched is None:
        _call("sp_dps_residual", desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv, coefs,
              v.ptr(), part.ptr())
    else:
        _call("sp_dps_residual_sched", desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), batch, ydiv,
              sched.data_ptr(), cursor.data_ptr(), v.ptr(), part.ptr())
    torch.cuda.synchronize()
    return v.check(), part.check()


def run_map(dev, desc, name, x, batch):
    xd = _dev(x, dev)
    out = ec.Guarded(tuple(x.shape), x.shape[1], dev)
    _call(name, desc, xd.data_ptr(), out.ptr(), batch)
    torch.cuda.synchronize()
    return out.check().cpu().numpy()


def bitwise_failure(got, want64, shape, radius, what):
    """None if got (fp32) equals the fp64 reference, itself an fp32 number, in every element; else
    where it differs (plane, row, column; fold band or seam)."""
    want = want64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), "the reference is not an fp32 number"
    if np.array_equal(got, want):
        return None
    return f"{what}: {br.describe_mismatch(got, want, shape, radius)}"


def worst_ratio(got, ref64, bound):
    """max |got - ref| / bound over the elements, and where."""
    ratio = np.abs(got.astype(np.float64) - ref64) / bound
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), i


def dps_tapsets(dev, kernel, radius, shape, batch, ydiv, record):
    """The exact and the two random tap sets through the fused pass of one plane."""
    worst, fails = 0.0, []
    for tapname in TAPSETS:
        op, _ = make_op(shape, radius, tapname, dev)
        desc = op.hip_descriptor()
        p = check_partials(desc, kernel, shape)
        x, eps, y, ref = dps_case(radius, shape, batch, ydiv, tapname, "plain")
        v, part = run_residual(dev, desc, p, x, eps, y, batch, ydiv, _coefs(*coefs_of(tapname)))
        v, rsq = v.cpu().numpy(), part.sum(1).cpu().numpy()
        what = f"{kernel} dps R{radius} {sid(shape)} {tapname}"
        if tapname == "exact":
            fails.append(bitwise_failure(v, ref.v, shape, radius, what))
        else:
            ratio, i = worst_ratio(v, ref.v, br.rounding_count(radius) * br.U32 * ref.E_v)
            worst = max(worst, ratio)
            print(f"{what}: worst ratio {ratio:.4f} at flat index {i}")
            fails.append(None if ratio <= 1.0 else f"{what}: ratio {ratio} at flat index {i}")
        rel = float(np.abs(rsq / ref.rsq - 1).max())
        print(f"{what}: rsq rel err {rel:.3e}")
        fails.append(None if rel <= RSQ_RTOL else f"{what}: rsq {rsq} against {ref.rsq}")
    record(f"blur_{kernel}_dps_R{radius}_ratio", worst, 1.0, shape=list(shape), batch=batch, y_div=ydiv)
    fails = [f for f in fails if f]
    assert not fails, fails


@pytest.mark.parametrize("radius,shape,batch,ydiv", TILE, ids=TILE_IDS)
def test_tile_dps(cuda, parity_record, radius, shape, batch, ydiv):
    """k_blur<R, MODE_DPS>."""
    dps_tapsets(cuda, "tile", radius, shape, batch, ydiv, parity_record)


@pytest.mark.parametrize("kernel,radius,shape,batch,ydiv", STREAM, ids=STREAM_IDS)
def test_streaming_dps(cuda, parity_record, kernel, radius, shape, batch, ydiv):
    """k_blur_dps_reg<R> (even H / 32) and k_blur_dps_dma<R> (odd H / 32)."""
    dps_tapsets(cuda, kernel, radius, shape, batch, ydiv, parity_record)


@pytest.mark.parametrize("radius,shape,batch,ydiv", TILE, ids=TILE_IDS)
def test_tile_apply_adjoint(cuda, parity_record, radius, shape, batch, ydiv):
    """k_blur<R, MODE_APPLY> and k_blur<R, MODE_ADJOINT>."""
    worst, fails = {"apply": 0.0, "adjoint": 0.0}, []
    for tapname in TAPSETS:
        op, taps = make_op(shape, radius, tapname, cuda)
        desc = op.hip_descriptor()
        check_partials(desc, "tile", shape)
        x = dps_case(radius, shape, batch, ydiv, tapname, "plain")[0]
        for mode, entry, ref_fn, count in (("apply", "sp_op_apply", br.apply64, br.apply_count(radius)),
                                           ("adjoint", "sp_op_adjoint", br.adjoint64, br.adjoint_count(radius))):
            got = run_map(cuda, desc, entry, x, batch)
            ref = ref_fn(x, taps, shape)
            what = f"tile {mode} R{radius} {sid(shape)} {tapname}"
            if tapname == "exact":
                fails.append(bitwise_failure(got, ref, shape, radius, what))
            else:
                env = ref_fn(np.abs(x), np.abs(taps), shape)
                ratio, i = worst_ratio(got, ref, count * br.U32 * env)
                worst[mode] = max(worst[mode], ratio)
                print(f"{what}: worst ratio {ratio:.4f} at flat index {i}")
                fails.append(None if ratio <= 1.0 else f"{what}: ratio {ratio} at flat index {i}")
    for mode, w in worst.items():
        parity_record(f"blur_tile_{mode}_R{radius}_ratio", w, 1.0, shape=list(shape), batch=batch)
    fails = [f for f in fails if f]
    assert not fails, fails


@pytest.mark.parametrize("kernel,radius,shape", NEAR, ids=NEAR_IDS)
def test_near_consistent_residual(cuda, parity_record, kernel, radius, shape):
    """y = A x0 + 1e-3 randn at |x0| ~ 100: v per element within the derived bound of its envelope
    (not of its own size), rsq within what a per-element residual error of
    delta = (2K + 6) 2^-24 E_r allows: 2 sum |r| delta + sum delta^2, plus the summation's 2e-5."""
    batch, ydiv, tapname = 2, 1, "gauss"
    op, _ = make_op(shape, radius, tapname, cuda)
    desc = op.hip_descriptor()
    p = check_partials(desc, kernel, shape)
    x, eps, y, ref = dps_case(radius, shape, batch, ydiv, tapname, "near")
    assert np.abs(ref.r).max() < 1e-4 * np.abs(ref.x0).max()  # four orders below the operands
    v, part = run_residual(cuda, desc, p, x, eps, y, batch, ydiv, _coefs(*br.RANDOM_COEFS))
    v, rsq = v.cpu().numpy(), part.sum(1).cpu().numpy().astype(np.float64)
    ratio, i = worst_ratio(v, ref.v, br.rounding_count(radius) * br.U32 * ref.E_v)
    delta = (2 * (2 * radius + 1) + 6) * br.U32 * ref.E_r
    bound = 2 * (np.abs(ref.r) * delta).sum(1) + (delta * delta).sum(1) + RSQ_RTOL * ref.rsq
    rratio = float((np.abs(rsq - ref.rsq) / bound).max())
    print(f"{kernel} near R{radius} {sid(shape)}: v ratio {ratio:.4f} at {i}, rsq ratio {rratio:.4f}, "
          f"rsq rel err {np.abs(rsq / ref.rsq - 1).max():.3e}")
    parity_record(f"blur_{kernel}_near_R{radius}_ratio", ratio, 1.0, shape=list(shape))
    parity_record(f"blur_{kernel}_near_R{radius}_rsq_ratio", rratio, 1.0, shape=list(shape))
    assert ratio <= 1.0, (ratio, i)
    assert rratio <= 1.0, (rsq, ref.rsq, bound)


@pytest.mark.parametrize("kernel,radius,shape,batch,ydiv", [("reg", 4, (2, 128, 256), 3, 3), ("dma", 1, (1, 32, 256), 3, 3)],
                         ids=["reg-R4-2x128x256", "dma-R1-1x32x256"])
def test_update_reads_the_streaming_partial_layout(cuda, parity_record, kernel, radius, shape, batch, ydiv):
    """sp_dps_update after a streaming residual pass, with that pass's own v and its C H / 32
    partials per sample, against the closed form fed the fp64 v and rsq."""
    tapname = "gauss"
    op, _ = make_op(shape, radius, tapname, cuda)
    desc = op.hip_descriptor()
    p = check_partials(desc, kernel, shape)
    x, eps, y, ref = dps_case(radius, shape, batch, ydiv, tapname, "plain")
    a, k, gs = br.RANDOM_COEFS
    coefs = _coefs(a, k, gs)
    v, part = run_residual(cuda, desc, p, x, eps, y, batch, ydiv, coefs)
    g = np.random.default_rng(radius)
    w, xi = (g.standard_normal(x.shape).astype(np.float32) for _ in range(2))
    xd, ed, yd, wd, xid = (_dev(t, cuda) for t in (x, eps, y, w, xi))
    out = ec.Guarded(tuple(x.shape), x.shape[1], cuda)
    _call("sp_dps_update", desc, xd.data_ptr(), ed.data_ptr(), yd.data_ptr(), v.data_ptr(), wd.data_ptr(),
          part.data_ptr(), xid.data_ptr(), 0, 0, 0, batch, ydiv, coefs, out.ptr())
    torch.cuda.synchronize()
    got = out.check().cpu().numpy()
    want = closed_form.update_pass(x, eps, ref.v, w, ref.rsq, xi, br.f32(a), br.f32(k), *UPD[:4])
    err = float(np.abs(got - want).max() / np.abs(want).max())
    parity_record(f"blur_{kernel}_update_R{radius}_max_err_over_max", err, 2e-5, shape=list(shape))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5 * np.abs(want).max())


@pytest.mark.parametrize("kernel,radius,shape,batch,ydiv", [("reg", 1, (1, 64, 256), 2, 1), ("tile", 7, (2, 35, 67), 2, 2)],
                         ids=["reg-R1-1x64x256", "tile-R7-2x35x67"])
def test_scheduled_entry_reads_the_cursor_record(cuda, kernel, radius, shape, batch, ydiv):
    """sp_dps_residual_sched with the cursor on record 1 of 2 has the bits of the by-value call with
    record 1's coefficients, and not those of record 0's."""
    op, _ = make_op(shape, radius, "asym", cuda)
    desc = op.hip_descriptor()
    p = check_partials(desc, kernel, shape)
    x, eps, y = br.random_inputs(radius, batch, ydiv, shape)
    records = [(0.7, 0.71, 50.0, 0.95, 0.1, 0.3, 0.03, 1e-9), (0.3, 0.95, 400.0, *UPD)]
    recs = (_hip.SpStepRec * 2)()
    for r, c in zip(recs, records):
        r.c = _hip.SpDpsCoefs(*c)
        r.step, r.t = 1, 1
    sched = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(cuda)
    cursor = torch.zeros(1, dtype=torch.int32, device=cuda)
    _call("sp_sched_advance", cursor.data_ptr())
    assert cursor.item() == 1
    got = run_residual(cuda, desc, p, x, eps, y, batch, ydiv, None, sched=sched, cursor=cursor)
    assert cursor.item() == 1  # the pass does not move it
    want = run_residual(cuda, desc, p, x, eps, y, batch, ydiv, _hip.SpDpsCoefs(*records[1]))
    other = run_residual(cuda, desc, p, x, eps, y, batch, ydiv, _hip.SpDpsCoefs(*records[0]))
    for name, g, r, o in zip(("v", "partials"), got, want, other):
        assert torch.equal(g, r), (name, float((g - r).abs().max()))
        assert not torch.equal(o, r), name
