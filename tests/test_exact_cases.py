"""The condition the bit-exact GPU tests (test_conv_exact_gpu.py, test_gemm_x6_exact_gpu.py) rely on,
checked on the CPU for every case tests/exact_cases.py generates: the fp64 reference is an fp32 number,
each fp32 emulation of a kernel's algorithm (direct accumulation over (ci, tap) forward and reversed,
the F(2x2,3x3) Winograd algebra, the bf16x6 split with its six kept products) returns it bit for bit,
and the sum of absolute values of everything added stays below 2^24 quanta, so that no order of
summation, split-K or atomics included, can round.  The reference alone therefore stays inside
"bitwise"; a GPU mismatch is the kernel's."""

import pytest
import torch

import exact_cases as ec

S1_FAMILIES = {"wino_w32": ec.WINO_W32, "wino_w16": ec.WINO_W16, "wino_mosaic": ec.WINO_MOSAIC,
               "wino_split": ec.WINO_SPLIT, "direct": ec.DIRECT, "thin": ec.THIN}
CONV_CASES = [(fam, "s1", s) for fam, shapes in S1_FAMILIES.items() for s in shapes] + \
             [("wino_up", "up", s) for s in ec.WINO_UP] + \
             [("s2", "s2", s) for s in ec.S2_FWD + ec.S2_VJP]


def _f32(t):
    return torch.equal(t.float().double(), t)


def _same(emu, ref64):
    return emu.dtype == torch.float32 and torch.equal(emu.double(), ref64)


@pytest.mark.parametrize("fam,kind,shape", CONV_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_integer_conv_cases_are_exact_in_fp32(fam, kind, shape):
    n, cin, cout, h, w = shape
    wino = fam.startswith("wino")
    shapes = [shape] if kind != "s1" or fam == "thin" else [shape, ec.swapped(shape)]  # (the VJP's layer)
    for sh in shapes:
        c = ec.int_conv_case(sh, kind=kind)
        r = ec.int_bound(max(sh[1], sh[2]))
        assert 9 * max(sh[1], sh[2]) * r * r * 4 < 2 ** 24
        assert all(float(t.abs().max()) <= r and torch.equal(t, t.round()) for t in (c.x, c.w, c.bias, c.res, c.dy))
        assert _f32(c.y64) and _f32(c.dx64)
        for rev in (False, True):
            assert _same(ec.emu_forward(c, ec.emu_direct, reverse=rev), c.y64)
            assert _same(ec.emu_vjp(c, ec.emu_direct, reverse=rev), c.dx64)
        # every order of summation: the direct envelope (the Winograd one, in quarters) below 2^24
        assert float(ec.emu_forward(c, ec.emu_direct, dtype=torch.float64, absolute=True).max()) < 2 ** 24
        assert float(ec.emu_vjp(c, ec.emu_direct, dtype=torch.float64, absolute=True).max()) < 2 ** 24
        if wino:
            assert _same(ec.emu_forward(c, ec.emu_wino), c.y64)
            assert _same(ec.emu_vjp(c, ec.emu_wino), c.dx64)
            env = ec.emu_forward(c, ec.emu_wino, dtype=torch.float64, absolute=True)
            venv = ec.emu_vjp(c, ec.emu_wino, dtype=torch.float64, absolute=True)
            assert 4 * float(env.max()) < 2 ** 24 and 4 * float(venv.max()) < 2 ** 24
            assert bool((env >= c.y64.abs()).all())


@pytest.mark.parametrize("kind,shape", ec.IMPULSE, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_impulse_fields_leave_most_outputs_exactly_zero(kind, shape):
    c = ec.impulse_conv_case(shape, kind=kind)
    assert set(c.x.unique().tolist()) == {0.0, 1.0} and not c.bias.any() and not c.res.any()
    zero = c.y64 == 0
    assert float(zero.double().mean()) >= 0.5 and int((~zero).sum()) >= 8
    assert _f32(c.y64) and _f32(c.dx64)
    assert _same(ec.emu_forward(c, ec.emu_direct), c.y64)
    if c.x.shape[2] % 2 == 0 and c.x.shape[3] % 2 == 0:
        assert _same(ec.emu_forward(c, ec.emu_wino), c.y64)
        assert _same(ec.emu_vjp(c, ec.emu_wino), c.dx64)


def test_wino_envelope_dominates_the_direct_one():
    """The Winograd envelope counts the algebra's cross terms: never below the direct envelope, and
    several times it on real data (which is why rho of a Winograd tile is taken against its own)."""
    c = ec.real_conv_case((1, 16, 64, 8, 32), "randn")
    ew = ec.emu_forward(c, ec.emu_wino, dtype=torch.float64, absolute=True)
    ed = ec.emu_forward(c, ec.emu_direct, dtype=torch.float64, absolute=True)
    assert bool((ew >= ed * (1 - 1e-12)).all()) and 2 < float((ew / ed).max()) < 20
    y = ec.emu_forward(c, ec.emu_wino)
    assert ec.rho(y, c.y64, ew) < 2 and ec.rel_l2(y, c.y64) < 1e-6


GEMM_CASES = [(cls, m, k, cols) for cls in ec.GEMM_CLASSES for k in ec.GEMM_K for m, cols in ((128, 256), (32, 256))] + \
             [(cls, 256, 768, 256) for cls in ec.GEMM_CLASSES] + [(cls, 160, 512, 512) for cls in ec.GEMM_CLASSES]
LIVE = {"a": ("x", 1, 0.5), "b": ("w", 1, 0.5), "c": ("x", 2, 0.5), "d": ("both", 1, 0.3)}


@pytest.mark.parametrize("cls,m,k,cols", GEMM_CASES)
def test_dyadic_gemm_cases_are_exact_under_the_x6_split(cls, m, k, cols):
    """Per class: the three terms sum to the operand, every product the kernel drops is zero, the
    term the class is about is non-zero for the stated share of the non-zero elements (a, b: the
    second term of the wide operand for >= 50 %; c: the third term of x for >= 50 %; d: the second
    term of both for >= 30 %), and sum |w||x| + |bias| + |res| < 2^24 quanta."""
    c = ec.dyadic_gemm_case(cls, m, k, cols)
    wt, xt = ec.g6_split(c.W), ec.g6_split(c.X)
    for t, v in ((wt, c.W), (xt, c.X)):
        assert torch.equal(t[0].double() + t[1].double() + t[2].double(), v.double())
    for tu, tv in ((1, 2), (2, 1), (2, 2)):  # the dropped products
        assert not bool((wt[tu].double().abs() @ xt[tv].double().abs()).any())
    which, term, share = LIVE[cls]
    for name, t, v in (("w", wt, c.W), ("x", xt, c.X)):
        if which in (name, "both"):
            assert float((t[term][v != 0] != 0).float().mean()) >= share
    units = c.env / c.quantum
    assert float(units.max()) < 2 ** 24 and torch.equal(units, units.round())
    assert _f32(c.y64)
    assert _same(ec.emu_x6(c.W, c.X, c.bias.float(), c.res.float()), c.y64)
    assert _same(ec.emu_x6(c.W, c.X), c.y64 - c.bias.double().view(-1, 1) - c.res.double())


@pytest.mark.parametrize("cls", ec.GEMM_CLASSES)
def test_every_k_step_of_a_dyadic_case_shows(cls):
    """A k-step skipped or run twice changes some output of every class (the sparse rows of c and d
    included): each 16-column block of W meets non-zero x in some row."""
    c = ec.dyadic_gemm_case(cls, 32, 208, 256)
    for s in range(0, 208, 16):
        part = c.W[:, s:s + 16].double() @ c.X[s:s + 16].double()
        assert bool((part != 0).any())


def test_every_input_channel_of_an_integer_case_shows():
    """Likewise for the convolutions: dropping any one input channel changes some output."""
    import torch.nn.functional as F

    c = ec.int_conv_case((1, 40, 64, 16, 96))
    for ci in range(40):
        assert bool(F.conv2d(c.x[:, ci:ci + 1].double(), c.w[:, ci:ci + 1].double(), padding=1).ne(0).any())


@pytest.mark.parametrize("split,shape", [(s, sh) for s in (False, True)
                                         for sh in ec.WINO_EMU_L2["split" if s else "raw"] if sh[0] * sh[1] * sh[2] <= 2 ** 16])
def test_recorded_emulation_errors_are_the_emulations(split, shape):
    """WINO_EMU_L2 (the yardstick of tests/test_conv_gpu.py's raw Winograd tests) is what emu_wino gives on
    those tests' operands, to the table's three digits; the small shapes are recomputed here."""
    import torch.nn.functional as F

    x, w, b, res, dy = ec.raw_wino_operands(shape, split)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + (0 if res is None else res.double())
    gref = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), padding=1)
    ef = ec.rel_l2(ec.emu_wino(x, w, b, res), ref)
    ev = ec.rel_l2(ec.emu_wino(dy, w.transpose(0, 1).flip(2, 3).contiguous()), gref)
    tf, tv = ec.WINO_EMU_L2["split" if split else "raw"][shape]
    assert abs(ef / tf - 1) < 0.01 and abs(ev / tv - 1) < 0.01, (ef, tf, ev, tv)


def test_g6_split_emulation_on_real_values():
    """On randn the split is exact and the six kept products give an fp32-class result."""
    c = ec.real_gemm_case("randn", 128, 208, 256)
    t = ec.g6_split(c.X)
    assert torch.equal(t[0].double() + t[1].double() + t[2].double(), c.X.double())
    assert all(bool(((p.view(torch.int32) & 0xFFFF) == 0).all()) for p in t)
    y = ec.emu_x6(c.W, c.X, c.bias, c.res)
    assert ec.rho(y, c.y64, c.env) < 4 and ec.rel_l2(y, c.y64) < 2e-7
