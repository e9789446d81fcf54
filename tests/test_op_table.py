"""The library's per-kind dispatch on the host: partial and workspace counts, the return codes
every entry point gives before any launch, the trait bits and each kind's geometry rules.

No GPU: the library loads without one, and every call here returns before a launch.  The counts
are literals recorded from the library as it was before the kinds got one dispatch table; each
carries the formula it follows."""

import ctypes

import pytest

from kind_harness import make_descriptor as make
from samplers_amd import _hip

OK, EINVAL, EUNSUPPORTED = 0, -1, -3

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)  # a non-null dummy pointer: nothing here dereferences it


def identity(n=12, m=None):
    return make(_hip.SP_OP_IDENTITY, n, n if m is None else m)


def inpaint(n=128, m=64):
    return make(_hip.SP_OP_INPAINT, n, m, keep=PTR, rank=PTR)


def mask(n=128):
    return make(_hip.SP_OP_MASK, n, n, keep=PTR)


def blur(c=1, h=8, w=8, r=1):
    return make(_hip.SP_OP_BLUR, c * h * w, c * h * w, c, h, w, radius=r, taps=PTR)


def sr(c=1, h=8, w=8, s=2):
    return make(_hip.SP_OP_SR, c * h * w, c * h * w // (s * s), c, h, w, factor=s)


def psf(c=1, h=8, w=8, r=1):
    return make(_hip.SP_OP_PSF, c * h * w, c * h * w, c, h, w, radius=r, taps=PTR)


def phase(c=1, h=8, w=8, pad=(0, 0)):
    return make(_hip.SP_OP_PHASE, c * h * w, c * (h + 2 * pad[0]) * (w + 2 * pad[1]), c, h, w,
                radius=pad[0], factor=pad[1])


SMALL = {"identity": identity, "inpaint": inpaint, "mask": mask, "blur": blur, "sr": sr, "psf": psf,
         "phase": phase}
LINEAR = ("identity", "inpaint", "mask", "blur", "sr", "psf")

# descriptor -> (sp_rsq_partials, sp_dps_workspace(., 3), sp_op_workspace(., 3))
COUNTS = [
    (identity(), (1, 0, 0)),                  # ceil(n / 2048): 2 float4 groups x 256 threads per tile
    (inpaint(), (1, 0, 0)),                   # ceil(n / 2048)
    (mask(), (1, 0, 0)),                      # ceil(n / 2048)
    (identity(5000), (3, 0, 0)),              # ceil(5000 / 2048)
    (identity(5001), (10, 0, 0)),             # n % 4 != 0, scalar tiles: ceil(5001 / 512)
    (blur(), (1, 0, 0)),                      # C * ceil(H / 32) * ceil(W / 64)
    (blur(3, 40, 72), (12, 0, 0)),            # 3 * 2 * 2
    (blur(1, 64, 256, 2), (2, 0, 0)),         # streamed pass (W = 256, R <= 4): C * H / 32
    (sr(), (1, 0, 0)),                        # ceil((n / (4 s)) patches / 512 per tile), s = 2
    (sr(3, 32, 32, 2), (1, 0, 0)),            # ceil(384 / 512)
    (sr(3, 32, 32, 8), (1, 0, 0)),            # ceil((n / (4 s)) = 96 patches / 256 per tile), s = 8
    (sr(3, 64, 64, 2), (3, 0, 0)),            # ceil(1536 / 512)
    (sr(1, 6, 6, 2), (1, 0, 0)),              # W % 4 != 0: ceil((n / (2 s)) = 9 patches / 256)
    (psf(), (1, 3 * 64, 0)),                  # C * ceil(H / 32) * ceil(W / 64); workspace batch * m
    (psf(3, 40, 72), (12, 3 * 8640, 0)),      # 3 * 2 * 2; 3 * m
    (phase(), (1, 384, 384)),                 # C * ceil(Nw / 16 lines); 2 * batch * C * Nw * H
    (phase(2, 24, 48, (4, 8)), (8, 18432, 18432)),  # 2 * ceil(64 / 16); 2 * 3 * 2 * 64 * 24
]


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_partial_and_workspace_counts(lib, i):
    d, (partials, dps_ws, op_ws) = COUNTS[i]
    assert lib.sp_rsq_partials(d) == partials
    assert lib.sp_dps_workspace(d, 3) == dps_ws
    assert lib.sp_op_workspace(d, 3) == op_ws
    assert lib.sp_dps_workspace(d, 0) == EINVAL and lib.sp_op_workspace(d, 0) == EINVAL


def entry_calls(lib, d, *, v=PTR, work=PTR, ata_u=PTR):
    """Every entry point that takes an sp_op, on non-null dummy arguments."""
    c, a = _hip.SpDpsCoefs(), _hip.SpAdamWCoefs()
    return {
        "sp_rsq_partials": lambda: lib.sp_rsq_partials(d),
        "sp_dps_workspace": lambda: lib.sp_dps_workspace(d, 3),
        "sp_op_workspace": lambda: lib.sp_op_workspace(d, 3),
        "sp_dps_residual": lambda: lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR, None),
        "sp_dps_residual_ws": lambda: lib.sp_dps_residual_ws(d, PTR, PTR, PTR, 3, 1, c, PTR, PTR,
                                                            work, None),
        "sp_dps_residual_sched": lambda: lib.sp_dps_residual_sched(d, PTR, PTR, PTR, 3, 1, PTR, PTR,
                                                                  PTR, PTR, None),
        "sp_dps_residual_sched_ws": lambda: lib.sp_dps_residual_sched_ws(d, PTR, PTR, PTR, 3, 1, PTR,
                                                                        PTR, PTR, PTR, work, None),
        "sp_dps_update": lambda: lib.sp_dps_update(d, PTR, PTR, PTR, v, PTR, PTR, None, 0, 0, 0, 3,
                                                  1, c, PTR, None),
        "sp_dps_update_sched": lambda: lib.sp_dps_update_sched(d, PTR, PTR, PTR, v, PTR, PTR, 0, 0,
                                                              3, 1, PTR, PTR, PTR, None),
        "sp_op_apply": lambda: lib.sp_op_apply(d, PTR, PTR, 3, None),
        "sp_op_adjoint": lambda: lib.sp_op_adjoint(d, PTR, PTR, 3, None),
        "sp_op_apply_ws": lambda: lib.sp_op_apply_ws(d, PTR, PTR, 3, work, None),
        "sp_op_vjp_ws": lambda: lib.sp_op_vjp_ws(d, PTR, PTR, PTR, 3, work, None),
        "sp_psld_pixel": lambda: lib.sp_psld_pixel(d, PTR, PTR, 3, 1, PTR, PTR, PTR, None),
        "sp_psld_cotangent": lambda: lib.sp_psld_cotangent(d, PTR, PTR, ata_u, PTR, 0.1, 3, PTR,
                                                          None),
        "sp_pixel_opt_step": lambda: lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 3, 1, 1.0, a,
                                                          None, PTR, None),
    }


GEOMETRY_VIOLATIONS = {
    "unknown kind": make(7, 64, 64, 1, 8, 8),
    "blur R = 9": blur(1, 32, 32, 9),
    "sr factor 3": sr(1, 9, 9, 3),
    "psf H = 2R": psf(1, 8, 16, 4),
    "phase padded size 20": phase(1, 16, 16, (2, 0)),
    "inpaint m > n": inpaint(128, 129),
    "identity m != n": identity(12, 8),
}


@pytest.mark.parametrize("what", list(GEOMETRY_VIOLATIONS) + ["null op"])
def test_rejected_descriptor_is_einval_everywhere(lib, what):
    d = GEOMETRY_VIOLATIONS.get(what)  # None: a null op
    for name, call in entry_calls(lib, d).items():
        assert call() == EINVAL, name


def test_more_descriptor_rules(lib):
    """One further violation per rule of the kinds' geometry checks."""
    bad = [blur(1, 8, 8, 0), blur(1, 2, 8, 1), make(_hip.SP_OP_BLUR, 64, 64, 1, 8, 8, radius=1),
           make(_hip.SP_OP_BLUR, 64, 64, 1, 8, 9, radius=1, taps=PTR),
           make(_hip.SP_OP_SR, 64, 15, 1, 8, 8, factor=2), sr(1, 8, 12, 8), sr(0, 8, 8, 2),
           psf(1, 64, 64, 31), psf(1, 8, 8, 0), make(_hip.SP_OP_PSF, 64, 64, 1, 8, 8, radius=1),
           phase(1, 8, 8, (-1, 0)), phase(1, 2048, 8), phase(1, 4, 8),
           make(_hip.SP_OP_PHASE, 64, 64, 1, 8, 8, taps=PTR),
           make(_hip.SP_OP_PHASE, 64, 65, 1, 8, 8),
           make(_hip.SP_OP_INPAINT, 128, 64, keep=PTR), make(_hip.SP_OP_MASK, 128, 128),
           make(_hip.SP_OP_MASK, 128, 64, keep=PTR), identity(0), make(-1, 12, 12)]
    for d in bad:
        assert lib.sp_rsq_partials(d) == EINVAL, (d.kind, d.n, d.m, d.height, d.width, d.radius)
    ok = [psf(1, 64, 64, 30), blur(1, 32, 32, 8), phase(1, 8, 24), phase(1, 1024, 8), sr(1, 8, 16, 8)]
    for d in ok:
        assert lib.sp_rsq_partials(d) > 0, (d.kind, d.height, d.width, d.radius)


@pytest.mark.parametrize("name", ["psf", "phase"])
def test_workspace_kinds_run_in_the_ws_forms_only(lib, name):
    calls = entry_calls(lib, SMALL[name](), work=None)
    assert calls["sp_dps_residual"]() == EUNSUPPORTED
    assert calls["sp_dps_residual_sched"]() == EUNSUPPORTED
    assert calls["sp_dps_residual_ws"]() == EINVAL       # work == NULL
    assert calls["sp_dps_residual_sched_ws"]() == EINVAL


@pytest.mark.parametrize("name", ["blur", "sr", "psf", "phase"])
def test_update_needs_v(lib, name):
    calls = entry_calls(lib, SMALL[name](), v=None)
    assert calls["sp_dps_update"]() == EINVAL
    assert calls["sp_dps_update_sched"]() == EINVAL


def test_update_needs_v_or_y(lib):
    c = _hip.SpDpsCoefs()
    for name in ("identity", "inpaint", "mask"):
        assert lib.sp_dps_update(SMALL[name](), PTR, PTR, None, None, PTR, PTR, None, 0, 0, 0, 3, 1, c,
                                 PTR, None) == EINVAL, name


def test_phase_has_no_linear_maps(lib):
    calls = entry_calls(lib, phase())
    for name in ("sp_op_apply", "sp_op_adjoint", "sp_psld_pixel", "sp_psld_cotangent",
                 "sp_pixel_opt_step"):
        assert calls[name]() == EUNSUPPORTED, name
    calls = entry_calls(lib, phase(), work=None)
    assert calls["sp_op_apply_ws"]() == EINVAL and calls["sp_op_vjp_ws"]() == EINVAL  # work == NULL


@pytest.mark.parametrize("name", LINEAR)
def test_linear_kinds_ws_forms(lib, name):
    d = SMALL[name]()
    assert entry_calls(lib, d)["sp_op_vjp_ws"]() == EUNSUPPORTED
    assert entry_calls(lib, d, work=None)["sp_op_vjp_ws"]() == EUNSUPPORTED
    # sp_op_apply_ws forwards to sp_op_apply, whose argument checks answer (work is not looked at)
    for work in (PTR, None):
        assert lib.sp_op_apply_ws(d, None, PTR, 3, work, None) == EINVAL
        assert lib.sp_op_apply_ws(d, PTR, PTR, 65536, work, None) == EINVAL
        assert lib.sp_op_apply_ws(d, PTR, PTR, 0, work, None) == EINVAL


@pytest.mark.parametrize("name", ["blur", "psf"])
def test_halo_kinds_have_no_fused_latent_pass(lib, name):
    calls = entry_calls(lib, SMALL[name](), ata_u=None)
    assert calls["sp_psld_pixel"]() == EUNSUPPORTED
    assert calls["sp_pixel_opt_step"]() == EUNSUPPORTED
    assert calls["sp_psld_cotangent"]() == EINVAL  # ata_u == NULL


def test_null_arguments_come_before_unsupported(lib):
    """The common argument checks answer first: a null buffer is SP_EINVAL on a kind the entry
    does not support."""
    a = _hip.SpAdamWCoefs()
    for d in (blur(), psf(), phase()):
        assert lib.sp_psld_pixel(d, None, PTR, 3, 1, PTR, PTR, PTR, None) == EINVAL
        assert lib.sp_pixel_opt_step(d, PTR, PTR, PTR, PTR, 0, 1, 1.0, a, None, PTR, None) == EINVAL
    assert lib.sp_psld_cotangent(phase(), PTR, None, PTR, PTR, 0.1, 3, PTR, None) == EINVAL
    assert lib.sp_op_apply(phase(), None, PTR, 3, None) == EINVAL
    assert lib.sp_op_adjoint(phase(), PTR, PTR, 0, None) == EINVAL
    c = _hip.SpDpsCoefs()
    for d in (psf(), phase()):
        assert lib.sp_dps_residual(d, None, PTR, PTR, 3, 1, c, PTR, PTR, None) == EINVAL
        assert lib.sp_dps_residual(d, PTR, PTR, PTR, 3, 1, None, PTR, PTR, None) == EINVAL


TRAITS = {  # UPDATE_READS_V, DPS_WORKSPACE, FUSED_LATENT, LINEAR, NEEDS_ATA_U
    "identity": (0, 0, 1, 1, 0), "inpaint": (0, 0, 1, 1, 0), "mask": (0, 0, 1, 1, 0),
    "blur": (1, 0, 0, 1, 1), "sr": (1, 0, 1, 1, 0), "psf": (1, 1, 0, 1, 1),
    "phase": (1, 1, 0, 0, 0),
}


@pytest.mark.parametrize("name", list(TRAITS))
def test_traits(lib, name):
    bits = (_hip.SP_TRAIT_UPDATE_READS_V, _hip.SP_TRAIT_DPS_WORKSPACE, _hip.SP_TRAIT_FUSED_LATENT,
            _hip.SP_TRAIT_LINEAR, _hip.SP_TRAIT_NEEDS_ATA_U)
    assert len(set(bits)) == 5 and all(b and b & (b - 1) == 0 for b in bits)
    t = lib.sp_op_traits(SMALL[name]())
    assert tuple(int(bool(t & b)) for b in bits) == TRAITS[name]
    assert t & ~sum(bits) == 0


def test_traits_of_a_rejected_descriptor_are_zero(lib):
    for d in GEOMETRY_VIOLATIONS.values():
        assert lib.sp_op_traits(d) == 0
    assert lib.sp_op_traits(None) == 0
