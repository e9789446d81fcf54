"""Pins tests/chanmix_ref.py on the CPU: the two fp64 statements of every pass of the channel-mixing
kind agree, the standard identities hold, the prox and the DDRM step equal their dense definitions,
the kept sets and DDRM classes of the GPU cases are decided alike in fp32 and fp64, and on the
exact cases the fp32 emulation of every kernel pass returns the fp64 result bit for bit while every
listed mistake breaks it."""

import numpy as np
import pytest
import torch

import chanmix_ref as cr
import ddrm_ref as dr
import prox_ref as pr
from samplers_amd import _hip
from samplers_amd.operators import ChannelMixOperator
from samplers_amd.samplers.ddrm import ddrm_step_svd
from samplers_amd.samplers.utils.bridge_kernels import DDRMCoefficients

assert _hip.SP_OP_CHANNEL_MIX == 13

# shapes small enough for dense matrices: every matrix of the GPU cases on a few pixels
SMALL = [(cr.CASES[i][0], cr.CASES[i][1][:2] + hw, i) for i, hw in
         ((0, (1, 1)), (1, (2, 2)), (2, (3, 5)), (3, (3, 4)), (4, (4, 3)), (5, (2, 4)), (7, (2, 3)), (8, (4, 4)),
          (9, (3, 3)))]
SMALL_IDS = [s[0] for s in SMALL]
REGIMES = {"big": (3.0, 0.05, 0.85, 1.0), "blend": (0.5, 0.05, 0.5, 0.5), "small": (0.041, 0.05, 0.85, 1.0),
           "sig_y=0": (0.23, 0.0, 0.85, 1.0), "sig_prev=0": (0.0, 0.05, 0.85, 1.0)}


def _data(shape, batch=3, seed=0):
    c, cy, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x, eps, xi = (torch.randn(batch, c, h, w, generator=g, dtype=torch.float64) for _ in range(3))
    return x, eps, xi, torch.randn(batch, cy, h, w, generator=g, dtype=torch.float64)


def _both(name, shape, i):
    tab = cr.round32(cr.case(i)[2])
    return tab, cr.Mix(shape, tab), cr.Dense(shape, tab)


@pytest.mark.parametrize("name,shape,i", SMALL, ids=SMALL_IDS)
def test_the_two_statements_agree(name, shape, i):
    tab, mix, dense = _both(name, shape, i)
    x, eps, xi, y = _data(shape)
    flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
    c = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)
    pairs = [(mix.apply(x), dense.apply(flat(x))), (mix.adjoint(y), dense.adjoint(flat(y))),
             (mix.pinv(y), dense.pinv(flat(y))), (mix.pinv_t(x), dense.pinv_t(flat(x))),
             (mix.pgdm(x, eps, y, 0.8, 0.6, -2.0), dense.pgdm(flat(x), flat(eps), flat(y), 0.8, 0.6, -2.0)),
             (mix.prox(x, y, 0.37), dense.prox(flat(x), flat(y), 0.37)),
             (mix.diffpir(x, eps, y, xi, c), dense.diffpir(flat(x), flat(eps), flat(y), flat(xi), c))]
    v, rsq = mix.dps(x, eps, y, 0.8, 0.6, 400.0)
    vd, rsqd = dense.dps(flat(x), flat(eps), flat(y), 0.8, 0.6, 400.0)
    pairs += [(v / 400, vd / 400), (rsq, rsqd)]
    for reg in REGIMES.values():
        cc = dr.make_coefs(*reg)
        pairs.append((mix.ddrm(x, eps, y, xi, cc), dense.ddrm(flat(x), flat(eps), flat(y), flat(xi), cc)))
    for a, b in pairs:
        assert float((flat(a) - flat(b)).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name,shape,i", SMALL, ids=SMALL_IDS)
def test_identities(name, shape, i):
    _, _, tab64, _ = cr.case(i)
    t = {k: torch.as_tensor(v) for k, v in tab64.items() if k != "keep"}
    cy = shape[1]
    assert float((t["U"] @ torch.diag(t["S"]) @ t["V"][:, :cy].T - t["M"]).abs().max()) <= 1e-14
    assert float((t["U"].T @ t["U"] - torch.eye(cy)).abs().max()) <= 1e-14
    assert float((t["V"].T @ t["V"] - torch.eye(shape[0])).abs().max()) <= 1e-14
    mix = cr.Mix(shape, tab64)
    x, eps, xi, y = _data(shape)
    assert abs(float((mix.apply(x) * y).sum() - (x * mix.adjoint(y)).sum())) <= 1e-12
    assert abs(float((mix.pinv(y) * x).sum() - (y * mix.pinv_t(x)).sum())) <= 1e-12
    assert float((mix.pinv(mix.apply(mix.pinv(y))) - mix.pinv(y)).abs().max()) <= 1e-12
    proj = lambda v: mix.pinv(mix.apply(v))  # noqa: E731
    assert float((proj(proj(x)) - proj(x)).abs().max()) <= 1e-12
    assert abs(float((proj(x) * eps).sum() - (x * proj(eps)).sum())) <= 1e-12
    # the PGDM gradient: autograd of |A^+ y - A^+ A x0|^2, the chain rule, and -2 (A^+ y - A^+ A x0)
    x0 = x.clone().requires_grad_()
    (g,) = torch.autograd.grad((mix.pinv(y) - mix.pinv(mix.apply(x0))).square().sum(), x0)
    want = -2.0 * mix.pinv(y - mix.apply(x))
    assert float((g - want).abs().max()) <= 1e-11 and float((mix.pgdm_gradient(x, y) - want).abs().max()) <= 1e-11
    assert float((mix.pgdm(x, eps, y, 0.8, 0.6, -2.0) + 2.0 * mix.pinv(y - mix.apply((x - 0.6 * eps) / 0.8))).abs().max()) <= 1e-12


def test_mean_colorization_pinv_is_c_times_the_transpose():
    for c in (1, 3, 4, 8):
        tab = cr.svd_tables(np.full((1, c), 1.0 / c))
        assert float(np.abs(tab["N"] - c * tab["M"].T).max()) <= 1e-14


@pytest.mark.parametrize("name,shape,i", SMALL, ids=SMALL_IDS)
def test_prox_is_the_dense_solve(name, shape, i):
    tab64 = cr.case(i)[2]  # in fp64 M = U S V^T holds to the last bit or two, as the closed form needs
    mix, dense = cr.Mix(shape, tab64), cr.Dense(shape, tab64)
    x, _, _, y = _data(shape, seed=1)
    flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
    for rho in pr.RHOS:
        A = dense.A
        want = torch.linalg.solve(A.T @ A + rho * torch.eye(A.shape[1], dtype=torch.float64),
                                  (flat(y) @ A + rho * flat(x)).T).T
        assert float((flat(mix.prox(x, y, rho)) - want).abs().max()) <= 1e-10
        assert float((pr.dense_prox(A, flat(x), flat(y), rho) - want).abs().max()) <= 1e-10


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name,shape,i", SMALL, ids=SMALL_IDS)
def test_ddrm_is_the_dense_eigh_form_and_ddrm_step_svd(name, shape, i, regime):
    tab64, rtol = cr.case(i)[2], cr.case(i)[3]
    mix, dense = cr.Mix(shape, tab64), cr.Dense(shape, tab64)
    x, eps, xi, y = _data(shape, seed=2)
    flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
    c = dr.make_coefs(*REGIMES[regime])
    got = mix.ddrm(x, eps, y, xi, c)
    # the dense definition drops eigenvalues of A^T A below rtol^2 of the largest
    want = dr.dense_step(dense.A, flat(x), flat(eps), flat(y), flat(xi), c, rtol=max(rtol, 1e-6) ** 2)
    assert float((flat(got) - want).abs().max()) <= 1e-10


# matrices whose SVD factors are dyadic and whose singular values are distinct: the operator's own
# SVD returns them to 1e-16, so its fp32 tables are exact and ddrm_step_svd can be held to 1e-10
DYADIC_OPS = {"4x4": (np.diag([2.0, 1.0, 0.5, 0.25]), 1e-6), "2x4": (np.diag([2.0, 0.5])[:, :2], 1e-6),
              "2x4-rtol": (np.diag([2.0, 2.0 ** -12]), 1e-2)}


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("which", list(DYADIC_OPS))
def test_ddrm_step_svd_on_the_operator_is_the_dense_eigh_form(which, regime):
    d, rtol = DYADIC_OPS[which]
    cy = d.shape[0]
    u = cr.PERM if cy == 4 else np.array([[0.0, 1.0], [-1.0, 0.0]])  # a signed permutation
    m = u @ d @ cr.H4[:, :cy].T
    shape = (4, cy, 2, 3)
    op = ChannelMixOperator((4, 2, 3), m, rtol=rtol)
    assert int(op.keep.sum()) == (1 if "rtol" in which else cy)
    x, eps, xi, y = _data(shape, seed=3)
    flat = lambda t: t.reshape(t.shape[0], -1)  # noqa: E731
    c = dr.make_coefs(*REGIMES[regime])
    A = cr.Dense(shape, cr.svd_tables(m, rtol)).A
    want = dr.dense_step(A, flat(x), flat(eps), flat(y), flat(xi), c, rtol=rtol ** 2)
    step = ddrm_step_svd(op, x, eps, y, xi, DDRMCoefficients(**c))
    assert float((flat(step) - want).abs().max()) <= 1e-10


@pytest.mark.parametrize("i", range(len(cr.CASES)), ids=[c[0] for c in cr.CASES])
def test_kept_sets_and_classes_of_the_gpu_cases_are_decided_alike(i):
    name, shape, tab, rtol = cr.case(i)
    t32 = cr.round32(tab)
    s, thr = tab["S"], rtol * tab["S"].max()
    for sv, kept in zip(s, tab["keep"]):
        assert (sv >= 10 * thr) if kept else (sv == 0 or sv <= thr / 10), (name, sv, thr)
    assert np.array_equal(t32["P"] != 0, tab["keep"])
    assert np.array_equal(t32["S"] > np.float32(rtol) * t32["S"].max(), tab["keep"])
    for reg in REGIMES.values():
        c = dr.make_coefs(*reg)
        if c["sig_y"] > 0:
            for sv in s[tab["keep"]]:
                assert abs(c["sig_prev"] ** 2 * sv ** 2 / c["sig_y"] ** 2 - 1.0) > 1e-5, (name, reg, sv)
        big32 = cr.big_mask32(t32, dr.round32(c))
        big64 = dr.big_mask64(torch.as_tensor(s * s), c)
        assert torch.equal(big32[torch.as_tensor(tab["keep"])], big64[torch.as_tensor(tab["keep"])])


# --- exact cases ------------------------------------------------------------------------------------
def _exact_runs(shape, tab, batch=4, ydiv=2, regime="big", emu_tab=None, stride=None):
    x, eps, xi, y = cr.exact_data(shape, batch, ydiv)
    ye = cr.expand(y, batch, ydiv)
    ref = cr.run_passes(cr.Mix(shape, tab), x.double(), eps.double(), ye.double(), xi.double(), regime)
    f = lambda t: t.reshape(batch, -1).numpy()  # noqa: E731
    emu = cr.run_passes(cr.Emu(shape, emu_tab or tab, stride), f(x), f(eps), f(ye), f(xi), regime)
    return {k: np.array_equal(emu[k].astype(np.float64), ref[k].reshape(batch, -1).numpy()) for k in ref}


@pytest.mark.parametrize("regime", ["big", "small"])
@pytest.mark.parametrize("name,shape,tab,passes", cr.EXACT_CASES, ids=[c[0] for c in cr.EXACT_CASES])
def test_exact_cases_emulate_bit_for_bit(name, shape, tab, passes, regime):
    t32 = cr.round32(tab)
    if name != "dyadic-colorization":  # dyadic tables: fp32 holds them exactly
        assert all(np.array_equal(t32[k].astype(np.float64), tab[k]) for k in "MNUVSP")
    for batch, ydiv in cr.FORMS:
        same = _exact_runs(shape, t32, batch, ydiv, regime)
        assert all(same[k] for k in passes), same


def _broken(tab, how):
    t = {k: np.array(v) for k, v in tab.items()}
    if how == "M transposed":
        t["M"] = t["M"].T.copy()
    elif how == "N without P":
        t["N"] = t["V"] @ t["U"].T
    elif how == "U and V swapped":
        t["U"], t["V"] = t["V"], t["U"]
    elif how == "S in place of P":
        t["P"] = t["S"].copy()
    elif how == "kept mask shifted":
        t["P"] = np.roll(t["P"], 1)
    return t


@pytest.mark.parametrize("how,passes", [("M transposed", ("apply", "adjoint", "dps")),
                                        ("N without P", ("pinv", "pinv_t", "pgdm")),
                                        ("U and V swapped", ("prox", "diffpir", "ddrm")),
                                        ("S in place of P", ("ddrm",)),
                                        ("kept mask shifted", ("ddrm",)),
                                        ("plane stride", cr.ALL_PASSES)])
def test_every_mistake_breaks_the_exact_cases(how, passes):
    name, shape, tab, _ = cr.EXACT_CASES[1]  # the Hadamard tables with a dropped component
    t32 = cr.round32(tab)
    if how == "plane stride":
        same = _exact_runs(shape, t32, stride=shape[2] * shape[3] - 1)
    else:
        same = _exact_runs(shape, t32, emu_tab=cr.round32(_broken(tab, how)))
    assert not any(same[k] for k in passes), (how, same)
