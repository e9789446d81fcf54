"""The separable-SVD kind's semantics on the CPU (tests/svd_sep_ref.py): the factorisation against
A_H ⊗ A_W, the convenience constructors against the host maps they restate, the algebra of A, Aᵀ,
A⁺ and the prox, the DDRM step against the dense eigh form and ``ddrm_step_svd``, the kept shares of
the GPU cases, and the exact cases: the fp32 evaluation returns the fp64 result bit for bit in both
side orders and both summation orders, and four wrong answers do not."""

import itertools

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import svd_sep_ref as sr
from samplers_amd.operators import SeparableSVDOperator
from samplers_amd.operators.blur import blur_reflect_torch, gaussian_taps
from samplers_amd.operators.sr_filter import bicubic_taps, gaussian_filter_taps, sr_filter_torch
from samplers_amd.operators.svd_separable import reflect_blur_matrix, symmetric_decimate_matrix
from samplers_amd.samplers.ddrm import ddrm_step_svd
from samplers_amd.samplers.utils.bridge_kernels import DDRMCoefficients

SMALL = [c for c in sr.FACTOR_CASES if "256" not in c[0] and "129" not in c[0]]
DENSE = [c for c in SMALL if c[0] in ("1x3x5", "1x12x10-zero", "1x24x16-sr2x4")] + [
    ("1x9x11-g5", 1, lambda: (sr.reflect_matrix(sr._gauss(5, 1.2), 9), sr.reflect_matrix(sr._gauss(5, 1.2), 11)),
     3e-2, (0.1, 0.9))]
ids = lambda cases: [c[0] for c in cases]  # noqa: E731


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("case", sr.FACTOR_CASES, ids=ids(sr.FACTOR_CASES))
def test_kept_share_of_the_gpu_cases(case):
    name, _, make, rtol, (lo, hi) = case
    t = sr.Tables.from_factors(*make(), rtol)
    share = t.kept_share()
    print(f"{name}: kept {share:.3f} at rtol {rtol}")
    assert lo <= share <= hi
    if name.endswith("zero"):
        assert t.S.min() <= 1e-15 * t.S.max()


@pytest.mark.parametrize("case", SMALL, ids=ids(SMALL))
def test_factorisation_is_the_kronecker_matrix(case):
    name, _, make, rtol, _ = case
    ah, aw = make()
    A = sr.kron_dense(ah, aw)
    t = sr.Tables.from_factors(ah, aw, rtol)
    for m in (t.VH, t.VW, t.UH, t.UW):
        assert np.abs(m.T @ m - np.eye(m.shape[0])).max() <= 1e-12
    assert np.abs(sr.Dense(t).A - A).max() <= 1e-12 * np.abs(A).max()
    # the operator's own fp64 factors and its rounded fp32 tables
    op = SeparableSVDOperator((1, ah.shape[1], aw.shape[1]), ah, aw, rtol=rtol)
    H, W, Hy, Wy = t.dims
    t32 = sr.Tables.from_flat(op.tables, H, W, Hy, Wy)
    own = np.abs(sr.kron_dense(ah.astype(np.float32), aw.astype(np.float32)) - A).max()
    err = np.abs(sr.Dense(t32).A - A).max()
    print(f"{name}: fp32 tables {err:.3g}, fp32-rounded A itself {own:.3g}")
    assert err <= 4 * max(own, np.finfo(np.float32).eps * np.abs(A).max())
    # the sign rule: the largest-magnitude entry of every V column is positive (a tie in fp32 may
    # have been decided in fp64)
    for v in (t32.VH, t32.VW):
        assert (v.max(0) >= -v.min(0) - 1e-6).all()
    assert np.array_equal(op.keep.numpy(), t32.P != 0)
    assert torch.equal(op.get_singular_values(), torch.where(op.keep, op.singular_values_full, torch.zeros(())))


def test_constructors_restate_the_host_maps():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 2, 24, 20, generator=g, dtype=torch.float64)
    flat = x.reshape(4, -1).numpy()
    taps = gaussian_taps(9, 3.0)
    A = sr.kron_dense(reflect_blur_matrix(taps, 24), reflect_blur_matrix(taps, 20))
    assert _rel(flat @ A.T, blur_reflect_torch(x, taps).reshape(4, -1).numpy()) <= 1e-12
    assert np.array_equal(reflect_blur_matrix(taps, 24), sr.reflect_matrix(taps.double().numpy(), 24))
    for t, s in ((bicubic_taps(4), 4), (bicubic_taps(2), 2), (gaussian_filter_taps(10, 1.5), 4)):
        A = sr.kron_dense(symmetric_decimate_matrix(t, 24, s), symmetric_decimate_matrix(t, 20, s))
        assert _rel(flat @ A.T, sr_filter_torch(x, t, s).reshape(4, -1).numpy()) <= 1e-12
        assert np.array_equal(symmetric_decimate_matrix(t, 24, s), sr.fold_matrix(t.double().numpy(), 24, s))
    # the operators' host maps in fp64, to the rounding of their fp32 tables
    for op, ref in ((SeparableSVDOperator.gaussian_blur((2, 24, 20)), blur_reflect_torch(x, taps)),
                    (SeparableSVDOperator.uniform_blur((2, 24, 20), 5),
                     blur_reflect_torch(x, torch.full((5,), 0.2))),
                    (SeparableSVDOperator.from_taps((2, 24, 20), taps, gaussian_taps(3, 0.8)), None),
                    (SeparableSVDOperator.bicubic_sr((2, 24, 20), 4), sr_filter_torch(x, bicubic_taps(4), 4)),
                    (SeparableSVDOperator.filtered_sr((2, 24, 20), gaussian_filter_taps(10, 1.5), 2),
                     sr_filter_torch(x, gaussian_filter_taps(10, 1.5), 2))):
        if ref is not None:
            assert _rel(op.apply(x).numpy(), ref.numpy()) <= 2e-6
        y = torch.randn(2, *op.y_shape, generator=g, dtype=torch.float64)
        lhs, rhs = float((op.apply(x) * y).sum()), float((x * op.apply_transpose(y)).sum())
        assert abs(lhs - rhs) <= 1e-12 * float(op.apply(x).norm() * y.norm())


@pytest.mark.parametrize("case", DENSE, ids=ids(DENSE))
def test_algebra_and_passes_against_the_dense_statement(case):
    name, C, make, rtol, _ = case
    ah, aw = make()
    t = sr.Tables.from_factors(ah, aw, rtol)
    H, W, Hy, Wy = t.dims
    D, S = sr.Dense(t), sr.Sep(t)
    g = torch.Generator().manual_seed(11)
    x, eps, xi = (torch.randn(3, H, W, generator=g, dtype=torch.float64) for _ in range(3))
    y = torch.randn(3, Hy, Wy, generator=g, dtype=torch.float64)
    fx, fe, fxi, fy = (v.reshape(3, -1).numpy() for v in (x, eps, xi, y))
    f = lambda v: v.reshape(3, -1).numpy()  # noqa: E731
    # <A x, y> = <x, A^T y>; A^+ A A^+ = A^+; A^+ A symmetric and idempotent
    assert abs((fx @ D.A.T * fy).sum() - (fx * (fy @ D.A)).sum()) <= 1e-12 * np.linalg.norm(fx) * np.linalg.norm(fy)
    assert np.abs(D.Apinv @ D.A @ D.Apinv - D.Apinv).max() <= 1e-10 * np.abs(D.Apinv).max()
    PA = D.Apinv @ D.A
    assert np.abs(PA - PA.T).max() <= 1e-10 and np.abs(PA @ PA - PA).max() <= 1e-10
    assert np.abs(PA - D.Pi).max() <= 1e-10
    # the separable evaluation is the dense one, in both side orders
    for rf in (False, True):
        S = sr.Sep(t, right_first=rf)
        assert _rel(f(S.apply(x)), fx @ D.A.T) <= 1e-12
        assert _rel(f(S.adjoint(y)), fy @ D.A) <= 1e-12
        assert _rel(f(S.pinv(y)), fy @ D.Apinv.T) <= 1e-10
        assert _rel(f(S.pinv_t(x)), fx @ D.Apinv) <= 1e-10
        a, k, gs = 0.3, np.sqrt(1 - 0.09), 400.0
        x0 = (fx - k * fe) / a
        v, rsq = S.dps(x, eps, y, a, k, gs)
        r = fy - x0 @ D.A.T
        assert _rel(f(v), gs * (r @ D.A)) <= 1e-10 and _rel(rsq.numpy(), (r * r).sum(1)) <= 1e-12
        # the PGDM gradient identity: d/dx0 |A^+ y - A^+ A x0|^2 = -2 (A^+ y - Pi x0)
        want = -2.0 * (fy @ D.Apinv.T - x0 @ D.Pi)
        assert _rel(f(S.pgdm(x, eps, y, a, k, -2.0)), want) <= 1e-10
        diff = fy @ D.Apinv.T - x0 @ PA.T
        assert _rel(want, -2.0 * diff @ PA) <= 1e-9
        for rho in (1e-4, 1e-2, 1.0, 50.0):
            assert _rel(f(S.prox(x, y, rho)), D.prox(fx, fy, rho)) <= 1e-10
        c = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)
        z = D.prox((fx - 0.6 * fe) / 0.8, fy, 0.37)
        want = 0.9 * z + (0.3 * ((fx - 0.8 * z) / 0.6) + 0.2 * fxi)
        assert _rel(f(S.diffpir(x, eps, y, xi, c)), want) <= 1e-10


@pytest.mark.parametrize("case", DENSE, ids=ids(DENSE))
def test_ddrm_step_is_the_dense_eigh_form_and_ddrm_step_svd(case):
    name, C, make, rtol, _ = case
    ah, aw = make()
    t = sr.Tables.from_factors(ah, aw, rtol)
    H, W, Hy, Wy = t.dims
    D, S = sr.Dense(t), sr.Sep(t)
    g = torch.Generator().manual_seed(13)
    x, eps, xi = (torch.randn(3, H, W, generator=g, dtype=torch.float64) for _ in range(3))
    y = S.apply(torch.randn(3, H, W, generator=g, dtype=torch.float64)) + 0.05 * torch.randn(
        3, Hy, Wy, generator=g, dtype=torch.float64)
    f = lambda v: v.reshape(3, -1)  # noqa: E731
    op = SeparableSVDOperator((1, H, W), ah, aw, rtol=rtol)
    t32 = sr.Tables.from_flat(op.tables, H, W, Hy, Wy)
    S32, A32 = sr.Sep(t32), torch.from_numpy(sr.Dense(t32).A_kept)
    worst = worst_svd = 0.0
    for sp, sy, (eta, eb) in itertools.product(dr.SIG_PREVS, dr.SIG_YS, dr.ETAS):
        c = dr.make_coefs(sp, sy, eta, eb)
        ref = dr.dense_step(torch.from_numpy(D.A_kept), f(x), f(eps), f(y), f(xi), c)
        worst = max(worst, _rel(f(S.ddrm(x, eps, y, xi, c)).numpy(), ref.numpy()))
        # ddrm_step_svd on the operator (its fp32 tables promoted) against the same tables' forms
        co = DDRMCoefficients(**c)
        got = ddrm_step_svd(op, x[:, None], eps[:, None], y[:, None], xi[:, None], co)[:, 0]
        worst_svd = max(worst_svd, _rel(f(got).numpy(), f(S32.ddrm(x, eps, y, xi, c)).numpy()))
    print(f"{name}: separable against dense eigh {worst:.3g}, ddrm_step_svd against separable {worst_svd:.3g}")
    assert worst <= 1e-10
    # P = fl32(1 / S) is not 1 / fl32(S): ddrm_step_svd divides, the tables multiply, 1.2e-7 apart
    assert worst_svd <= 1e-6
    assert A32.shape == (Hy * Wy, H * W)


# --- exact cases ----------------------------------------------------------------------------------------------
def _exact_results(t, tp, data, sep_kw, wrong=None):
    """Every pass on the exact tables (t: S in {1, 1/2, 1/4}; tp: S in {1, 0} for the prox);
    ``data``: (x, eps, xi, y of every sample)."""
    dt = sep_kw["dtype"]
    x, eps, xi, y = (v.to(dt) for v in data)
    S, Sp = sr.Sep(t, wrong=wrong, **sep_kw), sr.Sep(tp, wrong=wrong, **sep_kw)
    e, px = sr.EXACT_DPS, sr.EXACT_PROX
    out = {"A": S.apply(x), "AT": S.adjoint(y), "pinv": S.pinv(y), "pinvT": S.pinv_t(x)}
    out["dps_v"], _ = S.dps(x, eps, y, e["a"], e["k"], e["gs"])
    out["pgdm_v"] = S.pgdm(x, eps, y, e["a"], e["k"], -e["gs"])
    out["prox_z"] = Sp.prox(x, y, px["rho"])
    out["diffpir"] = Sp.diffpir(x, eps, y, xi, px)
    for regime in ("big", "small"):
        out[f"ddrm_{regime}"] = S.ddrm(x, eps, y, xi, dr.exact_coefs(regime, 1))
    return out


@pytest.mark.parametrize("i", range(len(sr.EXACT_CASES)), ids=ids(sr.EXACT_CASES))
def test_exact_cases_fp32_returns_the_fp64_result_in_every_order(i):
    name, C, H, W, bh, bw, amp = sr.EXACT_CASES[i]
    t, tp = sr.exact_tables(i), sr.exact_tables(i, prox=True)
    for tab in (t, tp):
        assert np.array_equal(tab.rounded().flat32().numpy(), tab.flat32().numpy())
        nz = tab.S[tab.S > 0]
        assert np.array_equal(np.log2(nz), np.round(np.log2(nz)))  # powers of two
        assert 0.1 <= tab.kept_share() <= 0.9
    for batch, ydiv in sr.BATCH_FORMS:  # the data of the GPU test, in both of its batch forms
        x, eps, xi, _, ye = sr.exact_form(i, batch, ydiv)
        data = (x, eps, xi, ye)
        ref = _exact_results(t, tp, data, dict(dtype=torch.float64))
        for rf, rev in itertools.product((False, True), (False, True)):
            got = _exact_results(t, tp, data, dict(dtype=torch.float32, right_first=rf, reverse=rev))
            for key, want in ref.items():
                assert torch.equal(want.float().double(), want), key  # an fp32 number
                assert torch.equal(got[key].double(), want), (key, rf, rev)
    # both DDRM regimes see all three classes or the small one alone
    s2 = torch.from_numpy(t.S.astype(np.float32) ** 2)
    assert bool(dr.big_mask32(s2, dr.exact_coefs("big", 1)).any())
    assert not bool(dr.big_mask32(s2, dr.exact_coefs("small", 1)).any())


# U_H and U_W can be exchanged only where Hy = Wy
WRONG = [(i, w) for i, c in enumerate(sr.EXACT_CASES) for w in ("transposed", "swap_u", "p_for_s", "shifted_keep")
         if w != "swap_u" or c[2] == c[3]]


@pytest.mark.parametrize("i,wrong", WRONG, ids=[f"{sr.EXACT_CASES[i][0]}-{w}" for i, w in WRONG])
def test_exact_cases_tell_wrong_answers_apart(i, wrong):
    t, tp = sr.exact_tables(i), sr.exact_tables(i, prox=True)
    x, eps, xi, _, ye = sr.exact_form(i, 4, 2)
    data = (x, eps, xi, ye)
    ref = _exact_results(t, tp, data, dict(dtype=torch.float64))
    got = _exact_results(t, tp, data, dict(dtype=torch.float32), wrong=wrong)
    affected = {"transposed": ("A", "AT", "pinv", "pinvT", "dps_v", "pgdm_v", "prox_z", "diffpir", "ddrm_big"),
                "swap_u": ("A", "AT", "pinv", "pinvT", "dps_v", "pgdm_v", "prox_z", "diffpir", "ddrm_big"),
                "p_for_s": ("A", "AT", "dps_v", "ddrm_big", "ddrm_small"),
                "shifted_keep": ("pinv", "pinvT", "pgdm_v", "ddrm_big", "ddrm_small")}[wrong]
    for key in affected:
        assert not torch.equal(got[key].double(), ref[key]), key
