"""tests/hadamard_ref.py against itself (no GPU, no operator code): the dense Sylvester statement
and the butterfly statement of every pass agree, the operator's algebra holds, the exact cases are
exact in fp32 in both level orders, and each of five wrong evaluations is told apart by them."""

import numpy as np
import pytest
import torch

import ddrm_ref as dr
import hadamard_ref as hr

TOL = 1e-12
SMALL = [i for i, c in enumerate(hr.CASES) if c[1][1] * c[1][2] <= 4096]  # the dense statement's planes
IDS = [c[0] for c in hr.CASES]
DPS = dict(a=0.3, k=0.95, gs=400.0)
PROX = dict(a=0.8, k=0.6, rho=0.37, a_prev=0.9, c_eps=0.3, c_xi=0.2)


def _data(i, b=2, dtype=torch.float64):
    _, (C, H, W), keep, _ = hr.case(i)
    g = torch.Generator().manual_seed(50 + i)
    x, eps, xi = (torch.randn(b, C, H, W, generator=g, dtype=dtype) for _ in range(3))
    y = torch.randn(b, C, int(keep.sum()), generator=g, dtype=dtype)
    return x, eps, xi, y


def _close(a, b, tol=TOL):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_sylvester_matrix_and_butterflies():
    for n in (2, 8, 64):
        h = hr.sylvester(n)
        assert np.array_equal(h, h.T) and np.array_equal(h @ h, n * np.eye(n))
        blocks = np.block([[hr.sylvester(n // 2), hr.sylvester(n // 2)], [hr.sylvester(n // 2), -hr.sylvester(n // 2)]])
        assert np.array_equal(h, blocks)  # the Sylvester recursion: natural order
        v = np.random.default_rng(n).standard_normal((3, n))
        for desc in (False, True):
            assert np.abs(hr.fwht(v, desc) - v @ h).max() <= 1e-12
            assert float((hr.fwht(torch.from_numpy(v), desc) - torch.from_numpy(v @ h)).abs().max()) <= 1e-12
    p = hr.sequency_permutation(8)
    changes = [(np.diff(hr.sylvester(8)[r]) != 0).sum() for r in p]
    assert changes == list(range(8))  # row p[s] has s sign changes


def test_kept_share_of_every_case():
    """Stated: every case keeps some coefficients and drops some, but the one all-kept case."""
    want = {"1x8x8-r50": 0.5, "3x8x16-r25": 0.25, "1x16x64-words": 0.75, "1x64x64-r10": 0.1, "2x64x128-r25": 0.25,
            "3x128x128-all": 1.0, "3x256x256-r25": 0.25, "1x1024x1024-r10": 0.1, "1x512x512-one": 2.0 ** -18}
    for i, name in enumerate(IDS):
        share = hr.kept_share(i)
        assert abs(share - want[name]) <= 1e-3, (name, share)
        assert (share == 1.0) == (name == "3x128x128-all") and share > 0
    assert sum(hr.case(i)[3] is None for i in range(len(hr.CASES))) == 1  # taps = NULL on one case
    _, _, keep, _ = hr.case(IDS.index("1x16x64-words"))
    words = keep.reshape(-1, 64)
    assert set(words.sum(1).tolist()) == {0, 64} and (words.sum(1) == 0).any()
    assert sorted(len(hr.forms_of(i)) for i in range(len(hr.CASES))) == [1] + [2] * 8
    assert [IDS[i] for i in hr.EXACT] == ["1x8x8-r50", "1x16x64-words", "1x64x64-r10", "3x128x128-all",
                                           "3x256x256-r25", "1x1024x1024-r10", "1x512x512-one"]


@pytest.mark.parametrize("i", SMALL, ids=[IDS[i] for i in SMALL])
def test_the_two_statements_agree(i):
    _, shape, keep, d = hr.case(i)
    x, eps, xi, y = _data(i)
    D, S = hr.Had(shape, keep, d, dense=True), hr.Had(shape, keep, d)
    _close(D.apply(x), S.apply(x))
    _close(D.adjoint(y), S.adjoint(y))
    vd, rd = D.dps(x, eps, y, **DPS)
    vs, rs = S.dps(x, eps, y, **DPS)
    _close(vd, vs), _close(rd, rs)
    _close(D.pgdm(x, eps, y, DPS["a"], DPS["k"], -2.0), S.pgdm(x, eps, y, DPS["a"], DPS["k"], -2.0))
    for rho in (1e-4, 1e-2, 1.0, 50.0):  # the dense solve against the closed form
        _close(D.prox(x, y, rho), S.prox(x, y, rho), 1e-9 if rho < 1e-3 else 1e-11)
    _close(D.diffpir(x, eps, y, xi, PROX), S.diffpir(x, eps, y, xi, PROX), 1e-11)


@pytest.mark.parametrize("i", SMALL, ids=[IDS[i] for i in SMALL])
def test_partial_isometry(i):
    _, shape, keep, d = hr.case(i)
    D = hr.Had(shape, keep, d, dense=True)
    A = D.A
    m, n = A.shape
    _close(A @ A.T, torch.eye(m, dtype=torch.float64))                 # A Aᵀ = I_m
    _close(torch.linalg.pinv(A), A.T, 1e-10)                            # A⁺ = Aᵀ
    P = A.T @ A
    _close(P, P.T), _close(P @ P, P)                                    # AᵀA a symmetric idempotent
    x, _, _, y = _data(i)
    S = hr.Had(shape, keep, d)
    lhs, rhs = (S.apply(x) * y).sum(), (x * S.adjoint(y)).sum()
    assert abs(float(lhs - rhs)) <= TOL * float(x.norm() * y.norm())  # <A x, y> = <x, Aᵀ y>
    assert torch.equal(S.pinv(y), S.adjoint(y)) and torch.equal(S.pinv_t(x), S.apply(x))


def test_pgdm_gradient_identity():
    """∂/∂x0 ‖A⁺y − A⁺A x0‖² = −2 Aᵀ(y − A x0): what pass 1 returns at gs = −2 with a = 1, k = 0."""
    i = 1
    _, shape, keep, d = hr.case(i)
    S = hr.Had(shape, keep, d)
    x, eps, _, y = _data(i)
    x0 = x.clone().requires_grad_()
    loss = (S.pinv(y) - S.pinv(S.apply(x0))).pow(2).sum()
    (grad,) = torch.autograd.grad(loss, x0)
    _close(grad, S.pgdm(x, eps, y, 1.0, 0.0, -2.0), 1e-11)


@pytest.mark.parametrize("sig_prev", dr.SIG_PREVS)
@pytest.mark.parametrize("sig_y", dr.SIG_YS)
def test_ddrm_forms_agree(sig_prev, sig_y):
    """The dense ``eigh`` definition, the projector form and ``ddrm_step_svd`` on the operator, over
    the scalar regimes of tests/test_ddrm_ref.py."""
    from samplers_amd.operators import HadamardOperator
    from samplers_amd.samplers.ddrm import ddrm_step_svd
    from samplers_amd.samplers.utils.bridge_kernels import DDRMCoefficients

    i = 0
    _, shape, keep, d = hr.case(i)
    x, eps, xi, y = _data(i)
    D, S = hr.Had(shape, keep, d, dense=True), hr.Had(shape, keep, d)
    op = HadamardOperator(shape, kept=keep, signs=d)
    for eta, eta_b in dr.ETAS:
        c = dr.make_coefs(sig_prev, sig_y, eta, eta_b)
        want = D.ddrm(x, eps, y, xi, c)
        _close(S.ddrm(x, eps, y, xi, c), want, 1e-10)
        got = ddrm_step_svd(op, x, eps, y, xi, DDRMCoefficients(**c))
        _close(got, want, 1e-10)


# --- exact cases ------------------------------------------------------------------------------------------
def _emulations(i, b, yd, **kw):
    _, shape, keep, d = hr.case(i)
    x, eps, xi, y = hr.exact_data(i, b, yd)
    ye = hr.expand(y, b, yd)
    n = lambda t: t.numpy()  # noqa: E731
    em = lambda what, **a: hr.emulate(what, shape, keep, d, **a, **kw)  # noqa: E731
    return {"apply": em("apply", x=n(x)), "adjoint": em("adjoint", y=n(ye)),
            "dps": em("dps", x=n(x), eps=n(eps), y=n(ye), c=hr.EXACT_DPS)[0],
            "pgdm": em("pgdm", x=n(x), eps=n(eps), y=n(ye), c=dict(hr.EXACT_DPS, gs=-2.0)),
            "prox": em("prox", x=n(x), y=n(ye), c=hr.EXACT_PROX),
            "diffpir": em("diffpir", x=n(x), eps=n(eps), y=n(ye), xi=n(xi), c=hr.EXACT_PROX),
            "ddrm": em("ddrm", x=n(x), eps=n(eps), y=n(ye), xi=n(xi), c=hr.EXACT_DDRM)}


def _fp64(i, b, yd):
    _, shape, keep, d = hr.case(i)
    x, eps, xi, y = hr.exact_data(i, b, yd)
    ye = hr.expand(y, b, yd)
    S, e = hr.Had(shape, keep, d), hr.EXACT_DPS
    return {"apply": S.apply(x), "adjoint": S.adjoint(ye), "dps": S.dps(x, eps, ye, **e)[0],
            "pgdm": S.pgdm(x, eps, ye, e["a"], e["k"], -2.0), "prox": S.prox(x, ye, hr.EXACT_PROX["rho"]),
            "diffpir": S.diffpir(x, eps, ye, xi, hr.EXACT_PROX), "ddrm": S.ddrm(x, eps, ye, xi, hr.EXACT_DDRM)}


@pytest.mark.parametrize("i", hr.EXACT, ids=[IDS[i] for i in hr.EXACT])
def test_exact_cases_do_not_round_in_fp32(i):
    """Every fp32 emulation, levels low-then-high and high-then-low, returns the fp64 result bit
    for bit: integer data, dyadic scalars, even k."""
    b, yd = hr.forms_of(i)[-1]
    want = _fp64(i, b, yd)
    assert set(want) == set(hr.EXACT_PASSES)
    for desc in (False, True):
        got = _emulations(i, b, yd, descending=desc)
        for what in hr.EXACT_PASSES:
            assert got[what].dtype == np.float32
            assert np.array_equal(got[what].astype(np.float64), want[what].numpy()), (what, desc)


@pytest.mark.parametrize("wrong", hr.WRONG)
def test_wrong_emulations_are_told_apart(wrong):
    """A dropped sign vector, a rank shifted by one, a misread word boundary of keep_bits, sequency
    order in place of natural order, a missing second scale: none returns the fp64 result."""
    touched = {"no_signs": ("apply", "adjoint", "dps", "prox", "diffpir", "ddrm"),
               "rank_shift": ("apply", "adjoint", "dps", "prox", "diffpir", "ddrm"),
               "word_boundary": ("apply", "adjoint", "dps", "prox", "diffpir", "ddrm"),
               "sequency": ("apply", "adjoint", "dps", "prox", "diffpir", "ddrm"),
               "one_scale": ("adjoint", "dps", "pgdm", "prox", "diffpir", "ddrm")}[wrong]
    for i in (hr.EXACT[0], hr.EXACT[2]):  # one keep_bits word; 64 words at 10 %
        b, yd = hr.forms_of(i)[-1]
        want, got = _fp64(i, b, yd), _emulations(i, b, yd, wrong=wrong)
        for what in touched:
            assert not np.array_equal(got[what].astype(np.float64), want[what].numpy()), (wrong, what, IDS[i])


def test_roundings_are_counted_from_the_algorithm():
    for k in (6, 7, 12, 16, 20):
        t = k + 2
        assert hr.roundings("apply", k) == hr.roundings("adjoint", k) == t
        assert hr.roundings("dps", k) == hr.roundings("pgdm", k) == hr.roundings("prox", k) == 2 * t + 5
        assert hr.roundings("diffpir", k) == hr.roundings("ddrm", k) == 2 * t + 15
    assert hr.roundings("rsq", 16, 3 * 16384) == 16 + 16 + 4
    # the envelope dominates the pass it bounds
    i = 1
    _, shape, keep, d = hr.case(i)
    S = hr.Had(shape, keep, d)
    x, eps, xi, y = _data(i)
    c = dict(DPS)
    assert bool((S.envelope("apply", x=x) >= S.apply(x).abs()).all())
    assert bool((S.envelope("adjoint", y=y) >= S.adjoint(y).abs()).all())
    assert bool((S.envelope("dps", x=x, eps=eps, y=y, c=c) >= S.dps(x, eps, y, **c)[0].abs()).all())
    assert bool((S.envelope("rsq", x=x, eps=eps, y=y, c=c) >= S.dps(x, eps, y, **c)[1]).all())
    assert bool((S.envelope("diffpir", x=x, eps=eps, y=y, xi=xi, c=PROX) >= S.diffpir(x, eps, y, xi, PROX).abs()).all())
    cc = dr.make_coefs(0.5, 0.05, 0.5, 0.5)
    assert bool((S.envelope("ddrm", x=x, eps=eps, y=y, xi=xi, c=cc) >= S.ddrm(x, eps, y, xi, cc).abs()).all())
