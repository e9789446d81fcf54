"""fp64 semantics of the latent-sampler entry points — TEST INFRASTRUCTURE ONLY.

Plain float64 numpy restatements of what ``include/samplers_hip.h`` documents for
``sp_psld_pixel``, ``sp_psld_cotangent``, ``sp_pixel_opt_step``, ``sp_adamw_step``,
``sp_ddim_eps_step``, ``sp_stochastic_resample``, ``sp_scaled_combine`` and the two stop rules
(``sp_opt_check`` / ``sp_opt_check_plateau``), on flat ``(B, n)`` arrays.  The operator enters as
an ``(apply, adjoint)`` pair as in ``oracle/closed_form.py`` (``identity_ops``, ``inpaint_ops``,
``mask_ops``, ``oracle.blur.blur_ops``, ``sr_ops.sr_ops``).

The coefficient structs are taken exactly as the kernels get them — the fp32-rounded fields of
``adamw_coefficients``, ``eps_step_coefficients`` and ``SpDpsCoefs`` widened to float64 — so a
comparison measures the kernel's arithmetic and not the host's rounding of the scalars.

The comparison helpers carry the project's standing bounds for a fused pass against its closed
form (tolerances): 2e-5 x max|reference| per element, 2e-5 relative on a residual
norm.  Both reject non-finite values.
"""

from __future__ import annotations

from typing import Callable

import numpy as np

Arr = np.ndarray
Map = Callable[[Arr], Arr]

ELEMENT_BOUND = 2e-5  # x max|reference|, per element
RSQ_BOUND = 2e-5      # relative, per-sample residual norms


def _f64(t) -> Arr:
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def _rows(batch: int, y_div: int) -> Arr:
    return np.arange(batch) // y_div


# --- comparison helpers ----------------------------------------------------------------------
def assert_close_scaled(got, ref, bound: float = ELEMENT_BOUND) -> float:
    """|got - ref| <= bound x max|ref| for every element (NaN / inf in ``got`` fail); returns the
    measured maximum error over max|ref|."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = np.abs(got - ref)
    bad = ~(err <= bound * scale)  # NaN compares false, so it lands here
    if bad.any():
        first = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(
            f"{int(bad.sum())} of {got.size} elements differ by more than {bound:g} x max|ref| "
            f"(= {bound * scale:.3g}); first at flat index {first}: got "
            f"{got.reshape(-1)[first]!r}, reference {ref.reshape(-1)[first]!r}")
    return float(err.max() / scale) if scale > 0 else 0.0


def assert_rsq(partials, ref, bound: float = RSQ_BOUND) -> float:
    """Row sums of the (B, P) partials against the (B,) reference norms, ``bound`` relative;
    returns the measured maximum relative error."""
    got = _f64(partials)
    got = got.reshape(got.shape[0], -1).sum(axis=1)
    ref = _f64(ref).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound * np.abs(ref))
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"residual norm of sample {b}: got {got[b]!r}, reference {ref[b]!r} "
                             f"(bound {bound:g} relative)")
    rel = err / np.where(ref != 0, np.abs(ref), 1.0)
    return float(rel.max())


# --- PSLD --------------------------------------------------------------------------------------
def psld_pixel64(x0, y_rows, y_div: int, apply: Map, adjoint: Map):
    """``sp_psld_pixel``: r = y - A x0;  returns (x_eff = A^T y + x0 - A^T A x0, atr = A^T r,
    rsq[b] = ||r_b||^2)."""
    x0 = _f64(x0)
    y = _f64(y_rows)[_rows(x0.shape[0], y_div)]
    ax = apply(x0)
    r = y - ax
    x_eff = adjoint(y) + x0 - adjoint(ax)
    return x_eff, adjoint(r), (r.reshape(r.shape[0], -1) ** 2).sum(axis=1)


def psld_cotangent64(atr, u, norm_sq: float, omega: float, apply: Map, adjoint: Map) -> Arr:
    """``sp_psld_cotangent``: -omega atr / sqrt(norm_sq) + (I - A^T A) u; the first term is zero
    at a zero norm (torch's norm backward)."""
    atr, u = _f64(atr), _f64(u)
    nrm = float(np.sqrt(np.float64(norm_sq)))
    cl = -float(omega) / nrm if nrm > 0 else 0.0
    return cl * atr + (u - adjoint(apply(u)))


# --- AdamW -------------------------------------------------------------------------------------
def adamw64(p, g, m, v, coefs):
    """One ``torch.optim.AdamW`` step from the ``SpAdamWCoefs`` scalars; returns new (p, m, v)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    decay, b1, b2 = float(coefs.decay), float(coefs.beta1), float(coefs.beta2)
    eps, step_size, bc2 = float(coefs.eps), float(coefs.step_size), float(coefs.bc2_sqrt)
    p = p * decay
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    p = p - step_size * m / (np.sqrt(v) / bc2 + eps)
    return p, m, v


def pixel_opt64(x, m, v, y_rows, y_div: int, gs: float, coefs, apply: Map, adjoint: Map):
    """``sp_pixel_opt_step``: r = y - A x, g = A^T(gs r), AdamW on x; returns new (x, m, v) and
    rsq[b] = ||r_b||^2 of x BEFORE the update."""
    x = _f64(x)
    y = _f64(y_rows)[_rows(x.shape[0], y_div)]
    r = y - apply(x)
    g = adjoint(float(gs) * r)
    xn, mn, vn = adamw64(x, g, m, v, coefs)
    return xn, mn, vn, (r.reshape(r.shape[0], -1) ** 2).sum(axis=1)


# --- ReSample elementwise steps ------------------------------------------------------------------
def ddim_eps64(x, eps, coefs, xi):
    """``sp_ddim_eps_step`` from the ``SpEpsCoefs`` scalars; returns (x_prev, x0, pseudo_x0)."""
    x, eps, xi = _f64(x), _f64(eps), _f64(xi)
    sqrt_oma, oma, sqrt_a = float(coefs.sqrt_oma), float(coefs.oma), float(coefs.sqrt_a)
    x0 = (x - sqrt_oma * eps) / sqrt_a
    pseudo = (x - oma * eps) / sqrt_a
    x_prev = float(coefs.sqrt_a_prev) * x0 + float(coefs.dir) * eps + float(coefs.sigma) * xi
    return x_prev, x0, pseudo


def stochastic_resample64(px0, xt, a_t: float, sigma: float, xi) -> Arr:
    """``sp_stochastic_resample`` (a_t, sigma: the fp32 scalars the kernel is passed)."""
    px0, xt, xi = _f64(px0), _f64(xt), _f64(xi)
    a_t, sigma = float(np.float32(a_t)), float(np.float32(sigma))
    oma = 1.0 - a_t
    mean = (sigma * np.sqrt(a_t) * px0 + oma * xt) / (sigma + 1.0 - a_t)
    return mean + xi * np.sqrt(1.0 / (1.0 / sigma + 1.0 / oma))


def scaled_combine64(a, alpha: float, b, beta: float, norm_sq) -> Arr:
    """``sp_scaled_combine``: alpha a + beta / sqrt(norm_sq) b  (a None: no first term; norm_sq
    None: 1; a zero norm gives a zero second term)."""
    b = _f64(b)
    cb = float(beta)
    if norm_sq is not None:
        nrm = float(np.sqrt(np.float64(norm_sq)))
        cb = cb / nrm if nrm > 0 else 0.0
    out = cb * b
    return out if a is None else float(alpha) * _f64(a) + out


def predict_x0_64(x, eps, a: float, k: float) -> Arr:
    """``sp_predict_x0`` (a, k: the fp32 scalars the kernel is passed)."""
    return (_f64(x) - float(np.float32(k)) * _f64(eps)) / float(np.float32(a))


# --- stop rules ----------------------------------------------------------------------------------
class StopRule:
    """Host model of ``sp_opt_check`` (``plateau_from`` None) and ``sp_opt_check_plateau``.

    ``loss`` (the last loss written, None = never written), ``prev`` (the plateau rule's previous
    loss, None = never written) and ``stop`` mirror the device words.  The loss is fp32
    (sum / total), the threshold compare is in double and strict, a set stop flag is sticky and
    makes every later check a no-op."""

    def __init__(self, total: float, threshold: float, plateau_from: int | None = None):
        self.total = np.float32(total)
        self.threshold = float(threshold)
        self.plateau_from = plateau_from
        self.stop = 0
        self.loss: float | None = None
        self.prev: float | None = None

    def check(self, partials, itr: int = 0) -> bool:
        """One check on the iteration's partials; returns whether anything was written."""
        if self.stop:
            return False
        s = np.float32(_f64(partials).sum())
        loss = np.float32(s / self.total)
        self.loss = float(loss)
        if self.plateau_from is not None and itr >= self.plateau_from:
            if itr > self.plateau_from and self.prev is not None and self.prev < float(loss):
                self.stop = 1
            self.prev = float(loss)
        if float(loss) < self.threshold:
            self.stop = 1
        return True
