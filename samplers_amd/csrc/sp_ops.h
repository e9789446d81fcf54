// Per-kind dispatch of the operator entry points (internal; includes sp_common.h).  Every
// `extern "C"` entry that takes an sp_op checks its common arguments, looks the kind's row up and
// calls through it.  The rows are filled in sp_dps.hip; a kind's functions live in its own file
// (IDENTITY / INPAINT / MASK share one set, next to their kernels in sp_dps.hip and sp_latent.hip;
// PSF_FFT / PSF_PERIODIC share the maps and DPS pass 1 of sp_psf_fft.hip; the kinds that transform
// in LDS launch every stage through fft_stage of sp_fft.h) and are called with a descriptor that passed valid_op() and the entry's arguments checked.
#pragma once

#include "sp_common.h"

namespace sp {

struct dps_residual_args {
    const float *x, *eps, *y;
    int64_t batch, y_div;
    float a, k, gs;
    const sp_step_rec* sched;  // with cursor: the device-resident schedule, else both null
    const int32_t* cursor;
    float *v, *partial;
    float* work;  // null in the forms without a workspace and where the kind needs none
};

// sp_op_prox_ws (eps null: x holds x0, out = z) and sp_diffpir_step_ws (eps set: out = x')
struct prox_args {
    const float *x, *eps, *y, *q, *xi;  // y: the one-launch kinds; q: the kinds with a prepare
    uint64_t seed;
    int64_t step, sample_offset, batch, y_div;
    sp_prox_coefs c;  // the prox form reads rho alone
    float *out, *work;
};

// sp_ddrm_step_ws
struct ddrm_args {
    const float *x, *eps, *y, *q, *xi;  // y: the one-launch kinds; q: PSF_PERIODIC (sp_pgdm_prepare's)
    uint64_t seed;
    int64_t step, sample_offset, batch, y_div;
    sp_ddrm_coefs c;
    float *out, *work;
};

// The four coefficients of one spectral component of the DDRM step (samplers_hip.h): s2 is the
// squared singular value, `observed` false outside the operator's kept set.  Every operation
// rounds on its own; the class is decided without a division or a square root, so numpy float32
// returns the same mask (tests/ddrm_ref.py).
struct ddrm_f {
    float th, ep, y, xi;
};
__host__ __device__ inline ddrm_f ddrm_class_coefs(const sp_ddrm_coefs& c, float s2, bool observed) {
#pragma clang fp contract(off)
    const float sp2 = c.sig_prev * c.sig_prev;
    const float es = c.eta * c.sig_prev;
    if (!observed || s2 == 0.f) return {1.f, c.c1 * c.sig_prev, 0.f, es};
    if (sp2 * s2 >= c.sig_y * c.sig_y) {  // big: the measured value replaces (eta_b = 1) x0's
        const float e = c.eta_b * c.sig_y;
        const float v = sp2 - (e * e) / s2;
        return {1.f - c.eta_b, 0.f, c.eta_b, __builtin_sqrtf(v > 0.f ? v : 0.f)};
    }
    const float r = ((c.c1 * c.sig_prev) * __builtin_sqrtf(s2)) / c.sig_y;  // < 1, sig_y > 0 here
    return {1.f - r, 0.f, r, es};
}

// The DiffPIR update from the proximal point z: eps_hat = (x - a z) / k (inv_k = 1 / k, taken once
// per thread) and x' = a_prev z + (c_eps eps_hat + c_xi xi).  Every product and sum rounds on its
// own: the bits are those of the expressions as written, whichever noise form the kernel was built
// for.  The pragma is lexical, so it stands here and not only at the call sites.
__host__ __device__ inline float diffpir_update(const sp_prox_coefs& c, float inv_k, float x, float z,
                                                float xi) {
#pragma clang fp contract(off)
    const float eh = (x - c.a * z) * inv_k;
    return c.a_prev * z + (c.c_eps * eh + c.c_xi * xi);
}

typedef bool valid_fn(const sp_op* op);
typedef int64_t partials_fn(const sp_op* op);
typedef int64_t workspace_fn(const sp_op* op, int64_t batch);
typedef int dps_residual_fn(const sp_op* op, const dps_residual_args& r, hipStream_t s);
typedef int map_fn(const sp_op* op, const float* in, float* out, int64_t batch, hipStream_t s);
typedef int apply_ws_fn(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                        hipStream_t s);
typedef int vjp_ws_fn(const sp_op* op, const float* x, const float* gy, float* dx, int64_t batch,
                      float* work, hipStream_t s);
typedef int psld_pixel_fn(const sp_op* op, const float* x0, const float* y, int64_t batch,
                          int64_t y_div, float* x_eff, float* atr, float* partial, hipStream_t s);
typedef int psld_cotangent_fn(const sp_op* op, const float* atr, const float* u, const float* ata_u,
                              const float* norm_sq, float omega, int64_t batch, float* out,
                              hipStream_t s);
typedef int pixel_opt_fn(const sp_op* op, float* x, float* exp_avg, float* exp_avg_sq,
                         const float* y, int64_t batch, int64_t y_div, float gs,
                         const sp_adamw_coefs* c, const int32_t* stop, float* partial, hipStream_t s);
typedef int pinv_ws_fn(const sp_op* op, const float* y, float* x, int64_t batch, int transpose,
                       float* work, hipStream_t s);
typedef int pgdm_prepare_fn(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s);
typedef int pgdm_residual_fn(const sp_op* op, const float* x, const float* eps, const float* q,
                             int64_t batch, int64_t y_div, const sp_dps_coefs& c, float* v,
                             float* work, hipStream_t s);
typedef int prox_fn(const sp_op* op, const prox_args& p, hipStream_t s);
typedef int ddrm_fn(const sp_op* op, const ddrm_args& p, hipStream_t s);

// One row per sp_op kind.  A null member is the library's answer for a kind without that pass:
// 0 floats of workspace, or SP_EUNSUPPORTED (apply_ws: sp_op_apply).  The conjugate-gradient
// proximal step (sp_cg.hip) has no column: it calls apply / adjoint, or apply_ws / vjp_ws with
// op_workspace, of whichever linear kind it is given.
struct op_kind {
    valid_fn* valid;        // the kind's geometry rules
    partials_fn* partials;  // r^2 partials per sample
    workspace_fn *dps_workspace, *op_workspace;
    dps_residual_fn* dps_residual;
    map_fn *apply, *adjoint;  // the linear kinds
    apply_ws_fn* apply_ws;    // the kinds whose maps need a workspace (with vjp_ws)
    vjp_ws_fn* vjp_ws;
    psld_pixel_fn* psld_pixel;
    psld_cotangent_fn* psld_cotangent;
    pixel_opt_fn* pixel_opt;
    uint32_t traits;  // SP_TRAIT_* (samplers_hip.h)
    // the kinds with a pseudo-inverse of their own (SP_TRAIT_PINV): A^+ / A^+T through the
    // workspace and the fused PGDM pass 1
    pinv_ws_fn* pinv_ws;
    pgdm_prepare_fn* pgdm_prepare;
    pgdm_residual_fn* pgdm_residual;
    // the kinds with a closed-form proximal map (sp_prox_workspace answers for the others): the
    // floats of work and of q (null: none, and nothing to prepare), q's two launches, z alone and
    // the whole DiffPIR step
    workspace_fn* prox_workspace;
    pgdm_prepare_fn* prox_prepare;
    prox_fn *prox, *diffpir_step;
    // the kinds with a DDRM step (sp_ddrm_workspace answers for the others): the floats of work
    // (null: none) and the step's launches
    workspace_fn* ddrm_workspace;
    ddrm_fn* ddrm_step;
};

const op_kind* kind_of(const sp_op* op);  // null for an unknown kind or a null op
bool valid_op(const sp_op* op);
int64_t tiles_elementwise(int64_t n);

// the kinds' functions, one line per column of the table (sp_blur.hip, sp_sr.hip, sp_psf.hip,
// sp_phase.hip, sp_psf_fft.hip, sp_radon.hip; elementwise_*: sp_latent.hip, the cotangent serves
// BLUR, PSF and RADON over A^T A u too).  sp_psf_fft.hip holds two kinds on one pipeline: the
// psf_fft_* functions serve PSF_FFT and PSF_PERIODIC alike (they branch on op->kind where the
// geometry differs); psf_periodic_* are the periodic kind's own rules and pseudo-inverse passes.
valid_fn blur_valid, sr_valid, psf_valid, phase_valid, psf_fft_valid, psf_periodic_valid, radon_valid;
partials_fn blur_partials, sr_partials, psf_partials, phase_partials, psf_fft_partials,
    radon_partials;
workspace_fn psf_workspace, phase_workspace, psf_fft_workspace, radon_workspace;
dps_residual_fn blur_dps_residual, sr_dps_residual, psf_dps_residual, phase_dps_residual,
    psf_fft_dps_residual, radon_dps_residual;
map_fn blur_apply, blur_adjoint, sr_apply, sr_adjoint, psf_apply, psf_adjoint, radon_apply,
    radon_adjoint;
apply_ws_fn phase_apply, psf_fft_apply;
vjp_ws_fn phase_vjp, psf_fft_vjp;
pinv_ws_fn psf_periodic_pinv;
pgdm_prepare_fn psf_periodic_pgdm_prepare;
pgdm_residual_fn psf_periodic_pgdm_residual;
psld_pixel_fn elementwise_psld_pixel, sr_psld_pixel;
psld_cotangent_fn elementwise_psld_cotangent, sr_psld_cotangent;
pixel_opt_fn elementwise_pixel_opt, sr_pixel_opt;
pgdm_prepare_fn psf_periodic_prox_prepare;
prox_fn sr_prox, psf_periodic_prox;  // both forms: p.eps selects (elementwise kinds: sp_dps.hip)
workspace_fn psf_periodic_ddrm_workspace;
ddrm_fn sr_ddrm, psf_periodic_ddrm;  // the elementwise kinds' launch: sp_dps.hip
// SP_OP_SR_PERIODIC (sp_psf_fft.hip, on the periodic kind's pipeline; psf_fft_workspace serves it)
valid_fn sr_periodic_valid;
partials_fn sr_periodic_partials;
dps_residual_fn sr_periodic_dps_residual;
apply_ws_fn sr_periodic_apply;
vjp_ws_fn sr_periodic_vjp;
pinv_ws_fn sr_periodic_pinv;
pgdm_prepare_fn sr_periodic_pgdm_prepare, sr_periodic_prox_prepare;
pgdm_residual_fn sr_periodic_pgdm_residual;
prox_fn sr_periodic_prox;
// SP_OP_SVD_SEPARABLE (sp_svd_sep.hip: per-plane dense products on the fp32-input MFMA)
valid_fn svd_sep_valid;
partials_fn svd_sep_partials;
workspace_fn svd_sep_op_workspace, svd_sep_dps_workspace, svd_sep_ddrm_workspace;
dps_residual_fn svd_sep_dps_residual;
apply_ws_fn svd_sep_apply;
vjp_ws_fn svd_sep_vjp;
pinv_ws_fn svd_sep_pinv;
pgdm_prepare_fn svd_sep_pgdm_prepare, svd_sep_prox_prepare;
pgdm_residual_fn svd_sep_pgdm_residual;
prox_fn svd_sep_prox;  // both forms: p.eps selects
ddrm_fn svd_sep_ddrm;
// SP_OP_HADAMARD (sp_hadamard.hip: Walsh-Hadamard butterflies in LDS; one workspace function serves
// every pass)
valid_fn hadamard_valid;
partials_fn hadamard_partials;
workspace_fn hadamard_workspace;
dps_residual_fn hadamard_dps_residual;
apply_ws_fn hadamard_apply;
vjp_ws_fn hadamard_vjp;
pinv_ws_fn hadamard_pinv;
pgdm_prepare_fn hadamard_pgdm_prepare;
pgdm_residual_fn hadamard_pgdm_residual;
prox_fn hadamard_prox;  // both forms: p.eps selects
ddrm_fn hadamard_ddrm;
// SP_OP_CHANNEL_MIX (sp_chanmix.hip: a small matrix across the channel axis at every pixel; every
// pass one launch without a workspace, the PGDM pass reads y itself)
valid_fn chanmix_valid;
partials_fn chanmix_partials;
dps_residual_fn chanmix_dps_residual;
map_fn chanmix_apply, chanmix_adjoint;
pinv_ws_fn chanmix_pinv;
pgdm_prepare_fn chanmix_pgdm_prepare;
pgdm_residual_fn chanmix_pgdm_residual;
prox_fn chanmix_prox;  // both forms: p.eps selects
ddrm_fn chanmix_ddrm;

}  // namespace sp
