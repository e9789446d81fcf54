/*
 * samplers_hip.h — C ABI of libsamplers_hip.so, the MI355X (gfx950) hot path of
 * diffusion posterior sampling (DPS / PSLD / PGDM / ReSample / DiffPIR / DDRM guidance steps).
 *
 * The reference (thomashirtz/samplers) is pure Python over PyTorch; every entry
 * point below replaces a group of eager ATen calls that the reference issues
 * per reverse-diffusion step.  Each declaration cites the reference code it
 * replaces (paths relative to the reference repository root).
 *
 * Conventions (all entry points):
 *   - device pointers to contiguous fp32 data; a "sample" is one row of
 *     n = C*H*W elements (x-space) or m elements (y-space, observation);
 *   - `stream` is the caller's hipStream_t (PyTorch passes its current stream);
 *     every call is asynchronous on that stream and never synchronises;
 *   - the library allocates nothing; callers pass every buffer;
 *   - return 0 on success, a negative SP_E* code on bad arguments or a failed
 *     launch (the launch error is also readable through sp_last_error()).
 *   - observation row for sample b is b / y_div (y_div = number of
 *     reconstructions sharing one observation, >= 1).
 *   - alignment.  The elementwise kernels move one float4 per lane when the row length allows.
 *     Entry points over a flat `count` check their pointers and fall back to scalar access
 *     (the same arithmetic per element) when count % 4 != 0 or any buffer is not 16-byte aligned:
 *     sp_scaled_combine, sp_adamw_step, sp_adamw_step_until, sp_predict_x0.  Every other entry
 *     point over rows of n (or m) elements chooses float4 access from n % 4 == 0 alone and then
 *     REQUIRES 16-byte aligned row buffers, y included where m == n (rows are n floats apart,
 *     so the base pointer decides): sp_dps_residual / sp_dps_update and their _sched forms, sp_residual_grad (m),
 *     sp_randn, sp_op_apply / sp_op_adjoint, sp_op_prox_ws, sp_diffpir_step_ws, sp_ddrm_step_ws, sp_psld_pixel, sp_psld_cotangent,
 *     sp_pixel_opt_step, sp_ddim_eps_step, sp_stochastic_resample, sp_op_prox_cg_ws and
 *     sp_diffpir_step_cg_ws (x-space rows by n; y rows by m % 4 == 0, INPAINT's packed rows
 *     included; work 16-byte aligned).  Elsewhere packed INPAINT observation
 *     rows (m elements) and partial-sum buffers are read by scalar loads and need only 4-byte
 *     alignment.  With n % 4 != 0 all access is scalar and 4-byte alignment suffices.
 *     PHASE: the kind's own launches read x, eps, y, g and write y, v, dx by scalar access (any
 *     width, any pads, 4-byte alignment); its workspace holds (re, im) pairs and must be 8-byte
 *     aligned.  Pass 2 over its v follows the rule above (n % 4 == 0 -> 16-byte aligned rows).
 *     CHANNEL_MIX: its launches choose float4 access from height * width % 4 == 0 and then
 *     REQUIRE 16-byte aligned rows of x and of y (every plane of a row then starts 16-byte
 *     aligned); otherwise all its access is scalar and 4-byte alignment suffices.  Pass 2 over its v
 *     follows the rule above.
 */
#ifndef SAMPLERS_HIP_H
#define SAMPLERS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sp_stream_t; /* hipStream_t */

enum {
    SP_OK = 0,
    SP_EINVAL = -1,   /* bad argument (null pointer, size, unsupported operator kind) */
    SP_ELAUNCH = -2,  /* kernel launch failed */
    SP_EUNSUPPORTED = -3
};

/* Operator kinds (reference: samplers/operators/). */
enum {
    SP_OP_IDENTITY = 0, /* identity.py:8-68        y = x                      */
    SP_OP_INPAINT = 1,  /* inpainting.py:8-195     y = x.flat[kept]            */
    SP_OP_BLUR = 2,     /* new (BASELINE config 3): depthwise separable Gaussian
                           blur with reflect padding; adjoint = exact transpose */
    SP_OP_MASK = 3,     /* inpainting.py:106-109 (flatten=False): y = x with the
                           masked pixels zeroed; uses keep_bits only, m == n   */
    SP_OP_SR = 4,       /* new: x factor super-resolution, y = the factor x factor
                           average pooling of every channel plane (factor 2, 4
                           or 8 dividing height and width, m = n / factor^2);
                           adjoint = exact transpose, A^+ = factor^2 A^T       */
    SP_OP_PSF = 5,      /* new: depthwise dense 2-D point-spread function of
                           (2*radius+1)^2 taps (motion blur, defocus, measured
                           PSFs), correlation with reflect padding; adjoint =
                           exact transpose; no pseudo-inverse; m == n           */
    SP_OP_PHASE = 6,    /* new, NONLINEAR: Fourier phase retrieval,
                           y = |FFT2(zero-pad(x))| per channel plane, norm "ortho",
                           unshifted (DC at [0][0]); pad_h = radius rows and
                           pad_w = factor columns of zeros on each side; the padded
                           sizes Nh = height + 2*radius, Nw = width + 2*factor are
                           2^k or 3*2^k in [8, 1024]; m = channels*Nh*Nw.  No
                           adjoint: sp_op_apply_ws / sp_op_vjp_ws                */
    SP_OP_PSF_FFT = 7,  /* new: the correlation of SP_OP_PSF through in-LDS FFTs, for
                           any radius 1 <= radius <= min(height, width) - 1 with
                           height + 2*radius, width + 2*radius <= 1024, the image
                           extended by reflection, wrap-around or zeros (factor =
                           0, 1, 2).  Nh (Nw) is the smallest 2^k or 3*2^k in
                           [8, 1024] >= height + 2*radius (width + 2*radius); taps
                           holds the PSF's SPECTRUM (below).  Linear, m == n, no
                           pseudo-inverse; the maps need a workspace:
                           sp_op_apply_ws = A, sp_op_vjp_ws = A^T (x not read)   */
    SP_OP_PSF_PERIODIC = 8, /* new: the wrap-around correlation of a (2*radius+1)^2 PSF on
                           an image whose own sizes are transform lengths: height and
                           width each 2^k or 3*2^k in [8, 1024], radius >= 1,
                           2*radius+1 <= min(height, width), factor = 0.  The map is
                           diagonal in the H x W transform, A = IFFT2 M FFT2, so it has
                           a spectral pseudo-inverse; taps holds M and P (below).
                           Linear, m == n; sp_op_apply_ws = A, sp_op_vjp_ws = A^T,
                           sp_op_pinv_ws = A^+ / A^+T, sp_pgdm_prepare and
                           sp_pgdm_residual_ws the fused PGDM pass 1             */
    SP_OP_RADON = 9,    /* new: parallel-beam CT projector (Joseph's method, unit pixel
                           and detector spacing), depthwise over channel planes:
                           y is (channels, radius, factor) = (C, angles, detector
                           bins), m = channels*radius*factor != n in general;
                           8 <= height, width <= 512, 1 <= radius <= 512 angles,
                           1 <= factor <= 1024 bins; taps holds one row per angle
                           (below).  Linear, adjoint = exact transpose (a gather per
                           pixel, no atomics); no pseudo-inverse                */
    SP_OP_SR_PERIODIC = 10, /* new: periodic blur-and-decimate x factor super-resolution
                           (bicubic, Gaussian blur + decimation), depthwise:
                           y[c][i][j] = sum_{u,v} h[u][v] x[c][(factor*i + u - P) mod H]
                           [(factor*j + v - P) mod W] over radius^2 taps, P = (radius -
                           factor) / 2.  factor 2, 4 or 8 dividing height and width,
                           each 2^k or 3*2^k in [8, 1024]; factor <= radius <=
                           min(height, width), radius - factor even; m = n / factor^2.
                           A = S IFFT2 M FFT2 with S the lattice [::factor, ::factor],
                           so A A^T is diagonal in the low-resolution transform: exact
                           transpose, spectral pseudo-inverse and closed-form proximal
                           map; taps holds M, P and Lambda (below).  The maps need a
                           workspace: sp_op_apply_ws = A, sp_op_vjp_ws = A^T,
                           sp_op_pinv_ws = A^+ / A^+T, and the fused PGDM and prox
                           passes as PSF_PERIODIC                                 */
    SP_OP_SVD_SEPARABLE = 11, /* new: A X = A_H X A_W^T on every channel plane, A_H (Hy x H)
                           and A_W (Wy x W) any dense matrices (a blur under any boundary
                           rule, filter-and-decimate super-resolution), given by their
                           SVDs: A = (U_H (x) U_W) diag(s_H[i] s_W[j]) (V_H (x) V_W)^T.  y is
                           (channels, radius, factor) = (C, Hy, Wy); 2 <= height, width <=
                           512, 1 <= Hy <= height, 1 <= Wy <= width, any integers;
                           m = channels*Hy*Wy; taps holds the six tables (below).  Per-plane
                           dense products on the fp32-input MFMA (csrc/sp_svd_sep.hip).
                           The maps need a workspace: sp_op_apply_ws = A, sp_op_vjp_ws =
                           A^T, sp_op_pinv_ws = A^+ / A^+T, the fused DPS, PGDM, proximal
                           and DDRM passes as PSF_PERIODIC                           */
    SP_OP_HADAMARD = 12, /* new: compressed sensing on a scrambled Walsh-Hadamard transform.  Per
                           channel plane, with i = h*width + w and n_p = height*width = 2^k,
                           (A x)[c][r] = n_p^(-1/2) sum_i (-1)^popcount(j_r & i) d[i] x[c][i]:
                           j_r the r-th kept coefficient in ascending natural (Sylvester)
                           order, d the sign vector in taps (n_p floats, each exactly +-1;
                           NULL: all +1), the kept set and d shared by the channels.
                           keep_bits (n_p / 64 words, bit j%64 of word j/64 set <=>
                           coefficient j observed) and word_rank (the observed count before
                           word w) as INPAINT over one plane, both non-null; radius = factor
                           = 0; 6 <= k <= 20, height, width >= 1; n = channels*n_p;
                           m % channels == 0 and 1 <= m/channels <= n_p; y is (channels,
                           m/channels).  A A^T = I_m and A^+ = A^T (U = I, s = 1, V^T the
                           transform).  n_p^(-1/2) is applied once per transform: a power of
                           two for even k, the fp32 rounding of 2^(-k/2) for odd k.
                           csrc/sp_hadamard.hip: add/subtract levels in LDS, one launch per
                           map for n_p <= 4096, else a low stage (chunks of 4096 floats), a
                           high stage (all high rows by a run of columns) through work.  The
                           maps need a workspace: sp_op_apply_ws = A, sp_op_vjp_ws = A^T,
                           sp_op_pinv_ws = A^T / A; the fused DPS, PGDM, proximal, DiffPIR
                           and DDRM passes are out = base + A^T(g y + A w) in one launch
                           (n_p <= 4096) or three; every workspace (sp_dps_workspace,
                           sp_op_workspace, sp_prox_workspace, sp_ddrm_workspace) is
                           batch * n floats; sp_rsq_partials is channels * (1 or the high
                           stage's tiles per plane); the q of sp_pgdm_prepare is y copied,
                           rows of m floats (sp_pgdm_residual_ws and sp_ddrm_step_ws read
                           it), sp_prox_prepare prepares nothing: the prox entries read y */
    SP_OP_CHANNEL_MIX = 13 /* new: y = M x across the channel axis at every pixel, M a Cy x C
                           matrix (colorization by mean or luma weights, a colour-correction or
                           sensor-response matrix, spectral bands mixed down to RGB):
                           y[i][h][w] = sum_c M[i][c] x[c][h][w].  channels = C, radius = Cy,
                           factor = 0; 1 <= Cy <= C <= 8; height, width >= 1 with height * width
                           < 2^31; n = C*height*width, m = Cy*height*width, y is (Cy, height,
                           width); taps holds the six tables (below); keep_bits and word_rank
                           NULL.  Block-diagonal over the pixels and the SVD of the operator is
                           the SVD of M, so every pass is ONE launch with no halo and no workspace
                           (csrc/sp_chanmix.hip): sp_op_apply / sp_op_adjoint (from M),
                           sp_op_pinv_ws = A^+ / A^+T (from N), DPS pass 1, the PGDM pass 1 (it
                           reads the observation rows themselves), the proximal map, the DiffPIR
                           step and the DDRM step.  sp_rsq_partials is the tiles per sample:
                           ceil(G / 256) with G = height*width / 4 groups of four pixels where
                           height*width % 4 == 0, else G = height*width.  Every workspace size
                           (sp_dps_workspace, sp_op_workspace, sp_prox_workspace,
                           sp_prox_prepare_size, sp_ddrm_workspace) is 0 and every `work` and the
                           q of the prox and DDRM entries may be NULL; sp_pgdm_prepare writes
                           nothing and returns SP_OK, and sp_pgdm_residual_ws takes y as its q */
};

/* Forward-operator descriptor.  Device arrays are owned by the caller
 * (the Python Operator's buffers) and must outlive every call using them. */
typedef struct sp_op {
    int32_t kind;
    int32_t channels, height, width; /* x_shape = (C, H, W); n = C*H*W        */
    int64_t n;                       /* elements per x sample                 */
    int64_t m;                       /* elements per y sample                 */
    const uint64_t* keep_bits;       /* INPAINT: ceil(n/64) words; bit (j%64) of
                                        word j/64 set <=> x[j] observed (= ~mask) */
    const int32_t* word_rank;        /* INPAINT: observed count before word w.
                                        HADAMARD: both over one plane's n_p
                                        coefficients, shared by the channels      */
    const float* taps;               /* BLUR: 2*radius+1 normalised taps.  PSF: the
                                        dense row-major (2*radius+1)^2 taps, used
                                        as given (any finite values).  PSF_FFT: the
                                        PSF's spectrum, 2*(Nw/2+1)*Nh floats:
                                        Hs[kw][kh] = sum_{u,v} h[u][v] *
                                        exp(-2 pi i (u kh / Nh + v kw / Nw)) over the
                                        (2*radius+1)^2 taps h (row u, column v),
                                        unnormalised, computed in fp64 and rounded to
                                        fp32, as (re, im) pairs at
                                        taps[2*(kw*Nh + kh)], 0 <= kw <= Nw/2,
                                        0 <= kh < Nh.  PSF_PERIODIC: two such half
                                        spectra back to back with Nh = height,
                                        Nw = width, 2*2*(width/2+1)*height floats:
                                        first M = conj(FFT2 of h with its centre tap
                                        at [0][0], tap (u, v) at ((u-R) mod H,
                                        (v-R) mod W)), the multiplier of A; then
                                        P = 1/M on the kept frequencies and 0 on the
                                        others, the multiplier of A^+.  P must be
                                        conjugate-symmetric under k -> -k like M (a
                                        symmetric kept set).  SR_PERIODIC: M (tap
                                        (u, v) at ((u-P) mod H, (v-P) mod W)) and P in
                                        that layout, then Lambda_t as plain fp32
                                        [width/2+1][height], 5*(width/2+1)*height floats
                                        in all.  With s = factor, on the (H/s, W/s)
                                        grid Lambda[kh][kw] = (1/s^2) sum_{a,b<s}
                                        |M[kh + a H/s][kw + b W/s]|^2; Lambda_t is
                                        Lambda tiled s x s to H x W, and P =
                                        conj(M) / Lambda_t where sqrt(Lambda) exceeds
                                        the caller's threshold, 0 elsewhere (tiled
                                        alike).  All computed in fp64 by the caller
                                        and rounded to fp32.  RADON: 4*radius floats,
                                        one row (alpha, beta, length, axis) per angle
                                        theta: axis 0 (|cos| >= |sin|): (1/cos,
                                        -sin/cos, 1/|cos|, 0), ray s crosses image row
                                        i at column alpha*(s - (factor-1)/2) +
                                        (beta*(i - (height-1)/2) + (width-1)/2); axis
                                        1: (1/sin, -cos/sin, 1/|sin|, 1), rows and
                                        columns swapped.  y[a][s] = length * the sum
                                        over the rows (columns) of the image linearly
                                        interpolated at the crossing, 0 off the image.
                                        The map is defined by these fp32 values taken
                                        as exact; the library does not read them on
                                        the host.  Preconditions: |alpha| >= 1,
                                        |beta| <= 1, length finite, axis 0 or 1 (other
                                        values stay in bounds, the result is then
                                        unspecified).  SVD_SEPARABLE: six row-major
                                        tables back to back, H*H + W*W + Hy*Hy +
                                        Wy*Wy + 2*Hy*Wy floats: V_H[H][H] and
                                        V_W[W][W], full orthogonal, column c the c-th
                                        right singular vector of A_H (A_W) by
                                        descending singular value, the null-space
                                        completion after them; U_H[Hy][Hy] and
                                        U_W[Wy][Wy], orthogonal, column c the c-th
                                        left singular vector; S[Hy][Wy] = s_H[i] *
                                        s_W[j]; P[Hy][Wy] = 1 / S on the kept set, 0
                                        elsewhere.  Computed in fp64 by the caller
                                        and rounded to fp32; the map is defined by
                                        these fp32 tables taken as exact, the library
                                        does not read them on the host.  CHANNEL_MIX:
                                        six row-major tables back to back, 2*C*Cy +
                                        Cy*Cy + C*C + 2*Cy floats, with M = U S V^T the
                                        SVD of the matrix: M[Cy][C]; N[C][Cy] = A^+ =
                                        V diag(P) U^T; U[Cy][Cy], orthogonal, column j
                                        the j-th left singular vector; V[C][C], full
                                        orthogonal, column j the j-th right singular
                                        vector by descending singular value, the
                                        null-space completion after them; S[Cy]; P[Cy]
                                        = 1 / S on the kept set, 0 elsewhere.  A and A^T
                                        are evaluated from M, A^+ and A^+T from N, the
                                        proximal map and the DDRM step from U, V, S, P.
                                        Computed in fp64 by the caller and rounded to
                                        fp32; the map is defined by these fp32 tables
                                        taken as exact, the library does not read them
                                        on the host                                  */
    int32_t radius;                  /* BLUR: 1..8.  PSF: 1..30.  PHASE: pad_h >= 0,
                                        zero rows added above and below.  PSF_FFT:
                                        1..min(height, width) - 1.  PSF_PERIODIC:
                                        1..(min(height, width) - 1) / 2.  SR_PERIODIC:
                                        the taps per axis K, factor..min(height,
                                        width), K - factor even.  RADON: the
                                        number of angles, 1..512.  SVD_SEPARABLE: Hy,
                                        the rows of y, 1..height.  CHANNEL_MIX: Cy, the
                                        channels of y, 1..channels               */
    int32_t factor;                  /* SR, SR_PERIODIC: 2, 4 or 8.  PHASE: pad_w >= 0, zero
                                        columns added left and right.  PSF_FFT: the
                                        boundary: 0 reflect, 1 circular, 2 zeros (0
                                        for the other kinds).  RADON: the number of
                                        detector bins, 1..1024.  SVD_SEPARABLE: Wy, the
                                        columns of y, 1..width (keep_bits and
                                        word_rank NULL).  PHASE: keep_bits,
                                        word_rank and taps must be NULL; PSF_FFT
                                        PSF_PERIODIC and SR_PERIODIC: keep_bits and word_rank;
                                        RADON: keep_bits and word_rank too       */
} sp_op;

/* Scalars of one DPS step (all fp32, computed on the host exactly as the
 * reference computes them). */
typedef struct sp_dps_coefs {
    float a;          /* sqrt(alpha_bar[t])      networks/base.py:41-43          */
    float k;          /* sqrt(1 - alpha_bar[t])                                   */
    float grad_scale; /* d logp / d(Ax): 1/sigma^2 (noise.py:77-79) or
                         2/(rate+1e-3) (noise.py:121-123)                          */
    float c_ell;      /* bridge_coeff_ell        bridge_kernels.py:36            */
    float c_s;        /* bridge_coeff_s          bridge_kernels.py:37            */
    float std;        /* bridge_std              bridge_kernels.py:33-35         */
    float gamma;      /* DPS step size           dps.py:121                      */
    float norm_eps;   /* 1e-9                    dps.py:121                      */
} sp_dps_coefs;

/* Scalars of the epsilon-form DDIM step (bridge_kernels.py:82-115), fp32 as there. */
typedef struct sp_eps_coefs {
    float sqrt_oma;    /* sqrt(1 - acp_t)                                   */
    float oma;         /* 1 - acp_t                  (pseudo-x0)            */
    float sqrt_a;      /* sqrt(acp_t)                                       */
    float sqrt_a_prev; /* sqrt(acp_prev)                                    */
    float sigma;       /* eta*sqrt(clamp((1-acp_prev)/(1-acp_t)*(1-acp_t/acp_prev)))      */
    float dir;         /* sqrt(clamp(1 - acp_prev - sigma^2))                */
} sp_eps_coefs;

/* One torch.optim.AdamW step (resample_kernels.py:32-93 optimisers). */
typedef struct sp_adamw_coefs {
    float decay;      /* 1 - lr*weight_decay                                 */
    float beta1;      /* 0.9                                                 */
    float beta2;      /* 0.999                                               */
    float eps;        /* 1e-8                                                */
    float step_size;  /* lr / (1 - beta1^step)                               */
    float bc2_sqrt;   /* sqrt(1 - beta2^step)                                */
} sp_adamw_coefs;

/* Kernel timing (instrumentation, off by default).  While enabled, every
 * sp_dps_residual / sp_dps_update launch gets a start/stop hipEvent pair attached
 * to its dispatch packet (hipExtLaunchKernel), i.e. the kernel's own execution
 * interval.  sp_timing_collect waits for the recorded launches, writes up to
 * max_records (kind, milliseconds) pairs — kind 1 = residual pass, 2 = update
 * pass — clears the log and returns the number written. */
int sp_timing_enable(int on);
int sp_timing_collect(int32_t* kinds, float* ms, int max_records);
/* As sp_timing_collect, plus each launch's algorithmic work: samples for kinds 1-2 (DPS
 * passes), FLOPs for kinds 3-4 (sp_conv3x3_fwd / _bwd_input: 18*N*Cin*Cout*H*W) and
 * executed MFMA FLOPs for kinds 5-6 (sp_wino3x3_fwd / _bwd_input: 8*N*Cin*Cout*H*W) and FLOPs
 * for kind 7 (sp_conv3x3_bf16, forward or input VJP: 18*N*Cin*Cout*H*W). */
int sp_timing_collect_work(int32_t* kinds, float* ms, double* work, int max_records);

/* Library / ABI version (major*10000 + minor*100 + patch). */
int sp_version(void);
/* Text of the last launch error on this thread ("" if none). */
const char* sp_last_error(void);

/* Bounds-checked debug build (`make debug` -> samplers_amd/lib/debug/libsamplers_hip.so,
 * -DSP_DEBUG=1; SURVEY.md §5 "race detection / sanitizers"): the kernels' index / range
 * invariants (SP_DCHECK) are checked on the device and counted.  No reference counterpart
 * (the reference has no native code); test and diagnosis tooling.
 *   sp_debug_build       1 in the debug library, 0 in the release one.
 *   sp_debug_violations  waits for the device, returns the number of violated checks since the
 *                        last reset (0 in the release build, < 0 on error); *first_site
 *                        (nullable) = (source file id << 16) | line of the first one.
 *   sp_debug_selftest    debug build: one launch whose 64 threads each violate a check (no
 *                        memory access), to prove the counting works; SP_EINVAL otherwise. */
int sp_debug_build(void);
int64_t sp_debug_violations(int32_t reset, int32_t* first_site);
int sp_debug_selftest(sp_stream_t stream);

/* Number of per-sample partial sums written by sp_dps_residual for `op`
 * (callers allocate batch * sp_rsq_partials(op) floats).  SR: the tiles per sample of its
 * residual pass.  SP_EINVAL for a descriptor the library rejects (SR: factor not 2 / 4 / 8,
 * channels * height * width != n, a spatial size not divisible by the factor, or
 * m * factor^2 != n).  PSF: the 32 x 64 tiles per sample of its residual launch; rejected
 * unless taps != NULL, 1 <= radius <= 30, m == n == channels * height * width and
 * height, width > 2 * radius.  PHASE: the column tiles per sample of its column launch
 * (csrc/sp_phase.hip); rejected unless radius, factor >= 0, both padded sizes are 2^k or 3*2^k in
 * [8, 1024], n == channels*height*width, m == channels*Nh*Nw and keep_bits, word_rank and taps
 * are NULL.  PSF_FFT: the row tiles per sample of its fused rows^-1 + rows launch
 * (csrc/sp_psf_fft.hip); rejected unless taps != NULL, factor is 0, 1 or 2,
 * 1 <= radius <= min(height, width) - 1, height + 2*radius <= 1024, width + 2*radius <= 1024,
 * m == n == channels*height*width and keep_bits and word_rank are NULL.  PSF_PERIODIC: the same
 * count with Nw = width; rejected unless taps != NULL, factor == 0, height and width are each 2^k
 * or 3*2^k in [8, 1024], radius >= 1, 2*radius + 1 <= min(height, width),
 * m == n == channels*height*width and keep_bits and word_rank are NULL.  SR_PERIODIC: the tiles
 * of min(lines of a width-point transform, height / factor) lattice rows per sample of its fused
 * launch; rejected unless taps != NULL, factor is 2, 4 or 8 and divides height and width, each 2^k
 * or 3*2^k in [8, 1024], factor <= radius <= min(height, width), radius - factor even,
 * n == channels*height*width, m * factor^2 == n and keep_bits and word_rank are NULL.  RADON: the
 * workgroups per sample of its project launch, channels * radius * ceil(factor / 256) (csrc/sp_radon.hip);
 * rejected unless taps != NULL, 1 <= radius <= 512, 1 <= factor <= 1024, 8 <= height, width <= 512,
 * n == channels*height*width, m == channels*radius*factor and keep_bits and word_rank are NULL.
 * SVD_SEPARABLE: the 64 x 64 tiles of the observed grid per sample, channels * ceil(Hy / 64) *
 * ceil(Wy / 64) (csrc/sp_svd_sep.hip); rejected unless taps != NULL, 2 <= height, width <= 512,
 * 1 <= radius (Hy) <= height, 1 <= factor (Wy) <= width, n == channels*height*width,
 * m == channels*Hy*Wy and keep_bits and word_rank are NULL.  CHANNEL_MIX: the tiles of 256 pixel
 * groups per sample (csrc/sp_chanmix.hip; four pixels to a group where height*width % 4 == 0, else
 * one); rejected unless taps != NULL, 1 <= radius (Cy) <= channels <= 8, factor == 0, height, width
 * >= 1, height*width < 2^31, n == channels*height*width, m == radius*height*width and keep_bits and
 * word_rank are NULL. */
int64_t sp_rsq_partials(const sp_op* op);
/* Floats of `work` that sp_dps_residual_ws / _sched_ws need for `batch` samples of `op`:
 * 0 for every kind but those below (one pass, no workspace), batch * m for PSF (its residual launch
 * leaves grad_scale * r there for the adjoint launch), 2 * batch * channels * Nw * height for
 * PHASE (the complex row transforms, stored transposed), 2 * batch * channels * (Nw/2 + 1) * height
 * for PSF_FFT (the same, half the spectrum: the rows are real) and for PSF_PERIODIC and SR_PERIODIC
 * (Nw = width),
 * batch * m for RADON (grad_scale * r in sinogram space, between project and backproject),
 * 3 * batch * n for SVD_SEPARABLE (two intermediates of the per-side products and T_y(y)).  SP_EINVAL for a rejected
 * descriptor or batch <= 0.  The library allocates nothing. */
int64_t sp_dps_workspace(const sp_op* op, int64_t batch);
/* Floats of `work` that sp_op_apply_ws / sp_op_vjp_ws need: 0 for the linear kinds, the figure
 * of sp_dps_workspace for PHASE, PSF_FFT, PSF_PERIODIC and SR_PERIODIC (sp_op_pinv_ws and
 * sp_pgdm_residual_ws take the same), 2 * batch * n for SVD_SEPARABLE (two intermediates; the
 * same for sp_op_pinv_ws, sp_pgdm_residual_ws and the proximal entries).  SP_EINVAL for a rejected
 * descriptor or batch <= 0. */
int64_t sp_op_workspace(const sp_op* op, int64_t batch);

/* What the kind of `op` does at the entry points below, as bits; 0 for a rejected descriptor.
 * A caller branches on these instead of listing kinds (no reference counterpart). */
enum {
    SP_TRAIT_UPDATE_READS_V = 1, /* sp_dps_update requires v (it cannot re-derive it)          */
    SP_TRAIT_DPS_WORKSPACE = 2,  /* sp_dps_workspace > 0: pass 1 runs in the _ws forms only    */
    SP_TRAIT_FUSED_LATENT = 4,   /* sp_psld_pixel and sp_pixel_opt_step exist for the kind     */
    SP_TRAIT_LINEAR = 8,         /* sp_op_apply / sp_op_adjoint exist (else _apply_ws/_vjp_ws) */
    SP_TRAIT_NEEDS_ATA_U = 16,   /* sp_psld_cotangent requires ata_u                           */
    SP_TRAIT_PINV = 32           /* sp_op_pinv_ws, sp_pgdm_prepare, sp_pgdm_residual_ws exist  */
};
uint32_t sp_op_traits(const sp_op* op);

/* DPS pass 1 — replaces dps.py:99-103 up to the prior's VJP and dps.py:117-118:
 *   x0  = (x - k*eps)/a                         (networks/base.py:41-43)
 *   r   = y - A(x0)                             (inverse_problem.py:17-18)
 *   v   = A^T(grad_scale * r)  -> v_out         (autograd of noise.log_prob through A)
 *   rsq_partial[b][p] = partial sums of r^2 over sample b (dps.py:117-120).
 * v_out is the cotangent of x0; the caller feeds it to the prior's VJP.
 * SR: one pass over the factor x factor blocks, v = (grad_scale / factor^2) * r replicated
 * over each block; one partial per tile of the pass (sp_rsq_partials). */
int sp_dps_residual(const sp_op* op, const float* x, const float* eps, const float* y,
                    int64_t batch, int64_t y_div, const sp_dps_coefs* c,
                    float* v_out, float* rsq_partial, sp_stream_t stream);
/* The same with a workspace (sp_dps_workspace floats; NULL where that is 0, and then exactly
 * sp_dps_residual).  PSF runs here only (sp_dps_residual / _sched return SP_EUNSUPPORTED for
 * it), as two launches: `residual` forms x0 while staging its tile, writes
 * work = grad_scale * (y - A x0) and one |r|^2 partial per tile, `adjoint` gathers
 * v = A^T work (csrc/sp_psf.hip).  PHASE runs here only too, as three launches
 * (csrc/sp_phase.hip): row FFTs of x0 -> work; per column tile the forward column FFT,
 * r = y - |z|, one r^2 partial, u = grad_scale * r * z/|z| (0 at |z| = 0) and the inverse column
 * FFT, in LDS, back into work; inverse row FFTs, real part, crop -> v = J(x0)^T(grad_scale * r).
 * PSF_FFT runs here only as well, as five launches (csrc/sp_psf_fft.hip): row FFTs of the extended
 * x0 -> work; per column tile the forward column FFT, times conj(spectrum), inverse column FFT;
 * per row tile the inverse row FFT, g = grad_scale * (y - A x0), one r^2 partial and the forward
 * row FFT of g; the column launch again with the spectrum and the fold; inverse row FFTs and the
 * fold -> v = A^T g.  PSF_PERIODIC: the same five launches on exact-size transforms (Nh = height,
 * Nw = width), nothing extended or folded.  SR_PERIODIC: five launches too: row FFTs of x0; the
 * column launch with M, which stores the height / factor lattice rows alone; per tile of lattice
 * rows the inverse row FFT, g = grad_scale * (y - A x0) on the lattice columns, one r^2 partial,
 * g zero-inserted along the row and transformed forward; the column launch that inserts the zero
 * rows in LDS, with conj(M); inverse row FFTs -> v = A^T g.  SVD_SEPARABLE runs here only too, as
 * six launches of one per-plane product kernel on the fp32-input MFMA (csrc/sp_svd_sep.hip):
 * U_H^T y and its product with U_W -> yhat = T_y(y) per observation row; V_H[:, :Hy]^T x0 (x0 formed in
 * the loads); its product with V_W[:, :Wy] with the epilogue r = yhat - S d, one r^2 partial per
 * 64 x 64 tile, g = grad_scale * (S r) (U is orthogonal, so |y - A x0| = |r|); V_H[:, :Hy] g; its
 * product with V_W[:, :Wy]^T -> v = A^T(grad_scale (y - A x0)).  RADON runs here only too, as two launches
 * (csrc/sp_radon.hip): `project` forms x0 while it stages its slab of the plane, sums every ray in
 * row (column) order, writes work = grad_scale * (y - A x0) and one |r|^2 partial per workgroup;
 * `backproject` gathers v = A^T work per pixel, angles in order.  The result has the same bits on
 * every run and for a sample in any batch.
 * work must not alias any other argument. */
int sp_dps_residual_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                       int64_t batch, int64_t y_div, const sp_dps_coefs* c,
                       float* v_out, float* rsq_partial, float* work, sp_stream_t stream);

/* DPS pass 2 — replaces dps.py:106-122 (ddim_step -> sample_bridge_kernel and
 * the guidance correction):
 *   g   = v/a - (k/a) * w          (w = J_eps^T v from the prior's VJP)
 *   x'  = c_ell*x + c_s*x0 + std*xi + gamma/(sqrt(sum_p rsq_partial[b][p]) + norm_eps) * g
 * v: pass NULL to recompute v from (x, eps, y) (IDENTITY/INPAINT/MASK), else
 *    the buffer written by sp_dps_residual (required for BLUR, SR, PSF, PHASE, PSF_FFT, PSF_PERIODIC and RADON, which run the
 *    identity-kind update over it: the Philox element index stays the flat element index).
 * rsq_partial: NULL selects a fixed factor, x' = ... + gamma * g — the PGDM update
 *    (pgdm.py:126-135, gamma = -guidance_weight*sqrt(1-acp_t), v = -2 A^T r) and the
 *    PSLD update (psld.py:144-153, gamma = -1, v = the latent cotangent).
 * xi: injected standard-normal noise (B*n) or NULL to draw Philox4x32-10
 *    normals keyed by (seed, step, sample_offset + b, element) — invariant to
 *    how the batch is sharded across GPUs.  x_out may alias x. */
int sp_dps_update(const sp_op* op, const float* x, const float* eps, const float* y,
                  const float* v, const float* w, const float* rsq_partial, const float* xi,
                  uint64_t seed, int64_t step, int64_t sample_offset,
                  int64_t batch, int64_t y_div, const sp_dps_coefs* c,
                  float* x_out, sp_stream_t stream);

/* x0 = (x - k*eps)/a over `count` elements (networks/base.py:41-43; final
 * prediction dps.py:125-126). out may alias x. */
int sp_predict_x0(const float* x, const float* eps, int64_t count, float a, float k,
                  float* out, sp_stream_t stream);

/* Standard normals, Philox4x32-10 keyed by (seed, step, sample_offset+b, j);
 * replaces torch.randn / randn_like (dps.py:83-87, bridge_kernels.py:59). */
int sp_randn(float* out, int64_t batch, int64_t n, uint64_t seed, int64_t step,
             int64_t sample_offset, sp_stream_t stream);

/* y = A x (operators/base.py:91-92; linear.py:141-152; inpainting.py:132-145).  SR: the block
 * means, each block summed in the fixed order documented in csrc/sp_sr.hip.  PSF: the
 * reflect-padded correlation, every pixel summed tap row by tap row over the rows' non-zero
 * spans (csrc/sp_psf.hip).  RADON: the line integrals, every ray summed in row (column) order
 * (csrc/sp_radon.hip). */
int sp_op_apply(const sp_op* op, const float* x, float* y, int64_t batch, sp_stream_t stream);
/* x = A^T y (linear.py:154-165; inpainting.py:169-187).  SR: y / factor^2 replicated over
 * each block (exact); the pseudo-inverse is factor^2 times this.  PSF: a gather (no atomics):
 * the zero-extended correlation plus the fold terms of the reflect padding, in a fixed order.
 * RADON: a gather per pixel over the <= 2 rays per angle that touch it, with the weights of
 * sp_op_apply bit for bit, angles in order. */
int sp_op_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, sp_stream_t stream);
/* y = A(x) with a workspace of sp_op_workspace floats: sp_op_apply for the linear kinds (work
 * unused, may be NULL); PHASE: y = |FFT2(pad(x))| (sp_op_apply and sp_op_adjoint return
 * SP_EUNSUPPORTED for PHASE, as do sp_psld_pixel, sp_psld_cotangent and sp_pixel_opt_step);
 * PSF_FFT: y = A x, the extended correlation (the same entries return SP_EUNSUPPORTED for it);
 * PSF_PERIODIC: y = A x = Re IFFT2(FFT2(x) * M), likewise; SR_PERIODIC: the lattice
 * [::factor, ::factor] of that, y of m = n / factor^2 (the column launch stores the lattice rows
 * alone, the inverse-row launch transforms those and stores the lattice columns). */
int sp_op_apply_ws(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                   sp_stream_t stream);
/* dx = J(x)^T g for the nonlinear kinds (g: batch rows of m, dx: batch rows of n).  PHASE:
 * crop(Re(IFFT2(g * z/|z|))) with z = FFT2(pad(x)) recomputed, z/|z| = 0 at |z| = 0 (never NaN
 * or inf).  PSF_FFT: dx = A^T g, the exact adjoint (x is not read); PSF_PERIODIC the same, with
 * the multiplier conj(M); SR_PERIODIC: dx = Re IFFT2(FFT2(up g) * conj(M)), up the zero insertion
 * onto the lattice (only the lattice rows are read and row-transformed; the column launch inserts
 * the zero rows in LDS).  SVD_SEPARABLE: sp_op_apply_ws is y = U_H (S * (V_H^T x V_W)[:Hy, :Wy])
 * U_W^T and sp_op_vjp_ws its exact transpose dx = V_H[:, :Hy] (S * (U_H^T g U_W)) V_W[:, :Wy]^T, four
 * launches each (one per side and transform, the multiplier in the second one's epilogue).
 * SP_EUNSUPPORTED for the
 * linear kinds without a workspace, whose VJP is sp_op_adjoint. */
int sp_op_vjp_ws(const sp_op* op, const float* x, const float* g, float* dx, int64_t batch,
                 float* work, sp_stream_t stream);

/* The kinds with SP_TRAIT_PINV (PSF_PERIODIC, SR_PERIODIC, SVD_SEPARABLE, HADAMARD: A^+ = A^T, q = y); SP_EUNSUPPORTED for every other kind, SP_EINVAL
 * for a rejected descriptor or argument first.  No reference counterpart: the reference's
 * SVDOperator.apply_pseudo_inverse (linear.py) is the dense form of the same map.
 *   sp_op_pinv_ws        x = A^+ y = Re IFFT2(FFT2(y) * P) (transpose = 0) or A^+T y (transpose =
 *                        1, multiplier conj(P)): rows, columns, rows^-1 through `work`
 *                        (sp_op_workspace floats), three launches.
 *   sp_pgdm_prepare      q = P * FFT2(y) / (H W) for each of `rows` observation rows, as (re, im)
 *                        pairs [row][channels][width/2 + 1][height] (the intermediate's layout);
 *                        q is the caller's, 2 * rows * channels * (width/2 + 1) * height floats.
 *                        Two launches.  Once per sampler call: y is fixed across its steps.
 *   sp_pgdm_residual_ws  PGDM pass 1 (pgdm.py:104-119 up to the prior's VJP):
 *                          x0 = (x - k*eps)/a,  v = grad_scale * (A^+ y - A^+ A x0) -> v_out
 *                        which with grad_scale = -2 is the gradient of |A^+ y - A^+ A x0|^2 in
 *                        x0 (A^+ A is an orthogonal projection).  Three launches: row FFTs of
 *                        x0 -> work; per column tile the forward column FFT,
 *                        z <- grad_scale * (q[b / y_div] - (P != 0 ? z / (H W) : 0)) and the inverse
 *                        column FFT, in LDS; inverse row FFTs, real part -> v.  Sample b uses
 *                        row b / y_div of q.  Pass 2 is sp_dps_update with rsq_partial = NULL.
 * SR_PERIODIC: sp_op_pinv_ws is x = Re IFFT2(FFT2(up y) * P) (y: rows of m, x: rows of n) or, with
 * transpose = 1, the lattice of Re IFFT2(FFT2(y) * conj(P)) (y: rows of n, x: rows of m).
 * sp_pgdm_prepare copies each observation row (m floats) to the head of its row of q (q sized and
 * strided as above: the residual is formed on the lattice, where y is 2 factor^2 times smaller
 * than a spectrum of up y); sp_pgdm_residual_ws is v = grad_scale * A^+ (y - A x0) in the five
 * launches of its DPS pass 1 with P in the second column launch and no partials.
 * SVD_SEPARABLE: sp_op_pinv_ws is the launches of sp_op_vjp_ws (transpose = 0: x = A^+ y) or of
 * sp_op_apply_ws (transpose = 1: A^+T) with P in S's place.  sp_pgdm_prepare writes q = P * T_y(y),
 * T_y(Y) = U_H^T Y U_W, per observation row: q has sp_op_workspace(op, rows) = 2 * rows * n floats,
 * a row every 2 n floats, whose first m floats hold q as [channels][Hy][Wy] and whose next m the
 * launches' intermediate; two launches.  sp_pgdm_residual_ws is
 * v = grad_scale * T^-1[q - K * T(x0)] with T(X) = V_H^T X V_W on the observed grid and K = (P != 0),
 * i.e. grad_scale * (A^+ y - Pi x0), in four launches (the subtraction in the second one's epilogue).
 * CHANNEL_MIX: one launch each and no workspace: sp_op_workspace is 0 and `work` may be NULL in
 * sp_op_pinv_ws and sp_pgdm_residual_ws (for every other kind a NULL work is SP_EINVAL, as before).
 * sp_op_pinv_ws is x[c] = sum_i N[c][i] y[i] per pixel (transpose = 1: y[i] = sum_c N[c][i] x[c]).
 * sp_pgdm_prepare writes nothing and returns SP_OK (q must still be non-null): the residual launch
 * reads the observation rows themselves, so the caller passes y as the q of sp_pgdm_residual_ws,
 * rows of m floats; v = grad_scale * N (y - M x0) per pixel, nothing proportional to the batch is
 * allocated or copied.
 * work and q must not alias any other argument. */
int sp_op_pinv_ws(const sp_op* op, const float* y, float* x, int64_t batch, int32_t transpose,
                  float* work, sp_stream_t stream);
int sp_pgdm_prepare(const sp_op* op, const float* y, int64_t rows, float* q, sp_stream_t stream);
int sp_pgdm_residual_ws(const sp_op* op, const float* x, const float* eps, const float* q,
                        int64_t batch, int64_t y_div, const sp_dps_coefs* c, float* v_out,
                        float* work, sp_stream_t stream);

/* ---- DiffPIR / proximal data step (no reference counterpart: Zhu et al. 2023, semantics in
 * DESIGN.md §3 and tests/prox_ref.py) -------------------------------------------------------
 * The proximal map of the operator at x0 with weight rho > 0,
 *   z = argmin_u |y - A u|^2 + rho |u - x0|^2 = (A^T A + rho I)^-1 (A^T y + rho x0),
 * in closed form for the kinds where it has one (r = y - A x0):
 *   IDENTITY, INPAINT, MASK (A A^T = I)   z = x0 + A^T r / (1 + rho); unobserved pixels keep x0;
 *   SR x s (A A^T = I / s^2)              z = x0 + (r replicated over its block) / (1 + rho s^2),
 *                                         the block mean of x0 in the order of csrc/sp_sr.hip;
 *   PSF_PERIODIC (A = IFFT2 M FFT2)       Z = (conj(M) Y + rho X0) / (|M|^2 + rho), z = Re IFFT2(Z).
 *   SR_PERIODIC (A A^T diagonal, Lambda)  z = x0 + Re IFFT2(FFT2(up r) conj(M) / (Lambda_t + rho)):
 *                                         every frequency divided, not only the kept ones;
 *   SVD_SEPARABLE (A = U S V_obs^T)       Z = (S * T_y(y) + rho T(x0)) / (S^2 + rho) on the observed
 *                                         grid, T(x0) itself outside it (a select), z = T^-1 Z: exact
 *                                         for the full A, every component divided.
 *   CHANNEL_MIX (M = U S V^T per pixel)   z = x0 + V diag(S / (S^2 + rho)) U^T r over all Cy singular
 *                                         values, one launch that reads y (csrc/sp_chanmix.hip).
 * Every other kind: SP_EUNSUPPORTED (after the common argument checks, which answer SP_EINVAL).
 * The scalars are applied as reciprocals computed once per thread (1 / a, 1 / k, 1 / (1 + rho s^2),
 * 1 / (|M|^2 + rho)), as sp_dps_update does.  Plain stores, no atomics; every sample is computed
 * alone, so the bits do not depend on the batch, y_div or the shard. */
typedef struct sp_prox_coefs {
    float a;      /* sqrt(alpha_bar[t])                                       */
    float k;      /* sqrt(1 - alpha_bar[t])                                   */
    float rho;    /* guidance_weight * max(sigma_n, sigma_min)^2 * alpha_bar[t] / (1 - alpha_bar[t]) */
    float a_prev; /* sqrt(alpha_bar[t_prev])                                  */
    float c_eps;  /* sqrt(1 - alpha_bar[t_prev]) * sqrt(1 - zeta)             */
    float c_xi;   /* sqrt(1 - alpha_bar[t_prev]) * sqrt(zeta)                 */
} sp_prox_coefs;  /* 24 bytes */
/* Floats of `work` that sp_op_prox_ws / sp_diffpir_step_ws need for `batch` samples: 0 for the
 * elementwise kinds and SR, the sp_op_workspace figure for PSF_PERIODIC, SR_PERIODIC and SVD_SEPARABLE.  This is the capability
 * probe: SP_EUNSUPPORTED for a valid kind without a closed-form prox, SP_EINVAL for a rejected
 * descriptor or batch <= 0. */
int64_t sp_prox_workspace(const sp_op* op, int64_t batch);
/* Floats of `q` for `rows` observation rows: 0 but for PSF_PERIODIC and SR_PERIODIC,
 * 2 * rows * channels * (width/2 + 1) * height there, and SVD_SEPARABLE, 2 * rows * n (a row every
 * 2 n floats: q = S * T_y(y) in the first m, the launches' intermediate after it).  Codes as
 * sp_prox_workspace. */
int64_t sp_prox_prepare_size(const sp_op* op, int64_t rows);
/* q = conj(M) * FFT2(y) / (H W) per observation row, as (re, im) pairs
 * [row][channels][width/2 + 1][height] (the intermediate's layout): sp_pgdm_prepare's two launches
 * with the multiplier conj(M); SR_PERIODIC: the copy of sp_pgdm_prepare.  Once per sampler call.
 * The kinds whose sp_prox_prepare_size is 0:
 * SP_OK, nothing launched, q may be NULL. */
int sp_prox_prepare(const sp_op* op, const float* y, int64_t rows, float* q, sp_stream_t stream);
/* z_out = prox(x0; y, rho) for `batch` rows of x0, sample b against observation row b / y_div.
 * One launch (elementwise kinds, SR: y read, q and work may be NULL) or three (PSF_PERIODIC: row
 * FFTs of x0 -> work; per column tile z <- (q[b / y_div] + rho z / (H W)) / (|M|^2 + rho) between
 * the transforms; inverse row FFTs, real part -> z_out; q and work required, y not read) or five
 * (SR_PERIODIC: its DPS pass 1 with grad_scale = 1, no partials and conj(M) / (Lambda_t + rho) in
 * the second column launch; the last launch adds x0 in space; q and work required, y not read) or four
 * (SVD_SEPARABLE: V_H^T x0; its product with V_W with the quotient in the epilogue; V_H times that;
 * the product with V_W^T, in the step form with the DiffPIR update and the noise tile in its
 * epilogue; q and work required, y not read).
 * z_out may alias x0; work and q must not alias any other argument. */
int sp_op_prox_ws(const sp_op* op, const float* x0, const float* y, const float* q, int64_t batch,
                  int64_t y_div, float rho, float* z_out, float* work, sp_stream_t stream);
/* The whole guided DiffPIR step after the network call, in the same launches:
 *   x0 = (x - k eps) / a,  z = prox(x0; y, rho),  eps_hat = (x - a z) / k,
 *   x' = a_prev z + (c_eps eps_hat + c_xi xi)
 * xi: injected standard normals (batch * n) or NULL to draw Philox4x32-10 normals keyed as
 * sp_dps_update does, (seed, step, sample_offset + b, flat element index).  x_out may alias x.
 * rho <= 0, a non-finite rho or k == 0: SP_EINVAL. */
int sp_diffpir_step_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                       const float* q, const float* xi, uint64_t seed, int64_t step,
                       int64_t sample_offset, int64_t batch, int64_t y_div,
                       const sp_prox_coefs* coefs, float* x_out, float* work, sp_stream_t stream);

/* ---- the proximal data step by conjugate gradients (csrc/sp_cg.hip; semantics in DESIGN.md §3
 * and tests/prox_cg_ref.py) -----------------------------------------------------------------
 * The same map z = (A^T A + rho I)^-1 (A^T y + rho x0) for EVERY linear kind, the ones without a
 * closed form included, by regularised CGLS in d = z - x0, per sample:
 *   s = y - A x0;  d = 0;  g = A^T s;  p = g;  gamma = |g|^2;  gamma0 = gamma;  iters = 0
 *   max_iter times:
 *     q = A p;  delta = |q|^2 + rho |p|^2
 *     live = gamma > tol^2 gamma0  and  delta > 0  and  gamma, delta finite
 *     live:  alpha = gamma / delta;  d += alpha p;  s -= alpha q;  g = A^T s - rho d;
 *            gamma' = |g|^2;  p = g + (gamma' / gamma) p;  gamma = gamma';  iters += 1
 *     else:  nothing of the sample changes (a select, never a product by 0), so the sample takes
 *            the same decision at every later iteration: stopping is sticky
 *   z = x0 + d
 * The stop is part of the map, not an optimisation: without it gamma reaches rounding level, beta
 * becomes noise and the fp32 recurrence leaves every bound.  y = A x0 gives
 * gamma0 = 0, iters = 0 and z = x0 bit for bit.  A and A^T are the kind's own maps (sp_op_apply /
 * sp_op_adjoint, or sp_op_apply_ws / sp_op_vjp_ws for the kinds whose maps need a workspace).
 * Kinds: IDENTITY, INPAINT, MASK, BLUR, SR, PSF, RADON, PSF_FFT, PSF_PERIODIC, SR_PERIODIC,
 * SVD_SEPARABLE; PHASE
 * (nonlinear): SP_EUNSUPPORTED, after the argument checks.
 * A call is one launch sequence of fixed length, max_iter x (A, A^T and four vector launches; the
 * last iteration three), whatever the samples do: alpha, beta, gamma, delta and iters stay on the
 * device, nothing synchronises with the host, there are no atomics and no grid-wide barriers.
 * Every squared norm is sp_vec_partials(n) (x-space) or sp_vec_partials(m) (y-space) partials per
 * sample summed in a fixed order and every sample is computed alone, so the bits of a sample do
 * not depend on the batch, y_div, the shard or the other samples' stops.
 *
 * sp_prox_cg_workspace: floats of `work` for `batch` samples, step_form 0 (sp_op_prox_cg_ws) or 1
 * (sp_diffpir_step_cg_ws).  With r4(v) = v rounded up to a multiple of 4,
 *   (3 + step_form) * r4(batch * n)                       d, p, A^T s (g in place) [, x0]
 *   + 2 * r4(batch * m)                                   s, q
 *   + r4(batch * (3 * sp_vec_partials(n) + sp_vec_partials(m)))   gamma, gamma0, |p|^2; |q|^2
 *   + 4 * batch                                           gamma, alpha, live, iters per sample
 *   + sp_op_workspace(op, batch)                          the maps' own, last
 * SP_EINVAL for a rejected descriptor, batch <= 0 or > 65535, step_form not 0 / 1;
 * SP_EUNSUPPORTED for PHASE.  The library allocates nothing and writes nothing past that size.
 *
 * sp_op_prox_cg_ws: z_out = the map at x0 (batch rows of n), sample b against observation row
 * b / y_div of y.  iters_out (batch int32, device) receives the live iterations of each sample;
 * it may be NULL.  z_out may alias x0; work aliases nothing.  SP_EINVAL: rho <= 0 or non-finite,
 * max_iter < 1, tol < 0 or non-finite, a null x0 / y / z_out / work, batch <= 0 or > 65535,
 * y_div <= 0, a rejected descriptor.  Rows are 16-byte aligned where n (m) is a multiple of 4, as
 * for every entry.
 *
 * sp_diffpir_step_cg_ws: the whole guided DiffPIR step of sp_diffpir_step_ws with this data step:
 *   x0 = (x - k eps) / a,  z as above,  eps_hat = (x - a z) / k,
 *   x' = a_prev z + (c_eps eps_hat + c_xi xi)
 * with the reciprocals 1 / a and 1 / k taken once, xi injected or NULL for the Philox normals of
 * sp_dps_update / sp_diffpir_step_ws, (seed, step, sample_offset + b, flat element index): the
 * bits of sp_randn.  x_out may alias x.  SP_EINVAL as above, and for a null eps / coefs or
 * k == 0. */
int64_t sp_prox_cg_workspace(const sp_op* op, int64_t batch, int32_t step_form);
int sp_op_prox_cg_ws(const sp_op* op, const float* x0, const float* y, int64_t batch, int64_t y_div,
                     float rho, int32_t max_iter, float tol, float* z_out, int32_t* iters_out,
                     float* work, sp_stream_t stream);
int sp_diffpir_step_cg_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                          const float* xi, uint64_t seed, int64_t step, int64_t sample_offset,
                          int64_t batch, int64_t y_div, const sp_prox_coefs* coefs,
                          int32_t max_iter, float tol, float* x_out, int32_t* iters_out,
                          float* work, sp_stream_t stream);

/* ---- DDRM / spectral step (no reference counterpart: Kawar et al. 2022, eq. 7-8 in the VP
 * variables; semantics in DESIGN.md §3 and tests/ddrm_ref.py) --------------------------------
 * With A = U S V^T, x0 = (x - k eps) / a and ybar = S^+ U^T y, every spectral component of the
 * next sample is set by the class of its singular value s (sig_prev = sqrt(1 - abar') / sqrt(abar'),
 * c1 = sqrt(1 - eta^2)):
 *   unobserved (s = 0 or outside the kept set)   f_th = 1, f_eps = c1 sig_prev, f_y = 0, f_xi = eta sig_prev
 *   observed, small (sig_prev s < sig_y)         f_th = 1 - r, f_y = r = c1 sig_prev s / sig_y, f_xi = eta sig_prev
 *   observed, big   (sig_prev s >= sig_y)        f_th = 1 - eta_b, f_y = eta_b,
 *                                                f_xi = sqrt(max(sig_prev^2 - eta_b^2 sig_y^2 / s^2, 0))
 *   x' = a_prev V [f_th V^T x0 + f_eps V^T eps + f_y ybar + f_xi V^T xi],  xi ~ N(0, I) in space.
 * The class is the one fp32 expression (sig_prev * sig_prev) * s2 >= sig_y * sig_y with
 * s2 = re * re + im * im of the multiplier M (PSF_PERIODIC) or the kind's constant (1; SR: 1 / factor^2),
 * every operation rounded on its own: no division, no square root, no contraction.  The kinds:
 *   IDENTITY, INPAINT, MASK (A A^T = I)  one launch; an observed element is f_th x0 + f_y y + f_xi xi,
 *                                        an unobserved one x0 + c1 sig_prev eps + eta sig_prev xi;
 *   SR x s (A A^T = I / s^2)             one launch, the projector form: with mean() the block mean
 *                                        in the order of csrc/sp_sr.hip,
 *        x' / a_prev = x0 + c1 sig_prev eps + eta sig_prev xi + (f_th - 1) mean(x0)
 *                      - c1 sig_prev mean(eps) + (f_xi - eta sig_prev) mean(xi) + f_y y;
 *   PSF_PERIODIC (V^T = FFT2)            three launches through work: row transforms of x0, eps and
 *                                        xi (drawn while staging); per column tile the three column
 *                                        transforms, F = f_th X0 + f_eps E + f_xi Xi + f_y q
 *                                        (s = |M| where P != 0, unobserved elsewhere; q as
 *                                        sp_pgdm_prepare writes it), one inverse column transform;
 *                                        inverse rows, real part, times a_prev.
 *   SVD_SEPARABLE (V^T = T)              four launches through work: V_H^T of x0, eps and xi (read, or
 *                                        drawn by Philox in the loads) in one launch; their products
 *                                        with V_W with F = f_y q + f_th X0 + f_eps E + f_xi Xi in the
 *                                        epilogue (s = S where P != 0 on the observed grid, unobserved
 *                                        elsewhere; q as sp_pgdm_prepare writes it); V_H F; its product
 *                                        with V_W^T times a_prev.
 * Every other kind: SP_EUNSUPPORTED.  1 / a is taken once per thread.  Plain stores, no atomics;
 * every sample is computed alone, so the bits do not depend on the batch, y_div or the shard. */
typedef struct sp_ddrm_coefs {
    float a;        /* sqrt(alpha_bar[t])                                      */
    float k;        /* sqrt(1 - alpha_bar[t])                                  */
    float a_prev;   /* sqrt(alpha_bar[t_prev])                                 */
    float sig_prev; /* sqrt(1 - alpha_bar[t_prev]) / sqrt(alpha_bar[t_prev])   */
    float sig_y;    /* observation noise std, >= 0                             */
    float eta;      /* in [0, 1]                                               */
    float eta_b;    /* in [0, 1]                                               */
    float c1;       /* sqrt(1 - eta^2), computed in fp64 by the caller         */
} sp_ddrm_coefs;    /* 32 bytes */
/* Floats of `work` that sp_ddrm_step_ws needs for `batch` samples: 0 for the one-launch kinds,
 * three intermediates (3 * sp_op_workspace) for PSF_PERIODIC, 4 * batch * n for SVD_SEPARABLE (the
 * three transformed sources and the combined spectrum).  This is the capability probe:
 * SP_EUNSUPPORTED for a valid kind without a DDRM step (BLUR, PSF, PHASE, PSF_FFT, RADON,
 * SR_PERIODIC), SP_EINVAL for a rejected descriptor or batch <= 0. */
int64_t sp_ddrm_workspace(const sp_op* op, int64_t batch);
/* The whole DDRM step after the network call.  q: PSF_PERIODIC and SVD_SEPARABLE read what
 * sp_pgdm_prepare wrote (P FFT2(y) / (H W), or P T_y(y); row b / y_div) and not y; the one-launch kinds read y and q may be NULL.
 * xi: injected standard normals (batch * n) or NULL to draw the Philox normals of sp_randn,
 * (seed, step, sample_offset + b, flat element index).  x_out may alias x; work aliases nothing.
 * SP_EINVAL: a null x, eps, coefs or x_out; a null y (or q) or work where it is read; batch <= 0
 * or > 65535; y_div <= 0; a == 0; eta or eta_b outside [0, 1]; a negative or non-finite sig_y or
 * sig_prev. */
int sp_ddrm_step_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                    const float* q, const float* xi, uint64_t seed, int64_t step,
                    int64_t sample_offset, int64_t batch, int64_t y_div,
                    const sp_ddrm_coefs* coefs, float* x_out, float* work, sp_stream_t stream);

/* Likelihood gradient in y-space (noise.py:19-27 score, 77-79, 121-123):
 *   r = y[b/y_div] - z[b];  g[b] = grad_scale * r;  rsq_partial[b][p] += r^2 partials.
 * g may be NULL (norm only).  Partials per sample: sp_vec_partials(m). */
int64_t sp_vec_partials(int64_t count);
int sp_residual_grad(const float* y, const float* z, int64_t batch, int64_t m, int64_t y_div,
                     float grad_scale, float* g, float* rsq_partial, sp_stream_t stream);

/* ---- latent samplers (PSLD psld.py:118-153, ReSample resample.py:131-228) ---------- */

/* PSLD pixel pass for IDENTITY / INPAINT / MASK / SR (BLUR and PSF, the kinds with a halo,
 * return SP_EUNSUPPORTED: the caller composes it from sp_op_apply / sp_op_adjoint):
 *   r = y - A x0,  x_eff = A^T y + x0 - A^T A x0,  atr = A^T r,
 *   rsq_partial[b][p] = partial sums of r^2 (sp_rsq_partials(op) per sample). */
int sp_psld_pixel(const sp_op* op, const float* x0, const float* y, int64_t batch, int64_t y_div,
                  float* x_eff, float* atr, float* rsq_partial, sp_stream_t stream);
/* out[0] = sum of count partials (one workgroup, fixed order; a device scalar). */
int sp_sum_partials(const float* partials, int64_t count, float* out, sp_stream_t stream);
/* out = alpha*a + beta/sqrt(*norm_sq)*b  (a may be NULL; norm_sq NULL means 1; a zero norm
 * gives 0, as torch's norm backward).  Gluing-term cotangents of psld.py:138-141. */
int sp_scaled_combine(const float* a, float alpha, const float* b, float beta, const float* norm_sq,
                      int64_t count, float* out, sp_stream_t stream);
/* c_x0 = -omega * atr / sqrt(*norm_sq) + (I - A^T A) u   (ata_u = A^T A u, BLUR and PSF only,
 * required there; SR
 * computes A^T A u = the block mean of u / factor^2 in the kernel, ata_u may be NULL). */
int sp_psld_cotangent(const sp_op* op, const float* atr, const float* u, const float* ata_u,
                      const float* norm_sq, float omega, int64_t batch, float* out,
                      sp_stream_t stream);
/* epsilon-form DDIM step: x_prev = sqrt_a_prev*x0 + dir*eps + sigma*xi, x0 and pseudo-x0;
 * any output may be NULL; xi NULL = Philox(seed, step, sample_offset+b). */
int sp_ddim_eps_step(const float* x, const float* eps, int64_t batch, int64_t n,
                     const sp_eps_coefs* c, const float* xi, uint64_t seed, int64_t step,
                     int64_t sample_offset, float* x_prev, float* x0, float* pseudo_x0,
                     sp_stream_t stream);
/* ReSample stochastic resample (resample_kernels.py:96-107), a_t / sigma scalars. */
int sp_stochastic_resample(const float* pseudo_x0, const float* x_t, int64_t batch, int64_t n,
                           float a_t, float sigma, const float* xi, uint64_t seed, int64_t step,
                           int64_t sample_offset, float* out, sp_stream_t stream);
/* In-place AdamW update of `count` parameters. */
int sp_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  int64_t count, const sp_adamw_coefs* c, sp_stream_t stream);
/* The same with a device-side stop flag: no-op once *stop != 0. */
int sp_adamw_step_until(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        int64_t count, const sp_adamw_coefs* c, const int32_t* stop,
                        sp_stream_t stream);
/* One iteration of ReSample's pixel-space hard data consistency (resample_kernels.py:32-54:
 * AdamW(lr=1e-2) on MSELoss(y, A x)) for IDENTITY / INPAINT / MASK / SR in one pass over x:
 *   r = y[b/y_div] - A x,  g = A^T(grad_scale * r)  (grad_scale = -2/M, M = elements of the
 *   MSE mean), AdamW update of x / exp_avg / exp_avg_sq in place, r^2 partials
 *   (sp_rsq_partials(op) per sample) of the loss at x before the update.
 * No-op once *stop != 0 (stop may be NULL).  BLUR and PSF: SP_EUNSUPPORTED (the caller composes
 * sp_op_apply / sp_residual_grad / sp_op_adjoint / sp_adamw_step_until). */
int sp_pixel_opt_step(const sp_op* op, float* x, float* exp_avg, float* exp_avg_sq,
                      const float* y, int64_t batch, int64_t y_div, float grad_scale,
                      const sp_adamw_coefs* c, const int32_t* stop, float* rsq_partial,
                      sp_stream_t stream);
/* Early-stop test of the optimisation loops (resample_kernels.py:50-51):
 *   loss = (sum of count partials, fixed order) / total;  *loss_out = loss (may be NULL);
 *   *stop = 1 if loss < threshold (compared in double).  Skipped once *stop != 0. */
int sp_opt_check(const float* partials, int64_t count, float total, double threshold,
                 int32_t* stop, float* loss_out, sp_stream_t stream);
/* The latent-space loop's rule (resample_kernels.py:75-91): as sp_opt_check, and from
 * iteration plateau_from (200 in the reference) on also *stop = 1 when the loss exceeds the
 * previous iteration's (*prev_loss, updated here).  itr is the 0-based iteration. */
int sp_opt_check_plateau(const float* partials, int64_t count, float total, double threshold,
                         int64_t itr, int64_t plateau_from, float* prev_loss, int32_t* stop,
                         float* loss_out, sp_stream_t stream);

/* ---- prior building blocks (SURVEY.md §8b "groupnorm_silu_fwd/bwd") -------------------
 * GroupNorm over NCHW x (n, channels, hw = H*W) with `groups` groups, eps, optional
 * per-(sample, channel) bias added to x first (chan_bias [n, channels] or NULL: the UNet's
 * time-embedding add), optional affine (gamma/beta [channels] or NULL) and, if act != 0,
 * SiLU on the output.  Replaces torch GroupNorm + SiLU inside diffusers' ResnetBlock2D /
 * Attention / conv_norm_out (called from ddpm.py:40-43 and stable_diffusion.py:330-345).
 * work: sp_groupnorm_workspace() floats.  mean/rstd [n*groups] are written by the
 * forward and read by the backward, which returns the input VJP dx (= the VJP w.r.t.
 * chan_bias after a sum over H*W). */
int64_t sp_groupnorm_workspace(int64_t n, int32_t channels, int64_t hw, int32_t groups);
int sp_groupnorm_silu_fwd(const float* x, const float* chan_bias, const float* gamma,
                          const float* beta, int64_t n, int32_t channels, int64_t hw,
                          int32_t groups, float eps, int32_t act, float* z, float* mean,
                          float* rstd, float* work, sp_stream_t stream);
int sp_groupnorm_silu_bwd(const float* dz, const float* x, const float* chan_bias,
                          const float* gamma, const float* beta, const float* mean,
                          const float* rstd, int64_t n, int32_t channels, int64_t hw,
                          int32_t groups, int32_t act, float* dx, float* work,
                          sp_stream_t stream);
/* The same over a channel concatenation x = cat(x1, x2) (x1: c1 channels, x2: the other
 * channels - c1; x2 NULL: one tensor), read in place — the up-path ResnetBlocks'
 * torch.cat([h, skip]) is never materialised.  The backward writes the input VJP into the
 * two parts (dx1, dx2) and adds the optional addends (add1, add2: e.g. the residual
 * branch's gradient; an addend may alias its output).
 * team (or NULL): the caller's region for the single-pass kernels' team words, team_bytes
 * >= sp_groupnorm_team_bytes(); zeroed once by the caller (e.g. at allocation), left zero by
 * every launch, and used by one stream at a time — then a call issues no memset.  NULL: the
 * words live in `work`, zeroed by a memset each call (what sp_groupnorm_silu_fwd / _bwd do).
 * The library allocates nothing. */
int sp_groupnorm_silu_fwd2(const float* x1, const float* x2, int32_t c1, const float* chan_bias,
                           const float* gamma, const float* beta, int64_t n, int32_t channels,
                           int64_t hw, int32_t groups, float eps, int32_t act, float* z,
                           float* mean, float* rstd, float* work, void* team, int64_t team_bytes,
                           sp_stream_t stream);
int sp_groupnorm_silu_bwd2(const float* dz, const float* x1, const float* x2, int32_t c1,
                           const float* chan_bias, const float* gamma, const float* beta,
                           const float* mean, const float* rstd, int64_t n, int32_t channels,
                           int64_t hw, int32_t groups, int32_t act, float* dx1, float* dx2,
                           const float* add1, const float* add2, const float* add1b,
                           float* work, void* team, int64_t team_bytes, sp_stream_t stream);

/* Single-pass GroupNorm (default on): a team of workgroups per group keeps the group in
 * registers across its reduction (forward reads x once, backward x and dz once).  enable:
 * 1 on, 0 off (the two-pass kernels), < 0 query; returns the previous setting.  Process-wide;
 * results are bit-identical either way.  A team member that has not published its chunk
 * partials within the poll bound (not resident: another process or stream holds CUs) has
 * them recomputed by the waiting workgroup from the chunk's inputs, in the member's own
 * order, so the result stays bit-identical.  team_timeouts: how many chunk partials were
 * recomputed that way (a cost, not an error).  set_spin_limit: the poll bound (< 0 default;
 * 0 recomputes every partial not present at the first poll — a test of that path). */
int sp_groupnorm_single_pass(int32_t enable);
int64_t sp_groupnorm_team_bytes(int64_t n, int32_t channels, int64_t hw, int32_t groups);
int64_t sp_groupnorm_team_timeouts(void);
int sp_groupnorm_set_spin_limit(int32_t spins);

/* ---- device-resident step schedule (hipGraph capture of a step) ----
 * One record per guided step, precomputed on the host in the same fp64->fp32 arithmetic
 * as the by-value calls; a device cursor selects the current record, so a captured step
 * (timestep write, UNet forward/VJP, both passes, cursor advance) replays unchanged. */
typedef struct sp_step_rec {
    sp_dps_coefs c;   /* this step's scalars                          */
    int64_t step;     /* Philox step index (the sampler's loop index) */
    int64_t t;        /* the prior's timestep                          */
} sp_step_rec;       /* 48 bytes */

/* *t_out = sched[*cursor].t (the prior's timestep tensor, int64) */
int sp_sched_timestep(const sp_step_rec* sched, const int32_t* cursor, int64_t* t_out,
                      sp_stream_t stream);
/* *cursor += 1 */
int sp_sched_advance(int32_t* cursor, sp_stream_t stream);
/* sp_dps_residual / sp_dps_update with the scalars (and the Philox step) read from
 * sched[*cursor] on the device; every operator kind of the by-value forms (SR included,
 * which needs v in the update as there). */
int sp_dps_residual_sched(const sp_op* op, const float* x, const float* eps, const float* y,
                          int64_t batch, int64_t y_div, const sp_step_rec* sched,
                          const int32_t* cursor, float* v_out, float* rsq_partial,
                          sp_stream_t stream);
/* sp_dps_residual_ws with the scalars read from sched[*cursor] (PSF under graph replay; the
 * other kinds as sp_dps_residual_sched, work may be NULL). */
int sp_dps_residual_sched_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                             int64_t batch, int64_t y_div, const sp_step_rec* sched,
                             const int32_t* cursor, float* v_out, float* rsq_partial,
                             float* work, sp_stream_t stream);
int sp_dps_update_sched(const sp_op* op, const float* x, const float* eps, const float* y,
                        const float* v, const float* w, const float* rsq_partial,
                        uint64_t seed, int64_t sample_offset, int64_t batch, int64_t y_div,
                        const sp_step_rec* sched, const int32_t* cursor, float* x_out,
                        sp_stream_t stream);

/* 3x3 / stride 1 / pad 1 convolution on fp32 MFMA (SURVEY.md §8b "vae_conv3x3_fwd/bwd_input",
 * §8f f1): the ResnetBlock / mid / up-sampling convolutions of the SD VAE and DDPM UNet
 * (diffusers Conv2d(k=3, p=1), reached from stable_diffusion.py:330-345, ddpm.py:40-43).
 * Weights are packed once per layer (sp_conv3x3_pack; input_vjp=1 packs the transposed,
 * flipped weights of the input VJP); NCHW fp32 activations.  Shapes: see _supported. */
int sp_conv3x3_supported(int32_t cin, int32_t cout, int32_t height, int32_t width);
int64_t sp_conv3x3_packed_size(int32_t cin, int32_t cout);
int sp_conv3x3_pack(const float* w, int32_t cout, int32_t cin, int32_t input_vjp, float* wp,
                    sp_stream_t stream);
int sp_conv3x3_fwd(const float* x, const float* wp, const float* bias, int64_t n, int32_t cin,
                   int32_t cout, int32_t height, int32_t width, float* y, sp_stream_t stream);
int sp_conv3x3_bwd_input(const float* dy, const float* wp_vjp, int64_t n, int32_t cin,
                         int32_t cout, int32_t height, int32_t width, float* dx,
                         sp_stream_t stream);

/* 3x3 / stride 1 / pad 1 convolutions with few channels on one side (cout <= 8 or cin <= 8:
 * the priors' conv_in / conv_out) as VALU direct convolutions on the raw weights
 * [cout][cin][3][3]; the input VJP reads the same weights transposed and flipped. */
int sp_conv3x3_thin_supported(int32_t cin, int32_t cout, int32_t height, int32_t width);
int sp_conv3x3_thin_fwd(const float* x, const float* w, const float* bias, int64_t n,
                        int32_t cin, int32_t cout, int32_t height, int32_t width, float* y,
                        sp_stream_t stream);
int sp_conv3x3_thin_bwd_input(const float* dy, const float* w, int64_t n, int32_t cin,
                              int32_t cout, int32_t height, int32_t width, float* dx,
                              sp_stream_t stream);

/* 3x3 / stride 2 convolution with one zero row / column on the bottom / right (diffusers'
 * Downsample2D, downsample_padding=0: the UNet's and the VAE encoder's downsampling layers;
 * reached from ddpm.py:40-43 and stable_diffusion.py:338-345), on fp32 MFMA, NCHW.
 * height / width are the INPUT's (even); the output is height/2 x width/2.  Forward: cin % 4,
 * cout % 128, (height/2) % 8, (width/2) % 32; input VJP (input_vjp=1): cout % 4, cin % 128,
 * (height/2) % 2, (width/2) % 32 — each output phase (row & 1, column & 1) of dx is its own
 * sum over the taps that reach it.  Weights packed once per layer by sp_conv3x3_s2_pack
 * (cin * cout * 9 floats; layouts differ for the two directions).  FLOPs recorded for
 * kinds 3-4 (18*N*Cin*Cout*(H/2)*(W/2)). */
int sp_conv3x3_s2_supported(int32_t cin, int32_t cout, int32_t height, int32_t width,
                            int32_t input_vjp);
/* 2x nearest-neighbour upsampling (Upsample2D of the UNet and the VAE decoder, before its
 * 3x3 conv) over `planes` = N*C planes of height x width (width % 4, 16-B aligned buffers),
 * and its VJP, the 2x2 block sum of dy (2*height x 2*width) into dx (height x width). */
int sp_upsample2x_supported(int32_t height, int32_t width);
int sp_upsample2x(const float* x, int64_t planes, int32_t height, int32_t width, float* y,
                  sp_stream_t stream);
int sp_upsample2x_vjp(const float* dy, int64_t planes, int32_t height, int32_t width, float* dx,
                      sp_stream_t stream);
int sp_conv3x3_s2_pack(const float* w, int32_t cout, int32_t cin, int32_t input_vjp, float* wp,
                       sp_stream_t stream);
int sp_conv3x3_s2_fwd(const float* x, const float* wp, const float* bias, int64_t n, int32_t cin,
                      int32_t cout, int32_t height, int32_t width, float* y, sp_stream_t stream);
int sp_conv3x3_s2_bwd_input(const float* dy, const float* wp_vjp, int64_t n, int32_t cin,
                            int32_t cout, int32_t height, int32_t width, int32_t accumulate,
                            float* dx, sp_stream_t stream);
/* Split-K forms (a workspace; same results to fp32 rounding, bitwise reproducible): a launch
 * whose workgroups fill less than half the CUs (batch 1) runs 2-16 parts over K that store
 * partial sums to ws, then adds them in a fixed order (+ bias, or onto dx with accumulate).
 * sp_conv3x3_s2_workspace = the bytes a launch needs, 0 = not split (ws may be NULL). */
int64_t sp_conv3x3_s2_workspace(int64_t n, int32_t cin, int32_t cout, int32_t height, int32_t width,
                                int32_t input_vjp);
int sp_conv3x3_s2_fwd_ws(const float* x, const float* wp, const float* bias, int64_t n, int32_t cin,
                         int32_t cout, int32_t height, int32_t width, float* y, float* ws, int64_t ws_bytes,
                         sp_stream_t stream);
int sp_conv3x3_s2_bwd_input_ws(const float* dy, const float* wp_vjp, int64_t n, int32_t cin,
                               int32_t cout, int32_t height, int32_t width, int32_t accumulate,
                               float* dx, float* ws, int64_t ws_bytes, sp_stream_t stream);

/* The same layers by Winograd F(2x2,3x3) on fp32 MFMA (2.25x fewer multiplies; the
 * transforms add F(2,3) rounding, as MIOpen's Winograd solver does).  up = U = G g G^T
 * packed by sp_wino3x3_pack (input_vjp=1: of the transposed, flipped weights). */
int sp_wino3x3_supported(int32_t cin, int32_t cout, int32_t height, int32_t width);
int64_t sp_wino3x3_packed_size(int32_t cin, int32_t cout);
int sp_wino3x3_pack(const float* w, int32_t cout, int32_t cin, int32_t input_vjp, float* up,
                    sp_stream_t stream);
int sp_wino3x3_fwd(const float* x, const float* up, const float* bias, int64_t n, int32_t cin,
                   int32_t cout, int32_t height, int32_t width, float* y, sp_stream_t stream);
/* y = conv(x) + bias + res: the ResnetBlock's residual added in the tile's epilogue
 * (res shaped like y, not aliasing it). */
int sp_wino3x3_fwd_res(const float* x, const float* up, const float* bias, const float* res,
                       int64_t n, int32_t cin, int32_t cout, int32_t height, int32_t width,
                       float* y, sp_stream_t stream);
int sp_wino3x3_bwd_input(const float* dy, const float* up_vjp, int64_t n, int32_t cin,
                         int32_t cout, int32_t height, int32_t width, float* dx,
                         sp_stream_t stream);
/* Split-K forms (round 4): where the launch's tiles leave CUs idle (small batches, the
 * low-resolution levels) K is cut into up to 32 parts, each part's partial output stored to
 * the caller's workspace and the parts summed in a fixed order (+ bias, + res) by a reduce
 * launch — deterministic.  sp_wino3x3_workspace = the bytes a shape's split needs (0: the
 * shape fills the chip unsplit); a smaller (or NULL) workspace runs unsplit.  res nullable. */
int64_t sp_wino3x3_workspace(int64_t n, int32_t cin, int32_t cout, int32_t height, int32_t width);
int sp_wino3x3_fwd_ws(const float* x, const float* up, const float* bias, const float* res,
                      int64_t n, int32_t cin, int32_t cout, int32_t height, int32_t width,
                      float* y, float* ws, int64_t ws_bytes, sp_stream_t stream);
int sp_wino3x3_bwd_input_ws(const float* dy, const float* up_vjp, int64_t n, int32_t cin,
                            int32_t cout, int32_t height, int32_t width, float* dx, float* ws,
                            int64_t ws_bytes, sp_stream_t stream);
/* Round 5: diffusers' Upsample2D (nearest 2x upsample, then this conv) fused into the tile, so
 * the upsampled tensor is never written (reference call sites: the UNet / VAE up blocks behind
 * ddpm.py:40-43 and stable_diffusion.py:330-336).  height x width = the conv's (upsampled) size.
 * sp_wino3x3_fwd_up: x is the [n][cin][height/2][width/2] source, y the [n][cout][height][width]
 * conv output (+ bias).  sp_wino3x3_bwd_input_pool: the input VJP of conv(upsample(x)), dy
 * [n][cout][height][width] -> dx [n][cin][height/2][width/2] (each 2x2 block's sum in
 * sp_upsample2x_vjp's order: bitwise the unfused pair's result when that runs unsplit).
 * Unsplit (no workspace); sp_wino3x3_up_supported says where both directions run.
 * sp_wino3x3_fwd_up runs 9 of the 16 transformed GEMMs: on a nearest-upsampled image the other
 * 7 are products with exact zeros (sp_wino.hip, "Live-ξ forms").  For finite x and weights its
 * output equals sp_wino3x3_fwd on the materialised upsample, the sign of a zero excepted; with
 * inf or NaN in x or the weights the two can differ (the skipped GEMMs held inf - inf or inf * 0
 * = NaN, which no longer reaches the output). */
int sp_wino3x3_up_supported(int32_t cin, int32_t cout, int32_t height, int32_t width);
int sp_wino3x3_fwd_up(const float* x, const float* up, const float* bias, int64_t n, int32_t cin,
                      int32_t cout, int32_t height, int32_t width, float* y, sp_stream_t stream);
int sp_wino3x3_bwd_input_pool(const float* dy, const float* up_vjp, int64_t n, int32_t cin,
                              int32_t cout, int32_t height, int32_t width, float* dx,
                              sp_stream_t stream);

/* 1x1 convolution as a per-pixel GEMM on bf16 MFMAs over exact three-term splits of the fp32
 * operands (fp32-class error): Y[n][co][p] = sum_k W[co][k] X[n][k][p] (+ bias[co]) (+ res),
 * X = cat(x1 [n][c1][hw], x2 [n][c2][hw]) read in place, Y split into y1 [n][o1][hw] and
 * y2 [n][o2][hw] (o2 may be 0).  Replaces diffusers ResnetBlock2D.conv_shortcut over the
 * up path's concatenation (forward) and its input VJP (W^T dy into both parts), SURVEY.md §8f
 * f1.  M = o1 + o2 % 128, K = c1 + c2 % 16, c1 % 8, c2 % 8, o1 % 32, o2 % 32, hw % 256;
 * res only with o2 == 0.  W packed by sp_gemm_x6_pack from a row-major [M][K] matrix, or
 * (trans = 1) from one stored [K][M]. */
int sp_gemm_x6_supported(int32_t m, int32_t k, int64_t hw);
int64_t sp_gemm_x6_packed_size(int32_t m, int32_t k);
int sp_gemm_x6_pack(const float* w, int32_t m, int32_t k, int32_t trans, float* wp, sp_stream_t stream);
int sp_gemm_x6(const float* x1, int32_t c1, const float* x2, int32_t c2, const float* wp,
               const float* bias, const float* res, int64_t n, int64_t hw, float* y1, int32_t o1,
               float* y2, int32_t o2, sp_stream_t stream);

/* nn.Linear on token-major activations with the same bf16x6 arithmetic:
 * y[t][o] = sum_k x[t][k] W[o][k] (+ bias[o]) (+ res[t][o]), tokens % 256, k % 16, m % 32
 * (W's rows padded to 128 with zeros by sp_gemm_x6_pack; pack W^T with trans = 1 for the
 * input VJP).  Replaces torch.nn.functional.linear in the ε-UNets' attention / transformer
 * blocks (diffusers Attention to_q/k/v/out, FeedForward), SURVEY.md §8f f1. */
int sp_linear_x6_supported(int64_t tokens, int32_t k, int32_t m);
int sp_linear_x6(const float* x, const float* wp, const float* bias, const float* res, int64_t tokens,
                 int32_t k, int32_t m, float* y, sp_stream_t stream);

/* The same GEMM between the two activation layouts of the transformer blocks' 1x1 proj_in /
 * proj_out (diffusers Transformer2DModel): x [n][k][hw] (in_tm = 0) or [n hw][k] (in_tm = 1),
 * y and res [n][m][hw] (out_tm = 0) or [n hw][m] (out_tm = 1); the NCHW <-> token transposes
 * happen in the tile's loads and stores.  hw % 256, k % 16, m % 32. */
int sp_gemm_x6_layout_supported(int64_t n, int64_t hw, int32_t k, int32_t m);
int sp_gemm_x6_layout(const float* x, const float* wp, const float* bias, const float* res, int64_t n,
                      int64_t hw, int32_t k, int32_t m, int32_t in_tm, int32_t out_tm, float* y,
                      sp_stream_t stream);

/* Split-K forms of the three (same arguments, plus a workspace): a launch whose tiles fill
 * less than half the CUs (batch 1, the 16² / 8² levels) runs 2-16 K parts that store their
 * partial products to ws, then adds them in a fixed order with the bias and the residual
 * (bitwise reproducible).  sp_gemm_x6_workspace(n, hw, k, m) = the bytes a launch over n
 * images of hw pixels (sp_linear_x6: n = 1, hw = tokens), K = k, M = m needs; 0 = not split
 * (ws may be NULL; a NULL or short ws runs unsplit). */
int64_t sp_gemm_x6_workspace(int64_t n, int64_t hw, int32_t k, int32_t m);
int sp_gemm_x6_ws(const float* x1, int32_t c1, const float* x2, int32_t c2, const float* wp,
                  const float* bias, const float* res, int64_t n, int64_t hw, float* y1, int32_t o1,
                  float* y2, int32_t o2, float* ws, int64_t ws_bytes, sp_stream_t stream);
int sp_linear_x6_ws(const float* x, const float* wp, const float* bias, const float* res, int64_t tokens,
                    int32_t k, int32_t m, float* y, float* ws, int64_t ws_bytes, sp_stream_t stream);
int sp_gemm_x6_layout_ws(const float* x, const float* wp, const float* bias, const float* res, int64_t n,
                         int64_t hw, int32_t k, int32_t m, int32_t in_tm, int32_t out_tm, float* y, float* ws,
                         int64_t ws_bytes, sp_stream_t stream);

/* Fused self-attention softmax(q k^T * scale) v of the SD 1.5 eps-UNet's transformer blocks
 * (attn1 over the latent tokens; diffusers UNet2DConditionModel, stable_diffusion.py:306-313;
 * replaces the scores / softmax / weighted-sum chain and its autograd VJP) on fp32 MFMA,
 * without materialising the score matrix.  q, k, v, out, dout, dq, dk, dv: [bh][n][d];
 * lse, delta: [bh][n] (lse = row log-sum-exp, natural log, written by the forward; delta =
 * rowsum(dout * out), written by the backward; at the split-bf16 forward's shapes the dq pass
 * replaces it by sum_j P dP / sum_j P of the P it rebuilds, which the dk / dv pass then reads).
 * Self-attention only (m == n); head dims 40,
 * 80, 160; n a multiple of the kernels' row blocks (see _supported).  The backward writes dq
 * when dq != NULL and dk, dv when both are given. */
int sp_attention_supported(int64_t bh, int64_t n, int64_t m, int32_t d);
int sp_attention_fwd(const float* q, const float* k, const float* v, int64_t bh, int64_t n,
                     int32_t d, float scale, float* out, float* lse, sp_stream_t stream);
int sp_attention_bwd(const float* q, const float* k, const float* v, const float* out,
                     const float* dout, const float* lse, int64_t bh, int64_t n, int32_t d,
                     float scale, float* delta, float* dq, float* dk, float* dv,
                     sp_stream_t stream);
/* The same on the token-major activations of the projections, without head split / merge
 * copies, and cross-attention: row i of head h of sample b of q (and dq) starts at
 * (b n + i) rs + h d, of out (and dout) at (b n + i) ro + h d, of k, v (and dk, dv) at
 * (b' m + j) rs_kv + h d with b' = b (kv_batch = batch) or 0 (kv_batch = 1: one context
 * shared by the batch).  Self-attention: m = n, rs_kv = rs (rs = 3 heads d when q, k, v are
 * the thirds of one fused qkv projection [b n][3 heads d]).  Cross-attention (m != n, any
 * m >= 1, e.g. the 77-token text context of attn2): forward and dq only (dk = dv = NULL).
 * lse, delta: [b heads][n]. */
int sp_attention_mh_supported(int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d);
int sp_attention_fwd_mh(const float* q, const float* k, const float* v, int64_t batch, int32_t heads,
                        int64_t n, int64_t m, int32_t d, int32_t rs, int32_t rs_kv, int64_t kv_batch,
                        int32_t ro, float scale, float* out, float* lse, sp_stream_t stream);
int sp_attention_bwd_mh(const float* q, const float* k, const float* v, const float* out,
                        const float* dout, const float* lse, int64_t batch, int32_t heads, int64_t n,
                        int64_t m, int32_t d, int32_t rs, int32_t rs_kv, int64_t kv_batch, int32_t ro,
                        float scale, float* delta, float* dq, float* dk, float* dv, sp_stream_t stream);
/* Self-attention forward on the bf16 MFMA datapath over exact three-term splits of the fp32
 * operands (six partial products per product, fp32 accumulation; error at or below the
 * exact-fp32 kernel's), head dims 40 / 80, n % 128 == 0; q / k / v rows of stride rs, out rows
 * of stride ro, lse as sp_attention_fwd_mh.  sp_attention_fwd / _fwd_mh route self-attention
 * at these shapes here while sp_attention_bf16x6 is on (default; 0: the exact-fp32 kernel,
 * < 0 query; returns the previous setting). */
int sp_attention6_supported(int64_t batch, int32_t heads, int64_t n, int32_t d);
int sp_attention6_fwd_mh(const float* q, const float* k, const float* v, int64_t batch, int32_t heads, int64_t n,
                         int32_t d, int32_t rs, int32_t ro, float scale, float* out, float* lse,
                         sp_stream_t stream);
/* ws (or NULL): sp_attention6_workspace() bytes, where K and V are split into their bf16 terms
 * once per head instead of once per 128-query workgroup. */
int64_t sp_attention6_workspace(int64_t batch, int32_t heads, int64_t n, int32_t d);
int sp_attention6_fwd_ws(const float* q, const float* k, const float* v, int64_t batch, int32_t heads, int64_t n,
                         int32_t d, int32_t rs, int32_t ro, float scale, float* out, float* lse, void* ws,
                         int64_t ws_bytes, sp_stream_t stream);
int sp_attention_bf16x6(int32_t enable);
int sp_attention_bf16x6_enabled(void);

/* Transformer-block glue of the SD 1.5 eps-UNet (diffusers BasicTransformerBlock,
 * stable_diffusion.py:306-313): torch.nn.LayerNorm over the C channels of token-major rows
 * [rows][C] (C % 4, C <= 2048; mean / rstd [rows] written for the VJP) and its input VJP
 * (frozen weights; add != NULL is summed into dx: the residual branch's gradient of the same
 * tensor), and the feed-forward's GEGLU gate y = a * gelu(gate) over h = [a | gate]
 * ([rows][2F] -> [rows][F], exact erf GELU, F % 4) and its input VJP dh. */
int sp_layernorm_supported(int64_t rows, int32_t c);
int sp_layernorm_fwd(const float* x, const float* w, const float* b, int64_t rows, int32_t c, float eps,
                     float* y, float* mean, float* rstd, sp_stream_t stream);
int sp_layernorm_bwd(const float* dy, const float* x, const float* w, const float* mean, const float* rstd,
                     const float* add, int64_t rows, int32_t c, float* dx, sp_stream_t stream);
int sp_geglu_fwd(const float* h, int64_t rows, int32_t f, float* y, sp_stream_t stream);
int sp_geglu_bwd(const float* h, const float* dy, int64_t rows, int32_t f, float* dh, sp_stream_t stream);

/* Row softmax of materialised attention scores [rows][n] in place (n % 4, n <= 4096; lse
 * [rows] = row log-sum-exp when non-NULL) and its VJP scaled by the score scale,
 * dp <- scale * p * (dp - rowsum(p * dp)): the single-head d = 512 attention of the SD VAE
 * mid blocks and the DDPM UNet (diffusers Attention, ddpm.py:40-43 / stable_diffusion.py:
 * 330-345), whose score GEMMs are hipBLASLt's. */
int sp_softmax_rows_supported(int64_t rows, int32_t n);
int sp_softmax_rows(float* s, int64_t rows, int32_t n, float* lse, sp_stream_t stream);
int sp_softmax_bwd_rows(const float* p, float* dp, int64_t rows, int32_t n, float scale, sp_stream_t stream);

/* 1x1 convolution over 4 or 8 channels (the SD VAE's quant_conv / post_quant_conv):
 * y[n][o][p] = sum_c w[o][c] x[n][c][p] (+ b[o]); trans = 1 applies W^T (input VJP, b NULL).
 * hw % 4. */
int sp_conv1x1_small_supported(int32_t cin, int32_t cout, int64_t hw);
int sp_conv1x1_small(const float* x, const float* w, const float* b, int64_t n, int32_t cin, int32_t cout,
                     int64_t hw, int32_t trans, float* y, sp_stream_t stream);

/* ---- The priors at reduced precision (bf16), NHWC activations (csrc/sp_bf16_*.hip) --------
 * The reference's adapters take any torch_dtype and its PSLD driver runs SD 1.5 in bf16
 * (reference: samplers/networks/diffusers/stable_diffusion.py:90-101, ddpm.py:23-34,
 * scripts/run_psld.py:14-20).  These entry points are the bf16 layers of those priors:
 * activations channels-last ([n][h][w][c]) bf16, bf16 MFMA operands, fp32 accumulation and
 * fp32 statistics.  Device pointers; bf16 buffers are passed as void*. */
int sp_conv3x3_bf16_supported(int32_t cin, int32_t cout, int32_t h, int32_t w);
/* bf16 elements of the packed weights: [ceil(cout/64)][cin/16][9 taps][64 co][16 ci] */
int64_t sp_conv3x3_bf16_packed_size(int32_t cin, int32_t cout);
/* y = conv3x3(x) + bias (+ res): stride 1, padding 1 (diffusers' ResnetBlock2D / conv_in /
 * conv_out / Upsample2D convolutions); the input VJP is the same call with the pack of
 * W'[ci][co][2-ky][2-kx].  bias fp32 [cout] or NULL, res bf16 like y or NULL. */
int sp_conv3x3_bf16(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                    int32_t cout, int32_t h, int32_t w, void* y, sp_stream_t stream);
/* split-K form for launches that leave CUs idle (the priors' 16x16 / 8x8 levels): the parts' fp32
 * sums in ws (sp_conv3x3_bf16_workspace bytes, 0 = unsplit), reduced in a fixed order */
int64_t sp_conv3x3_bf16_workspace(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w);
int sp_conv3x3_bf16_ws(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                       int32_t cout, int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes, sp_stream_t stream);
/* y = conv3x3(upsample_nearest2x(x)) + bias (+ res) (diffusers' Upsample2D): x [n][h/2][w/2][cin],
 * y [n][h][w][cout] — the upsampled tensor is never written; its VJP is sp_conv3x3_bf16 with the
 * VJP pack at full resolution followed by sp_pool2x2_bf16. */
int sp_conv3x3_bf16_up(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                       int32_t cout, int32_t h, int32_t w, void* y, sp_stream_t stream);
/* dx[n][h/2][w/2][c] = 2x2 block sums of dz[n][h][w][c], NHWC bf16 (c % 8 == 0) */
int sp_pool2x2_bf16(const void* dz, int64_t n, int32_t c, int32_t h, int32_t w, void* dx, sp_stream_t stream);
/* LayerNorm over bf16 token rows [rows][c] (BasicTransformerBlock's norm1-3 at bf16), fp32 weight /
 * bias / statistics (mean, rstd per row, for the VJP); the VJP (frozen weights) adds `add` (bf16,
 * nullable: the residual branch's gradient of the same tensor).  c % 8 == 0, c <= 2048. */
int sp_layernorm_bf16_supported(int64_t rows, int32_t c);
int sp_layernorm_bf16_fwd(const void* x, const float* w, const float* b, int64_t rows, int32_t c, float eps, void* y,
                          float* mean, float* rstd, sp_stream_t stream);
int sp_layernorm_bf16_bwd(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
                          const void* add, int64_t rows, int32_t c, void* dx, sp_stream_t stream);
/* GEGLU at bf16 (diffusers GEGLU after its projection, the SD 1.5 transformers' feed-forward,
 * reached from stable_diffusion.py:306-313): h = [a | gate] [rows][2f] -> y = a * gelu(gate)
 * [rows][f] (exact erf GELU, fp32 arithmetic); VJP dh = [dy gelu(gate) | dy a gelu'(gate)] as one
 * [rows][2f] buffer.  f % 8 == 0; bf16 throughout. */
int sp_geglu_bf16_fwd(const void* h, int64_t rows, int32_t f, void* y, sp_stream_t stream);
int sp_geglu_bf16_bwd(const void* h, const void* dy, int64_t rows, int32_t f, void* dh, sp_stream_t stream);
int sp_groupnorm_bf16_supported(int32_t c1, int32_t c2, int32_t groups);
int64_t sp_groupnorm_bf16_workspace(int64_t n, int32_t c, int64_t hw);
/* z = act(GroupNorm(cat(x1, x2) + chan_bias) * gamma + beta) over NHWC bf16 parts (channel
 * concatenation read in place); stats = [mean | rstd] per (n, group), fp32. */
int sp_groupnorm_bf16_fwd(const void* x1, const void* x2, int32_t c1, int32_t c2, const float* chan_bias,
                          const float* gamma, const float* beta, int64_t n, int64_t hw, int32_t groups, float eps,
                          int32_t act, void* z, float* stats, void* ws, int64_t ws_bytes, sp_stream_t stream);
/* its input VJP into the parts' layouts (+ addends; outputs may alias them) */
int sp_groupnorm_bf16_bwd(const void* dz, const void* x1, const void* x2, int32_t c1, int32_t c2,
                          const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                          int64_t n, int64_t hw, int32_t groups, int32_t act, void* dx1, void* dx2, const void* add1,
                          const void* add2, const void* add1b, void* ws, int64_t ws_bytes, sp_stream_t stream);
/* The same with a chosen layout for z (z_layout 1: channel-blocked [n][c/16][hw][16], c % 16 == 0:
 * the conv tile's preferred input, sp_conv3x3_bf16_ex) / for dx1 (dx_layout 1: one part, c1 % 16 == 0;
 * the addends stay NHWC; dx_layout 2: dx1 / dx2 NHWC, add1 one addend over the concatenated channels
 * [n][hw][c1 + c2] and add2 NULL — a 1x1 shortcut's input gradient from one GEMM). */
int sp_groupnorm_bf16_fwd_ex(const void* x1, const void* x2, int32_t c1, int32_t c2, const float* chan_bias,
                             const float* gamma, const float* beta, int64_t n, int64_t hw, int32_t groups, float eps,
                             int32_t act, void* z, int32_t z_layout, float* stats, void* ws, int64_t ws_bytes,
                             sp_stream_t stream);
int sp_groupnorm_bf16_bwd_ex(const void* dz, const void* x1, const void* x2, int32_t c1, int32_t c2,
                             const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                             int64_t n, int64_t hw, int32_t groups, int32_t act, void* dx1, void* dx2, int32_t dx_layout,
                             const void* add1, const void* add2, const void* add1b, void* ws, int64_t ws_bytes,
                             sp_stream_t stream);
/* sp_conv3x3_bf16_ws with the input in a chosen layout (in_layout 0 NHWC, 1 channel-blocked
 * [n][cin/16][h][w][16]: every 16-channel stage reads whole cache lines); in_layout 1 needs
 * sp_conv3x3_bf16_blk_supported (w % 32 == 0, h % 16 == 0).  The output stays NHWC. */
int sp_conv3x3_bf16_blk_supported(int32_t cin, int32_t cout, int32_t h, int32_t w);
int sp_conv3x3_bf16_ex(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* res, int64_t n,
                       int32_t cin, int32_t cout, int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes,
                       sp_stream_t stream);
/* y = conv3x3(x) + conv1x1(cat(xs1, xs2)) + bias: a ResnetBlock's conv2 with its conv_shortcut
 * summed as (cs1 + cs2) / 16 further stages of the same contraction (no shortcut tensor, no
 * residual read).  wsp: [ceil(cout/64)][cs/16][64 co][16 ci] bf16 (rows past cout zero,
 * sp_conv3x3_bf16_sc_packed_size elements); bias: conv2's + the shortcut's; x in in_layout as
 * sp_conv3x3_bf16_ex; xs1 / xs2 NHWC.  Replaces the shortcut GEMM + residual epilogue of
 * diffusers' ResnetBlock2D (reference: samplers/networks/diffusers/ddpm.py:40-43 prior call). */
int sp_conv3x3_bf16_sc_supported(int32_t cin, int32_t cout, int32_t cs1, int32_t cs2, int32_t h, int32_t w);
int64_t sp_conv3x3_bf16_sc_packed_size(int32_t cs, int32_t cout);
int64_t sp_conv3x3_bf16_sc_workspace(int64_t n, int32_t cin, int32_t cs, int32_t cout, int32_t h, int32_t w);
int sp_conv3x3_bf16_sc(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* xs1,
                       const void* xs2, int32_t cs1, int32_t cs2, const void* wsp, int64_t n, int32_t cin,
                       int32_t cout, int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes, sp_stream_t stream);
/* dz = the 3x3 conv input VJP of dy (flipped / transposed pack wp; dy in in_layout as
 * sp_conv3x3_bf16_ex), then dx1 / dx2 = the input VJP of sp_groupnorm_bf16_fwd over cat(x1, x2)
 * (c1 + c2 = cout) at dz (+ add1 / add2 / add1b; dx_layout as sp_groupnorm_bf16_bwd_ex): the
 * ResnetBlock VJP's conv2^T -> GN2^T and conv1^T -> GN1^T pairs, with the GroupNorm VJP's sums
 * taken in the conv's epilogue per 512-pixel tile (no pass re-reading dz and x).  dz: caller
 * buffer [n][h][w][cout]; ws: sp_conv3x3_bf16_gnvjp_workspace bytes.  TC = 32 unsplit shapes. */
int sp_conv3x3_bf16_gnvjp_supported(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t c1,
                                    int32_t groups);
int64_t sp_conv3x3_bf16_gnvjp_workspace(int64_t n, int32_t cout, int32_t h, int32_t w);
int sp_conv3x3_bf16_gnvjp(const void* dy, int32_t in_layout, const void* wp, int64_t n, int32_t cin, int32_t cout,
                          int32_t h, int32_t w, void* dz, const void* x1, const void* x2, int32_t c1,
                          const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                          int32_t groups, int32_t act, void* dx1, void* dx2, int32_t dx_layout, const void* add1,
                          const void* add2, const void* add1b, void* ws, int64_t ws_bytes, sp_stream_t stream);
/* y = conv3x3(x) + bias (+ res) (as sp_conv3x3_bf16_ex), then z = act(GroupNorm(y + chan_bias))
 * (as sp_groupnorm_bf16_fwd_ex: gamma / beta, z_layout, stats [mean | rstd]) — the ResnetBlock's
 * conv1 -> GN2 pair, with the GroupNorm moments taken in the conv's epilogue per 512-pixel tile
 * (shifted by the tile's first pixel; no statistics pass re-reading y).  ws:
 * sp_conv3x3_bf16_gn_workspace bytes.  TC = 32 unsplit shapes. */
int sp_conv3x3_bf16_gn_supported(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t groups);
int64_t sp_conv3x3_bf16_gn_workspace(int64_t n, int32_t cout, int32_t h, int32_t w);
int sp_conv3x3_bf16_gn(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* res,
                       int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, void* y, const float* chan_bias,
                       const float* gamma, const float* beta, int32_t groups, float eps, int32_t act, void* z,
                       int32_t z_layout, float* stats, void* ws, int64_t ws_bytes, sp_stream_t stream);
int sp_attention_bf16_supported(int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d);
/* multi-head softmax(q k^T scale) v on bf16 token rows (self: m = n; cross: kv_shared = 1 for
 * one context row for the whole batch); lse [batch heads][n] fp32 for the VJP. */
int sp_attention_bf16_fwd(const void* q, const void* k, const void* v, int64_t batch, int32_t heads, int64_t n,
                          int64_t m, int32_t d, int32_t rsq, int32_t rskv, int32_t kv_shared, int32_t ro, float scale,
                          void* out, float* lse, sp_stream_t stream);
/* its VJP on the bf16 MFMAs (P, dS never in HBM): delta = caller's [batch heads][n] fp32 scratch;
 * dq rows of stride rdq; dk / dv (self-attention only) rows of stride rdkv, or NULL. */
int sp_attention_bf16_bwd_supported(int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d);
int sp_attention_bf16_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                          const float* lse, int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d,
                          int32_t rsq, int32_t rskv, int32_t kv_shared, int32_t ro, int32_t rdq, int32_t rdkv,
                          float scale, float* delta, void* dq, void* dk, void* dv, sp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMPLERS_HIP_H */
