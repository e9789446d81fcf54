// Fourier phase retrieval (SP_OP_PHASE): y = |FFT2(zero-pad(x))| per channel plane, norm "ortho",
// unshifted (DC at [0][0]); the reference has no such operator, semantics in
// operators/phase.py, pinned in fp64 by tests/phase_ops.py.  x is (C, H, W), padded by
// pad_h = op.radius rows and pad_w = op.factor columns on each side to Nh x Nw, each 2^k or
// 3 * 2^k in [8, 1024].  With z = FFT2(pad(x)) the Jacobian-transpose product of a y-space
// cotangent g is  J^T g = crop(Re(IFFT2(g * z / |z|)))  with z / |z| := 0 at |z| = 0.
//
// Three launches through the caller's workspace, shared by apply (1, 2), the VJP (1, 2, 3)
// and DPS pass 1 (1, 2, 3):
//   1. rows     a workgroup stages TR image rows of one plane in LDS, forming
//               x0 = (x - k eps) / a (DPS) and zero-extending W -> Nw, runs an Nw-point FFT per
//               row and stores the complex rows TRANSPOSED.  Only the H image rows are
//               transformed: pad rows transform to zero and are never touched.
//   2. columns  a workgroup loads TC columns (contiguous in the transposed intermediate),
//               zero-extends H -> Nh, runs the forward Nh-point FFT, the pointwise step on the
//               whole column (|z|; r = y - |z|, r^2 partial, u = grad_scale r z / |z|; or
//               u = g z / |z|), the inverse Nh-point FFT in place, and stores rows
//               pad_h .. pad_h + H - 1 back over the columns it loaded.  The Nh x Nw spectrum
//               exists only in LDS.  apply stops after |z| and writes it to y.
//   3. rows^-1  TR rows of the intermediate -> LDS, inverse Nw-point FFT, real part, columns
//               pad_w .. pad_w + W - 1 -> v.
//
// Intermediate (the workspace): complex fp32 as (re, im) pairs, [sample][plane][Nw][H] — the
// row FFT's output index kw is the slow axis, the image row h the fast one, so launch 2 reads
// and writes each of its column tiles as ONE contiguous run of TC * H complex numbers.
// 2 * batch * C * Nw * H floats, 8-byte aligned.
//
// The host section at the end forms every launch with fft_stage (sp_fft.h): the grid from the
// tiles per sample and the batch, the LDS size from the transform length, the launch check.
//
// FFT (the core lives in sp_fft.h, shared with sp_psf_fft.hip): Stockham autosort, decimation in
// time, between two LDS buffers (one barrier per pass):
// radix-4 passes, one radix-2 pass when log2 is odd, and the radix-3 pass last, so every pass's
// sub-transform length Ns is a power of two.  Pass with radix R on a line of N points, for
// j < N / R, k = j mod Ns:
//   v_i = in[j + i N / R] * w^(i k N / (Ns R)),  out[(j - k) R + k + i Ns] = DFT_R(v)_i
// with w^q = exp(-2 pi i q / N) from an LDS table of N entries filled in the prologue by fp64
// sincospi (correct to fp32 rounding; the inverse conjugates).  The "ortho" factors of both
// axes, 1 / sqrt(Nh Nw), are applied once per transform in the pointwise step.
//
// LDS layout: a line of N complex numbers occupies NP = (N + N / 16) | 1 slots, element q at
// q + (q >> 4).  Reads of a pass are consecutive per lane; the first radix-4 pass writes with a
// stride of 4 complex numbers, which the pad every 16 spreads over all 32 banks of a 16-lane
// ds_write_b64 group (the Ns = 4 pass keeps a 2-way conflict, later passes write runs of >= 16).
// NP odd makes the transposing accesses (one lane per line) hit 32 distinct bank pairs.
// Lines per workgroup: as many as fit 32000 bytes with both buffers and the table (so five
// workgroups share a CU's 160 KiB), at most 16, at least 1 (Nh = 1024: one line, 25.6 KB).
//
// Every sample is computed alone: lines are assigned to workgroups by plane and tile only, the
// r^2 partial of a (plane, column tile) is block_sum's fixed order over a fixed assignment of
// elements to threads, so the bits do not depend on the batch, y_div or the shard.  No atomics.

#include <algorithm>

#define SP_TU 17  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"
#include "sp_fft.h"

namespace sp {

enum { PH_APPLY = 0, PH_VJP = 1, PH_RESIDUAL = 2 };

struct phase_geom {
    int C, H, W, ph, pw, Nh, Nw;
    __host__ __device__ explicit phase_geom(const sp_op& op)
        : C(op.channels), H(op.height), W(op.width), ph(op.radius), pw(op.factor),
          Nh(op.height + 2 * op.radius), Nw(op.width + 2 * op.factor) {}
};

// launch 1.  X0: x0 = (in - k eps) / a while staging, else x0 = in.
template <bool X0>
__global__ __launch_bounds__(kBlock) void k_phase_rows(sp_op op, const float* __restrict__ in,
                                                       const float* __restrict__ eps, float a,
                                                       float k, float2* __restrict__ ws, int T,
                                                       const sp_step_rec* __restrict__ sched,
                                                       const int32_t* __restrict__ cursor) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (X0 && sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = sched[*cursor].c;
        a = cf.a, k = cf.k;
    }
    const phase_geom g(op);
    const int N = g.Nw, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.H + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int h0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    SP_DCHECK(c < g.C && h0 < g.H);
    const float* __restrict__ ip = in + plane * g.H * g.W;
    const float* __restrict__ ep = X0 ? eps + plane * g.H * g.W : nullptr;

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t) {
        const int h = h0 + t;
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float val = 0.f;
            const int j = q - g.pw;
            if (h < g.H && j >= 0 && j < g.W) {
                SP_DCHECK(h * g.W + j < g.H * g.W);
                val = ip[h * g.W + j];
                if constexpr (X0) val = (val - k * ep[h * g.W + j]) / a;
            }
            A[t * NP + phase_slot(q)] = make_float2(val, 0.f);
        }
    }
    __syncthreads();
    const float2* res = phase_fft(A, B, tw, N, NP, T, false);
    // transposed store: ws[plane][kw][h], the tile's rows adjacent
    float2* __restrict__ wp = ws + plane * (int64_t)N * g.H;
    const int total = T * N;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, h = h0 + t;
        if (h < g.H) {
            SP_DCHECK(kw < N && kw * g.H + h < N * g.H);
            wp[kw * g.H + h] = res[t * NP + phase_slot(kw)];
        }
    }
}

// launch 2
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_phase_cols(sp_op op, float2* __restrict__ ws,
                                                       const float* __restrict__ yg, int64_t y_div,
                                                       float gs, float* __restrict__ yout,
                                                       float* __restrict__ partial, int P, int T,
                                                       const sp_step_rec* __restrict__ sched,
                                                       const int32_t* __restrict__ cursor) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    if (MODE == PH_RESIDUAL && sched) gs = sched[*cursor].c.grad_scale;
    const phase_geom g(op);
    const int N = g.Nh, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.Nw + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int kw0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t b = blockIdx.y;
    const int64_t plane = b * g.C + c;
    SP_DCHECK(c < g.C && kw0 < g.Nw && (MODE != PH_RESIDUAL || static_cast<int>(blockIdx.x) < P));
    float2* __restrict__ wp = ws + (plane * g.Nw + kw0) * (int64_t)g.H;  // the tile's columns
    const int lines = min(T, g.Nw - kw0);

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t)
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float2 val = make_float2(0.f, 0.f);
            const int h = q - g.ph;
            if (t < lines && h >= 0 && h < g.H) val = wp[t * g.H + h];
            A[t * NP + phase_slot(q)] = val;
        }
    __syncthreads();
    float2* z = phase_fft(A, B, tw, N, NP, T, false);

    // pointwise step over the whole columns: the tile's columns adjacent (y is row-major)
    const float s = 1.f / sqrtf((float)g.Nh * (float)g.Nw);  // "ortho", both axes
    const int64_t yrow = MODE == PH_RESIDUAL ? b / y_div : b;
    const int64_t yoff = (yrow * g.C + c) * (int64_t)g.Nh * g.Nw + kw0;
    float racc = 0.f;
    const int total = T * N;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kh = idx / T, t = idx - kh * T;
        if (t >= lines) continue;
        SP_DCHECK(kh < N && kw0 + t < g.Nw);
        float2* zp = z + t * NP + phase_slot(kh);
        const float2 zz = make_float2(zp->x * s, zp->y * s);
        const float mag = sqrtf(zz.x * zz.x + zz.y * zz.y);
        const int64_t yi = yoff + (int64_t)kh * g.Nw + t;
        if constexpr (MODE == PH_APPLY) {
            yout[yi] = mag;
        } else {
            float coef = yg[yi];  // VJP: the cotangent g
            if constexpr (MODE == PH_RESIDUAL) {
                const float r = coef - mag;
                racc += r * r;
                coef = gs * r;
            }
            // u = coef z / |z| (0 at |z| = 0), times the inverse transform's "ortho" factor
            const float q = mag > 0.f ? coef * s / mag : 0.f;
            *zp = make_float2(q * zz.x, q * zz.y);
        }
    }
    if constexpr (MODE == PH_RESIDUAL) {
        const float tsum = block_sum(racc, red);
        if (threadIdx.x == 0) partial[b * P + blockIdx.x] = tsum;
    }
    if constexpr (MODE == PH_APPLY) return;
    __syncthreads();
    const float2* u = phase_fft(z, z == A ? B : A, tw, N, NP, T, true);
    const int keep = lines * g.H;
    for (int idx = threadIdx.x; idx < keep; idx += kBlock) {
        const int t = idx / g.H, h = idx - t * g.H;
        SP_DCHECK(t < lines && g.ph + h < N);
        wp[idx] = u[t * NP + phase_slot(g.ph + h)];
    }
}

// launch 3
__global__ __launch_bounds__(kBlock) void k_phase_rows_inv(sp_op op, const float2* __restrict__ ws,
                                                           float* __restrict__ out, int T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const phase_geom g(op);
    const int N = g.Nw, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.H + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int h0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    SP_DCHECK(c < g.C && h0 < g.H);
    const float2* __restrict__ wp = ws + plane * (int64_t)N * g.H;

    phase_twiddles(tw, N);
    const int total = T * N;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, h = h0 + t;
        float2 val = make_float2(0.f, 0.f);
        if (h < g.H) {
            SP_DCHECK(kw * g.H + h < N * g.H);
            val = wp[kw * g.H + h];
        }
        A[t * NP + phase_slot(kw)] = val;
    }
    __syncthreads();
    const float2* res = phase_fft(A, B, tw, N, NP, T, true);
    float* __restrict__ op_out = out + plane * g.H * g.W;
    for (int t = 0; t < T; ++t) {
        const int h = h0 + t;
        if (h >= g.H) break;
        for (int j = threadIdx.x; j < g.W; j += kBlock) {
            SP_DCHECK(g.pw + j < N && h * g.W + j < g.H * g.W);
            op_out[h * g.W + j] = res[t * NP + phase_slot(g.pw + j)].x;
        }
    }
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip; `op` is valid)
// ---------------------------------------------------------------------------
bool phase_valid(const sp_op* op) {  // radius = pad_h, factor = pad_w
    return !op->taps && !op->keep_bits && !op->word_rank && op->radius >= 0 && op->factor >= 0 &&
           op->channels > 0 && op->height > 0 && op->width > 0 && op->height <= 1024 &&
           op->width <= 1024 && op->radius <= 512 && op->factor <= 512 &&
           phase_size_ok(op->height + 2 * op->radius) && phase_size_ok(op->width + 2 * op->factor) &&
           (int64_t)op->channels * op->height * op->width == op->n &&
           (int64_t)op->channels * (op->height + 2 * op->radius) * (op->width + 2 * op->factor) == op->m;
}

static inline int phase_col_tiles(const sp_op* op) {
    const phase_geom g(*op);
    const int T = phase_lines(g.Nh);
    return (g.Nw + T - 1) / T;
}
static inline int phase_row_tiles(const sp_op* op) {
    const phase_geom g(*op);
    const int T = phase_lines(g.Nw);
    return (g.H + T - 1) / T;
}

// column tiles per sample = workgroups per sample of launch 2 = r^2 partials per sample
int64_t phase_partials(const sp_op* op) { return (int64_t)op->channels * phase_col_tiles(op); }

// floats of the intermediate
int64_t phase_workspace(const sp_op* op, int64_t batch) {
    const phase_geom g(*op);
    return 2 * batch * g.C * (int64_t)g.Nw * g.H;
}

// The launches go through fft_stage (sp_fft.h).  rows (x -> ws), then the column pass of MODE:
// PH_APPLY (-> y) or PH_VJP (gy -> ws)
template <int MODE>
static int phase_forward(const char* what, const sp_op* op, const float* x, const float* gy, float* y,
                         int64_t batch, float2* ws, hipStream_t s) {
    const phase_geom g(*op);
    const int rc = fft_stage(what, 0, 0.0, k_phase_rows<false>, g.C * phase_row_tiles(op), batch, g.Nw,
                             s, *op, x, kNoIn, 1.f, 0.f, ws, phase_lines(g.Nw), kNoSched, kNoCursor);
    if (rc != SP_OK) return rc;
    return fft_stage(what, 0, 0.0, k_phase_cols<MODE>, g.C * phase_col_tiles(op), batch, g.Nh, s, *op,
                     ws, gy, (int64_t)1, 0.f, y, kNoOut, 0, phase_lines(g.Nh), kNoSched, kNoCursor);
}

// rows^-1 (ws -> out), the last launch of a pass
static int phase_rows_inv(const char* what, int kind, const sp_op* op, const float2* ws, float* out,
                          int64_t batch, hipStream_t s) {
    const phase_geom g(*op);
    return fft_stage(what, kind, 0.0, k_phase_rows_inv, g.C * phase_row_tiles(op), batch, g.Nw, s, *op,
                     ws, out, phase_lines(g.Nw));
}

int phase_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                hipStream_t s) {
    return phase_forward<PH_APPLY>("sp_op_apply_ws", op, x, nullptr, y, batch,
                                   reinterpret_cast<float2*>(work), s);
}

int phase_vjp(const sp_op* op, const float* x, const float* gy, float* dx, int64_t batch,
              float* work, hipStream_t s) {
    float2* ws = reinterpret_cast<float2*>(work);
    const int rc = phase_forward<PH_VJP>("sp_op_vjp_ws", op, x, gy, nullptr, batch, ws, s);
    return rc == SP_OK ? phase_rows_inv("sp_op_vjp_ws", 0, op, ws, dx, batch, s) : rc;
}

// rows (x, eps -> work), columns (work, y -> work, partials), rows^-1 (work -> v)
int phase_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const phase_geom g(*op);
    const char* what = "sp_dps_residual_ws";
    float2* ws = reinterpret_cast<float2*>(r.work);
    const int P = static_cast<int>(phase_partials(op));
    int rc = fft_stage(what, TK_DPS_RESIDUAL, (double)r.batch, k_phase_rows<true>,
                       g.C * phase_row_tiles(op), r.batch, g.Nw, s, *op, r.x, r.eps, r.a, r.k, ws,
                       phase_lines(g.Nw), r.sched, r.cursor);
    if (rc == SP_OK)
        rc = fft_stage(what, TK_DPS_RESIDUAL, 0.0, k_phase_cols<PH_RESIDUAL>, P, r.batch, g.Nh, s, *op,
                       ws, r.y, r.y_div, r.gs, kNoOut, r.partial, P, phase_lines(g.Nh), r.sched,
                       r.cursor);
    return rc == SP_OK ? phase_rows_inv(what, TK_DPS_RESIDUAL, op, ws, r.v, r.batch, s) : rc;
}

}  // namespace sp
