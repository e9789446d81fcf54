// Channel mixing (SP_OP_CHANNEL_MIX): y = M x across the channel axis at every pixel, M a small
// Cy x C matrix (colorization, a colour-correction or sensor-response matrix, spectral bands mixed
// down to RGB).  A is block-diagonal over the pixels, so A^T, A^+, the proximal map and the DDRM
// spectral update are local to one pixel: every entry point that takes an sp_op is ONE launch over
// x with no halo and no workspace (the reference has no such operator; semantics in
// operators/channel_mix.py).  The tables of the descriptor (samplers_hip.h: M, N = A^+, U, V, S, P,
// fp32, taken as exact) are staged in LDS once per workgroup and read at wave-uniform addresses.
//
// Tile: a thread owns one group of pixels in all C planes of x (and all Cy planes of y).  With
// H W % 4 == 0 a group is four consecutive pixels and every access one float4 per plane (PW = 4),
// otherwise one pixel and scalar access (PW = 1).  Consecutive lanes take consecutive groups, so
// one load instruction of a wave covers contiguous bytes of a plane; all plane loads of a thread
// are issued before any arithmetic.  A workgroup of 256 threads covers 256 groups: the tile.  The
// channel counts are run-time: the kernels are built for CT = 3, 4 or 8 planes (the smallest
// CT >= C), their loops over channels and components fully unrolled to CT with a wave-uniform
// guard `index < C` (or `< Cy`) around each trip, so every plane stays in registers whatever C and
// Cy are ("Channel-mixing operator").
//
// Arithmetic (contraction off in the whole file: every product and every sum rounds on its own,
// but for the one explicit fma noted below).
// dot(t, v; K) below is the sum over k = 0 .. K-1 in ascending order, left to right:
//   t[0] v[0], then acc = acc + t[k] v[k].
//   A        y[i] = dot(M[i][.], x; C)             A^T    x[c] = dot(M[.][c], y; Cy)
//   A^+      x[c] = dot(N[c][.], y; Cy)            A^+T   y[i] = dot(N[.][i], x; C)
//   DPS      x0[c] = fma(-k, eps[c], x[c]) / a;  r[i] = y[i] - dot(M[i][.], x0; C);  g[i] = gs r[i];
//            v[c] = dot(M[.][c], g; Cy);  the thread's r^2: acc = acc + r[i][e] r[i][e] over i
//            ascending, inside i over its pixels e ascending; one partial per tile (block_sum).
//   PGDM     x0 and r as DPS;  v[c] = gs dot(N[c][.], r; Cy)   (gs = -2 from the sampler)
//   prox     x0 = x (sp_op_prox_ws) or (x - k eps) (1 / a) (sp_diffpir_step_ws);  r as DPS;
//            t[j] = dot(U[.][j], r; Cy);  d[j] = (S[j] / (S[j] S[j] + rho)) t[j];
//            z[c] = x0[c] + dot(V[c][.], d; Cy);  the step: x' = diffpir_update(x, z, xi) (sp_ops.h)
//   DDRM     x0 = (x - k eps) (1 / a);  ybar[j] = P[j] dot(U[.][j], y; Cy) for j < Cy;
//            f_j = ddrm_class_coefs(c, S[j] S[j], P[j] != 0) for j < Cy, (c, 0, false) for
//            Cy <= j < C (taken once per workgroup);  with a0 = dot(V[.][j], x0; C), ae the same
//            of eps and ax of xi:  w[j] = ((f_th a0 + f_ep ae) + f_y ybar[j]) + f_xi ax for j < Cy,
//            w[j] = (f_th a0 + f_ep ae) + f_xi ax for j >= Cy;  x'[c] = a_prev dot(V[c][.], w; C)
// The one fused operation is the numerator of x0 in pass 1 of DPS and PGDM: x - k eps rounds once,
// as in pass 1 of the elementwise kinds (their expression compiles to that fused multiply-add), so
// M = I gives SP_OP_IDENTITY's v bit for bit.  It is written as an explicit fma, not left to the
// compiler.
// xi is read, or drawn by Philox at the flat element index of the group in every plane (the plane
// of sp_randn).  A group is read and written by its own lane alone, so the output may alias x.

#include <algorithm>

#define SP_TU 26  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

#pragma clang fp contract(off)

namespace sp {

constexpr int kCmMax = 8;  // the widest C

// offsets of the tables in taps (and in LDS), in floats
struct cm_tabs {
    int M, N, U, V, S, P, total;
    __host__ __device__ cm_tabs(int C, int Cy)
        : M(0), N(Cy * C), U(2 * Cy * C), V(2 * Cy * C + Cy * Cy), S(2 * Cy * C + Cy * Cy + C * C),
          P(2 * Cy * C + Cy * Cy + C * C + Cy), total(2 * Cy * C + Cy * Cy + C * C + 2 * Cy) {}
};
constexpr int kCmTabMax = 2 * 64 + 64 + 64 + 16;

// where the thread's group lies: its offset inside a plane, and whether it exists
template <int PW>
struct cm_group {
    int64_t hw, off;
    bool in;
    __device__ __forceinline__ cm_group(const sp_op& op) {
        hw = (int64_t)op.height * op.width;
        const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
        in = g * PW < hw;
        off = in ? g * PW : 0;
        SP_DCHECK(off >= 0 && off + PW <= hw && hw * op.channels == op.n && hw * op.radius == op.m);
    }
};

__device__ __forceinline__ void cm_stage(const sp_op& op, float* __restrict__ tab) {
    const cm_tabs t(op.channels, op.radius);
    SP_DCHECK(t.total <= kCmTabMax);
    for (int i = threadIdx.x; i < t.total; i += kBlock) tab[i] = op.taps[i];
    __syncthreads();
}

// planes 0 .. K-1 of one row (K <= CT), the group at `off`
template <int CT, int PW, bool NT = false>
__device__ __forceinline__ void cm_load(const float* __restrict__ row, int64_t hw, int64_t off, int K,
                                        float (&r)[CT][PW]) {
#pragma unroll
    for (int c = 0; c < CT; ++c)
        if (c < K) load_v<PW, NT>(row + c * hw + off, r[c]);
}

// o = dot(t[0], t[stride], ..; v; K): ascending, every product and sum on its own
template <int CT, int PW>
__device__ __forceinline__ void cm_dot(const float* __restrict__ t, int stride, int K,
                                       const float (&v)[CT][PW], float (&o)[PW]) {
    const float t0 = t[0];
#pragma unroll
    for (int e = 0; e < PW; ++e) o[e] = t0 * v[0][e];
#pragma unroll
    for (int k = 1; k < CT; ++k)
        if (k < K) {
            const float tk = t[k * stride];
#pragma unroll
            for (int e = 0; e < PW; ++e) o[e] = o[e] + tk * v[k][e];
        }
}

// out[r] = dot(tab[toff + r rs + k ks], in[k]; K) for r < R: the four maps
template <int CT, int PW>
__global__ __launch_bounds__(kBlock) void k_cm_map(sp_op op, const float* __restrict__ in,
                                                   float* __restrict__ out, int toff, int R, int K,
                                                   int rs, int ks) {
    __shared__ float tab[kCmTabMax];
    cm_stage(op, tab);
    const cm_group<PW> g(op);
    if (!g.in) return;
    const int64_t b = blockIdx.y;
    float v[CT][PW] = {};
    cm_load<CT, PW>(in + b * K * g.hw, g.hw, g.off, K, v);
    // a real loop over the output rows: r indexes the table and the output plane alone
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        float o[PW];
        cm_dot<CT, PW>(tab + toff + r * rs, ks, K, v, o);
        store_v<PW>(out + (b * R + r) * g.hw + g.off, o);
    }
}

// pass 1 of DPS (PINV false: v = M^T (gs r), r^2 partials) and of PGDM (PINV true: v = gs N r)
template <int CT, int PW, bool PINV>
__global__ __launch_bounds__(kBlock) void k_cm_residual(sp_op op, const float* __restrict__ x,
                                                        const float* __restrict__ eps,
                                                        const float* __restrict__ y, int64_t y_div,
                                                        float a, float k, float gs,
                                                        float* __restrict__ v,
                                                        float* __restrict__ partial, int P,
                                                        const sp_step_rec* __restrict__ sched,
                                                        const int32_t* __restrict__ cursor) {
    __shared__ float tab[kCmTabMax];
    __shared__ float red[4];
    cm_stage(op, tab);
    if (sched) {  // device-resident schedule (graph replay): uniform scalar loads
        const sp_dps_coefs& c = sched[*cursor].c;
        a = c.a, k = c.k, gs = c.grad_scale;
    }
    const int C = op.channels, Cy = op.radius;
    const cm_tabs t(C, Cy);
    const cm_group<PW> g(op);
    const int64_t b = blockIdx.y;
    float xv[CT][PW] = {}, ev[CT][PW] = {}, rv[CT][PW] = {};
    if (g.in) {  // every load of the group first (memory-level parallelism), then compute
        cm_load<CT, PW, true>(x + b * op.n, g.hw, g.off, C, xv);
        cm_load<CT, PW, true>(eps + b * op.n, g.hw, g.off, C, ev);
        cm_load<CT, PW>(y + (b / y_div) * op.m, g.hw, g.off, Cy, rv);
    }
    if (g.in) {  // an absent group keeps its zeros whatever a is
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[c][e] = __builtin_fmaf(-k, ev[c][e], xv[c][e]) / a;  // x0
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < CT; ++i)
        if (i < Cy) {
            float ax[PW];
            cm_dot<CT, PW>(tab + t.M + i * C, 1, C, xv, ax);
#pragma unroll
            for (int e = 0; e < PW; ++e) {
                const float r = rv[i][e] - ax[e];
                if constexpr (!PINV) acc = acc + r * r;  // an absent group holds zeros
                rv[i][e] = PINV ? r : gs * r;
            }
        }
    if (g.in) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (c < C) {
                float o[PW];
                if constexpr (PINV) {
                    cm_dot<CT, PW>(tab + t.N + c * Cy, 1, Cy, rv, o);
#pragma unroll
                    for (int e = 0; e < PW; ++e) o[e] = gs * o[e];
                } else {
                    cm_dot<CT, PW>(tab + t.M + c, C, Cy, rv, o);
                }
                store_v<PW>(v + b * op.n + c * g.hw + g.off, o);
            }
    }
    if constexpr (!PINV) {
        const float s = block_sum(acc, red);
        SP_DCHECK(static_cast<int>(blockIdx.x) < P);
        if (threadIdx.x == 0) partial[b * P + blockIdx.x] = s;
    }
}

// xi of the group in planes 0 .. C-1: read, or drawn at the flat element index c H W + off
template <int CT, int PW, bool XI_IN>
__device__ __forceinline__ void cm_noise(const float* __restrict__ xi, uint64_t seed, int64_t step,
                                         int64_t sample_offset, int64_t b, const sp_op& op,
                                         const cm_group<PW>& g, float (&nz)[CT][PW]) {
#pragma unroll
    for (int c = 0; c < CT; ++c)
        if (c < op.channels) {
            SP_DCHECK(PW == 1 || (c * g.hw + g.off) % 4 == 0);
            noise_v<PW, XI_IN>(xi, seed, step, sample_offset, b, op.n, c * g.hw + g.off, nz[c]);
        }
}

// The proximal data step, z = x0 + V diag(S / (S^2 + rho)) U^T (y - M x0) over all Cy singular
// values (exact for the full M): alone (STEP false, x holds x0) or inside the DiffPIR step.
template <int CT, int PW, bool STEP, bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_cm_prox(sp_op op, const float* __restrict__ x,
                                                    const float* __restrict__ eps,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ xi, uint64_t seed,
                                                    int64_t step, int64_t sample_offset,
                                                    int64_t y_div, sp_prox_coefs c,
                                                    float* __restrict__ out) {
    __shared__ float tab[kCmTabMax];
    cm_stage(op, tab);
    const int C = op.channels, Cy = op.radius;
    const cm_tabs t(C, Cy);
    const cm_group<PW> g(op);
    if (!g.in) return;
    const int64_t b = blockIdx.y;
    float xv[CT][PW] = {}, zv[CT][PW] = {}, rv[CT][PW] = {}, nz[CT][PW] = {};
    cm_load<CT, PW, true>(x + b * op.n, g.hw, g.off, C, xv);
    if constexpr (STEP) cm_load<CT, PW, true>(eps + b * op.n, g.hw, g.off, C, zv);
    cm_load<CT, PW>(y + (b / y_div) * op.m, g.hw, g.off, Cy, rv);
    if constexpr (STEP) cm_noise<CT, PW, XI_IN>(xi, seed, step, sample_offset, b, op, g, nz);
    const float inv_a = STEP ? 1.f / c.a : 1.f, inv_k = STEP ? 1.f / c.k : 1.f;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
#pragma unroll
        for (int e = 0; e < PW; ++e)
            zv[ch][e] = STEP ? (xv[ch][e] - c.k * zv[ch][e]) * inv_a : xv[ch][e];  // x0
#pragma unroll
    for (int i = 0; i < CT; ++i)
        if (i < Cy) {
            float ax[PW];
            cm_dot<CT, PW>(tab + t.M + i * C, 1, C, zv, ax);
#pragma unroll
            for (int e = 0; e < PW; ++e) rv[i][e] = rv[i][e] - ax[e];
        }
    float dv[CT][PW] = {};
#pragma unroll
    for (int j = 0; j < CT; ++j)
        if (j < Cy) {
            const float s = tab[t.S + j];
            const float w = s / (s * s + c.rho);
            cm_dot<CT, PW>(tab + t.U + j, Cy, Cy, rv, dv[j]);
#pragma unroll
            for (int e = 0; e < PW; ++e) dv[j][e] = w * dv[j][e];
        }
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
        if (ch < C) {
            float o[PW];
            cm_dot<CT, PW>(tab + t.V + ch * C, 1, Cy, dv, o);
#pragma unroll
            for (int e = 0; e < PW; ++e) {
                const float z = zv[ch][e] + o[e];
                o[e] = STEP ? diffpir_update(c, inv_k, xv[ch][e], z, nz[ch][e]) : z;
            }
            store_v<PW, STEP>(out + b * op.n + ch * g.hw + g.off, o);
        }
}

// The DDRM step on the SVD of M (file comment): the spectral form over the full V, the C - Cy
// null-space components unobserved.
template <int CT, int PW, bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_cm_ddrm(sp_op op, const float* __restrict__ x,
                                                    const float* __restrict__ eps,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ xi, uint64_t seed,
                                                    int64_t step, int64_t sample_offset,
                                                    int64_t y_div, sp_ddrm_coefs c,
                                                    float* __restrict__ out) {
    __shared__ float tab[kCmTabMax];
    __shared__ ddrm_f fs[kCmMax];
    const int C = op.channels, Cy = op.radius;
    const cm_tabs t(C, Cy);
    if (static_cast<int>(threadIdx.x) < C) {  // the class of every component, once per workgroup
        const int j = threadIdx.x;
        const float s = j < Cy ? op.taps[t.S + j] : 0.f;
        fs[j] = ddrm_class_coefs(c, s * s, j < Cy && op.taps[t.P + j] != 0.f);
    }
    cm_stage(op, tab);  // its barrier publishes fs too
    const cm_group<PW> g(op);
    if (!g.in) return;
    const int64_t b = blockIdx.y;
    float xv[CT][PW] = {}, ev[CT][PW] = {}, yv[CT][PW] = {}, nz[CT][PW] = {};
    cm_load<CT, PW, true>(x + b * op.n, g.hw, g.off, C, xv);
    cm_load<CT, PW, true>(eps + b * op.n, g.hw, g.off, C, ev);
    cm_load<CT, PW>(y + (b / y_div) * op.m, g.hw, g.off, Cy, yv);
    cm_noise<CT, PW, XI_IN>(xi, seed, step, sample_offset, b, op, g, nz);
    const float inv_a = 1.f / c.a;
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
#pragma unroll
        for (int e = 0; e < PW; ++e) xv[ch][e] = (xv[ch][e] - c.k * ev[ch][e]) * inv_a;  // x0
    float wv[CT][PW] = {};
#pragma unroll
    for (int j = 0; j < CT; ++j)
        if (j < C) {
            const ddrm_f f = fs[j];
            float a0[PW], ae[PW], ax[PW];
            cm_dot<CT, PW>(tab + t.V + j, C, C, xv, a0);
            cm_dot<CT, PW>(tab + t.V + j, C, C, ev, ae);
            cm_dot<CT, PW>(tab + t.V + j, C, C, nz, ax);
            if (j < Cy) {
                const float p = tab[t.P + j];
                float yb[PW];
                cm_dot<CT, PW>(tab + t.U + j, Cy, Cy, yv, yb);
#pragma unroll
                for (int e = 0; e < PW; ++e)
                    wv[j][e] = ((f.th * a0[e] + f.ep * ae[e]) + f.y * (p * yb[e])) + f.xi * ax[e];
            } else {
#pragma unroll
                for (int e = 0; e < PW; ++e) wv[j][e] = (f.th * a0[e] + f.ep * ae[e]) + f.xi * ax[e];
            }
        }
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
        if (ch < C) {
            float o[PW];
            cm_dot<CT, PW>(tab + t.V + ch * C, 1, C, wv, o);
#pragma unroll
            for (int e = 0; e < PW; ++e) o[e] = c.a_prev * o[e];
            store_v<PW, true>(out + b * op.n + ch * g.hw + g.off, o);
        }
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip; `op` is valid)
// ---------------------------------------------------------------------------
static inline int64_t cm_plane(const sp_op* op) { return (int64_t)op->height * op->width; }
static inline bool cm_vec(const sp_op* op) { return cm_plane(op) % 4 == 0; }

bool chanmix_valid(const sp_op* op) {
    if (op->channels < 1 || op->channels > kCmMax || op->radius < 1 || op->radius > op->channels ||
        op->factor != 0 || !op->taps || op->keep_bits || op->word_rank || op->height < 1 ||
        op->width < 1)
        return false;
    const int64_t hw = cm_plane(op);
    return hw <= 0x7fffffff && hw * op->channels == op->n && hw * op->radius == op->m;
}

// tiles per sample = r^2 partials per sample: 256 groups of 4 pixels (H W % 4 == 0) or of 1
int64_t chanmix_partials(const sp_op* op) {
    return cdiv(cm_vec(op) ? cm_plane(op) / 4 : cm_plane(op), kBlock);
}

// f(CT, PW) for the operator's channel count and path
template <typename F>
static void cm_select(const sp_op* op, F&& f) {
    select_width(cm_plane(op), [&](auto pw) {
        if (op->channels <= 3) f(int_c<3>{}, pw);
        else if (op->channels == 4) f(int_c<4>{}, pw);
        else f(int_c<kCmMax>{}, pw);
    });
}

static dim3 cm_grid(const sp_op* op, int64_t batch) { return sample_grid(chanmix_partials(op), batch); }

// one of the four maps: rows R of the output, K of the input, the table's offset and strides
static int cm_map(const sp_op* op, const float* in, float* out, int64_t batch, int toff, int R, int K,
                  int rs, int ks, const char* what, hipStream_t s) {
    cm_select(op, [&](auto ct, auto pw) {
        launch(0, k_cm_map<ct(), pw()>, cm_grid(op, batch), dim3(kBlock), s, *op, in, out, toff, R, K,
               rs, ks);
    });
    return check_launch(what);
}

int chanmix_apply(const sp_op* op, const float* x, float* y, int64_t batch, hipStream_t s) {
    const int C = op->channels, Cy = op->radius;
    return cm_map(op, x, y, batch, cm_tabs(C, Cy).M, Cy, C, C, 1, "sp_op_apply (channel mix)", s);
}

int chanmix_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, hipStream_t s) {
    const int C = op->channels, Cy = op->radius;
    return cm_map(op, y, x, batch, cm_tabs(C, Cy).M, C, Cy, 1, C, "sp_op_adjoint (channel mix)", s);
}

// A^+ (y -> x, from N) or A^+T (x -> y, from N^T); no workspace
int chanmix_pinv(const sp_op* op, const float* in, float* out, int64_t batch, int transpose,
                 float* /*work*/, hipStream_t s) {
    const int C = op->channels, Cy = op->radius, N = cm_tabs(C, Cy).N;
    return transpose ? cm_map(op, in, out, batch, N, Cy, C, 1, Cy, "sp_op_pinv_ws (channel mix)", s)
                     : cm_map(op, in, out, batch, N, C, Cy, Cy, 1, "sp_op_pinv_ws (channel mix)", s);
}

int chanmix_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const int P = static_cast<int>(chanmix_partials(op));
    cm_select(op, [&](auto ct, auto pw) {
        launch_w(TK_DPS_RESIDUAL, (double)r.batch, k_cm_residual<ct(), pw(), false>,
                 cm_grid(op, r.batch), dim3(kBlock), s, *op, r.x, r.eps, r.y, r.y_div, r.a, r.k, r.gs,
                 r.v, r.partial, P, r.sched, r.cursor);
    });
    return check_launch("sp_dps_residual (channel mix)");
}

// nothing to prepare: the PGDM launch reads the observation rows themselves (q = y, not written)
int chanmix_pgdm_prepare(const sp_op*, const float*, int64_t, float*, hipStream_t) { return SP_OK; }

int chanmix_pgdm_residual(const sp_op* op, const float* x, const float* eps, const float* q,
                          int64_t batch, int64_t y_div, const sp_dps_coefs& c, float* v,
                          float* /*work*/, hipStream_t s) {
    cm_select(op, [&](auto ct, auto pw) {
        launch(0, k_cm_residual<ct(), pw(), true>, cm_grid(op, batch), dim3(kBlock), s, *op, x, eps, q,
               y_div, c.a, c.k, c.grad_scale, v, static_cast<float*>(nullptr), 0,
               static_cast<const sp_step_rec*>(nullptr), static_cast<const int32_t*>(nullptr));
    });
    return check_launch("sp_pgdm_residual_ws (channel mix)");
}

// one launch, alone (p.eps null) or inside the DiffPIR step (xi read or drawn)
int chanmix_prox(const sp_op* op, const prox_args& p, hipStream_t s) {
    cm_select(op, [&](auto ct, auto pw) {
        select_bool(p.eps, [&](auto step) {
            select_bool(p.xi, [&](auto xin) {  // the prox form has no noise: one kernel
                launch(0, k_cm_prox<ct(), pw(), step(), step() && xin()>, cm_grid(op, p.batch),
                       dim3(kBlock), s, *op, p.x, p.eps, p.y, p.xi, p.seed, p.step, p.sample_offset,
                       p.y_div, p.c, p.out);
            });
        });
    });
    return check_launch(p.eps ? "sp_diffpir_step_ws (channel mix)" : "sp_op_prox_ws (channel mix)");
}

int chanmix_ddrm(const sp_op* op, const ddrm_args& p, hipStream_t s) {
    cm_select(op, [&](auto ct, auto pw) {
        select_bool(p.xi, [&](auto xin) {
            launch(0, k_cm_ddrm<ct(), pw(), xin()>, cm_grid(op, p.batch), dim3(kBlock), s, *op, p.x,
                   p.eps, p.y, p.xi, p.seed, p.step, p.sample_offset, p.y_div, p.c, p.out);
        });
    });
    return check_launch("sp_ddrm_step_ws (channel mix)");
}

}  // namespace sp
