// DPS guidance hot path for IDENTITY and INPAINT operators (elementwise in
// x-space), plus the elementwise helpers every sampler uses (x0 prediction,
// Philox normals, y-space likelihood gradient, inpaint gather/scatter).
//
// Memory model: every kernel streams contiguous fp32 rows of n elements with
// one float4 per lane (1 KiB per wave-instruction); a block covers
// kIter*1024 consecutive elements of ONE sample, grid = (tiles, batch), so the
// per-sample residual norm is a fixed-order sum of per-block partials — no
// atomics, bitwise reproducible.  Observation rows y are read in the packed
// order of the reference (kept pixels ascending), the keep bit-mask and
// per-word ranks (12 B per 64 pixels) stay L2-resident.

#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#define SP_TU 1  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

namespace sp {

static thread_local char g_err[256] = "";

void set_error(const char* what, hipError_t e) {
    std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
}

int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(what, e);
        return SP_ELAUNCH;
    }
    return SP_OK;
}

#if SP_DEBUG
// readers of every translation unit's debug words (SP_DCHECK), registered at load time
static std::vector<dcheck_reader>& dcheck_readers() {
    static std::vector<dcheck_reader> v;
    return v;
}
void dcheck_register(dcheck_reader r) { dcheck_readers().push_back(r); }

// debug build self-test: every thread of one block states a false invariant (no memory access)
__global__ void k_dcheck_selftest(int limit) { SP_DCHECK(static_cast<int>(threadIdx.x) < limit); }
#endif

struct TimingRecord {
    int kind;
    double work;
    hipEvent_t start, stop;
};
static std::mutex g_timing_mu;
static bool g_timing = false;
static std::vector<TimingRecord> g_records;
static std::vector<hipEvent_t> g_event_pool;

bool timing_on() { return g_timing; }

static hipEvent_t take_event() {
    if (!g_event_pool.empty()) {
        hipEvent_t e = g_event_pool.back();
        g_event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void timing_events(int kind, double work, hipEvent_t* start, hipEvent_t* stop) {
    std::lock_guard<std::mutex> lock(g_timing_mu);
    *start = take_event();
    *stop = take_event();
    if (*start && *stop) g_records.push_back({kind, work, *start, *stop});
}

// ---------------------------------------------------------------------------
// K1: x0 -> residual -> v = A^T(grad_scale * r), per-block sum r^2
// ---------------------------------------------------------------------------
#ifndef SP_UPD_NT
#define SP_UPD_NT 1  // non-temporal loads of the DPS passes' once-read streams (measured +4-5 %)
#endif
template <int OPK, int V>
__global__ __launch_bounds__(kBlock) void k_dps_residual(sp_op op, const float* __restrict__ x,
                                                         const float* __restrict__ eps,
                                                         const float* __restrict__ y, int64_t y_div,
                                                         float a, float k, float gs,
                                                         float* __restrict__ v,
                                                         float* __restrict__ partial, int P,
                                                         const sp_step_rec* __restrict__ sched,
                                                         const int32_t* __restrict__ cursor) {
    __shared__ float red[4];
    if (sched) {  // device-resident schedule (graph replay): uniform scalar loads
        const sp_dps_coefs& c = sched[*cursor].c;
        a = c.a, k = c.k, gs = c.grad_scale;
    }
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const float* xb = x + b * n;
    const float* eb = eps + b * n;
    const float* yb = y + (b / y_div) * op.m;
    float* vb = v + b * n;
    const int64_t j0 = (int64_t)blockIdx.x * kIter * (kBlock * V) + threadIdx.x * V;
    // issue every load of the tile first (memory-level parallelism), then compute
    float xv[kIter][V], ev[kIter][V];
    obs_tile<OPK, V> yt;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            load_v<V, SP_UPD_NT>(xb + j, xv[it]);
            load_v<V, SP_UPD_NT>(eb + j, ev[it]);
            yt.issue(op, yb, j, it);
        }
    }
    yt.gather(op, yb, j0);
    const auto& yv = yt.y;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            float vv[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const bool kept = yt.kept(it, e);
                const float x0 = (xv[it][e] - k * ev[it][e]) / a;
                // MASK: unobserved pixels still add y^2 to the residual (A x0 = 0 there)
                const float r = yv[it][e] - (kept ? x0 : 0.f);
                vv[e] = kept ? gs * r : 0.f;
                if (OPK != SP_OP_INPAINT || kept) acc += r * r;
            }
            store_v<V>(vb + j, vv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) partial[b * P + blockIdx.x] = t;
}

// ---------------------------------------------------------------------------
// K2: bridge mean + std*xi + gamma/(||r_b|| + eps) * (v - k*w)/a
// ---------------------------------------------------------------------------
#ifndef SP_UPD_RCP
#define SP_UPD_RCP 1  // 1: multiply by 1/a instead of dividing (1 ulp from the reference's division)
#endif
#ifndef SP_UPD_WAVES
#define SP_UPD_WAVES 5  // waves per SIMD the update pass is built for (<= 80 VGPRs, see below)
#endif
// 6 waves per SIMD = 6 blocks per CU = 1536 resident blocks: the 3072 blocks of the B = 64,
// 256^2 step run in exactly two rounds (at 5, 83 VGPRs, they took 2.4 with a partial tail)
template <int OPK, int V, bool V_IN, bool XI_IN>
__global__ __launch_bounds__(kBlock, SP_UPD_WAVES) void k_dps_update(
    sp_op op, const float* __restrict__ x, const float* __restrict__ eps,
    const float* __restrict__ y, const float* __restrict__ v, const float* __restrict__ w,
    const float* __restrict__ partial, int P, const float* __restrict__ xi, uint64_t seed,
    int64_t step, int64_t sample_offset, int64_t y_div, sp_dps_coefs c, float* __restrict__ xo,
    const sp_step_rec* __restrict__ sched, const int32_t* __restrict__ cursor) {
    if (sched) {  // device-resident schedule (graph replay)
        const sp_step_rec& rec = sched[*cursor];
        c = rec.c;
        step = rec.step;
    }
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const float* xb = x + b * n;
    const float* eb = eps + b * n;
    const float* wb = w + b * n;
    const float* yb = y + (b / y_div) * op.m;
    float* ob = xo + b * n;
    const int64_t j0 = (int64_t)blockIdx.x * kIter * (kBlock * V) + threadIdx.x * V;
    float xv[kIter][V], ev[kIter][V], wv[kIter][V];
    obs_tile<OPK, V> yt;
    auto& yv = yt.y;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            load_v<V, SP_UPD_NT>(xb + j, xv[it]);
            load_v<V, SP_UPD_NT>(eb + j, ev[it]);
            load_v<V, SP_UPD_NT>(wb + j, wv[it]);
            if constexpr (V_IN) {
                load_v<V, SP_UPD_NT>(v + b * n + j, yv[it]);  // yv holds v in this variant
            } else {
                yt.issue(op, yb, j, it);
            }
        }
    }
    if constexpr (!V_IN) yt.gather(op, yb, j0);
    SP_DCHECK(!partial || P > 0);
    const float inv_a = 1.f / c.a;
    // DPS: gamma / (||r_b|| + eps); without partials a fixed factor (PGDM, PSLD)
    __shared__ float red4[4];
    const float scale =
        partial ? c.gamma / (sqrtf(block_sum_partials(partial + b * P, P, red4)) + c.norm_eps) : c.gamma;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            float z[V];
            noise_v<V, XI_IN>(xi, seed, step, sample_offset, b, n, j, z);
            float out[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float x0 = SP_UPD_RCP ? (xv[it][e] - c.k * ev[it][e]) * inv_a
                                            : (xv[it][e] - c.k * ev[it][e]) / c.a;
                float vv;
                if constexpr (V_IN) {
                    vv = yv[it][e];
                } else {
                    const bool kept = yt.kept(it, e);
                    vv = kept ? c.grad_scale * (yv[it][e] - x0) : 0.f;
                }
                const float mean = c.c_ell * xv[it][e] + c.c_s * x0;
                const float g = SP_UPD_RCP ? (vv - c.k * wv[it][e]) * inv_a : (vv - c.k * wv[it][e]) / c.a;
                out[e] = (mean + c.std * z[e]) + scale * g;
            }
            store_v<V, true>(ob + j, out);
        }
    }
}

// ---------------------------------------------------------------------------
// K3: the proximal data step of IDENTITY / INPAINT / MASK (A A^T = I), one launch:
//   z = x0 + A^T (y - A x0) / (1 + rho); unobserved pixels keep x0
// STEP false (sp_op_prox_ws): x holds x0, z is written.  STEP true (sp_diffpir_step_ws):
//   x0 = (x - k eps) / a,  eps_hat = (x - a z) / k,  x' = a_prev z + (c_eps eps_hat + c_xi xi)
// with xi read or drawn as in K2 (flat element index).  The three divisions are multiplications
// by reciprocals taken once per thread.  Same tiles as K2: a block covers kIter * kBlock * V
// consecutive elements of one sample, every element is read and written by one thread (the output
// may alias x).  Bytes per element: 12 + 4 per observed one (x, eps read, x' written, y read); the
// prox form 8 + 4; the keep words add 12 B per 64 elements.
// ---------------------------------------------------------------------------
template <int OPK, int V, bool STEP, bool XI_IN>
__global__ __launch_bounds__(kBlock, SP_UPD_WAVES) void k_prox(
    sp_op op, const float* __restrict__ x, const float* __restrict__ eps,
    const float* __restrict__ y, const float* __restrict__ xi, uint64_t seed, int64_t step,
    int64_t sample_offset, int64_t y_div, sp_prox_coefs c, float* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const float* xb = x + b * n;
    const float* eb = STEP ? eps + b * n : nullptr;
    const float* yb = y + (b / y_div) * op.m;
    float* ob = out + b * n;
    const int64_t j0 = (int64_t)blockIdx.x * kIter * (kBlock * V) + threadIdx.x * V;
    float xv[kIter][V], ev[kIter][V];
    obs_tile<OPK, V> yt;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            load_v<V, SP_UPD_NT>(xb + j, xv[it]);
            if constexpr (STEP) load_v<V, SP_UPD_NT>(eb + j, ev[it]);
            yt.issue(op, yb, j, it);
        }
    }
    yt.gather(op, yb, j0);
    const auto& yv = yt.y;
    const float inv_d = 1.f / (1.f + c.rho);
    const float inv_a = STEP ? 1.f / c.a : 1.f, inv_k = STEP ? 1.f / c.k : 1.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            float nz[V] = {};
            if constexpr (STEP) noise_v<V, XI_IN>(xi, seed, step, sample_offset, b, n, j, nz);
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
// every product and sum below rounds on its own: the bits are those of the expression as written,
// whichever noise form the kernel was built for
#pragma clang fp contract(off)
                const bool kept = yt.kept(it, e);
                const float x0 = STEP ? (xv[it][e] - c.k * ev[it][e]) * inv_a : xv[it][e];
                const float z = kept ? x0 + (yv[it][e] - x0) * inv_d : x0;
                o[e] = STEP ? diffpir_update(c, inv_k, xv[it][e], z, nz[e]) : z;
            }
            store_v<V, STEP>(ob + j, o);
        }
    }
}

// ---------------------------------------------------------------------------
// K4: the DDRM step of IDENTITY / INPAINT / MASK (A A^T = I: every singular value is 1 and V is
// the identity), one launch on K3's tiles and noise path.  With x0 = (x - k eps) / a:
//   observed    x' = a_prev ((f_th x0 + f_y y) + f_xi xi)          f of ddrm_class_coefs(c, 1, true)
//   unobserved  x' = a_prev ((x0 + (c1 sig_prev) eps) + (eta sig_prev) xi)
// Both coefficient sets are the same for every element, so the host takes them once per launch
// (ddrm_class_coefs is the one function on both sides).  Bytes per element: 12 + 4 per observed one
// (x, eps read, x' written, y read), + 4 with xi injected; the keep words add 12 B per 64.
// Roundings of the longest path (observed, small class): 1 / a, k eps, the difference, the product
// with 1 / a (4, x0); f_th = 1 - r with r = ((c1 sig_prev) sqrt(1)) / sig_y (4) and its product
// with x0 (1); two sums (2); the product with a_prev (1): 12.
// ---------------------------------------------------------------------------
template <int OPK, int V, bool XI_IN>
__global__ __launch_bounds__(kBlock, SP_UPD_WAVES) void k_ddrm(
    sp_op op, const float* __restrict__ x, const float* __restrict__ eps,
    const float* __restrict__ y, const float* __restrict__ xi, uint64_t seed, int64_t step,
    int64_t sample_offset, int64_t y_div, sp_ddrm_coefs c, ddrm_f fo, ddrm_f fu,
    float* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const float* xb = x + b * n;
    const float* eb = eps + b * n;
    const float* yb = y + (b / y_div) * op.m;
    float* ob = out + b * n;
    const int64_t j0 = (int64_t)blockIdx.x * kIter * (kBlock * V) + threadIdx.x * V;
    float xv[kIter][V], ev[kIter][V];
    obs_tile<OPK, V> yt;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            load_v<V, SP_UPD_NT>(xb + j, xv[it]);
            load_v<V, SP_UPD_NT>(eb + j, ev[it]);
            yt.issue(op, yb, j, it);
        }
    }
    yt.gather(op, yb, j0);
    const auto& yv = yt.y;
    const float inv_a = 1.f / c.a;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = j0 + it * (kBlock * V);
        if (j < n) {
            float nz[V];
            noise_v<V, XI_IN>(xi, seed, step, sample_offset, b, n, j, nz);
            float o[V];
#pragma unroll
            for (int e = 0; e < V; ++e) {
// every product and sum rounds on its own: the bits of the expression as written, in both noise forms
#pragma clang fp contract(off)
                const bool kept = yt.kept(it, e);
                const float x0 = (xv[it][e] - c.k * ev[it][e]) * inv_a;
                o[e] = kept ? c.a_prev * ((fo.th * x0 + fo.y * yv[it][e]) + fo.xi * nz[e])
                            : c.a_prev * ((x0 + fu.ep * ev[it][e]) + fu.xi * nz[e]);
            }
            store_v<V, true>(ob + j, o);
        }
    }
}

// ---------------------------------------------------------------------------
// elementwise helpers
// ---------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void k_predict_x0(const float* __restrict__ x,
                                                       const float* __restrict__ eps, int64_t count,
                                                       float a, float k, float* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock * V;
    for (int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V; j < count; j += stride) {
        float xv[V], ev[V], o[V];
        load_v<V>(x + j, xv);
        load_v<V>(eps + j, ev);
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = (xv[e] - k * ev[e]) / a;
        store_v<V>(out + j, o);
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_randn(float* __restrict__ out, int64_t n, uint64_t seed,
                                                  int64_t step, int64_t sample_offset) {
    const int64_t b = blockIdx.y;
    const int64_t stride = (int64_t)gridDim.x * kBlock * V;
    for (int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V; j < n; j += stride) {
        float z[V];
        philox_normals<V>(seed, step, sample_offset + b, j, z);
        store_v<V>(out + b * n + j, z);
    }
}

template <int V>
__global__ __launch_bounds__(kBlock) void k_residual_grad(const float* __restrict__ y,
                                                          const float* __restrict__ z, int64_t m,
                                                          int64_t y_div, float gs,
                                                          float* __restrict__ g,
                                                          float* __restrict__ partial, int P) {
    __shared__ float red[4];
    const int64_t b = blockIdx.y;
    const float* yb = y + (b / y_div) * m;
    const float* zb = z + b * m;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = ((int64_t)blockIdx.x * kIter + it) * (kBlock * V) + threadIdx.x * V;
        if (j < m) {
            float yv[V], zv[V], gv[V];
            load_v<V>(yb + j, yv);
            load_v<V>(zb + j, zv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float r = yv[e] - zv[e];
                gv[e] = gs * r;
                acc += r * r;
            }
            if (g) store_v<V>(g + b * m + j, gv);
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0 && partial) partial[b * P + blockIdx.x] = t;
}

// y[b][rank(j)] = x[b][j] for observed j (gather, inpainting.py:132-145)
template <int V>
__global__ __launch_bounds__(kBlock) void k_inpaint_gather(sp_op op, const float* __restrict__ x,
                                                           float* __restrict__ y) {
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const int64_t stride = (int64_t)gridDim.x * kBlock * V;
    for (int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V; j < n; j += stride) {
        float xv[V];
        load_v<V>(x + b * n + j, xv);
        uint32_t bits;
        int64_t rank;
        inpaint_lookup(op, j, bits, rank);
#pragma unroll
        for (int e = 0; e < V; ++e)
            if ((bits >> e) & 1u) y[b * op.m + rank++] = xv[e];
        SP_DCHECK(rank <= op.m);
    }
}

// x[b][j] = observed(j) ? y[b][rank(j)] : 0 (scatter into zeros, inpainting.py:169-187)
template <int V>
__global__ __launch_bounds__(kBlock) void k_inpaint_scatter(sp_op op, const float* __restrict__ y,
                                                            float* __restrict__ x) {
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const int64_t stride = (int64_t)gridDim.x * kBlock * V;
    for (int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V; j < n; j += stride) {
        float xv[V];
        uint32_t bits;
        int64_t rank;
        inpaint_lookup(op, j, bits, rank);
#pragma unroll
        for (int e = 0; e < V; ++e) xv[e] = ((bits >> e) & 1u) ? y[b * op.m + rank++] : 0.f;
        SP_DCHECK(rank <= op.m);
        store_v<V>(x + b * n + j, xv);
    }
}

// y = keep ? x : 0 (inpainting.py:106-109 / :180-187 with flatten=False); self-adjoint
template <int V>
__global__ __launch_bounds__(kBlock) void k_mask(sp_op op, const float* __restrict__ x,
                                                 float* __restrict__ y) {
    const int64_t b = blockIdx.y;
    const int64_t n = op.n;
    const int64_t stride = (int64_t)gridDim.x * kBlock * V;
    for (int64_t j = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V; j < n; j += stride) {
        float xv[V];
        load_v<V>(x + b * n + j, xv);
        const uint32_t bits = mask_bits(op, j);
#pragma unroll
        for (int e = 0; e < V; ++e) xv[e] = ((bits >> e) & 1u) ? xv[e] : 0.f;
        store_v<V>(y + b * n + j, xv);
    }
}

int64_t tiles_elementwise(int64_t n) {
    const int V = (n % 4 == 0) ? 4 : 1;
    return cdiv(n, (int64_t)kIter * kBlock * V);
}

// IDENTITY / INPAINT / MASK: one set of row functions (the latent passes: sp_latent.hip)
static bool identity_valid(const sp_op* op) { return op->m == op->n; }
static bool inpaint_valid(const sp_op* op) { return op->keep_bits && op->word_rank && op->m <= op->n; }
static bool mask_valid(const sp_op* op) { return op->keep_bits && op->m == op->n; }

static int64_t elementwise_partials(const sp_op* op) { return tiles_elementwise(op->n); }

// f(kind, width) for the elementwise kernel of `kind` over rows of n floats (select_width)
template <typename F>
static void select_elementwise(int kind, int64_t n, F&& f) {
    select_width(n, [&](auto v) {
        switch (kind) {
            case SP_OP_IDENTITY: f(int_c<SP_OP_IDENTITY>{}, v); break;
            case SP_OP_MASK: f(int_c<SP_OP_MASK>{}, v); break;
            default: f(int_c<SP_OP_INPAINT>{}, v); break;
        }
    });
}

static int elementwise_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const int P = static_cast<int>(tiles_elementwise(op->n));
    const dim3 grid(P, static_cast<unsigned>(r.batch));
    select_elementwise(op->kind, op->n, [&](auto opk, auto v) {
        launch_w(TK_DPS_RESIDUAL, (double)r.batch, k_dps_residual<opk(), v()>, grid, dim3(kBlock), s,
                 *op, r.x, r.eps, r.y, r.y_div, r.a, r.k, r.gs, r.v, r.partial, P, r.sched, r.cursor);
    });
    return check_launch("sp_dps_residual");
}

// y = A x, or x = A^T y: a copy, the mask (self-adjoint), the gather or its scatter
template <bool ADJOINT>
static int elementwise_map(const sp_op* op, const float* in, float* out, int64_t batch, hipStream_t s) {
    const char* what = ADJOINT ? "sp_op_adjoint" : "sp_op_apply";
    if (op->kind == SP_OP_IDENTITY) {
        const hipError_t e = hipMemcpyAsync(out, in, sizeof(float) * op->n * batch,
                                            hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { set_error(what, e); return SP_ELAUNCH; }
        return SP_OK;
    }
    const bool v4 = op->n % 4 == 0;
    const dim3 grid(stride_blocks(op->n, v4 ? 4 : 1, batch), batch);
#define SP_MAP(KERNEL)                                                                \
    if (v4) hipLaunchKernelGGL(KERNEL<4>, grid, dim3(kBlock), 0, s, *op, in, out);    \
    else hipLaunchKernelGGL(KERNEL<1>, grid, dim3(kBlock), 0, s, *op, in, out)
    if (op->kind == SP_OP_MASK) { SP_MAP(k_mask); }
    else if (ADJOINT) { SP_MAP(k_inpaint_scatter); }
    else { SP_MAP(k_inpaint_gather); }
#undef SP_MAP
    return check_launch(what);
}

// the proximal data step, alone (p.eps null) or inside the DiffPIR step: one launch of K3
static int elementwise_prox(const sp_op* op, const prox_args& p, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(tiles_elementwise(op->n)), static_cast<unsigned>(p.batch));
    select_elementwise(op->kind, op->n, [&](auto opk, auto v) {
        select_bool(p.eps, [&](auto step) {
            select_bool(p.xi, [&](auto xin) {  // the prox form has no noise: one kernel
                launch(0, k_prox<opk(), v(), step(), step() && xin()>, grid, dim3(kBlock), s, *op, p.x,
                       p.eps, p.y, p.xi, p.seed, p.step, p.sample_offset, p.y_div, p.c, p.out);
            });
        });
    });
    return check_launch(p.eps ? "sp_diffpir_step_ws" : "sp_op_prox_ws");
}

// the DDRM step of the elementwise kinds: one launch of K4
static int elementwise_ddrm(const sp_op* op, const ddrm_args& p, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(tiles_elementwise(op->n)), static_cast<unsigned>(p.batch));
    const ddrm_f fo = ddrm_class_coefs(p.c, 1.f, true), fu = ddrm_class_coefs(p.c, 1.f, false);
    select_elementwise(op->kind, op->n, [&](auto opk, auto v) {
        select_bool(p.xi, [&](auto xin) {
            launch(0, k_ddrm<opk(), v(), xin()>, grid, dim3(kBlock), s, *op, p.x, p.eps, p.y, p.xi,
                   p.seed, p.step, p.sample_offset, p.y_div, p.c, fo, fu, p.out);
        });
    });
    return check_launch("sp_ddrm_step_ws");
}

// The dispatch table: one row per kind, indexed by sp_op.kind (sp_ops.h).  Members are named, in
// op_kind's order; one a row leaves out is null.
static constexpr op_kind elementwise_row(valid_fn* valid) {
    return {.valid = valid, .partials = elementwise_partials,
            .dps_residual = elementwise_dps_residual, .apply = elementwise_map<false>,
            .adjoint = elementwise_map<true>, .psld_pixel = elementwise_psld_pixel,
            .psld_cotangent = elementwise_psld_cotangent, .pixel_opt = elementwise_pixel_opt,
            .traits = SP_TRAIT_FUSED_LATENT | SP_TRAIT_LINEAR, .prox = elementwise_prox,
            .diffpir_step = elementwise_prox, .ddrm_step = elementwise_ddrm};
}
static constexpr op_kind g_kinds[] = {
    /* SP_OP_IDENTITY */ elementwise_row(identity_valid),
    /* SP_OP_INPAINT */ elementwise_row(inpaint_valid),
    /* SP_OP_BLUR: no fused latent pass (its adjoint needs a halo), A^T A u from the caller */
    {.valid = blur_valid, .partials = blur_partials, .dps_residual = blur_dps_residual,
     .apply = blur_apply, .adjoint = blur_adjoint, .psld_cotangent = elementwise_psld_cotangent,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_LINEAR | SP_TRAIT_NEEDS_ATA_U},
    /* SP_OP_MASK */ elementwise_row(mask_valid),
    /* SP_OP_SR */
    {.valid = sr_valid, .partials = sr_partials, .dps_residual = sr_dps_residual, .apply = sr_apply,
     .adjoint = sr_adjoint, .psld_pixel = sr_psld_pixel, .psld_cotangent = sr_psld_cotangent,
     .pixel_opt = sr_pixel_opt,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_FUSED_LATENT | SP_TRAIT_LINEAR, .prox = sr_prox,
     .diffpir_step = sr_prox, .ddrm_step = sr_ddrm},
    /* SP_OP_PSF: as BLUR, and two launches through the caller's work buffer (_ws forms) */
    {.valid = psf_valid, .partials = psf_partials, .dps_workspace = psf_workspace,
     .dps_residual = psf_dps_residual, .apply = psf_apply, .adjoint = psf_adjoint,
     .psld_cotangent = elementwise_psld_cotangent,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_LINEAR | SP_TRAIT_NEEDS_ATA_U},
    /* SP_OP_PHASE: nonlinear (no adjoint, no A^T A, no PSLD), three launches through work */
    {.valid = phase_valid, .partials = phase_partials, .dps_workspace = phase_workspace,
     .op_workspace = phase_workspace, .dps_residual = phase_dps_residual, .apply_ws = phase_apply,
     .vjp_ws = phase_vjp, .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE},
    /* SP_OP_PSF_FFT: linear, but its maps need the workspace: apply_ws = A, vjp_ws = A^T (x not
       read); five pass-1 launches through work; no sp_op_apply / _adjoint, no latent passes */
    {.valid = psf_fft_valid, .partials = psf_fft_partials, .dps_workspace = psf_fft_workspace,
     .op_workspace = psf_fft_workspace, .dps_residual = psf_fft_dps_residual,
     .apply_ws = psf_fft_apply, .vjp_ws = psf_fft_vjp,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE},
    /* SP_OP_PSF_PERIODIC: PSF_FFT's functions on exact-size transforms (nothing extended or
       folded), and the only kind with the pseudo-inverse columns: A^+, the PGDM pass 1; its
       proximal map is one more multiplier between the column transforms */
    {.valid = psf_periodic_valid, .partials = psf_fft_partials, .dps_workspace = psf_fft_workspace,
     .op_workspace = psf_fft_workspace, .dps_residual = psf_fft_dps_residual,
     .apply_ws = psf_fft_apply, .vjp_ws = psf_fft_vjp,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_PINV,
     .pinv_ws = psf_periodic_pinv, .pgdm_prepare = psf_periodic_pgdm_prepare,
     .pgdm_residual = psf_periodic_pgdm_residual, .prox_workspace = psf_fft_workspace,
     .prox_prepare = psf_periodic_prox_prepare, .prox = psf_periodic_prox,
     .diffpir_step = psf_periodic_prox, .ddrm_workspace = psf_periodic_ddrm_workspace,
     .ddrm_step = psf_periodic_ddrm},
    /* SP_OP_RADON: as PSF (project, then backproject through the caller's work buffer), with an
       observation space of its own geometry: m = channels * radius * factor */
    {.valid = radon_valid, .partials = radon_partials, .dps_workspace = radon_workspace,
     .dps_residual = radon_dps_residual, .apply = radon_apply, .adjoint = radon_adjoint,
     .psld_cotangent = elementwise_psld_cotangent,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_LINEAR | SP_TRAIT_NEEDS_ATA_U},
    /* SP_OP_SR_PERIODIC: the periodic kind's columns with a lattice between the transforms: every
       pass PSF_PERIODIC has, y of (C, H / s, W / s) */
    {.valid = sr_periodic_valid, .partials = sr_periodic_partials,
     .dps_workspace = psf_fft_workspace, .op_workspace = psf_fft_workspace,
     .dps_residual = sr_periodic_dps_residual, .apply_ws = sr_periodic_apply,
     .vjp_ws = sr_periodic_vjp,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_PINV,
     .pinv_ws = sr_periodic_pinv, .pgdm_prepare = sr_periodic_pgdm_prepare,
     .pgdm_residual = sr_periodic_pgdm_residual, .prox_workspace = psf_fft_workspace,
     .prox_prepare = sr_periodic_prox_prepare, .prox = sr_periodic_prox,
     .diffpir_step = sr_periodic_prox},
    /* SP_OP_SVD_SEPARABLE: every column of PSF_PERIODIC on the SVDs of the two 1-D factors, as
       per-plane dense products; y of (C, Hy, Wy) */
    {.valid = svd_sep_valid, .partials = svd_sep_partials, .dps_workspace = svd_sep_dps_workspace,
     .op_workspace = svd_sep_op_workspace, .dps_residual = svd_sep_dps_residual,
     .apply_ws = svd_sep_apply, .vjp_ws = svd_sep_vjp,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_PINV,
     .pinv_ws = svd_sep_pinv, .pgdm_prepare = svd_sep_pgdm_prepare,
     .pgdm_residual = svd_sep_pgdm_residual, .prox_workspace = svd_sep_op_workspace,
     .prox_prepare = svd_sep_prox_prepare, .prox = svd_sep_prox, .diffpir_step = svd_sep_prox,
     .ddrm_workspace = svd_sep_ddrm_workspace, .ddrm_step = svd_sep_ddrm},
    /* SP_OP_HADAMARD: a partial isometry (A^+ = A^T) through butterflies in LDS: the columns of
       SVD_SEPARABLE but the prepare of the prox (its launches read y itself); q of PGDM and DDRM is
       y copied; y of (C, m / C) */
    {.valid = hadamard_valid, .partials = hadamard_partials, .dps_workspace = hadamard_workspace,
     .op_workspace = hadamard_workspace, .dps_residual = hadamard_dps_residual,
     .apply_ws = hadamard_apply, .vjp_ws = hadamard_vjp,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_DPS_WORKSPACE | SP_TRAIT_PINV,
     .pinv_ws = hadamard_pinv, .pgdm_prepare = hadamard_pgdm_prepare,
     .pgdm_residual = hadamard_pgdm_residual, .prox_workspace = hadamard_workspace,
     .prox = hadamard_prox, .diffpir_step = hadamard_prox,
     .ddrm_workspace = hadamard_workspace, .ddrm_step = hadamard_ddrm},
    /* SP_OP_CHANNEL_MIX: a Cy x C matrix across the channels at every pixel: SR's one-launch
       columns on the SVD of the matrix, and the pseudo-inverse columns without a workspace (the
       PGDM launch reads y itself); PSLD as BLUR, through the maps and the cotangent */
    {.valid = chanmix_valid, .partials = chanmix_partials, .dps_residual = chanmix_dps_residual,
     .apply = chanmix_apply, .adjoint = chanmix_adjoint,
     .psld_cotangent = elementwise_psld_cotangent,
     .traits = SP_TRAIT_UPDATE_READS_V | SP_TRAIT_LINEAR | SP_TRAIT_NEEDS_ATA_U | SP_TRAIT_PINV,
     .pinv_ws = chanmix_pinv, .pgdm_prepare = chanmix_pgdm_prepare,
     .pgdm_residual = chanmix_pgdm_residual, .prox = chanmix_prox, .diffpir_step = chanmix_prox,
     .ddrm_step = chanmix_ddrm},
};
constexpr int kKinds = sizeof(g_kinds) / sizeof(g_kinds[0]);
static_assert(SP_OP_IDENTITY == 0 && SP_OP_INPAINT == 1 && SP_OP_BLUR == 2 && SP_OP_MASK == 3 &&
                  SP_OP_SR == 4 && SP_OP_PSF == 5 && SP_OP_PHASE == 6 && SP_OP_PSF_FFT == 7 &&
                  SP_OP_PSF_PERIODIC == 8 && SP_OP_RADON == 9 && SP_OP_SR_PERIODIC == 10 &&
                  SP_OP_SVD_SEPARABLE == 11 && SP_OP_HADAMARD == 12 && SP_OP_CHANNEL_MIX == 13 &&
                  kKinds == 14,
              "g_kinds rows follow the sp_op kind numbering");

const op_kind* kind_of(const sp_op* op) {
    return op && op->kind >= 0 && op->kind < kKinds ? &g_kinds[op->kind] : nullptr;
}

bool valid_op(const sp_op* op) {
    const op_kind* k = kind_of(op);
    return k && op->n > 0 && op->m > 0 && k->valid(op);
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_version(void) { return 115; }

int sp_debug_build(void) { return SP_DEBUG; }

int64_t sp_debug_violations(int32_t reset, int32_t* first_site) {
    if (first_site) *first_site = 0;
#if SP_DEBUG
    if (hipDeviceSynchronize() != hipSuccess) return check_launch("sp_debug_violations");
    int64_t total = 0;
    for (dcheck_reader r : dcheck_readers()) {
        unsigned w[2] = {0u, 0u};
        if (r(w, reset) != 0) return check_launch("sp_debug_violations (read)");
        if (w[0] && first_site && !*first_site) *first_site = static_cast<int32_t>(w[1]);
        total += w[0];
    }
    return total;
#else
    (void)reset;
    return 0;
#endif
}

int sp_debug_selftest(sp_stream_t stream) {
#if SP_DEBUG
    launch(0, k_dcheck_selftest, dim3(1), dim3(64), static_cast<hipStream_t>(stream), 0);
    return check_launch("sp_debug_selftest");
#else
    (void)stream;
    return SP_EINVAL;
#endif
}

int sp_timing_enable(int on) {
    std::lock_guard<std::mutex> lock(g_timing_mu);
    g_timing = on != 0;
    return SP_OK;
}

int sp_timing_collect(int32_t* kinds, float* ms, int max_records) {
    return sp_timing_collect_work(kinds, ms, nullptr, max_records);
}

int sp_timing_collect_work(int32_t* kinds, float* ms, double* work, int max_records) {
    std::lock_guard<std::mutex> lock(g_timing_mu);
    int n = 0;
    for (const TimingRecord& r : g_records) {
        float t = -1.f;
        if (hipEventSynchronize(r.stop) == hipSuccess && hipEventElapsedTime(&t, r.start, r.stop) == hipSuccess &&
            n < max_records && kinds && ms) {
            kinds[n] = r.kind;
            ms[n] = t;
            if (work) work[n] = r.work;
            ++n;
        }
        g_event_pool.push_back(r.start);
        g_event_pool.push_back(r.stop);
    }
    g_records.clear();
    return n;
}

const char* sp_last_error(void) { return g_err; }

uint32_t sp_op_traits(const sp_op* op) { return valid_op(op) ? kind_of(op)->traits : 0; }

int64_t sp_rsq_partials(const sp_op* op) { return valid_op(op) ? kind_of(op)->partials(op) : SP_EINVAL; }

int64_t sp_dps_workspace(const sp_op* op, int64_t batch) {
    if (!valid_op(op) || batch <= 0) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    return k->dps_workspace ? k->dps_workspace(op, batch) : 0;
}

int64_t sp_op_workspace(const sp_op* op, int64_t batch) {
    if (!valid_op(op) || batch <= 0) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    return k->op_workspace ? k->op_workspace(op, batch) : 0;
}

int64_t sp_vec_partials(int64_t count) { return count > 0 ? tiles_elementwise(count) : SP_EINVAL; }

static int dps_residual_impl(const sp_op* op, const dps_residual_args& r, bool ws, sp_stream_t stream) {
    if (!valid_op(op) || !r.x || !r.eps || !r.y || !r.v || !r.partial || r.batch <= 0 || r.y_div <= 0 ||
        r.batch > 65535)
        return SP_EINVAL;
    const op_kind* kind = kind_of(op);
    if (kind->traits & SP_TRAIT_DPS_WORKSPACE) {  // several launches through the caller's work buffer
        if (!ws) return SP_EUNSUPPORTED;  // an entry without a work argument
        if (!r.work) return SP_EINVAL;
    }
    return kind->dps_residual(op, r, static_cast<hipStream_t>(stream));
}

int sp_dps_residual(const sp_op* op, const float* x, const float* eps, const float* y,
                    int64_t batch, int64_t y_div, const sp_dps_coefs* c, float* v_out,
                    float* rsq_partial, sp_stream_t stream) {
    if (!c) return SP_EINVAL;
    return dps_residual_impl(op, {x, eps, y, batch, y_div, c->a, c->k, c->grad_scale, nullptr, nullptr,
                                  v_out, rsq_partial, nullptr}, false, stream);
}

int sp_dps_residual_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                       int64_t batch, int64_t y_div, const sp_dps_coefs* c, float* v_out,
                       float* rsq_partial, float* work, sp_stream_t stream) {
    if (!c) return SP_EINVAL;
    return dps_residual_impl(op, {x, eps, y, batch, y_div, c->a, c->k, c->grad_scale, nullptr, nullptr,
                                  v_out, rsq_partial, work}, true, stream);
}

int sp_dps_residual_sched(const sp_op* op, const float* x, const float* eps, const float* y,
                          int64_t batch, int64_t y_div, const sp_step_rec* sched,
                          const int32_t* cursor, float* v_out, float* rsq_partial,
                          sp_stream_t stream) {
    if (!sched || !cursor) return SP_EINVAL;
    return dps_residual_impl(op, {x, eps, y, batch, y_div, 0.f, 0.f, 0.f, sched, cursor, v_out,
                                  rsq_partial, nullptr}, false, stream);
}

int sp_dps_residual_sched_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                             int64_t batch, int64_t y_div, const sp_step_rec* sched,
                             const int32_t* cursor, float* v_out, float* rsq_partial, float* work,
                             sp_stream_t stream) {
    if (!sched || !cursor) return SP_EINVAL;
    return dps_residual_impl(op, {x, eps, y, batch, y_div, 0.f, 0.f, 0.f, sched, cursor, v_out,
                                  rsq_partial, work}, true, stream);
}

static int dps_update_impl(const sp_op* op, const float* x, const float* eps, const float* y,
                           const float* v, const float* w, const float* rsq_partial,
                           const float* xi, uint64_t seed, int64_t step, int64_t sample_offset,
                           int64_t batch, int64_t y_div, sp_dps_coefs c,
                           const sp_step_rec* sched, const int32_t* cursor, float* x_out,
                           sp_stream_t stream) {
    if (!valid_op(op) || !x || !eps || !w || !x_out || batch <= 0 || y_div <= 0 ||
        batch > 65535)
        return SP_EINVAL;
    const bool reads_v = kind_of(op)->traits & SP_TRAIT_UPDATE_READS_V;
    if (!v && (reads_v || !y)) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = static_cast<int>(sp_rsq_partials(op));
    const int Pw = static_cast<int>(tiles_elementwise(op->n));
    const dim3 grid(Pw, static_cast<unsigned>(batch));
    // kinds that read v: the identity-kind kernel over it (flat Philox element index)
    select_elementwise(reads_v ? SP_OP_IDENTITY : op->kind, op->n, [&](auto opk, auto vw) {
        select_bool(v, [&](auto vin) {
            select_bool(xi, [&](auto xin) {
                launch_w(TK_DPS_UPDATE, (double)batch, k_dps_update<opk(), vw(), vin(), xin()>, grid,
                         dim3(kBlock), s, *op, x, eps, y, v, w, rsq_partial, P, xi, seed, step,
                         sample_offset, y_div, c, x_out, sched, cursor);
            });
        });
    });
    return check_launch("sp_dps_update");
}

int sp_dps_update(const sp_op* op, const float* x, const float* eps, const float* y,
                  const float* v, const float* w, const float* rsq_partial, const float* xi,
                  uint64_t seed, int64_t step, int64_t sample_offset, int64_t batch, int64_t y_div,
                  const sp_dps_coefs* c, float* x_out, sp_stream_t stream) {
    if (!c) return SP_EINVAL;
    return dps_update_impl(op, x, eps, y, v, w, rsq_partial, xi, seed, step, sample_offset, batch,
                           y_div, *c, nullptr, nullptr, x_out, stream);
}

int sp_dps_update_sched(const sp_op* op, const float* x, const float* eps, const float* y,
                        const float* v, const float* w, const float* rsq_partial,
                        uint64_t seed, int64_t sample_offset, int64_t batch, int64_t y_div,
                        const sp_step_rec* sched, const int32_t* cursor, float* x_out,
                        sp_stream_t stream) {
    if (!sched || !cursor) return SP_EINVAL;
    return dps_update_impl(op, x, eps, y, v, w, rsq_partial, nullptr, seed, 0, sample_offset,
                           batch, y_div, sp_dps_coefs{}, sched, cursor, x_out, stream);
}

__global__ void k_sched_timestep(const sp_step_rec* sched, const int32_t* cursor, int64_t* t) {
    *t = sched[*cursor].t;
}

__global__ void k_sched_advance(int32_t* cursor) { *cursor += 1; }

int sp_sched_timestep(const sp_step_rec* sched, const int32_t* cursor, int64_t* t_out,
                      sp_stream_t stream) {
    if (!sched || !cursor || !t_out) return SP_EINVAL;
    launch(0, k_sched_timestep, dim3(1), dim3(1), static_cast<hipStream_t>(stream), sched, cursor,
           t_out);
    return check_launch("sp_sched_timestep");
}

int sp_sched_advance(int32_t* cursor, sp_stream_t stream) {
    if (!cursor) return SP_EINVAL;
    launch(0, k_sched_advance, dim3(1), dim3(1), static_cast<hipStream_t>(stream), cursor);
    return check_launch("sp_sched_advance");
}

int sp_predict_x0(const float* x, const float* eps, int64_t count, float a, float k, float* out,
                  sp_stream_t stream) {
    if (!x || !eps || !out || count <= 0) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool v4 = count % 4 == 0 && aligned16(x) && aligned16(eps) && aligned16(out);
    if (v4)
        hipLaunchKernelGGL(k_predict_x0<4>, dim3(stride_blocks(count, 4, 1)), dim3(kBlock), 0, s,
                           x, eps, count, a, k, out);
    else
        hipLaunchKernelGGL(k_predict_x0<1>, dim3(stride_blocks(count, 1, 1)), dim3(kBlock), 0, s,
                           x, eps, count, a, k, out);
    return check_launch("sp_predict_x0");
}

int sp_randn(float* out, int64_t batch, int64_t n, uint64_t seed, int64_t step,
             int64_t sample_offset, sp_stream_t stream) {
    if (!out || batch <= 0 || n <= 0 || batch > 65535) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n % 4 == 0)
        hipLaunchKernelGGL(k_randn<4>, dim3(stride_blocks(n, 4, batch), batch), dim3(kBlock), 0, s,
                           out, n, seed, step, sample_offset);
    else
        hipLaunchKernelGGL(k_randn<1>, dim3(stride_blocks(n, 1, batch), batch), dim3(kBlock), 0, s,
                           out, n, seed, step, sample_offset);
    return check_launch("sp_randn");
}

int sp_residual_grad(const float* y, const float* z, int64_t batch, int64_t m, int64_t y_div,
                     float grad_scale, float* g, float* rsq_partial, sp_stream_t stream) {
    if (!y || !z || batch <= 0 || m <= 0 || y_div <= 0 || batch > 65535 || (!g && !rsq_partial))
        return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int P = static_cast<int>(tiles_elementwise(m));
    const dim3 grid(P, static_cast<unsigned>(batch));
    if (m % 4 == 0)
        hipLaunchKernelGGL(k_residual_grad<4>, grid, dim3(kBlock), 0, s, y, z, m, y_div,
                           grad_scale, g, rsq_partial, P);
    else
        hipLaunchKernelGGL(k_residual_grad<1>, grid, dim3(kBlock), 0, s, y, z, m, y_div,
                           grad_scale, g, rsq_partial, P);
    return check_launch("sp_residual_grad");
}

int sp_op_apply(const sp_op* op, const float* x, float* y, int64_t batch, sp_stream_t stream) {
    if (!valid_op(op) || !x || !y || batch <= 0 || batch > 65535) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->apply) return SP_EUNSUPPORTED;  // needs a workspace: sp_op_apply_ws
    return k->apply(op, x, y, batch, static_cast<hipStream_t>(stream));
}

int sp_op_apply_ws(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                   sp_stream_t stream) {
    if (!valid_op(op)) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->apply_ws) return sp_op_apply(op, x, y, batch, stream);
    if (!x || !y || !work || batch <= 0 || batch > 65535) return SP_EINVAL;
    return k->apply_ws(op, x, y, batch, work, static_cast<hipStream_t>(stream));
}

int sp_op_vjp_ws(const sp_op* op, const float* x, const float* g, float* dx, int64_t batch,
                 float* work, sp_stream_t stream) {
    if (!valid_op(op)) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->vjp_ws) return SP_EUNSUPPORTED;  // linear kinds: sp_op_adjoint
    if (!x || !g || !dx || !work || batch <= 0 || batch > 65535) return SP_EINVAL;
    return k->vjp_ws(op, x, g, dx, batch, work, static_cast<hipStream_t>(stream));
}

int sp_op_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, sp_stream_t stream) {
    if (!valid_op(op) || !x || !y || batch <= 0 || batch > 65535) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->adjoint) return SP_EUNSUPPORTED;  // nonlinear: sp_op_vjp_ws
    return k->adjoint(op, y, x, batch, static_cast<hipStream_t>(stream));
}

// a kind with pseudo-inverse passes and no workspace for them: `work` is not read
static bool pinv_without_work(const op_kind* k) { return k->pinv_ws && !k->op_workspace; }

int sp_op_pinv_ws(const sp_op* op, const float* y, float* x, int64_t batch, int32_t transpose,
                  float* work, sp_stream_t stream) {
    if (!valid_op(op)) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    // work may be null only for a kind whose pseudo-inverse needs none (sp_op_workspace is 0)
    if (!y || !x || (!work && !pinv_without_work(k)) || batch <= 0 || batch > 65535 ||
        (transpose != 0 && transpose != 1))
        return SP_EINVAL;
    if (!k->pinv_ws) return SP_EUNSUPPORTED;
    return k->pinv_ws(op, y, x, batch, transpose, work, static_cast<hipStream_t>(stream));
}

int sp_pgdm_prepare(const sp_op* op, const float* y, int64_t rows, float* q, sp_stream_t stream) {
    if (!valid_op(op) || !y || !q || rows <= 0 || rows > 65535) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->pgdm_prepare) return SP_EUNSUPPORTED;
    return k->pgdm_prepare(op, y, rows, q, static_cast<hipStream_t>(stream));
}

int sp_pgdm_residual_ws(const sp_op* op, const float* x, const float* eps, const float* q,
                        int64_t batch, int64_t y_div, const sp_dps_coefs* c, float* v_out,
                        float* work, sp_stream_t stream) {
    if (!valid_op(op)) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!x || !eps || !q || !c || !v_out || (!work && !pinv_without_work(k)) || batch <= 0 ||
        y_div <= 0 || batch > 65535)
        return SP_EINVAL;
    if (!k->pgdm_residual) return SP_EUNSUPPORTED;
    return k->pgdm_residual(op, x, eps, q, batch, y_div, *c, v_out, work,
                            static_cast<hipStream_t>(stream));
}

// ---- DiffPIR / proximal data step ----
int64_t sp_prox_workspace(const sp_op* op, int64_t batch) {
    if (!valid_op(op) || batch <= 0) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->prox) return SP_EUNSUPPORTED;
    return k->prox_workspace ? k->prox_workspace(op, batch) : 0;
}

// q has the intermediate's layout, so one row of it is one sample's workspace
int64_t sp_prox_prepare_size(const sp_op* op, int64_t rows) { return sp_prox_workspace(op, rows); }

int sp_prox_prepare(const sp_op* op, const float* y, int64_t rows, float* q, sp_stream_t stream) {
    if (!valid_op(op) || !y || rows <= 0 || rows > 65535) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->prox) return SP_EUNSUPPORTED;
    if (!k->prox_prepare) return SP_OK;  // nothing to prepare: the launch reads y itself
    if (!q) return SP_EINVAL;
    return k->prox_prepare(op, y, rows, q, static_cast<hipStream_t>(stream));
}

static bool prox_rho_ok(float rho) { return rho > 0.f && rho <= 3.402823466e+38f; }  // NaN fails both

// the kind's own buffers: y where the launch reads it, q and work where the kind prepares
static bool prox_buffers_ok(const op_kind* k, const prox_args& p) {
    return k->prox_prepare ? p.q && p.work : p.y != nullptr;
}

int sp_op_prox_ws(const sp_op* op, const float* x0, const float* y, const float* q, int64_t batch,
                  int64_t y_div, float rho, float* z_out, float* work, sp_stream_t stream) {
    if (!valid_op(op) || !x0 || !z_out || batch <= 0 || y_div <= 0 || batch > 65535 ||
        !prox_rho_ok(rho))
        return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->prox) return SP_EUNSUPPORTED;
    const prox_args p = {x0, nullptr, y, q, nullptr, 0, 0, 0, batch, y_div,
                         {1.f, 1.f, rho, 0.f, 0.f, 0.f}, z_out, work};
    if (!prox_buffers_ok(k, p)) return SP_EINVAL;
    return k->prox(op, p, static_cast<hipStream_t>(stream));
}

int sp_diffpir_step_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                       const float* q, const float* xi, uint64_t seed, int64_t step,
                       int64_t sample_offset, int64_t batch, int64_t y_div,
                       const sp_prox_coefs* coefs, float* x_out, float* work, sp_stream_t stream) {
    if (!valid_op(op) || !x || !eps || !coefs || !x_out || batch <= 0 || y_div <= 0 ||
        batch > 65535 || !prox_rho_ok(coefs->rho) || coefs->k == 0.f)
        return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->diffpir_step) return SP_EUNSUPPORTED;
    const prox_args p = {x, eps, y, q, xi, seed, step, sample_offset, batch, y_div, *coefs, x_out,
                         work};
    if (!prox_buffers_ok(k, p)) return SP_EINVAL;
    return k->diffpir_step(op, p, static_cast<hipStream_t>(stream));
}

// ---- DDRM / spectral step ----
int64_t sp_ddrm_workspace(const sp_op* op, int64_t batch) {
    if (!valid_op(op) || batch <= 0) return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->ddrm_step) return SP_EUNSUPPORTED;
    return k->ddrm_workspace ? k->ddrm_workspace(op, batch) : 0;
}

static bool ddrm_unit_ok(float v) { return v >= 0.f && v <= 1.f; }                  // NaN fails
static bool ddrm_sigma_ok(float v) { return v >= 0.f && v <= 3.402823466e+38f; }  // NaN, inf fail

int sp_ddrm_step_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                    const float* q, const float* xi, uint64_t seed, int64_t step,
                    int64_t sample_offset, int64_t batch, int64_t y_div,
                    const sp_ddrm_coefs* coefs, float* x_out, float* work, sp_stream_t stream) {
    if (!valid_op(op) || !x || !eps || !coefs || !x_out || batch <= 0 || y_div <= 0 ||
        batch > 65535 || coefs->a == 0.f || !ddrm_unit_ok(coefs->eta) ||
        !ddrm_unit_ok(coefs->eta_b) || !ddrm_sigma_ok(coefs->sig_y) ||
        !ddrm_sigma_ok(coefs->sig_prev))
        return SP_EINVAL;
    const op_kind* k = kind_of(op);
    if (!k->ddrm_step) return SP_EUNSUPPORTED;
    // the kind's own buffers: q and work for the kind with a workspace, y for the one-launch kinds
    if (k->ddrm_workspace ? !q || !work : !y) return SP_EINVAL;
    const ddrm_args p = {x, eps, y, q, xi, seed, step, sample_offset, batch, y_div, *coefs, x_out,
                         work};
    return k->ddrm_step(op, p, static_cast<hipStream_t>(stream));
}

}  // extern "C"
